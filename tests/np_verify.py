"""Independent numpy restatement of the RANSAC homography estimator of vulkansift_amd/csrc/hip/verify.hip (vksift_hip_ransac_homography,
vksift_ext_verifyHomography), in the manner of tests/np_restatement.py: what the kernels must compute, written down a second time.

  sampling   Python ints. key = first splitmix64 output of the state `seed`; the state of hypothesis j of slot i starts at
             key ^ (i << 32 | j); draw k (k = 0..3) is r = (hi32(next) * (n - k)) >> 32, stepped over the indices already drawn in
             increasing order. The hypothesis does not depend on nb_hypotheses.
  solve      np.float32, the kernel's operation order: coordinates scaled by 2^-13, cross products of the homogeneous source points,
             lambda / mu, H = B adj(A) with adj(A)'s rows lambda_j lambda_k (p_j x p_k); then H times the power of two that brings its
             largest entry into [1, 2), negated when d < 0 at the first sample point (evaluated before the scaling). A largest entry that is zero, subnormal, >= 2^127 or not finite: all-NaN (degenerate sample).
  test       u, v, d = H (xa, ya, 1); inlier iff d > 0 and (u - xb d)^2 + (v - yb d)^2 < (d d) t2, t2 = (t 2^-13)^2. No fused operation
             anywhere: fp32 add / sub / mul / div are correctly rounded here and on the GPU, so equality is bit for bit.
  winner     most inliers, ties to the lowest hypothesis; valid needs n >= 4, 4 inliers, h22 != 0 and finite H / h22 in pixels.

The same solve and test exist in float64 (no scaling needed, no normalisation) for the tests that ask how much fp32 costs."""
import numpy as np

MASK64 = (1 << 64) - 1
SCALE = np.float32(1.0 / 8192.0)
UNSCALE = np.float32(8192.0)


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def seed_key(seed):
    return _mix((seed + 0x9E3779B97F4A7C15) & MASK64)


def sample(seed, slot, hyp, n):
    """four distinct indices below n >= 4 in draw order"""
    st = seed_key(seed) ^ ((slot << 32) | hyp)
    drawn = []
    for k in range(4):
        st = (st + 0x9E3779B97F4A7C15) & MASK64
        r = ((_mix(st) >> 32) * (n - k)) >> 32
        for d in sorted(drawn):
            if r >= d:
                r += 1
        drawn.append(r)
    return drawn


def samples(seed, slot, nb_hyp, n):
    return np.array([sample(seed, slot, j, n) for j in range(nb_hyp)], np.int64).reshape(nb_hyp, 4)


def _solve_raw(c0, c1, c2, c3):
    """c_i: [k, 4] arrays {xa, ya, xb, yb} of one dtype -> [k, 9] un-normalised H, the kernel's operation order"""
    xa = [c[:, 0] for c in (c0, c1, c2, c3)]
    ya = [c[:, 1] for c in (c0, c1, c2, c3)]
    xb = [c[:, 2] for c in (c0, c1, c2, c3)]
    yb = [c[:, 3] for c in (c0, c1, c2, c3)]

    def cross(x, y, i, j):
        return y[i] - y[j], x[j] - x[i], x[i] * y[j] - x[j] * y[i]

    a, b, g = cross(xa, ya, 1, 2), cross(xa, ya, 2, 0), cross(xa, ya, 0, 1)
    lam = [(r[0] * xa[3] + r[1] * ya[3]) + r[2] for r in (a, b, g)]
    mu = [(r[0] * xb[3] + r[1] * yb[3]) + r[2] for r in (cross(xb, yb, 1, 2), cross(xb, yb, 2, 0), cross(xb, yb, 0, 1))]
    w = [mu[0] * (lam[1] * lam[2]), mu[1] * (lam[2] * lam[0]), mu[2] * (lam[0] * lam[1])]
    u = [w[i] * xb[i] for i in range(3)]
    v = [w[i] * yb[i] for i in range(3)]
    rows = []
    for q in (u, v, w):
        for col in range(3):
            rows.append((q[0] * a[col] + q[1] * b[col]) + q[2] * g[col])
    return np.stack(rows, axis=1)


def solve(c0, c1, c2, c3):
    """fp32: pixel correspondences [k, 4] float32 -> [k, 9] float32, scaled coordinates, largest entry in [1, 2) or all-NaN"""
    with np.errstate(all="ignore"):
        s = [np.ascontiguousarray(c, np.float32) * SCALE for c in (c0, c1, c2, c3)]
        H = _solve_raw(*s)
        assert H.dtype == np.float32
        e = (H.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1) >> np.uint32(23)
        ok = (e >= 1) & (e <= 253)
        f = ((np.uint32(254) - np.where(ok, e, 127).astype(np.uint32)) << np.uint32(23)).astype(np.uint32).view(np.float32)
        d0 = (H[:, 6] * s[0][:, 0] + H[:, 7] * s[0][:, 1]) + H[:, 8]
        f = np.where(d0 < 0, -f, f)          # the first sample point in front of the plane
        out = H * f[:, None]
        out[~ok] = np.uint32(0x7FC00000).view(np.float32)
    return out


def threshold2(threshold_px):
    ts = np.float32(threshold_px) * SCALE
    return np.float32(ts * ts)


def inliers(H, corr, t2, chunk=1 << 22):
    """fp32 test of every hypothesis against every correspondence: H [k, 9] (from solve), corr [n, 4] pixels -> bool [k, n]"""
    c = np.ascontiguousarray(corr, np.float32).reshape(-1, 4) * SCALE
    k, n = len(H), len(c)
    out = np.zeros((k, n), bool)
    step = max(1, chunk // max(n, 1))
    xa, ya, xb, yb = (c[None, :, i] for i in range(4))
    with np.errstate(all="ignore"):
        for s in range(0, k, step):
            h = [H[s:s + step, i, None] for i in range(9)]
            u = (h[0] * xa + h[1] * ya) + h[2]
            v = (h[3] * xa + h[4] * ya) + h[5]
            d = (h[6] * xa + h[7] * ya) + h[8]
            ru, rv = u - xb * d, v - yb * d
            e2 = ru * ru + rv * rv
            lim = (d * d) * t2
            assert e2.dtype == np.float32 and lim.dtype == np.float32
            out[s:s + step] = (d > 0) & (e2 < lim)
    return out


def inlier_counts(H, corr, t2s, chunk=1 << 21):
    """inlier counts of every hypothesis for several thresholds at once (what does not depend on the threshold is formed once), without
    the [k, n] matrix: -> int64 [len(t2s), k]"""
    c = np.ascontiguousarray(corr, np.float32).reshape(-1, 4) * SCALE
    k, n = len(H), len(c)
    out = np.zeros((len(t2s), k), np.int64)
    step = max(1, chunk // max(n, 1))
    xa, ya, xb, yb = (c[None, :, i] for i in range(4))
    with np.errstate(all="ignore"):
        for s in range(0, k, step):
            h = [H[s:s + step, i, None] for i in range(9)]
            d = (h[6] * xa + h[7] * ya) + h[8]
            ru = ((h[0] * xa + h[1] * ya) + h[2]) - xb * d
            rv = ((h[3] * xa + h[4] * ya) + h[5]) - yb * d
            e2 = ru * ru + rv * rv
            front = d > 0
            d *= d
            for i, t2 in enumerate(t2s):
                out[i, s:s + step] = (front & (e2 < d * np.float32(t2))).sum(axis=1)
    return out


def hypotheses(corr, nb_hyp, seed, slot):
    """(sample indices [nb_hyp, 4], H [nb_hyp, 9]) of a slot with n >= 4 correspondences"""
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    idx = samples(seed, slot, nb_hyp, len(corr))
    return idx, solve(*(corr[idx[:, i]] for i in range(4)))


def pick(counts):
    """best hypothesis of a count vector: most inliers, ties to the lowest index"""
    j = int(np.argmax(counts))  # argmax returns the first maximum
    return j, int(counts[j])


def finalise(corr, H_row, hyp, count, t2):
    """the result record and mask of a slot whose winner is hypothesis `hyp` with `count` inliers and scaled model H_row [9]"""
    n = len(corr)
    res = dict(H=np.zeros((3, 3), np.float32), nb_matches=n, nb_inliers=0, best_hypothesis=0, valid=0, mask=np.zeros(n, bool))
    if n < 4 or count < 4:
        return res
    with np.errstate(all="ignore"):
        g = np.array(H_row, np.float32)
        p = g.copy()
        p[2], p[5], p[6], p[7] = g[2] * UNSCALE, g[5] * UNSCALE, g[6] * SCALE, g[7] * SCALE
        o = p / g[8]
    if not (g[8] != 0 and np.isfinite(o).all()):
        return res
    res.update(H=o.reshape(3, 3), nb_inliers=count, best_hypothesis=hyp, valid=1, mask=inliers(g[None, :], corr, t2)[0])
    return res


def ransac(corr, nb_hyp, threshold_px, seed, slot=0, counts=None, hyps=None):
    """The estimator for one slot. corr: [n, 4] float32 pixels. `hyps` / `counts`: what hypotheses() / the inlier counts of at least nb_hyp
    hypotheses of this (corr, seed, slot, threshold) gave before (the hypotheses of a smaller nb_hyp are a prefix of a larger one's)."""
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    t2 = threshold2(threshold_px)
    if len(corr) < 4:
        return finalise(corr, None, 0, 0, t2)
    if hyps is None:
        hyps = hypotheses(corr, nb_hyp, seed, slot)
    H = hyps[1][:nb_hyp]
    if counts is None:
        counts = inliers(H, corr, t2).sum(axis=1)
    j, cnt = pick(np.asarray(counts)[:nb_hyp])
    return finalise(corr, H[j], j, cnt, t2)


# ---- float64 evaluation of the same hypotheses (what fp32 is measured against; never compared with the GPU) ----------------------------
def solve_f64(c0, c1, c2, c3):
    with np.errstate(all="ignore"):
        c = [np.asarray(x, np.float64) for x in (c0, c1, c2, c3)]
        H = _solve_raw(*c)
        d0 = (H[:, 6] * c[0][:, 0] + H[:, 7] * c[0][:, 1]) + H[:, 8]
        return np.where(d0[:, None] < 0, -H, H)   # the same sign rule: the first sample point in front of the plane


def inliers_f64(H, corr, threshold_px):
    c = np.asarray(corr, np.float64).reshape(-1, 4)
    xa, ya, xb, yb = (c[None, :, i] for i in range(4))
    h = [np.asarray(H, np.float64)[:, i, None] for i in range(9)]
    with np.errstate(all="ignore"):
        u = (h[0] * xa + h[1] * ya) + h[2]
        v = (h[3] * xa + h[4] * ya) + h[5]
        d = (h[6] * xa + h[7] * ya) + h[8]
        ru, rv = u - xb * d, v - yb * d
        return (d > 0) & (ru * ru + rv * rv < (d * d) * (float(threshold_px) ** 2))


def ransac_f64(corr, nb_hyp, threshold_px, seed, slot=0):
    """same samples, float64 solve and test: (winner, its count, its H [3, 3] normalised by h22, its mask, all counts)"""
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    idx = samples(seed, slot, nb_hyp, len(corr))
    H = solve_f64(*(corr[idx[:, i]] for i in range(4)))
    inl = inliers_f64(H, corr, threshold_px)
    counts = inl.sum(axis=1)
    j, cnt = pick(counts)
    with np.errstate(all="ignore"):
        Hn = (H[j] / H[j, 8]).reshape(3, 3)
    return j, cnt, Hn, inl[j], counts


def corner_error(H, H_true, w, h):
    """largest distance (px) between the images of the four image corners under H and under H_true (both 3x3, float64 arithmetic)"""
    H, H_true = np.asarray(H, np.float64), np.asarray(H_true, np.float64)
    err = 0.0
    for x, y in ((0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0)):
        p, q = H @ np.array([x, y, 1.0]), H_true @ np.array([x, y, 1.0])
        err = max(err, float(np.hypot(p[0] / p[2] - q[0] / q[2], p[1] / p[2] - q[1] / q[2])))
    return err


def synthetic_case(H_true, w, h, n=400, outliers=0.5, noise=0.5, seed=1):
    """n correspondences in a w x h image: a share `outliers` uniformly random on both sides, the rest mapped by H_true with Gaussian noise
    of `noise` px on the B side. Returns (corr float32 [n, 4], is_true_inlier bool [n])."""
    rng = np.random.default_rng(seed)
    xa, ya = rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)
    den = H_true[2, 0] * xa + H_true[2, 1] * ya + H_true[2, 2]
    xb = (H_true[0, 0] * xa + H_true[0, 1] * ya + H_true[0, 2]) / den + rng.normal(0, noise, n)
    yb = (H_true[1, 0] * xa + H_true[1, 1] * ya + H_true[1, 2]) / den + rng.normal(0, noise, n)
    out = rng.permutation(n) < int(round(n * outliers))
    xb[out], yb[out] = rng.uniform(0, w - 1, int(out.sum())), rng.uniform(0, h - 1, int(out.sum()))
    return np.stack([xa, ya, xb, yb], axis=1).astype(np.float32), ~out
