"""Independent numpy restatement of the RANSAC fundamental-matrix estimator of vulkansift_amd/csrc/hip/verify.hip
(vksift_hip_ransac_fundamental, vksift_ext_verifyFundamental), in the manner of tests/np_verify.py: what the kernels must compute, written
down a second time, vectorised over the hypotheses.

  sampling   np_verify's generator with seven draws: draw j is r = (hi32(next) * (n - j)) >> 32, stepped over the indices already drawn in
             increasing order (four draws give np_verify.sample).
  solve      np.float32, the kernel's operation order, no fused operation. Coordinates scaled by 2^-13; each side of the sample conditioned
             (centroid = fixed-order sum times 1.0f/7.0f, then the power of two that brings the largest |deviation| into [1, 2)); the 7x9
             system with rows (xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1); Gauss-Jordan on columns 0..6: for column k the rows
             k+1..6 are compared with row k one after the other and exchanged when their |entry| (bit pattern) is strictly larger, row k
             is multiplied by 1 / pivot, and every other row r loses a[r][k] * row k. F1 = (-a[.][7], 1, 0), F2 = (-a[.][8], 0, 1).
             det(F1 + a F2) = c0 + c1 a + c2 a^2 + c3 a^3 by cofactors along the last row (1 and a stand there).
  roots      c3 zero or subnormal, a non-finite coefficient or a non-finite bound: degenerate (no model). Else monic b_i = c_i / c3,
             R = 1 + max |b_i| (Cauchy), disc = b2 b2 - 3 b1, s = sqrt(disc > 0 ? disc : 0), lo = (-b2 - s) / 3, hi = (-b2 + s) / 3; on each
             of (-R, lo), (lo, hi), (hi, R) whose end points differ in `p(x) < 0` (Horner) BISECT_STEPS bisection steps, root = mid point
             of what is left. The roots present are numbered 0.. in increasing order.
  model      F^ = F1 + a F2, F = T_b^T F^ T_a in the common scaled coordinates, times the power of two that brings its largest entry into
             [1, 2); anything not finite: all-NaN.
  test       l = F (xa, ya, 1), m = F^T (xb, yb, 1), r = (xb, yb, 1) l; inlier iff r r < t2 ((l0 l0 + l1 l1) + (m0 m0 + m1 m1)).
  winner     largest (count, lowest model id), id = 4 hypothesis + root; valid needs n >= 7, 8 inliers and a finite model in pixels.

Not done, as in the kernels: no rank or chirality test beyond the construction, no handling of the planar degeneracy, no refit.
A float64 evaluation of the same samples (SVD null space, numpy.roots) exists for the tests that ask what fp32 costs."""
import numpy as np

import np_verify as V
from np_verify import MASK64, SCALE, _mix, pick, seed_key, threshold2  # noqa: F401  (re-exported for the tests)

F32 = np.float32
NAN32 = np.uint32(0x7FC00000).view(np.float32)
BISECT_STEPS = 48
SAMPLE = 7
# Largest number of true inliers by which the fp32 winner's mask fell short of the float64 evaluation's over the cases of
# test_np_verify_f.test_what_fp32_costs (computed and asserted there, recorded in DESIGN.md); the GPU test allows twice this.
FP32_MAX_SHORTFALL = 0


def sample_k(seed, slot, hyp, n, k):
    """k distinct indices below n >= k in draw order"""
    st = seed_key(seed) ^ ((slot << 32) | hyp)
    drawn = []
    for j in range(k):
        st = (st + 0x9E3779B97F4A7C15) & MASK64
        r = ((_mix(st) >> 32) * (n - j)) >> 32
        for d in sorted(drawn):
            if r >= d:
                r += 1
        drawn.append(r)
    return drawn


def samples(seed, slot, nb_hyp, n):
    return np.array([sample_k(seed, slot, j, n, SAMPLE) for j in range(nb_hyp)], np.int64).reshape(nb_hyp, SAMPLE)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def _unit_scale(mbits):
    """(ok, 2^(127 - e)) for the exponent e of the largest magnitude; ok: normal and below 2^127"""
    e = mbits >> np.uint32(23)
    ok = (e >= 1) & (e <= 253)
    f = ((np.uint32(254) - np.where(ok, e, 127).astype(np.uint32)) << np.uint32(23)).astype(np.uint32).view(np.float32)
    return ok, f


def _condition(x, y):
    """x, y: seven [k] arrays of one side -> (x^, y^, s, s cx, s cy); s is NaN where the deviations cannot be scaled"""
    cx = ((((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]) + x[6]) * (F32(1.0) / F32(7.0))
    cy = ((((((y[0] + y[1]) + y[2]) + y[3]) + y[4]) + y[5]) + y[6]) * (F32(1.0) / F32(7.0))
    dx, dy = [v - cx for v in x], [v - cy for v in y]
    m = _bits(dx[0])
    for v in dx[1:] + dy:
        m = np.maximum(m, _bits(v))
    ok, s = _unit_scale(m)
    s = np.where(ok, s, NAN32)
    return [v * s for v in dx], [v * s for v in dy], s, s * cx, s * cy


def _poly_coefficients(p, q):
    """det(P + a Q) with P = (p0..p6, 1, 0), Q = (q0..q6, 0, 1): [c0, c1, c2, c3]"""
    t1 = [-p[5], p[4] - q[5], q[4]]                                                       # m4 a - m5
    t2 = [-(p[5] * p[6]), p[3] - (p[5] * q[6] + q[5] * p[6]), q[3] - q[5] * q[6]]         # m3 a - m5 m6
    t3 = [p[3] - p[4] * p[6], q[3] - (p[4] * q[6] + q[4] * p[6]), -(q[4] * q[6])]         # m3 - m4 m6

    def lin_quad(i, t):
        return [p[i] * t[0], p[i] * t[1] + q[i] * t[0], p[i] * t[2] + q[i] * t[1], q[i] * t[2]]

    A, B, C = lin_quad(0, t1), lin_quad(1, t2), lin_quad(2, t3)
    return [(A[i] - B[i]) + C[i] for i in range(4)]


def cubic_roots(c0, c1, c2, c3):
    """real roots of c0 + c1 a + c2 a^2 + c3 a^3 for [k] float32 arrays -> (roots [k, 3] in increasing order, NaN where absent; count [k])"""
    with np.errstate(all="ignore"):
        c0, c1, c2, c3 = (np.ascontiguousarray(c, np.float32).reshape(-1) for c in (c0, c1, c2, c3))
        mc = np.maximum(np.maximum(_bits(c0), _bits(c1)), np.maximum(_bits(c2), _bits(c3)))
        b2, b1, b0 = c2 / c3, c1 / c3, c0 / c3
        R = F32(1.0) + np.maximum(np.maximum(_bits(b2), _bits(b1)), _bits(b0)).view(np.float32)
        deg = ((_bits(c3) >> np.uint32(23)) == 0) | ((mc >> np.uint32(23)) == 255) | ((_bits(R) >> np.uint32(23)) == 255)

        def neg(x):
            return (((x + b2) * x + b1) * x + b0) < 0

        disc = b2 * b2 - F32(3.0) * b1
        s = np.sqrt(np.where(disc > 0, disc, F32(0.0)).astype(np.float32))
        lo, hi = (-b2 - s) / F32(3.0), (-b2 + s) / F32(3.0)
        ends = [-R, lo, hi, R]
        ngs = [neg(e) for e in ends]
        roots, has = [], []
        for i in range(3):
            l, r, nl = ends[i].copy(), ends[i + 1].copy(), ngs[i]
            has.append((ngs[i] != ngs[i + 1]) & ~deg)
            for _ in range(BISECT_STEPS):
                m = (l + r) * F32(0.5)
                same = neg(m) == nl
                l, r = np.where(same, m, l), np.where(same, r, m)
            roots.append(((l + r) * F32(0.5)).astype(np.float32))
        k = len(c0)
        out = np.full((k, 3), NAN32, np.float32)
        cnt = np.zeros(k, np.int64)
        for i in range(3):
            for slot in range(3):
                put = has[i] & (cnt == slot)
                out[put, slot] = roots[i][put]
            cnt += has[i]
    return out, cnt


def solve(c):
    """fp32: pixel correspondences [k, 7, 4] float32 -> (models [k, 3, 9] float32 in scaled coordinates, largest entry in [1, 2) or all-NaN;
    number of roots [k])"""
    with np.errstate(all="ignore"):
        c = np.ascontiguousarray(c, np.float32).reshape(-1, SAMPLE, 4) * SCALE
        xa, ya, sa, ua, va = _condition([c[:, i, 0] for i in range(SAMPLE)], [c[:, i, 1] for i in range(SAMPLE)])
        xb, yb, sb, ub, vb = _condition([c[:, i, 2] for i in range(SAMPLE)], [c[:, i, 3] for i in range(SAMPLE)])
        one = np.ones(len(c), np.float32)
        a = [[xb[i] * xa[i], xb[i] * ya[i], xb[i], yb[i] * xa[i], yb[i] * ya[i], yb[i], xa[i], ya[i], one] for i in range(SAMPLE)]
        for k in range(7):
            for r in range(k + 1, 7):
                sw = _bits(a[r][k]) > _bits(a[k][k])
                for j in range(k, 9):
                    a[k][j], a[r][j] = np.where(sw, a[r][j], a[k][j]), np.where(sw, a[k][j], a[r][j])
            inv = F32(1.0) / a[k][k]
            for j in range(k + 1, 9):
                a[k][j] = a[k][j] * inv
            for r in range(7):
                if r != k:
                    f = a[r][k]
                    for j in range(k + 1, 9):
                        a[r][j] = a[r][j] - f * a[k][j]
        p, q = [-a[i][7] for i in range(7)], [-a[i][8] for i in range(7)]
        cf = _poly_coefficients(p, q)
        assert all(x.dtype == np.float32 for x in cf)
        roots, cnt = cubic_roots(*cf)
        models = np.empty((len(c), 3, 9), np.float32)
        for slot in range(3):
            al = roots[:, slot]
            fh = [p[i] + al * q[i] for i in range(7)] + [one, al]
            g = [None] * 9
            for r in range(3):
                g[3 * r], g[3 * r + 1] = fh[3 * r] * sa, fh[3 * r + 1] * sa
                g[3 * r + 2] = (fh[3 * r + 2] - fh[3 * r] * ua) - fh[3 * r + 1] * va
            F = [None] * 9
            for col in range(3):
                F[col], F[3 + col] = sb * g[col], sb * g[3 + col]
                F[6 + col] = (g[6 + col] - ub * g[col]) - vb * g[3 + col]
            F = np.stack(F, axis=1).astype(np.float32)
            ok, f = _unit_scale(_bits(F).max(axis=1))
            out = F * f[:, None]
            out[~ok] = NAN32
            models[:, slot] = out
    return models, cnt


def inliers(F, corr, t2, chunk=1 << 22):
    """fp32 Sampson test of every model against every correspondence: F [k, 9] (scaled coordinates), corr [n, 4] pixels -> bool [k, n]"""
    c = np.ascontiguousarray(corr, np.float32).reshape(-1, 4) * SCALE
    F = np.ascontiguousarray(F, np.float32).reshape(-1, 9)
    k, n = len(F), len(c)
    out = np.zeros((k, n), bool)
    step = max(1, chunk // max(n, 1))
    xa, ya, xb, yb = (c[None, :, i] for i in range(4))
    t2 = F32(t2)
    with np.errstate(all="ignore"):
        for s in range(0, k, step):
            f = [F[s:s + step, i, None] for i in range(9)]
            l0 = (f[0] * xa + f[1] * ya) + f[2]
            l1 = (f[3] * xa + f[4] * ya) + f[5]
            l2 = (f[6] * xa + f[7] * ya) + f[8]
            r = (xb * l0 + yb * l1) + l2
            m0 = (f[0] * xb + f[3] * yb) + f[6]
            m1 = (f[1] * xb + f[4] * yb) + f[7]
            g = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
            lhs, rhs = r * r, t2 * g
            assert lhs.dtype == np.float32 and rhs.dtype == np.float32
            out[s:s + step] = lhs < rhs
    return out


def inlier_counts(F, corr, t2s):
    return np.stack([inliers(F, corr, t2).sum(axis=1) for t2 in t2s]).astype(np.int64)


def hypotheses(corr, nb_hyp, seed, slot):
    """(sample indices [nb_hyp, 7], models [nb_hyp * 4, 9] indexed by model id = 4 hypothesis + root; id 4 j + 3 is always all-NaN)"""
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    idx = samples(seed, slot, nb_hyp, len(corr))
    m3, _ = solve(corr[idx])
    models = np.full((nb_hyp, 4, 9), NAN32, np.float32)
    models[:, :3] = m3
    return idx, models.reshape(nb_hyp * 4, 9)


def finalise(corr, F_row, model_id, count, t2):
    n = len(corr)
    res = dict(F=np.zeros((3, 3), np.float32), nb_matches=n, nb_inliers=0, best_hypothesis=0, best_root=0, valid=0, mask=np.zeros(n, bool))
    if n < SAMPLE or count < SAMPLE + 1:
        return res
    with np.errstate(all="ignore"):
        g = np.array(F_row, np.float32)
        o = g.copy()
        for i in (2, 5, 6, 7):
            o[i] = g[i] * F32(8192.0)
        o[8] = g[8] * F32(67108864.0)
        ok, f = _unit_scale(_bits(o).max(keepdims=True))
        o = o * f[0]
    if not ok[0]:
        return res
    res.update(F=o.reshape(3, 3), nb_inliers=count, best_hypothesis=model_id >> 2, best_root=model_id & 3, valid=1, mask=inliers(g[None, :], corr, t2)[0])
    return res


def ransac(corr, nb_hyp, threshold_px, seed, slot=0, counts=None, hyps=None):
    """The estimator for one slot. corr: [n, 4] float32 pixels. `hyps` / `counts`: what hypotheses() / the inlier counts per model id of at
    least nb_hyp hypotheses of this (corr, seed, slot, threshold) gave before (a smaller nb_hyp's models are a prefix of a larger one's)."""
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    t2 = threshold2(threshold_px)
    if len(corr) < SAMPLE:
        return finalise(corr, None, 0, 0, t2)
    if hyps is None:
        hyps = hypotheses(corr, nb_hyp, seed, slot)
    F = hyps[1][:nb_hyp * 4]
    if counts is None:
        counts = inliers(F, corr, t2).sum(axis=1)
    j, cnt = pick(np.asarray(counts)[:nb_hyp * 4])
    return finalise(corr, F[j], j, cnt, t2)


# ---- float64 evaluation of the same samples (what fp32 is measured against; never compared with the GPU) -------------------------------
def _hartley(x, y):
    cx, cy = x.mean(), y.mean()
    s = np.sqrt(2.0) / max(np.mean(np.hypot(x - cx, y - cy)), 1e-300)
    return np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])


def solve_f64(c):
    """seven correspondences [7, 4] (pixels) -> list of 3x3 float64 F (pixels), one per real root"""
    c = np.asarray(c, np.float64)
    Ta, Tb = _hartley(c[:, 0], c[:, 1]), _hartley(c[:, 2], c[:, 3])
    pa = (Ta @ np.stack([c[:, 0], c[:, 1], np.ones(7)])).T
    pb = (Tb @ np.stack([c[:, 2], c[:, 3], np.ones(7)])).T
    A = np.stack([pb[:, i] * pa[:, j] for i in range(3) for j in range(3)], axis=1)
    _, _, vt = np.linalg.svd(A)
    F1, F2 = vt[-1].reshape(3, 3), vt[-2].reshape(3, 3)
    # det(F1 + a F2) is a cubic: through its values at four points
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    coef = np.polyfit(xs, [np.linalg.det(F1 + x * F2) for x in xs], 3)
    out = []
    for r in np.roots(coef):
        if abs(r.imag) <= 1e-9 * (1.0 + abs(r.real)):
            out.append(Tb.T @ (F1 + r.real * F2) @ Ta)
    return out


def sampson_inliers_f64(F, corr, threshold_px):
    c = np.asarray(corr, np.float64).reshape(-1, 4)
    pa, pb = np.stack([c[:, 0], c[:, 1], np.ones(len(c))]), np.stack([c[:, 2], c[:, 3], np.ones(len(c))])
    l, m = F @ pa, F.T @ pb
    r = (pb * l).sum(axis=0)
    return r * r < float(threshold_px) ** 2 * (l[0] ** 2 + l[1] ** 2 + m[0] ** 2 + m[1] ** 2)


def ransac_f64(corr, nb_hyp, threshold_px, seed, slot=0):
    """same samples, float64 solve and test: (best count, its F, its mask)"""
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    idx = samples(seed, slot, nb_hyp, len(corr))
    best = (-1, None, None)
    for j in range(nb_hyp):
        for F in solve_f64(corr[idx[j]]):
            inl = sampson_inliers_f64(F, corr, threshold_px)
            if int(inl.sum()) > best[0]:
                best = (int(inl.sum()), F, inl)
    return best


def two_view_case(n, outliers, noise, seed, w, h):
    """n correspondences of two w x h views of random 3-D points in front of both cameras (focal length 0.9 w, the second camera rotated by
    (0.10, -0.15, 0.05) rad about x, y, z and moved by (1.0, 0.1, 0.2) against depths of 4 .. 10), Gaussian noise of `noise` px on the B
    side, a share `outliers` uniformly random on both sides. Returns (corr float32 [n, 4], is_true_inlier bool [n], F_true float64 3x3)."""
    rng = np.random.default_rng(seed)
    K = np.array([[0.9 * w, 0, 0.5 * (w - 1)], [0, 0.9 * w, 0.5 * (h - 1)], [0, 0, 1.0]])
    rx, ry, rz = 0.10, -0.15, 0.05
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    R, t = Rz @ Ry @ Rx, np.array([1.0, 0.1, 0.2])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F_true = Ki.T @ tx @ R @ Ki
    m = 8 * n + 64
    xa, ya, depth = rng.uniform(0, w - 1, m), rng.uniform(0, h - 1, m), rng.uniform(4.0, 10.0, m)
    X = (Ki @ np.stack([xa, ya, np.ones(m)])) * depth
    q = K @ (R @ X + t[:, None])
    xb, yb = q[0] / q[2], q[1] / q[2]
    keep = np.flatnonzero((q[2] > 0) & (xb >= 0) & (xb <= w - 1) & (yb >= 0) & (yb <= h - 1))[:n]
    assert len(keep) == n
    xa, ya = xa[keep], ya[keep]
    xb, yb = xb[keep] + rng.normal(0, noise, n), yb[keep] + rng.normal(0, noise, n)
    out = rng.permutation(n) < int(round(n * outliers))
    k = int(out.sum())
    xa[out], ya[out] = rng.uniform(0, w - 1, k), rng.uniform(0, h - 1, k)
    xb[out], yb[out] = rng.uniform(0, w - 1, k), rng.uniform(0, h - 1, k)
    return np.stack([xa, ya, xb, yb], axis=1).astype(np.float32), ~out, F_true


# ---- the inputs of the kernel-level GPU test, shared with the CPU test that measures what fp32 costs on them -----------------------------
SLOT_N = [0, 6, 7, 8, 63, 64, 65, 255, 256, 257, 1000]   # below / at the sample size, the wave and LDS-tile boundaries
SLOT_SIZES = [(640, 480), (4000, 3000)]
BIG_SLOT = 8                                              # this slot lies in a 16383 px image and holds the coordinate 16383.0


def kernel_test_slots():
    """[(corr, is_true_inlier, F_true)] per slot of SLOT_N: n <= 8 exact projections without outliers (so that a model with 8 inliers exists
    for n = 8), larger slots 50 % outliers and 0.5 px noise"""
    out = []
    for i, n in enumerate(SLOT_N):
        w, h = (16383, 12000) if i == BIG_SLOT else SLOT_SIZES[i % 2]
        small = n <= 8
        c, true, Ft = two_view_case(n, 0.0 if small else 0.5, 0.0 if small else 0.5, 70 + i, w, h)
        if i == BIG_SLOT:
            c[1, 0], c[n - 1, 2] = 16383.0, 16383.0       # on outliers or not: the largest coordinate the kernels are specified for
        out.append((c, true, Ft))
    return out
