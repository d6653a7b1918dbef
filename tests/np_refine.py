"""Independent numpy restatement of the locally optimised homography refit of vulkansift_amd/csrc/hip/refine.hip (vksift_hip_refit_homography,
vksift_ext_refineHomography), in the manner of tests/np_verify.py: what the kernel must compute, written down a second time. This file is the
specification of the operation order; every value is np.float32 with one rounding per operation, no fused operation anywhere.

  sums       every sum over correspondences has one order: thread t of 256 adds its elements k = t, t + 256, ... in increasing k (an element
             whose mask byte is not 1 adds +0, which changes no bit: a partial sum that starts at +0 is never -0); then the butterfly
             p[l] = p[l] + p[l ^ off], off = 32, 16, 8, 4, 2, 1 inside each wave of 64 (addition commutes: every lane holds the same bits);
             then ((w0 + w1) + w2) + w3 over the four waves. Counts and largest magnitudes are integers (any order).
  round      from a mask with m ones (m < 4: the round fails)
    1 conditioning, each side on its own: centroid = sum / float(m); s = the power of two that brings the largest |x - cx|, |y - cy| over the
      inliers (by bit pattern, NaN and infinity above everything) into [1, 2): 2^(127 - e); no such power (e = 0, 254, 255): the round fails.
      x = (xa - cxa) sa, y = (ya - cya) sa, X = (xb - cxb) sb, Y = (yb - cyb) sb.
    2 one accumulation serves the linear start and the Gauss-Newton steps: per inlier seven values (a, b, i, pu, pv, ru, rv) give the rows
      [a b i 0 0 0 -pu a -pu b | -ru] and [0 0 0 a b i -pv a -pv b | -rv]; their 8x8 normal equations are 27 distinct sums (SUMS below).
        linear start (h8 = 1):  (x, y, 1, X, Y, -X, -Y): the solution is h.
        Gauss-Newton step:      u = (h0 x + h1 y) + h2, v = (h3 x + h4 y) + h5, d = (h6 x + h7 y) + 1, i = 1 / d, a = x i, b = y i,
                                pu = u i, pv = v i, ru = pu - X, rv = pv - Y (the forward transfer error): the solution is added to h.
      GAUSS_NEWTON_STEPS = 2 of them.
    3 each 8x9 system by Gauss-Jordan: for column k the rows k+1..7 are compared with row k in turn and exchanged when their |entry| (bit
      pattern) is strictly larger; a pivot that is zero, subnormal or not finite fails the round; row k times 1 / pivot; every other row r
      minus a[r][k] times row k. A solution entry that is not finite fails the round.
    4 back to pixels: G = Hc Ta with ua = sa cxa, va = sa cya: G[r] = (Hc[r][0] sa, Hc[r][1] sa, (Hc[r][2] - Hc[r][0] ua) - Hc[r][1] va);
      H = Tb^-1 G with isb = 1 / sb: H[0] = G[0] isb + cxb G[2], H[1] = G[1] isb + cyb G[2], H[2] = G[2]; published o = H / H[8];
      H[8] == 0 or an entry of o not finite: the round fails.
    5 re-scoring of all n correspondences in pixels under o, np_guided.admissible(HOMOGRAPHY) with np_guided.threshold2(threshold_px).
  chain      kept = the RANSAC record (H, nb_inliers, mask), rounds = 0. Round r = 1 .. nb_rounds starts from the kept mask; it is accepted
             iff it did not fail and its count >= the kept count, and then becomes the kept result with rounds = r; the first round that is
             not accepted ends the loop. An invalid start record: an all-zero record and mask.

The same algorithm exists in float64 (refit_f64; numpy sums, numpy's solver) for the tests that ask how much fp32 costs.

Also the synthetic slots of the kernel-level GPU test, shared with the CPU tests."""
import numpy as np

import np_guided as G

F32 = np.float32
THREADS = 256
GAUSS_NEWTON_STEPS = 2
MAX_ROUNDS = 8
# the 27 sums of an accumulation, in the kernel's order
SUMS = ["aa", "ab", "ai", "bb", "bi", "ii", "Uaa", "Uab", "Ubb", "Uia", "Uib", "Vaa", "Vab", "Vbb", "Via", "Vib", "Waa", "Wab", "Wbb",
        "R0", "R1", "R2", "R3", "R4", "R5", "R6", "R7"]


def block_sum(values):
    """values float32 [q, n] (already zero where the mask is not 1) -> float32 [q]: the order of the module docstring"""
    v = np.ascontiguousarray(values, np.float32)
    q, n = v.shape
    rows = (n + THREADS - 1) // THREADS
    pad = np.zeros((q, rows * THREADS), np.float32)
    pad[:, :n] = v
    pad = pad.reshape(q, rows, THREADS)
    with np.errstate(all="ignore"):
        p = np.zeros((q, THREADS), np.float32)
        for j in range(rows):
            p = p + pad[:, j]
        p = p.reshape(q, 4, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            p = p + p[:, :, lane ^ off]
        w = p[:, :, 0]
        out = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    assert out.dtype == np.float32
    return out


def abs_bits(x):
    return np.asarray(x, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def unit_scale(mbits):
    e = int(mbits) >> 23
    ok = 1 <= e <= 253
    return np.array([(254 - (e if ok else 127)) << 23], np.uint32).view(np.float32)[0], ok


def condition(x, y, inl):
    """one side: (cx, cy, s) or None"""
    m = int(inl.sum())
    with np.errstate(all="ignore"):
        s = block_sum(np.stack([np.where(inl, x, F32(0)), np.where(inl, y, F32(0))]))
        cx, cy = s[0] / F32(m), s[1] / F32(m)
        dev = np.concatenate([abs_bits(x - cx)[inl], abs_bits(y - cy)[inl]])
    f, ok = unit_scale(dev.max() if len(dev) else 0)
    return (cx, cy, f) if ok else None


def accumulate(a, b, i, pu, pv, ru, rv, inl):
    with np.errstate(all="ignore"):
        aa, ab, ai, bb, bi, ii = a * a, a * b, a * i, b * b, b * i, i * i
        w = pu * pu + pv * pv
        q = pu * ru + pv * rv
        terms = [aa, ab, ai, bb, bi, ii, pu * aa, pu * ab, pu * bb, pu * ai, pu * bi, pv * aa, pv * ab, pv * bb, pv * ai, pv * bi, w * aa, w * ab, w * bb,
                 a * ru, b * ru, i * ru, a * rv, b * rv, i * rv, q * a, q * b]
        assert all(t.dtype == np.float32 for t in terms) and len(terms) == len(SUMS)
        return block_sum(np.stack([np.where(inl, t, F32(0)) for t in terms]))


def system(S):
    """the 8x9 augmented normal equations of the 27 sums"""
    s = dict(zip(SUMS, S))
    z = F32(0)
    P = [[s["aa"], s["ab"], s["ai"]], [s["ab"], s["bb"], s["bi"]], [s["ai"], s["bi"], s["ii"]]]
    U = [[s["Uaa"], s["Uab"]], [s["Uab"], s["Ubb"]], [s["Uia"], s["Uib"]]]
    V = [[s["Vaa"], s["Vab"]], [s["Vab"], s["Vbb"]], [s["Via"], s["Vib"]]]
    A = np.zeros((8, 9), np.float32)
    for r in range(3):
        A[r, :] = P[r] + [z, z, z] + [-U[r][0], -U[r][1]] + [-s["R%d" % r]]
        A[3 + r, :] = [z, z, z] + P[r] + [-V[r][0], -V[r][1]] + [-s["R%d" % (3 + r)]]
    A[6, :] = [-U[0][0], -U[1][0], -U[2][0], -V[0][0], -V[1][0], -V[2][0], s["Waa"], s["Wab"], s["R6"]]
    A[7, :] = [-U[0][1], -U[1][1], -U[2][1], -V[0][1], -V[1][1], -V[2][1], s["Wab"], s["Wbb"], s["R7"]]
    return A


def solve8(A):
    """Gauss-Jordan of the 8x9 system, the kernel's order: the solution [8] or None"""
    a = [[F32(v) for v in row] for row in np.asarray(A, np.float32)]
    with np.errstate(all="ignore"):
        for k in range(8):
            for r in range(k + 1, 8):
                if int(abs_bits(a[r][k])) > int(abs_bits(a[k][k])):
                    a[k], a[r] = a[r], a[k]
            e = int(abs_bits(a[k][k])) >> 23
            if e == 0 or e == 255:
                return None
            inv = F32(1) / a[k][k]
            for j in range(k + 1, 9):
                a[k][j] = a[k][j] * inv
            for r in range(8):
                if r != k:
                    f = a[r][k]
                    for j in range(k + 1, 9):
                        a[r][j] = a[r][j] - f * a[k][j]
    x = np.array([a[r][8] for r in range(8)], np.float32)
    return x if np.isfinite(x).all() else None


def fit(corr, inl):
    """steps 1 - 4 of a round: the published model float32 [9] or None"""
    inl = np.asarray(inl, bool)
    if int(inl.sum()) < 4:
        return None
    xa, ya, xb, yb = (np.ascontiguousarray(corr[:, i], np.float32) for i in range(4))
    ca, cb = condition(xa, ya, inl), condition(xb, yb, inl)
    if ca is None or cb is None:
        return None
    (cxa, cya, sa), (cxb, cyb, sb) = ca, cb
    one = F32(1)
    with np.errstate(all="ignore"):
        x, y, X, Y = (xa - cxa) * sa, (ya - cya) * sa, (xb - cxb) * sb, (yb - cyb) * sb
        h = solve8(system(accumulate(x, y, np.ones_like(x), X, Y, -X, -Y, inl)))
        for _ in range(GAUSS_NEWTON_STEPS):
            if h is None:
                return None
            u = (h[0] * x + h[1] * y) + h[2]
            v = (h[3] * x + h[4] * y) + h[5]
            d = (h[6] * x + h[7] * y) + one
            i = one / d
            a, b, pu, pv = x * i, y * i, u * i, v * i
            delta = solve8(system(accumulate(a, b, i, pu, pv, pu - X, pv - Y, inl)))
            h = None if delta is None else h + delta
        if h is None or not np.isfinite(h).all():
            return None
        assert h.dtype == np.float32
        hc = [h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], one]
        ua, va, isb = sa * cxa, sa * cya, one / sb
        g = []
        for r in range(3):
            g += [hc[3 * r] * sa, hc[3 * r + 1] * sa, (hc[3 * r + 2] - hc[3 * r] * ua) - hc[3 * r + 1] * va]
        H = [g[c] * isb + cxb * g[6 + c] for c in range(3)] + [g[3 + c] * isb + cyb * g[6 + c] for c in range(3)] + g[6:9]
        o = np.array([v / H[8] for v in H], np.float32)
    if not (H[8] != 0 and np.isfinite(o).all()):
        return None
    return o


def score(o, corr, threshold_px):
    """bool [n]: the admissibility of guided matching for the published model, correspondence by correspondence"""
    c = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    M = [F32(v) for v in np.asarray(o, np.float32).reshape(9)]
    xa, ya, xb, yb = (c[:, i] for i in range(4))
    t2 = G.threshold2(threshold_px)
    with np.errstate(all="ignore"):
        u = (M[0] * xa + M[1] * ya) + M[2]
        v = (M[3] * xa + M[4] * ya) + M[5]
        d = (M[6] * xa + M[7] * ya) + M[8]
        ru, rv = u - xb * d, v - yb * d
        e2, lim = ru * ru + rv * rv, (d * d) * t2
        assert e2.dtype == np.float32 and lim.dtype == np.float32
        return (d > 0) & (e2 < lim)


def zero_record(n):
    return dict(H=np.zeros((3, 3), np.float32), nb_matches=0, nb_inliers=0, rounds=0, valid=0, mask=np.zeros(n, np.uint8))


def refit(corr, start, start_mask, nb_rounds, threshold_px, fit_fn=fit, score_fn=score):
    """The estimator for one slot. corr float32 [n, 4] pixels; start: the RANSAC record (H, nb_inliers, valid); start_mask: n bytes.
    Returns dict(H [3, 3], nb_matches, nb_inliers, rounds, valid, mask uint8 [n])."""
    assert 1 <= nb_rounds <= MAX_ROUNDS
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    n = len(corr)
    start_mask = np.asarray(start_mask).astype(np.uint8).reshape(-1)[:n]
    if not int(start["valid"]):
        return zero_record(n)
    kept = dict(H=np.array(start["H"], np.float32).reshape(3, 3), nb_matches=n, nb_inliers=int(start["nb_inliers"]), rounds=0, valid=1, mask=start_mask.copy())
    for r in range(1, nb_rounds + 1):
        o = fit_fn(corr, kept["mask"] == 1)
        if o is None:
            break
        inl = score_fn(o, corr, threshold_px)
        if int(inl.sum()) < kept["nb_inliers"]:
            break
        kept.update(H=np.asarray(o).reshape(3, 3), nb_inliers=int(inl.sum()), rounds=r, mask=inl.astype(np.uint8))
    return kept


# ---- float64 evaluation of the same algorithm (what fp32 is measured against; never compared with the GPU) ------------------------------
def fit_f64(corr, inl):
    c = np.asarray(corr, np.float64)[np.asarray(inl, bool)]
    if len(c) < 4:
        return None
    with np.errstate(all="ignore"):
        ca, cb = c[:, :2].mean(axis=0), c[:, 2:].mean(axis=0)
        ma, mb = np.abs(c[:, :2] - ca).max(), np.abs(c[:, 2:] - cb).max()
        if not (np.isfinite(ma) and np.isfinite(mb) and ma > 0 and mb > 0):
            return None
        sa, sb = 2.0 ** -np.floor(np.log2(ma)), 2.0 ** -np.floor(np.log2(mb))
        x, y, X, Y = (c[:, 0] - ca[0]) * sa, (c[:, 1] - ca[1]) * sa, (c[:, 2] - cb[0]) * sb, (c[:, 3] - cb[1]) * sb

        def step(a, b, i, pu, pv, ru, rv):
            z = np.zeros_like(a)
            J = np.concatenate([np.stack([a, b, i, z, z, z, -pu * a, -pu * b], axis=1), np.stack([z, z, z, a, b, i, -pv * a, -pv * b], axis=1)])
            N, g = J.T @ J, -J.T @ np.concatenate([ru, rv])
            if not (np.isfinite(N).all() and np.isfinite(g).all()) or np.linalg.matrix_rank(N) < 8:
                return None
            return np.linalg.solve(N, g)

        h = step(x, y, np.ones_like(x), X, Y, -X, -Y)
        for _ in range(GAUSS_NEWTON_STEPS):
            if h is None:
                return None
            d = h[6] * x + h[7] * y + 1.0
            pu, pv = (h[0] * x + h[1] * y + h[2]) / d, (h[3] * x + h[4] * y + h[5]) / d
            delta = step(x / d, y / d, 1.0 / d, pu, pv, pu - X, pv - Y)
            h = None if delta is None else h + delta
        if h is None:
            return None
        Ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1.0]])
        Tbi = np.array([[1 / sb, 0, cb[0]], [0, 1 / sb, cb[1]], [0, 0, 1.0]])
        H = Tbi @ np.append(h, 1.0).reshape(3, 3) @ Ta
        o = (H / H[2, 2]).reshape(9)
    return o if H[2, 2] != 0 and np.isfinite(o).all() else None


def score_f64(o, corr, threshold_px):
    import np_verify as V

    return V.inliers_f64(np.asarray(o, np.float64).reshape(1, 9), corr, threshold_px)[0]


def refit_f64(corr, start, start_mask, nb_rounds, threshold_px):
    """the same chain from the same start, float64 arithmetic inside the rounds"""
    return refit(corr, start, start_mask, nb_rounds, threshold_px, fit_fn=fit_f64, score_fn=score_f64)


# ---- the slots of the kernel-level GPU test (tests/test_gpu_refine.py), shared with tests/test_np_refine.py -------------------------------
# the strided-sum boundaries (one element per thread, one more), the tree's (a wave, one more), several rows per thread, and the default
# vksift_getDefaultConfig().max_nb_sift_per_buffer once
SLOT_N = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 1000, 4097, 100000]
SPECIAL = ["invalid start record", "four ones in general position", "four collinear ones", "all ones over half outliers"]
SPECIAL_N = 300
SLOT_ROUNDS = [1, 3, 8]
SLOT_THRESHOLDS = [0.5, 2.5]
START_HYPOTHESES = 64
_SLOTS = {}


def kernel_test_slots(thr):
    """[(correspondences, start record, start mask, (w, h))] of every slot, computed once per threshold and to be left unchanged: planted
    homographies with outliers and noise in images up to 16383 px, start records and masks from np_verify.ransac at the same threshold;
    n = 4, 5 without outliers (so that a model exists); then the four special slots"""
    import np_verify as V
    import quality as Q

    if thr in _SLOTS:
        return _SLOTS[thr]
    out = []
    for i, n in enumerate(SLOT_N):
        w, h = [(640, 480), (16383, 12000), (4000, 3000)][i % 3]
        c, _ = V.synthetic_case(Q.homography(w, h, **Q.WARPS[i % 4]), w, h, n=n, outliers=0.0 if n < 63 else 0.5, noise=0.5, seed=60 + i)
        if n >= 255:
            c[7, 0], c[n - 1, 2] = 16383.0, 16383.0     # the largest coordinate the kernel is specified for
        s = V.ransac(c, START_HYPOTHESES, thr, 9, slot=i)
        out.append((c, s, s["mask"].astype(np.uint8), (w, h)))
    w, h = 16383, 12000
    Ht = Q.homography(w, h, **Q.WARPS[1])
    for j in range(len(SPECIAL)):
        c, true = V.synthetic_case(Ht, w, h, n=SPECIAL_N, outliers=0.5, noise=0.0 if j == 1 else 0.5, seed=90 + j)
        s = V.ransac(c, START_HYPOTHESES, thr, 9, slot=len(SLOT_N) + j)
        assert s["valid"] == 1
        mask = s["mask"].astype(np.uint8)
        if j == 0:
            s = dict(s, H=np.zeros((3, 3), np.float32), nb_inliers=0, best_hypothesis=0, valid=0)       # its mask still holds ones: never read
        elif j in (1, 2):
            four = np.flatnonzero(true)[[0, 11, 23, 57]]
            if j == 2:
                for q, k in enumerate(four):            # four points of one line, on both sides
                    c[k] = (1000.0 + 512.0 * q, 2000.0 + 256.0 * q, 3000.0 + 1024.0 * q, 500.0 + 512.0 * q)
            mask = np.zeros(SPECIAL_N, np.uint8)
            mask[four] = 1
            s = dict(s, nb_inliers=4)
        else:
            mask = np.ones(SPECIAL_N, np.uint8)
        out.append((c, s, mask, (w, h)))
    _SLOTS[thr] = out
    return out
