"""Independent numpy restatement of the locally optimised fundamental-matrix refit of vulkansift_amd/csrc/hip/refine_f.hip (vksift_hip_refit_fundamental,
vksift_ext_refineFundamental), in the manner of tests/np_refine.py: what the kernel must compute, written down a second time. This file is the
specification of the operation order; every value is np.float32 with one rounding per operation, no fused operation anywhere.

  sums       np_refine.block_sum, unchanged: thread t of 256 adds its elements k = t, t + 256, ... in increasing k (an element whose mask byte is
             not 1 adds +0), the butterfly over the 64 lanes of each wave, ((w0 + w1) + w2) + w3 over the four waves.
  round      from a mask with m ones (m < 8: the round fails) and the kept model F (pixels)
    1 conditioning: np_refine.condition per side: x = (xa - cxa) sa, y = (ya - cya) sa, X = (xb - cxb) sb, Y = (yb - cyb) sb.
    2 gauge: Fc = Tb^-T F Ta^-1 of the kept model with isa = 1 / sa, isb = 1 / sb:
        G[r] = (F[r][0] isa, F[r][1] isa, (F[r][0] cxa + F[r][1] cya) + F[r][2]);
        Fc[0] = G[0] isb, Fc[1] = G[1] isb, Fc[2] = (cxb G[0] + cyb G[1]) + G[2], column by column;
      j = the index of the largest |entry| of Fc by bit pattern, ties to the lowest index; f_j = 1 for the whole round. Per match the nine
      monomials a = (X x, X y, X, Y x, Y y, Y, x, y, 1); b = a with monomial j moved to the last place (b_i = a_i for i < j, a_(i+1) for
      j <= i < 8, b_8 = a_j).
    3 one accumulation: with wb_i = w b_i the 44 sums wb_i b_k (i = 0 .. 7, k = i .. 7, i outermost) and wb_i b_8 (i = 0 .. 7); the 8x9 system
      has the first 36 as its symmetric matrix and minus the last 8 as its right-hand side; np_refine.solve8 solves it; the solution is the
      eight free entries of Fc.
        linear start:      w = 1
        reweighted step:   Fc = the previous solution with 1 at j; l0 = (Fc0 x + Fc1 y) + Fc2, l1 = (Fc3 x + Fc4 y) + Fc5,
                           m0 = (Fc0 X + Fc3 Y) + Fc6, m1 = (Fc1 X + Fc4 Y) + Fc7; g = rho (l0 l0 + l1 l1) + (m0 m0 + m1 m1) with
                           rho = (sb / sa) (sb / sa), the Sampson denominator in pixels up to the common factor sa^2; w = 1 / g.
                           g zero, subnormal or not finite on a marked match: the round fails.
      REWEIGHTED_STEPS = 2 of them.
    4 rank 2: two steps F <- F - (det / |C|^2) C with the cofactors C00 = F4 F8 - F5 F7, C01 = F5 F6 - F3 F8, C02 = F3 F7 - F4 F6,
      C10 = F2 F7 - F1 F8, C11 = F0 F8 - F2 F6, C12 = F1 F6 - F0 F7, C20 = F1 F5 - F2 F4, C21 = F2 F3 - F0 F5, C22 = F0 F4 - F1 F3,
      det = (F0 C00 + F1 C01) + F2 C02, |C|^2 = the squares added in index order from C00 C00; |C|^2 zero, subnormal or not finite: the round fails.
    5 back to pixels, as np_verify_f.solve: ua = sa cxa, va = sa cya, ub = sb cxb, vb = sb cyb;
      G[r] = (Fc[r][0] sa, Fc[r][1] sa, (Fc[r][2] - Fc[r][0] ua) - Fc[r][1] va); F[0] = sb G[0], F[1] = sb G[1], F[2] = (G[2] - ub G[0]) - vb G[1];
      times the power of two that brings the largest |entry| into [1, 2); no such power (all zero, subnormal, not finite): the round fails.
    6 re-scoring of all n correspondences in pixels: np_guided.admissible(FUNDAMENTAL) with np_guided.threshold2(threshold_px).
  chain      np_refine.refit's, word for word: kept = the RANSAC record (F, nb_inliers, mask), rounds = 0; round r starts from the kept mask AND
             the kept model; accepted iff it did not fail and its count >= the kept count; the first round not accepted ends the loop. An
             invalid start record: an all-zero record and mask.

Not attempted: no chirality test, no handling of the planar degeneracy (coplanar inliers give a near-singular system; whatever comes out is
subject to the acceptance rule like any other model).

The same estimator exists in float64 (fit_f64; numpy sums, numpy.linalg.solve, an SVD truncation for the rank) for the tests that ask what fp32
costs. Also the synthetic slots of the kernel-level GPU test, shared with the CPU tests."""
import numpy as np

import np_guided as G
import np_refine as R
import np_verify_f as VF

F32 = np.float32
REWEIGHTED_STEPS = 2
PROJECTION_STEPS = 2
MIN_MATCHES = 8
MAX_ROUNDS = 8
N_SUMS = 44


def gauge(F, ca, cb):
    """the kept model in the conditioned frame, float32 [9], and the index of its largest |entry|"""
    (cxa, cya, sa), (cxb, cyb, sb) = ca, cb
    F = [F32(v) for v in np.asarray(F, np.float32).reshape(9)]
    with np.errstate(all="ignore"):
        isa, isb = F32(1) / sa, F32(1) / sb
        g = []
        for r in range(3):
            g += [F[3 * r] * isa, F[3 * r + 1] * isa, (F[3 * r] * cxa + F[3 * r + 1] * cya) + F[3 * r + 2]]
        fc = [g[c] * isb for c in range(3)] + [g[3 + c] * isb for c in range(3)] + [(cxb * g[c] + cyb * g[3 + c]) + g[6 + c] for c in range(3)]
    fc = np.array(fc, np.float32)
    return fc, int(np.argmax(R.abs_bits(fc)))          # argmax: the first of equal maxima


def monomials(x, y, X, Y, j):
    a = [X * x, X * y, X, Y * x, Y * y, Y, x, y, np.ones_like(x)]
    return a[:j] + a[j + 1:] + [a[j]]


def accumulate(b, w, inl, sum_fn=None):
    """the 44 sums of one step"""
    with np.errstate(all="ignore"):
        wb = [w * b[i] for i in range(8)]
        terms = [wb[i] * b[k] for i in range(8) for k in range(i, 8)] + [wb[i] * b[8] for i in range(8)]
        assert all(t.dtype == np.float32 for t in terms) and len(terms) == N_SUMS
        return (sum_fn or R.block_sum)(np.stack([np.where(inl, t, F32(0)) for t in terms]))


def system(S):
    A = np.zeros((8, 9), np.float32)
    q = 0
    for i in range(8):
        for k in range(i, 8):
            A[i, k] = A[k, i] = S[q]
            q += 1
    for i in range(8):
        A[i, 8] = -S[36 + i]
    return A


def with_one(f, j):
    return list(f[:j]) + [F32(1)] + list(f[j:])


def weights(fc, x, y, X, Y, rho, inl):
    """1 / g per match, or None where g is zero, subnormal or not finite on a marked match"""
    with np.errstate(all="ignore"):
        l0 = (fc[0] * x + fc[1] * y) + fc[2]
        l1 = (fc[3] * x + fc[4] * y) + fc[5]
        m0 = (fc[0] * X + fc[3] * Y) + fc[6]
        m1 = (fc[1] * X + fc[4] * Y) + fc[7]
        g = rho * (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
        assert g.dtype == np.float32
        e = R.abs_bits(g) >> np.uint32(23)
        if (((e == 0) | (e == 255)) & inl).any():
            return None
        return F32(1) / g


def project_rank2(F):
    """PROJECTION_STEPS Newton steps on det along its gradient: float32 [9] or None"""
    F = [F32(v) for v in F]
    with np.errstate(all="ignore"):
        for _ in range(PROJECTION_STEPS):
            C = [F[4] * F[8] - F[5] * F[7], F[5] * F[6] - F[3] * F[8], F[3] * F[7] - F[4] * F[6],
                 F[2] * F[7] - F[1] * F[8], F[0] * F[8] - F[2] * F[6], F[1] * F[6] - F[0] * F[7],
                 F[1] * F[5] - F[2] * F[4], F[2] * F[3] - F[0] * F[5], F[0] * F[4] - F[1] * F[3]]
            det = (F[0] * C[0] + F[1] * C[1]) + F[2] * C[2]
            nrm = C[0] * C[0]
            for i in range(1, 9):
                nrm = nrm + C[i] * C[i]
            e = int(R.abs_bits(nrm)) >> 23
            if e == 0 or e == 255:
                return None
            t = det / nrm
            F = [F[i] - t * C[i] for i in range(9)]
    return np.array(F, np.float32)


def to_pixels(fc, ca, cb):
    """step 5: the published model float32 [9] or None"""
    (cxa, cya, sa), (cxb, cyb, sb) = ca, cb
    with np.errstate(all="ignore"):
        ua, va, ub, vb = sa * cxa, sa * cya, sb * cxb, sb * cyb
        g = []
        for r in range(3):
            g += [fc[3 * r] * sa, fc[3 * r + 1] * sa, (fc[3 * r + 2] - fc[3 * r] * ua) - fc[3 * r + 1] * va]
        F = [sb * g[c] for c in range(3)] + [sb * g[3 + c] for c in range(3)] + [(g[6 + c] - ub * g[c]) - vb * g[3 + c] for c in range(3)]
        F = np.array(F, np.float32)
        f, ok = R.unit_scale(R.abs_bits(F).max())
        return F * f if ok else None


def fit(corr, inl, model, sum_fn=None, detail=None):
    """steps 1 - 5 of a round: the published model float32 [9] or None. detail: a dict that receives the conditioned model after the projection"""
    inl = np.asarray(inl, bool)
    if int(inl.sum()) < MIN_MATCHES:
        return None
    xa, ya, xb, yb = (np.ascontiguousarray(corr[:, i], np.float32) for i in range(4))
    ca, cb = R.condition(xa, ya, inl), R.condition(xb, yb, inl)
    if ca is None or cb is None:
        return None
    (cxa, cya, sa), (cxb, cyb, sb) = ca, cb
    _, j = gauge(model, ca, cb)
    with np.errstate(all="ignore"):
        x, y, X, Y = (xa - cxa) * sa, (ya - cya) * sa, (xb - cxb) * sb, (yb - cyb) * sb
        rho = (sb / sa) * (sb / sa)
        b = monomials(x, y, X, Y, j)
        f = R.solve8(system(accumulate(b, np.ones_like(x), inl, sum_fn)))
        for _ in range(REWEIGHTED_STEPS):
            if f is None:
                return None
            w = weights(with_one(f, j), x, y, X, Y, rho, inl)
            if w is None:
                return None
            f = R.solve8(system(accumulate(b, w, inl, sum_fn)))
        if f is None:
            return None
        fc = project_rank2(with_one(f, j))
    if fc is None:
        return None
    if detail is not None:
        detail.update(fc=fc, j=j)
    return to_pixels(fc, ca, cb)


def score(o, corr, threshold_px):
    """bool [n]: the admissibility of guided matching for the published model, correspondence by correspondence"""
    c = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    M = [F32(v) for v in np.asarray(o, np.float32).reshape(9)]
    xa, ya, xb, yb = (c[:, i] for i in range(4))
    t2 = G.threshold2(threshold_px)
    with np.errstate(all="ignore"):
        l0 = (M[0] * xa + M[1] * ya) + M[2]
        l1 = (M[3] * xa + M[4] * ya) + M[5]
        l2 = (M[6] * xa + M[7] * ya) + M[8]
        r = (xb * l0 + yb * l1) + l2
        m0 = (M[0] * xb + M[3] * yb) + M[6]
        m1 = (M[1] * xb + M[4] * yb) + M[7]
        g = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
        lhs, rhs = r * r, t2 * g
        assert lhs.dtype == np.float32 and rhs.dtype == np.float32
        return lhs < rhs


def zero_record(n):
    return dict(F=np.zeros((3, 3), np.float32), nb_matches=0, nb_inliers=0, rounds=0, valid=0, mask=np.zeros(n, np.uint8))


def refit(corr, start, start_mask, nb_rounds, threshold_px, fit_fn=fit, score_fn=score):
    """The estimator for one slot. corr float32 [n, 4] pixels; start: the RANSAC record (F, nb_inliers, valid); start_mask: n bytes.
    Returns dict(F [3, 3], nb_matches, nb_inliers, rounds, valid, mask uint8 [n])."""
    assert 1 <= nb_rounds <= MAX_ROUNDS
    corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 4)
    n = len(corr)
    start_mask = np.asarray(start_mask).astype(np.uint8).reshape(-1)[:n]
    if not int(start["valid"]):
        return zero_record(n)
    kept = dict(F=np.array(start["F"], np.float32).reshape(3, 3), nb_matches=n, nb_inliers=int(start["nb_inliers"]), rounds=0, valid=1, mask=start_mask.copy())
    for r in range(1, nb_rounds + 1):
        o = fit_fn(corr, kept["mask"] == 1, kept["F"])
        if o is None:
            break
        inl = score_fn(o, corr, threshold_px)
        if int(inl.sum()) < kept["nb_inliers"]:
            break
        kept.update(F=np.asarray(o).reshape(3, 3), nb_inliers=int(inl.sum()), rounds=r, mask=inl.astype(np.uint8))
    return kept


# ---- float64 evaluation of the same estimator (what fp32 is measured against; never compared with the GPU) -------------------------------
def fit_f64(corr, inl, model):
    c = np.asarray(corr, np.float64)[np.asarray(inl, bool)]
    if len(c) < MIN_MATCHES:
        return None
    with np.errstate(all="ignore"):
        ca, cb = c[:, :2].mean(axis=0), c[:, 2:].mean(axis=0)
        ma, mb = np.abs(c[:, :2] - ca).max(), np.abs(c[:, 2:] - cb).max()
        if not (np.isfinite(ma) and np.isfinite(mb) and ma > 0 and mb > 0):
            return None
        sa, sb = 2.0 ** -np.floor(np.log2(ma)), 2.0 ** -np.floor(np.log2(mb))
        Ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1.0]])
        Tb = np.array([[sb, 0, -sb * cb[0]], [0, sb, -sb * cb[1]], [0, 0, 1.0]])
        x, y, X, Y = (c[:, 0] - ca[0]) * sa, (c[:, 1] - ca[1]) * sa, (c[:, 2] - cb[0]) * sb, (c[:, 3] - cb[1]) * sb
        Fc0 = np.linalg.inv(Tb).T @ np.asarray(model, np.float64).reshape(3, 3) @ np.linalg.inv(Ta)
        j = int(np.argmax(np.abs(Fc0).reshape(9)))
        a = np.stack([X * x, X * y, X, Y * x, Y * y, Y, x, y, np.ones_like(x)], axis=1)
        free = [i for i in range(9) if i != j]
        rho = (sb / sa) ** 2

        def step(w):
            A = a[:, free] * np.sqrt(w)[:, None]
            N, g = A.T @ A, -(A.T @ (a[:, j] * np.sqrt(w)))
            if not (np.isfinite(N).all() and np.isfinite(g).all()) or np.linalg.matrix_rank(N) < 8:
                return None
            f = np.empty(9)
            f[free], f[j] = np.linalg.solve(N, g), 1.0
            return f

        f = step(np.ones(len(c)))
        for _ in range(REWEIGHTED_STEPS):
            if f is None:
                return None
            g = rho * (((f[0] * x + f[1] * y) + f[2]) ** 2 + ((f[3] * x + f[4] * y) + f[5]) ** 2) + (((f[0] * X + f[3] * Y) + f[6]) ** 2 + ((f[1] * X + f[4] * Y) + f[7]) ** 2)
            if not (np.isfinite(g).all() and (g > 0).all()):
                return None
            f = step(1.0 / g)
        if f is None:
            return None
        u, s, vt = np.linalg.svd(f.reshape(3, 3))
        Fp = Tb.T @ (u @ np.diag([s[0], s[1], 0.0]) @ vt) @ Ta
        m = np.abs(Fp).max()
        if not (np.isfinite(Fp).all() and m > 0):
            return None
        return (Fp * 2.0 ** -np.floor(np.log2(m))).reshape(9)


def score_f64(o, corr, threshold_px):
    return VF.sampson_inliers_f64(np.asarray(o, np.float64).reshape(3, 3), corr, threshold_px)


def refit_f64(corr, start, start_mask, nb_rounds, threshold_px):
    """the same chain from the same start, float64 arithmetic inside the rounds"""
    return refit(corr, start, start_mask, nb_rounds, threshold_px, fit_fn=fit_f64, score_fn=score_f64)


def rms_sampson(F, clean):
    """RMS Sampson distance (px, float64) of the noise-free true correspondences `clean` [k, 4] under F"""
    c = np.asarray(clean, np.float64).reshape(-1, 4)
    F = np.asarray(F, np.float64).reshape(3, 3)
    pa, pb = np.stack([c[:, 0], c[:, 1], np.ones(len(c))]), np.stack([c[:, 2], c[:, 3], np.ones(len(c))])
    l, m = F @ pa, F.T @ pb
    r = (pb * l).sum(axis=0)
    return float(np.sqrt(np.mean(r * r / (l[0] ** 2 + l[1] ** 2 + m[0] ** 2 + m[1] ** 2))))


def noisy_and_clean(n, outliers, noise, seed, w, h):
    """np_verify_f.two_view_case twice from one seed: (the noisy correspondences, is_true, F_true, the same correspondences without the noise)"""
    c, true, Ft = VF.two_view_case(n, outliers, noise, seed, w, h)
    clean, true0, _ = VF.two_view_case(n, outliers, 0.0, seed, w, h)
    assert np.array_equal(true, true0) and np.array_equal(c[:, :2], clean[:, :2])
    return c, true, Ft, clean


# ---- the slots of the kernel-level GPU test (tests/test_gpu_refine_f.py), shared with tests/test_np_refine_f.py -----------------------------
# below, at and above the minimum, the wave, and one, two and many trips of the strided loop
SLOT_N = [0, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4097]
SLOT_SIZES = [(640, 480), (4000, 3000)]
BIG_SLOT = 9        # this slot lies in a 16383 px image and holds the coordinate 16383.0
SPECIAL = ["all ones over half outliers", "exactly eight ones", "seven ones", "invalid start record"]
SPECIAL_N = 300
SLOT_ROUNDS = [1, 3, 8]
SLOT_THRESHOLDS = [0.5, 2.5]
START_HYPOTHESES = 512
_SLOTS = {}


def kernel_test_slots(thr):
    """[(correspondences, start record, start mask, (w, h), noise-free true correspondences)] of every slot, computed once per threshold and to be
    left unchanged: two views with 50 % outliers and 0.5 px noise (n <= 9: exact projections without outliers, so that a model with 8 inliers
    exists), start records and masks from np_verify_f.ransac at the same threshold; then the four special slots"""
    if thr in _SLOTS:
        return _SLOTS[thr]
    out = []
    for i, n in enumerate(SLOT_N):
        w, h = (16383, 12000) if i == BIG_SLOT else SLOT_SIZES[i % 2]
        small = n <= 9
        c, true, _, clean = noisy_and_clean(n, 0.0 if small else 0.5, 0.0 if small else 0.5, 170 + i, w, h)
        if i == BIG_SLOT:
            c[1, 0], c[n - 1, 2] = 16383.0, 16383.0       # the largest coordinate the kernel is specified for
        s = VF.ransac(c, START_HYPOTHESES, thr, 9, slot=i)
        out.append((c, s, s["mask"].astype(np.uint8), (w, h), clean[true]))
    w, h = 4000, 3000
    for q in range(len(SPECIAL)):
        c, true, _, clean = noisy_and_clean(SPECIAL_N, 0.5, 0.5, 190 + q, w, h)
        s = VF.ransac(c, START_HYPOTHESES, thr, 9, slot=len(SLOT_N) + q)
        assert s["valid"] == 1
        mask = s["mask"].astype(np.uint8)
        if q == 0:
            mask = np.ones(SPECIAL_N, np.uint8)
        elif q in (1, 2):
            few = np.flatnonzero(true)[[0, 11, 23, 37, 57, 71, 90, 101][:9 - q]]
            mask = np.zeros(SPECIAL_N, np.uint8)
            mask[few] = 1
            s = dict(s, nb_inliers=9 - q)
        else:
            s = dict(s, F=np.zeros((3, 3), np.float32), nb_inliers=0, best_hypothesis=0, best_root=0, valid=0)     # its mask still holds ones: never read
        out.append((c, s, mask, (w, h), clean[true]))
    _SLOTS[thr] = out
    return out
