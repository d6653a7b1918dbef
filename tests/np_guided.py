"""Independent numpy restatement of guided matching (vulkansift_amd/csrc/hip/guided.hip, vksift_hip_match_guided, vksift_ext_matchFeaturesGuided), in
the manner of tests/np_verify.py and tests/np_verify_f.py: what the kernels must compute, written down a second time.

  threshold   t2 = np_verify.threshold2(threshold_px) * 2^26: the verification's (t 2^-13)^2 brought back to pixels by an exact power of two (the test
              here runs on unscaled pixel coordinates with the published model), i.e. fp32 t * t.
  admissible  homography: u, v, d = M (xa, ya, 1); ru = u - xb d, rv = v - yb d; d > 0 and ru ru + rv rv < (d d) t2.
              fundamental: l = M (xa, ya, 1); r = (xb l0 + yb l1) + l2; m0 = (M0 xb + M3 yb) + M6, m1 = (M1 xb + M4 yb) + M7;
              r r < t2 ((l0 l0 + l1 l1) + (m0 m0 + m1 m1)). np.float32 throughout, one rounding per operation, the order written; a NaN fails.
              Both directions use the same relation on the ordered pair (a, b).
  records     key = d2 << 32 | index over the admissible candidates, d2 the exact integer squared descriptor distance; k1, k2 the two smallest (ties to
              the lowest index); dist = sqrt(float32(d2)), +inf where there is no second candidate.
  kept        (a, idx(k1(a))) iff dist1 <= max_distance, dist1 / dist2 < ratio (fp32 division: true for x / inf, false for 0 / 0) and, with cross_check,
              idx(k1_rev(b)) == a and the reverse record passes its own ratio test. Records {idx_a, idx_b, dist1, dist2} in increasing idx_a; a slot whose
              model is not valid has none.

Also the synthetic slots of the kernel-level GPU test, shared with the CPU tests."""
import numpy as np

import np_verify as V
import np_verify_f as VF

F32 = np.float32
HOMOGRAPHY, FUNDAMENTAL = 0, 1
NONE = np.int64(2 ** 63 - 1)
RECORD_DTYPE = np.dtype([("idx_a", "<u4"), ("idx_b", "<u4"), ("dist_a_b1", "<f4"), ("dist_a_b2", "<f4")])


def threshold2(threshold_px):
    return F32(V.threshold2(threshold_px) * F32(67108864.0))


def admissible(kind, M, xa, ya, xb, yb, t2):
    """bool [na, nb]: the relation on every ordered pair (a, b)"""
    M = [F32(v) for v in np.asarray(M, np.float32).reshape(9)]
    xa, ya = np.asarray(xa, np.float32).reshape(-1, 1), np.asarray(ya, np.float32).reshape(-1, 1)
    xb, yb = np.asarray(xb, np.float32).reshape(1, -1), np.asarray(yb, np.float32).reshape(1, -1)
    t2 = F32(t2)
    with np.errstate(all="ignore"):
        r0 = (M[0] * xa + M[1] * ya) + M[2]
        r1 = (M[3] * xa + M[4] * ya) + M[5]
        r2 = (M[6] * xa + M[7] * ya) + M[8]
        if kind == HOMOGRAPHY:
            ru, rv = r0 - xb * r2, r1 - yb * r2
            e2 = ru * ru + rv * rv
            lim = (r2 * r2) * t2
            assert e2.dtype == np.float32 and lim.dtype == np.float32
            return (r2 > 0) & (e2 < lim)
        assert kind == FUNDAMENTAL
        r = (xb * r0 + yb * r1) + r2
        m0 = (M[0] * xb + M[3] * yb) + M[6]
        m1 = (M[1] * xb + M[4] * yb) + M[7]
        g = (r0 * r0 + r1 * r1) + (m0 * m0 + m1 * m1)
        lhs, rhs = r * r, t2 * g
        assert lhs.dtype == np.float32 and rhs.dtype == np.float32
        return lhs < rhs


def distances2(desc_a, desc_b):
    """exact integer squared distances int64 [na, nb] (float64 products of bytes are exact)"""
    a, b = np.asarray(desc_a, np.float64).reshape(-1, 128), np.asarray(desc_b, np.float64).reshape(-1, 128)
    return ((a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2.0 * (a @ b.T)).astype(np.int64)


def top2(d2, adm):
    """per row of d2 [n, m] the two smallest keys over adm: (k1, k2) int64 [n], NONE where absent"""
    n, m = d2.shape
    keys = np.full((n, m + 2), NONE, np.int64)
    keys[:, :m] = np.where(adm, (d2 << 32) | np.arange(m, dtype=np.int64)[None, :], NONE)
    keys.partition((0, 1), axis=1)
    return keys[:, 0].copy(), keys[:, 1].copy()


def key_dist(k):
    k = np.asarray(k, np.int64)
    with np.errstate(all="ignore"):
        return np.where(k == NONE, F32(np.inf), np.sqrt((k >> 32).astype(np.float32))).astype(np.float32)


def key_index(k):
    return (np.asarray(k, np.int64) & 0xFFFFFFFF).astype(np.int64)


def decide(fwd, rev, ratio, max_distance, cross_check):
    """fwd = (k1, k2) per a, rev = (k1, k2) per b -> records"""
    k1, k2 = fwd
    d1, d2 = key_dist(k1), key_dist(k2)
    with np.errstate(all="ignore"):
        keep = (k1 != NONE) & (d1 <= F32(max_distance)) & ((d1 / d2) < F32(ratio))
        b = np.where(k1 != NONE, key_index(k1), 0)
        if cross_check:
            r1, r2 = rev[0][b] if len(rev[0]) else np.full(len(b), NONE), rev[1][b] if len(rev[1]) else np.full(len(b), NONE)
            keep &= (r1 != NONE) & (key_index(r1) == np.arange(len(k1))) & ((key_dist(r1) / key_dist(r2)) < F32(ratio))
    out = np.zeros(int(keep.sum()), RECORD_DTYPE)
    out["idx_a"], out["idx_b"], out["dist_a_b1"], out["dist_a_b2"] = np.flatnonzero(keep), b[keep], d1[keep], d2[keep]
    return out


def sweep(kind, M, xa, ya, desc_a, xb, yb, desc_b, threshold_px, d2=None):
    """what does not depend on ratio, max_distance and cross_check: (forward keys, reverse keys, admissible)"""
    adm = admissible(kind, M, xa, ya, xb, yb, threshold2(threshold_px))
    if d2 is None:
        d2 = distances2(desc_a, desc_b)
    return top2(d2, adm), top2(d2.T, adm.T), adm


def guided(kind, M, valid, xa, ya, desc_a, xb, yb, desc_b, threshold_px, ratio, max_distance, cross_check, swept=None):
    if not valid:
        return np.zeros(0, RECORD_DTYPE)
    fwd, rev, _ = swept if swept is not None else sweep(kind, M, xa, ya, desc_a, xb, yb, desc_b, threshold_px)
    return decide(fwd, rev, ratio, max_distance, cross_check)


# ---- the straightforward loop (tests/test_np_guided.py holds the vectorised form against it) ---------------------------------------------
def guided_scalar(kind, M, xa, ya, desc_a, xb, yb, desc_b, threshold_px, ratio, max_distance, cross_check):
    M = [F32(v) for v in np.asarray(M, np.float32).reshape(9)]
    t2 = threshold2(threshold_px)
    na, nb = len(xa), len(xb)

    def adm(a, b):
        x, y, p, q = F32(xa[a]), F32(ya[a]), F32(xb[b]), F32(yb[b])
        with np.errstate(all="ignore"):
            r0, r1, r2 = (M[0] * x + M[1] * y) + M[2], (M[3] * x + M[4] * y) + M[5], (M[6] * x + M[7] * y) + M[8]
            if kind == HOMOGRAPHY:
                ru, rv = r0 - p * r2, r1 - q * r2
                return bool(r2 > 0 and ru * ru + rv * rv < (r2 * r2) * t2)
            r = (p * r0 + q * r1) + r2
            m0, m1 = (M[0] * p + M[3] * q) + M[6], (M[1] * p + M[4] * q) + M[7]
            return bool(r * r < t2 * ((r0 * r0 + r1 * r1) + (m0 * m0 + m1 * m1)))

    def dist2(a, b):
        d = desc_a[a].astype(np.int64) - desc_b[b].astype(np.int64)
        return int((d * d).sum())

    A = [[adm(a, b) for b in range(nb)] for a in range(na)]
    D = [[dist2(a, b) for b in range(nb)] for a in range(na)]

    def record(cands):                                  # [(d2, index)] -> (index, dist1, dist2) or None
        if not cands:
            return None
        c = sorted(cands)
        return c[0][1], np.sqrt(F32(c[0][0])), np.sqrt(F32(c[1][0])) if len(c) > 1 else F32(np.inf)

    def ratio_ok(rec):
        with np.errstate(all="ignore"):
            return bool(rec[1] / rec[2] < F32(ratio))

    fwd = [record([(D[a][b], b) for b in range(nb) if A[a][b]]) for a in range(na)]
    rev = [record([(D[a][b], a) for a in range(na) if A[a][b]]) for b in range(nb)]
    out = []
    for a in range(na):
        f = fwd[a]
        if f is None or not (f[1] <= F32(max_distance)) or not ratio_ok(f):
            continue
        if cross_check and not (rev[f[0]] is not None and rev[f[0]][0] == a and ratio_ok(rev[f[0]])):
            continue
        out.append((a, f[0], f[1], f[2]))
    return np.array(out, RECORD_DTYPE).reshape(-1)


# ---- synthetic slots -----------------------------------------------------------------------------------------------------------------------
def _descriptors(rng, n):
    """SIFT-like rows: min(255, trunc(512 |g| / ||g||)), g ~ N(0, 1)^128"""
    g = np.abs(rng.normal(size=(n, 128)))
    return np.minimum(255, np.floor(512.0 * g / np.linalg.norm(g, axis=1, keepdims=True))).astype(np.uint8)


def _noisy(rng, d, amp):
    return np.clip(d.astype(np.int64) + rng.integers(-amp, amp + 1, d.shape), 0, 255).astype(np.uint8)


def unit_f(F):
    """float64 3x3 -> float32 [9] scaled by the power of two that brings its largest |entry| into [1, 2)"""
    F = np.asarray(F, np.float64)
    return (F * 2.0 ** -np.floor(np.log2(np.abs(F).max()))).astype(np.float32).reshape(9)


def fit_affine(c):
    """least-squares affine map of the correspondences [n, 4] as a homography, float32 [9] (the identity below three points)"""
    if len(c) < 3:
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    A = np.stack([c[:, 0], c[:, 1], np.ones(len(c))], axis=1).astype(np.float64)
    px, py = np.linalg.lstsq(A, c[:, 2].astype(np.float64), rcond=None)[0], np.linalg.lstsq(A, c[:, 3].astype(np.float64), rcond=None)[0]
    return np.array([px[0], px[1], px[2], py[0], py[1], py[2], 0, 0, 1], np.float32)


def slot_case(na, nb, seed, w=640, h=480, repeat=4, planar=False, dups=True, amp=3):
    """One pair: np_verify_f.two_view_case geometry for the features both images hold (planar: a homography of the plane instead), groups of `repeat` of
    them sharing one descriptor up to noise (repeated structure), for every seventh a second feature of B a quarter pixel beside the first with the SAME
    descriptor (a distance tie between two admissible candidates), distractors with random positions — a third of them look-alikes of a common descriptor —,
    all shuffled (dups=False: no such second features; amp: the descriptor noise). Returns a dict: xa, ya, desc_a, xb, yb, desc_b, truth (index in B of the true match of a, -1: none), F, H (float32 [9])."""
    rng = np.random.default_rng(seed)
    nc = (2 * min(na, nb)) // 3
    c, _, F_true = VF.two_view_case(max(nc, 8), 0.0, 0.3, seed, w, h)
    if planar:
        Ht = np.array([[0.98, 0.05, 12.0], [-0.04, 1.02, -7.0], [2e-5, -1e-5, 1.0]])
        q = Ht @ np.stack([c[:, 0], c[:, 1], np.ones(len(c))]).astype(np.float64)
        c[:, 2], c[:, 3] = (q[0] / q[2] + rng.normal(0, 0.3, len(c))).astype(np.float32), (q[1] / q[2] + rng.normal(0, 0.3, len(c))).astype(np.float32)
    H = Ht.astype(np.float32).reshape(9) if planar else fit_affine(c)
    c = c[:nc]
    base = _descriptors(rng, nc // repeat + 1)[np.arange(nc) // repeat]
    da_c, db_c = _noisy(rng, base, amp), _noisy(rng, base, amp)
    ndup = min(nc // 7, nb - nc) if dups else 0
    dup = np.arange(ndup) * 7
    n_da, n_db = na - nc, nb - nc - ndup

    def distract(n):
        d = _descriptors(rng, n)
        if nc:
            look = rng.random(n) < 1.0 / 3.0
            d[look] = _noisy(rng, base[rng.integers(0, nc, int(look.sum()))], amp)
        return rng.uniform(0, w - 1, n).astype(np.float32), rng.uniform(0, h - 1, n).astype(np.float32), d

    xda, yda, dda = distract(n_da)
    xdb, ydb, ddb = distract(n_db)
    xa, ya, desc_a = np.concatenate([c[:, 0], xda]), np.concatenate([c[:, 1], yda]), np.concatenate([da_c, dda])
    xb = np.concatenate([c[:, 2], c[dup, 2] + F32(0.25), xdb])
    yb = np.concatenate([c[:, 3], c[dup, 3], ydb])
    desc_b = np.concatenate([db_c, db_c[dup], ddb])
    truth = np.concatenate([np.arange(nc), np.full(n_da, -1)])
    pa, pb = rng.permutation(na), rng.permutation(nb)
    inv_b = np.empty(nb, np.int64)
    inv_b[pb] = np.arange(nb)
    truth = truth[pa]
    truth = np.where(truth >= 0, inv_b[np.maximum(truth, 0)], -1) if nb else np.full(na, -1)
    return dict(xa=xa[pa].astype(np.float32), ya=ya[pa].astype(np.float32), desc_a=np.ascontiguousarray(desc_a[pa]), xb=xb[pb].astype(np.float32),
                yb=yb[pb].astype(np.float32), desc_b=np.ascontiguousarray(desc_b[pb]), truth=truth, F=unit_f(F_true), H=H)


# (N_A, N_B) of the kernel-level GPU test: every size of {0, 1, 2, 63, 64, 65, 255, 256, 257, 700} on either side — below / at / above the wave, the
# chunk and the tile boundaries, more than one tile per side, one workgroup that drains its queue many times (257 x 700 at the widest threshold)
SLOT_SIZES = [(0, 5), (5, 0), (1, 1), (2, 2), (1, 63), (63, 64), (64, 65), (65, 63), (255, 256), (256, 255), (257, 700), (700, 257), (256, 2), (300, 300), (300, 300)]
BIG_SLOT = 13       # this slot lies in a 16383 px image and holds the coordinate 16383.0
INVALID_SLOT = 14   # its model is marked not valid


def kernel_test_slots():
    out = []
    for i, (na, nb) in enumerate(SLOT_SIZES):
        big = i == BIG_SLOT
        s = slot_case(na, nb, 900 + i, *((16383, 12000) if big else (640, 480)), planar=i % 2 == 1)   # a plane in every other slot: a homography that admits
        if big:
            s["xa"][1], s["xb"][nb - 1] = 16383.0, 16383.0
        s["valid"] = 0 if i == INVALID_SLOT else 1
        out.append(s)
    return out
