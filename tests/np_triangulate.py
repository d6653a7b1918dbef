"""Independent numpy restatement of the triangulation of vulkansift_amd/csrc/hip/triangulate.hip (vksift_hip_triangulate_tracks,
vksift_ext_triangulateTracks), in the manner of tests/np_refine.py: what the kernel must compute, written down a second time. This file is the
specification of the operation order; every value is np.float32 with one rounding per operation, no fused operation anywhere. "unusable" means zero,
subnormal or not finite (by exponent bits).

  per selected track m with members i = 0 .. n-1 in table order (offsets[m] .. offsets[m+1]; an extent that decreases or ends beyond the table's
  observation count: DEGENERATE with nb_observations 0); n > 1024: TOO_LONG; n < 2: DEGENERATE; a member whose gpu_buffer_id has no camera: DEGENERATE
  sums       every sum over members has one order: lane j of G = 16 adds its members j, j + 16, ... in increasing order to a partial sum that starts
             at +0 (a missing member adds +0, which changes no bit: such a partial sum is never -0); then the butterfly p[l] = p[l] + p[l ^ off],
             off = 8, 4, 2, 1 (addition commutes: every lane holds the same bits). Minima and maxima are taken on integer keys (any order).
  1 bearing  rows m1, m2, m3 of P's left 3x3 block; a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); b = (x (m2 x m3) + y (m3 x m1)) + (m1 x m2)
             per component; q = (b0 b0 + b1 b1) + b2 b2; s = 1 / sqrt(q); b = b s; q or s unusable: DEGENERATE.
             min_cos = min over i < j of (bi0 bj0 + bi1 bj1) + bi2 bj2 by the key that orders floats as integers (-0 below +0)
  2 start    per member the rows e = t P3 - Pr for (t, r) = (x, 1), (y, 2): q = (e0 e0 + e1 e1) + e2 e2, s = 1 / sqrt(q), p = (e0 s, e1 s, e2 s), pr = e3 s
             (q or s unusable: DEGENERATE); the nine sums S00 S01 S02 S11 S12 S22 r0 r1 r2 of (pa pb + qa qb) and (pa pr + qa qr) over the members' row
             pairs (p | pr), (q | qr); S X = -r by Gauss-Jordan: for column k the rows below compared with row k in turn and exchanged when their |entry|
             (bit pattern) is strictly larger; an unusable pivot fails; row k times 1 / pivot; every other row r minus a[r][k] times row k; a solution
             entry that is not finite fails: DEGENERATE
  3 steps    at X per member u = ((P0 X + P1 Y) + P2 Z) + P3, v and w alike; pu = u / w, pv = v / w, ru = pu - x, rv = pv - y, e2 = ru ru + rv rv,
             iw = 1 / w, ju[c] = (P1[c] - pu P3[c]) iw, jv[c] = (P2[c] - pv P3[c]) iw; cost = sum of e2; the nine sums of the row pairs (ju | ru),
             (jv | rv); N d = -g as in 2. GAUSS_NEWTON_STEPS = 2: a step is accepted iff no w at X is unusable, the solve succeeds, X + d is finite and
             cost(X + d) <= cost(X); the first step that is not accepted ends the loop
  4 scoring  at the final X: max_sq_error = the largest e2 by |bit pattern| (any NaN becomes 0x7fc00000); BEHIND iff some w <= 0; ERROR iff not
             max_sq_error < t2; ANGLE iff cos_min_angle < 1 and not min_cos < cos_min_angle. DEGENERATE / TOO_LONG points are zero but for status and
             nb_observations
  stats      {nb_points, nb_accepted (status 0), nb_failed (DEGENERATE or TOO_LONG), nb_rejected (the others)}

Tracks are evaluated in batches of equal padded length (vectorised over tracks; nothing in the arithmetic depends on the batching).

Also a float64 estimator (SVD DLT + Gauss-Newton, numpy.linalg) for the tests that ask how much fp32 costs, and the synthetic scene of the CPU tests."""
import numpy as np

F32, U32 = np.float32, np.uint32
G = 16
MAX_OBSERVATIONS = 1024
GAUSS_NEWTON_STEPS = 2
DEGENERATE, TOO_LONG, BEHIND, ERROR, ANGLE = 1, 2, 4, 8, 16
POINT_DTYPE = np.dtype([("X", "<f4", (3,)), ("max_sq_error", "<f4"), ("min_cos", "<f4"), ("status", "<u4"), ("steps", "<u4"), ("nb_observations", "<u4")])
STATS = ("nb_points", "nb_accepted", "nb_failed", "nb_rejected")
OBSERVATION_DTYPE = np.dtype([("gpu_buffer_id", "<u4"), ("row", "<u4"), ("x", "<f4"), ("y", "<f4")])
_LANE = np.arange(G)


def threshold2(threshold_px):
    """the squared threshold as vksift_ext_triangulateTracks forms it"""
    with np.errstate(all="ignore"):
        return F32(threshold_px) * F32(threshold_px)


def abs_bits(x):
    return np.asarray(x, F32).view(U32) & U32(0x7FFFFFFF)


def unusable(x):
    e = abs_bits(x) >> U32(23)
    return (e == 0) | (e == 255)


def order_key(x):
    """float32 -> int64 that orders like the float, -0 below +0"""
    i = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF)


def key_float(k):
    k = np.asarray(k, np.int64)
    return np.where(k >= 0, k, k ^ 0x7FFFFFFF).astype(np.int32).view(F32)


def group_sum(v):
    """float32 [T, W] (W a multiple of G, +0 where there is no member) -> float32 [T]: the order of the module docstring"""
    T, W = v.shape
    v = v.reshape(T, W // G, G)
    p = np.zeros((T, G), F32)
    for r in range(W // G):
        p = p + v[:, r]
    for off in (8, 4, 2, 1):
        p = p + p[:, _LANE ^ off]
    assert p.dtype == F32
    return p[:, 0]


def solve3(a):
    """float32 [T, 3, 4] -> (solution [T, 3], ok [T])"""
    a = np.array(a, F32)
    T = len(a)
    ok = np.ones(T, bool)
    one = F32(1)
    for k in range(3):
        for r in range(k + 1, 3):
            sw = abs_bits(a[:, r, k]) > abs_bits(a[:, k, k])
            top, low = a[:, k].copy(), a[:, r].copy()
            a[:, k], a[:, r] = np.where(sw[:, None], low, top), np.where(sw[:, None], top, low)
        ok &= ~unusable(a[:, k, k])
        inv = one / a[:, k, k]
        for c in range(k + 1, 4):
            a[:, k, c] = a[:, k, c] * inv
        for r in range(3):
            if r != k:
                f = a[:, r, k].copy()
                for c in range(k + 1, 4):
                    a[:, r, c] = a[:, r, c] - f * a[:, k, c]
    x = a[:, :, 3].copy()
    return x, ok & np.isfinite(x).all(axis=1)


def row_sums(p, pr, q, qr, valid):
    """the nine sums of the row pairs (p | pr), (q | qr): p, q are lists of three [T, W] arrays"""
    terms = [p[0] * p[0] + q[0] * q[0], p[0] * p[1] + q[0] * q[1], p[0] * p[2] + q[0] * q[2], p[1] * p[1] + q[1] * q[1], p[1] * p[2] + q[1] * q[2],
             p[2] * p[2] + q[2] * q[2], p[0] * pr + q[0] * qr, p[1] * pr + q[1] * qr, p[2] * pr + q[2] * qr]
    assert all(t.dtype == F32 for t in terms)
    return np.stack([group_sum(np.where(valid, t, F32(0))) for t in terms], axis=1)


def solve_normal(s):
    """s float32 [T, 9] -> the solution of S d = -r"""
    a = np.stack([np.stack([s[:, 0], s[:, 1], s[:, 2], -s[:, 6]], axis=1), np.stack([s[:, 1], s[:, 3], s[:, 4], -s[:, 7]], axis=1),
                  np.stack([s[:, 2], s[:, 4], s[:, 5], -s[:, 8]], axis=1)], axis=1)
    return solve3(a)


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def bearings(P, x, y):
    """P: list of twelve [T, W] arrays -> (b: three arrays, ok)"""
    m1, m2, m3 = P[0:3], P[4:7], P[8:11]
    c23, c31, c12 = cross3(m2, m3), cross3(m3, m1), cross3(m1, m2)
    b = [(x * c23[i] + y * c31[i]) + c12[i] for i in range(3)]
    q = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    s = F32(1) / np.sqrt(q)
    assert s.dtype == F32
    return [v * s for v in b], ~unusable(q) & ~unusable(s)


def scaled_row(P, t, r):
    e = [t * P[8 + c] - P[4 * r + c] for c in range(4)]
    q = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    s = F32(1) / np.sqrt(q)
    return [e[0] * s, e[1] * s, e[2] * s], e[3] * s, ~unusable(q) & ~unusable(s)


def evaluate(X, P, x, y, valid):
    """X float32 [T, 3] -> dict(s [T, 10] = cost + the nine sums, bad_w, behind, max_e2 (uint32 keys))"""
    X0, X1, X2 = (X[:, c:c + 1] for c in range(3))
    u = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3]
    v = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7]
    w = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11]
    pu, pv = u / w, v / w
    ru, rv = pu - x, pv - y
    e2 = ru * ru + rv * rv
    iw = F32(1) / w
    ju = [(P[c] - pu * P[8 + c]) * iw for c in range(3)]
    jv = [(P[4 + c] - pv * P[8 + c]) * iw for c in range(3)]
    assert e2.dtype == F32 and ju[0].dtype == F32
    cost = group_sum(np.where(valid, e2, F32(0)))
    s = np.concatenate([cost[:, None], row_sums(ju, ru, jv, rv, valid)], axis=1)
    return dict(s=s, bad_w=(valid & unusable(w)).any(axis=1), behind=(valid & (w <= 0)).any(axis=1),
                max_e2=np.where(valid, abs_bits(e2), U32(0)).max(axis=1))


def _batch(cam, x, y, valid, cameras, t2, cos_min_angle):
    """tracks of one padded length W: cam int64, x, y float32, valid bool, all [T, W] -> POINT_DTYPE [T] without nb_observations"""
    T, W = cam.shape
    out = np.zeros(T, POINT_DTYPE)
    cam_ok = cam < len(cameras)
    Pm = cameras[np.where(cam_ok & valid, cam, 0)]                     # [T, W, 12]
    P = [np.ascontiguousarray(Pm[:, :, c]) for c in range(12)]
    bad = (valid & ~cam_ok).any(axis=1)
    # 1
    b, ok = bearings(P, x, y)
    bad |= (valid & ~ok).any(axis=1)
    dots = (b[0][:, :, None] * b[0][:, None, :] + b[1][:, :, None] * b[1][:, None, :]) + b[2][:, :, None] * b[2][:, None, :]
    assert dots.dtype == F32
    pairs = valid[:, :, None] & valid[:, None, :] & np.triu(np.ones((W, W), bool), 1)[None]
    min_cos = key_float(np.where(pairs, order_key(dots), 0x7FFFFFFF).min(axis=(1, 2)))
    # 2
    p, pr, okp = scaled_row(P, x, 0)
    q, qr, okq = scaled_row(P, y, 1)
    bad |= (valid & ~(okp & okq)).any(axis=1)
    X, started = solve_normal(row_sums(p, pr, q, qr, valid))
    bad |= ~started
    X = np.where(bad[:, None], F32(0), X)
    # 3
    E = evaluate(X, P, x, y, valid)
    steps, active = np.zeros(T, U32), ~bad
    for it in range(GAUSS_NEWTON_STEPS):
        d, ok = solve_normal(E["s"][:, 1:])
        Y = X + d
        can = active & ~E["bad_w"] & ok & np.isfinite(Y).all(axis=1)
        Fv = evaluate(np.where(can[:, None], Y, X), P, x, y, valid)
        acc = can & (Fv["s"][:, 0] <= E["s"][:, 0])
        X = np.where(acc[:, None], Y, X)
        E = {k: np.where(acc[:, None] if E[k].ndim == 2 else acc, Fv[k], E[k]) for k in E}
        steps[acc] = it + 1
        active = acc
    # 4
    max_e2 = np.where(E["max_e2"] > U32(0x7F800000), U32(0x7FC00000), E["max_e2"]).astype(U32).view(F32)
    status = np.where(E["behind"], BEHIND, 0) | np.where(max_e2 < t2, 0, ERROR)
    if cos_min_angle < 1:
        status = status | np.where(min_cos < F32(cos_min_angle), 0, ANGLE)
    good = ~bad
    out["X"][good], out["max_sq_error"][good], out["min_cos"][good] = X[good], max_e2[good], min_cos[good]
    out["steps"][good] = steps[good]
    out["status"] = np.where(bad, DEGENERATE, status)
    return out


def triangulate(offsets, obs, cameras, t2, cos_min_angle, nb_tracks=None, nb_observations=None):
    """offsets: at least nb_tracks + 1 words; obs: OBSERVATION_DTYPE records; cameras float32 [nb_cameras, 12] (or [.., 3, 4]); t2 the squared
    threshold. nb_tracks / nb_observations: the table's counts (default: what the arrays hold). -> (stats dict, POINT_DTYPE [nb_tracks])"""
    offsets = np.asarray(offsets).astype(np.int64)
    M = len(offsets) - 1 if nb_tracks is None else int(nb_tracks)
    total = len(obs) if nb_observations is None else int(nb_observations)
    cameras = np.ascontiguousarray(cameras, F32).reshape(-1, 12)
    t2, cos_min_angle = F32(t2), F32(cos_min_angle)
    pts = np.zeros(M, POINT_DTYPE)
    begin, end = offsets[:M], offsets[1:M + 1]
    extent_ok = (end >= begin) & (end <= total)
    n = np.where(extent_ok, end - begin, 0)
    pts["nb_observations"] = n
    pts["status"] = np.where(~extent_ok | (n < 2), DEGENERATE, 0)
    pts["status"][extent_ok & (n > MAX_OBSERVATIONS)] = TOO_LONG
    live = np.flatnonzero(pts["status"] == 0)
    rows = (n[live] + G - 1) // G
    with np.errstate(all="ignore"):
        for R in np.unique(rows):
            sel = live[rows == R]
            chunk = max(1, (1 << 22) // int(R * G) ** 2)               # (the pair table of a batch stays small)
            for at in range(0, len(sel), chunk):
                t = sel[at:at + chunk]
                k = np.arange(int(R) * G)[None, :]
                valid = k < n[t][:, None]
                idx = np.where(valid, begin[t][:, None] + k, 0)
                o = obs[idx]
                res = _batch(o["gpu_buffer_id"].astype(np.int64), np.where(valid, o["x"], F32(0)), np.where(valid, o["y"], F32(0)), valid, cameras, t2,
                             cos_min_angle)
                for f in ("X", "max_sq_error", "min_cos", "status", "steps"):
                    pts[f][t] = res[f]
    failed = (pts["status"] & (DEGENERATE | TOO_LONG)) != 0
    stats = dict(nb_points=M, nb_accepted=int((pts["status"] == 0).sum()), nb_failed=int(failed.sum()), nb_rejected=int(((pts["status"] != 0) & ~failed).sum()))
    return stats, pts


# ---- float64 evaluation (what fp32 is measured against; never compared with the GPU) --------------------------------------------------------
def project_f64(P, X):
    """P [n, 3, 4], X [3] -> (pixels [n, 2], w [n])"""
    h = np.asarray(P, np.float64) @ np.append(np.asarray(X, np.float64), 1.0)
    with np.errstate(all="ignore"):
        return h[:, :2] / h[:, 2:3], h[:, 2]


def triangulate_f64(P, xy, steps=10):
    """homogeneous DLT by SVD on rows of unit length, then Gauss-Newton on the reprojection error: X [3]"""
    P, xy = np.asarray(P, np.float64).reshape(-1, 3, 4), np.asarray(xy, np.float64).reshape(-1, 2)
    A = np.concatenate([xy[:, 0:1] * P[:, 2] - P[:, 0], xy[:, 1:2] * P[:, 2] - P[:, 1]])
    A /= np.linalg.norm(A[:, :3], axis=1, keepdims=True)
    h = np.linalg.svd(A)[2][-1]
    X = h[:3] / h[3]
    for _ in range(steps):
        hom = P @ np.append(X, 1.0)
        px = hom[:, :2] / hom[:, 2:3]
        J = (P[:, :2, :3] - px[:, :, None] * P[:, 2:3, :3]) / hom[:, 2, None, None]
        d = np.linalg.lstsq(J.reshape(-1, 3), -(px - xy).reshape(-1), rcond=None)[0]
        X = X + d
    return X


# ---- the synthetic scene of the CPU tests ---------------------------------------------------------------------------------------------------
def scene(nb_points=200, origin=(0.0, 0.0, 0.0), seed=5):
    """8 perspective cameras (focal about 520 px, 640 x 480, baselines about 1 unit) that look at points 4 - 12 units in front of them, the world
    origin `origin` away from the rig: (cameras float32 [8, 3, 4], points float64 [nb_points, 3], offsets, observations) with exact projections rounded to
    fp32; every point is seen by 2 .. 8 cameras (each point a track, members in increasing camera)"""
    rng = np.random.RandomState(seed)
    origin = np.asarray(origin, np.float64)
    cams = []
    for c in range(8):
        f = 520.0 + 4.0 * c
        K = np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1.0]])
        ax, ay = 0.04 * np.sin(c), 0.05 * np.cos(2.0 * c)
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        R = Rx @ Ry
        C = origin + np.array([1.0 * (c % 4) - 1.5, 0.9 * (c // 4) - 0.45, 0.1 * np.sin(3.0 * c)])
        cams.append(K @ np.concatenate([R, (-R @ C)[:, None]], axis=1))
    cams32 = np.array(cams).astype(F32)
    pts = origin + np.stack([rng.uniform(-2.0, 2.0, nb_points), rng.uniform(-1.5, 1.5, nb_points), rng.uniform(4.0, 12.0, nb_points)], axis=1)
    offsets, obs = [0], []
    for i, X in enumerate(pts):
        seen = np.sort(rng.choice(8, 2 + i % 7, replace=False))
        px, w = project_f64(cams32[seen], X)               # exact projections under the fp32 cameras the estimator is given
        assert (w > 0).all()
        obs += [(int(c), i, F32(p[0]), F32(p[1])) for c, p in zip(seen, px)]
        offsets.append(len(obs))
    return cams32, pts, np.array(offsets, U32), np.array(obs, OBSERVATION_DTYPE)
