"""Independent numpy restatement of vulkansift_amd/csrc/hip/cameras.hip — the per-view index of the observation table (vksift_hip_index_views,
vksift_ext_indexObservationsByView) and the refinement of every camera on the triangulated points (vksift_hip_refine_cameras, vksift_ext_refineCameras) —
in the manner of tests/np_triangulate.py: what the kernels must compute, written down a second time. This file is the specification of the operation
order; every value is np.float32 with one rounding per operation, no fused operation anywhere. "unusable" means zero, subnormal or not finite.

  index      observation i < n (the table's count) is INDEXED iff its gpu_buffer_id < nb_cameras and the search lo = 0, hi = M; while hi - lo > 1:
             mid = lo + (hi - lo) // 2; offsets[mid] <= i ? lo = mid : hi = mid ends at a track m = lo with offsets[m] <= i < offsets[m+1] <= n (M = 0:
             nothing is indexed). The indexed observations grouped by gpu_buffer_id, inside a view in increasing i, each {point m, row, x, y};
             view_offsets the prefix sum of the views' sizes; stats {nb_views with an observation, nb_observations, largest_view, 0}
  refinement per gpu_buffer_id b < nb_cameras; b not among the buffers of the build: ABSENT, every field 0. The view's range view_offsets[b] ..
             view_offsets[b+1], the end clamped to the indexed count, the begin to the clamped end.
   1 used    a member is USED iff its point number < points_cap and the status word of that point is 0; fewer than 6: TOO_FEW
   2 at P    per used member with X its point: u = ((P0 X + P1 Y) + P2 Z) + P3, v and w alike; pu = u / w, pv = v / w, ru = pu - x, rv = pv - y,
             e2 = ru ru + rv rv, iw = 1 / w, ju[c] = (P1[c] - pu P3[c]) iw, jv[c] = (P2[c] - pv P3[c]) iw (np_triangulate's step 3); au = X x ju,
             av = X x jv with a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); rows p = (au, ju | ru), q = (av, jv | rv); the 28 sums: cost of e2,
             the 21 upper entries N[a][b] of (pa pb + qa qb) row by row, the 6 entries g[a] of (pa ru + qa rv). DEGENERATE iff at the input camera some w is
             unusable or the cost is not finite
   3 step    N d = -g by the 6x7 Gauss-Jordan with the refits' pivot rule (np_triangulate.solve3's, on six rows); a = 0.5 d[0..2], b = 2 a,
             q = (a0 a0 + a1 a1) + a2 a2, s = 1 / (1 + q), t = 1 - q, C[i][i] = (t + b[i] a[i]) s, C01 = (b0 a1 - b2) s, C02 = (b0 a2 + b1) s,
             C10 = (b1 a0 + b2) s, C12 = (b1 a2 - b0) s, C20 = (b2 a0 - b1) s, C21 = (b2 a1 + b0) s; P'[r][c] = (P[r][0] C[0][c] + P[r][1] C[1][c]) +
             P[r][2] C[2][c] for c < 3, P'[r][3] = ((P[r][0] d3 + P[r][1] d4) + P[r][2] d5) + P[r][3]. Accepted iff no w at P is unusable, the solve
             succeeds, P' is finite and cost(P') <= cost(P); the first step that is not accepted ends the loop; at most nb_steps steps
   4 sums    lane j of 256 adds the used members at positions j, j + 256, ... in increasing order to a partial sum that starts at +0 (an unused member
             adds +0, which changes no bit: such a partial sum is never -0); the 64 lanes of a wave by the butterfly p[l] + p[l ^ off], off = 32 .. 1;
             the four waves as ((w0 + w1) + w2) + w3
   5 record  P the final camera, cost_start and cost at the input and the final camera, max_sq_error the largest e2 by |bit pattern| at the final camera
             (any NaN becomes 0x7fc00000), BEHIND iff some w <= 0 there. TOO_FEW / DEGENERATE: the input camera and nb_observations, everything else 0
  stats      {nb_views (not ABSENT), nb_refined (steps > 0), nb_unchanged (neither TOO_FEW nor DEGENERATE, steps 0), nb_failed (TOO_FEW or DEGENERATE)}

Also a float64 estimator (Gauss-Newton by numpy.linalg.lstsq on the same parametrisation) for the tests that ask how much fp32 costs, and the
perturbation of the CPU tests' cameras."""
import numpy as np

from np_triangulate import OBSERVATION_DTYPE, POINT_DTYPE, abs_bits, cross3, unusable  # noqa: F401  (shared pieces, written once)

F32, U32 = np.float32, np.uint32
THREADS = 256
MIN_OBSERVATIONS = 6
MAX_STEPS = 8
ABSENT, TOO_FEW, DEGENERATE, BEHIND = 1, 2, 4, 8
NONE = 0xFFFFFFFF
VIEW_OBSERVATION_DTYPE = np.dtype([("point", "<u4"), ("row", "<u4"), ("x", "<f4"), ("y", "<f4")])
CAMERA_DTYPE = np.dtype([("P", "<f4", (12,)), ("cost_start", "<f4"), ("cost", "<f4"), ("max_sq_error", "<f4"), ("nb_observations", "<u4"), ("steps", "<u4"),
                         ("status", "<u4")])
VIEW_STATS = ("nb_views", "nb_observations", "largest_view", "reserved")
CAMERA_STATS = ("nb_views", "nb_refined", "nb_unchanged", "nb_failed")


# ---- the index -----------------------------------------------------------------------------------------------------------------------------------
def point_of(offsets, M, n, i):
    """the search of the module docstring for every observation number of i (int64 array) -> the track, NONE where the observation is left out"""
    offsets = np.asarray(offsets).astype(np.int64)
    i = np.asarray(i, np.int64)
    if M == 0:
        return np.full(len(i), NONE, np.int64)
    lo, hi = np.zeros(len(i), np.int64), np.full(len(i), M, np.int64)
    while ((hi - lo) > 1).any():
        go = (hi - lo) > 1
        mid = lo + (hi - lo) // 2
        left = offsets[mid] <= i
        lo, hi = np.where(go & left, mid, lo), np.where(go & ~left, mid, hi)
    ok = (offsets[lo] <= i) & (i < offsets[lo + 1]) & (offsets[lo + 1] <= n)
    return np.where(ok, lo, NONE)


def index_views(offsets, obs, nb_cameras, nb_tracks=None, nb_observations=None):
    """offsets: at least nb_tracks + 1 words; obs: OBSERVATION_DTYPE records; nb_tracks / nb_observations: the table's counts (default: what the arrays
    hold) -> (stats dict, view_offsets uint32 [nb_cameras + 1], VIEW_OBSERVATION_DTYPE records)"""
    M = len(offsets) - 1 if nb_tracks is None else int(nb_tracks)
    n = len(obs) if nb_observations is None else int(nb_observations)
    i = np.arange(n, dtype=np.int64)
    m = point_of(offsets, M, n, i)
    buf = obs["gpu_buffer_id"][:n].astype(np.int64)
    keep = (m != NONE) & (buf < nb_cameras)
    i, m, buf = i[keep], m[keep], buf[keep]
    order = np.argsort(buf, kind="stable")
    out = np.zeros(len(i), VIEW_OBSERVATION_DTYPE)
    src = obs[i[order]]
    out["point"], out["row"], out["x"], out["y"] = m[order], src["row"], src["x"], src["y"]
    sizes = np.bincount(buf, minlength=nb_cameras)[:nb_cameras]
    view_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(U32)
    stats = dict(nb_views=int((sizes > 0).sum()), nb_observations=int(len(i)), largest_view=int(sizes.max()) if nb_cameras else 0, reserved=0)
    return stats, view_offsets, out


# ---- the refinement ------------------------------------------------------------------------------------------------------------------------------
_LANE = np.arange(64)


def block_sum(v):
    """float32 [T, W] (W a multiple of 256, +0 where there is no used member) -> float32 [T]: the order of the module docstring"""
    T, W = v.shape
    v = v.reshape(T, W // THREADS, THREADS)
    p = np.zeros((T, THREADS), F32)
    for r in range(W // THREADS):
        p = p + v[:, r]
    p = p.reshape(T, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, :, _LANE ^ off]
    w = p[:, :, 0]
    out = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    assert out.dtype == F32
    return out


def solve6(a):
    """float32 [T, 6, 7] -> (solution [T, 6], ok [T])"""
    a = np.array(a, F32)
    ok = np.ones(len(a), bool)
    one = F32(1)
    for k in range(6):
        for r in range(k + 1, 6):
            sw = abs_bits(a[:, r, k]) > abs_bits(a[:, k, k])
            top, low = a[:, k].copy(), a[:, r].copy()
            a[:, k], a[:, r] = np.where(sw[:, None], low, top), np.where(sw[:, None], top, low)
        ok &= ~unusable(a[:, k, k])
        inv = one / a[:, k, k]
        for c in range(k + 1, 7):
            a[:, k, c] = a[:, k, c] * inv
        for r in range(6):
            if r != k:
                f = a[:, r, k].copy()
                for c in range(k + 1, 7):
                    a[:, r, c] = a[:, r, c] - f * a[:, k, c]
    x = a[:, :, 6].copy()
    assert x.dtype == F32
    return x, ok & np.isfinite(x).all(axis=1)


def solve_normal(s):
    """s float32 [T, 28] -> the solution of N d = -g"""
    T = len(s)
    a = np.zeros((T, 6, 7), F32)
    at = 1
    for r in range(6):
        for c in range(r, 6):
            a[:, r, c] = a[:, c, r] = s[:, at]
            at += 1
    for r in range(6):
        a[:, r, 6] = -s[:, 22 + r]
    return solve6(a)


def cayley(omega):
    """float32 [T, 3] -> C float32 [T, 3, 3] (step 3)"""
    omega = np.asarray(omega, F32)
    half, two, one = F32(0.5), F32(2), F32(1)
    a = [half * omega[:, i] for i in range(3)]
    b = [two * a[i] for i in range(3)]
    q = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    s, t = one / (one + q), one - q
    C = np.zeros((len(omega), 3, 3), F32)
    for i in range(3):
        C[:, i, i] = (t + b[i] * a[i]) * s
    C[:, 0, 1], C[:, 0, 2] = (b[0] * a[1] - b[2]) * s, (b[0] * a[2] + b[1]) * s
    C[:, 1, 0], C[:, 1, 2] = (b[1] * a[0] + b[2]) * s, (b[1] * a[2] - b[0]) * s
    C[:, 2, 0], C[:, 2, 1] = (b[2] * a[0] - b[1]) * s, (b[2] * a[1] + b[0]) * s
    return C


def step(P, d):
    """P float32 [T, 12], d float32 [T, 6] -> (P' [T, 12], finite [T])"""
    C = cayley(d[:, :3])
    Q = np.zeros_like(P)
    for r in range(3):
        p0, p1, p2 = P[:, 4 * r], P[:, 4 * r + 1], P[:, 4 * r + 2]
        for c in range(3):
            Q[:, 4 * r + c] = (p0 * C[:, 0, c] + p1 * C[:, 1, c]) + p2 * C[:, 2, c]
        Q[:, 4 * r + 3] = ((p0 * d[:, 3] + p1 * d[:, 4]) + p2 * d[:, 5]) + P[:, 4 * r + 3]
    assert Q.dtype == F32
    return Q, np.isfinite(Q).all(axis=1)


def evaluate(P, X, x, y, used):
    """P float32 [T, 12]; X: three [T, W] arrays; x, y [T, W]; used bool [T, W] -> dict(s [T, 28], bad_w, behind, max_e2 (uint32 keys))"""
    P = [P[:, c:c + 1] for c in range(12)]
    u = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3]
    v = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7]
    w = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11]
    pu, pv = u / w, v / w
    ru, rv = pu - x, pv - y
    e2 = ru * ru + rv * rv
    iw = F32(1) / w
    ju = [(P[c] - pu * P[8 + c]) * iw for c in range(3)]
    jv = [(P[4 + c] - pv * P[8 + c]) * iw for c in range(3)]
    p, q = cross3(X, ju) + ju, cross3(X, jv) + jv
    terms = [e2] + [p[a] * p[b] + q[a] * q[b] for a in range(6) for b in range(a, 6)] + [p[a] * ru + q[a] * rv for a in range(6)]
    assert all(t.dtype == F32 for t in terms) and len(terms) == 28
    s = np.stack([block_sum(np.where(used, t, F32(0))) for t in terms], axis=1)
    return dict(s=s, bad_w=(used & unusable(w)).any(axis=1), behind=(used & (w <= 0)).any(axis=1),
                max_e2=np.where(used, abs_bits(e2), U32(0)).max(axis=1))


def refine_cameras(view_offsets, view_obs, points, cameras, present, nb_steps, nb_indexed=None, points_cap=None):
    """view_offsets: nb_cameras + 1 words; view_obs: VIEW_OBSERVATION_DTYPE; points: POINT_DTYPE; cameras float32 [nb_cameras, 12] (or [.., 3, 4]);
    present: the gpu_buffer_ids that took part in the build; nb_indexed: the index's count (default: what view_obs holds); points_cap: the points there
    are (default: len(points)) -> (stats dict, CAMERA_DTYPE [nb_cameras])"""
    cameras = np.ascontiguousarray(cameras, F32).reshape(-1, 12)
    nb = len(cameras)
    assert 1 <= nb_steps <= MAX_STEPS and len(view_offsets) >= nb + 1
    total = len(view_obs) if nb_indexed is None else int(nb_indexed)
    cap = len(points) if points_cap is None else int(points_cap)
    vo = np.asarray(view_offsets).astype(np.int64)
    out = np.zeros(nb, CAMERA_DTYPE)
    is_present = np.isin(np.arange(nb), np.asarray(list(present), np.int64))
    out["status"][~is_present] = ABSENT
    views = np.flatnonzero(is_present)
    if len(views):
        end = np.minimum(vo[views + 1], total)
        begin = np.minimum(vo[views], end)
        n = end - begin
        W = max(THREADS, int((n.max() + THREADS - 1) // THREADS) * THREADS)
        k = np.arange(W)[None, :]
        there = k < n[:, None]
        rec = view_obs[np.where(there, begin[:, None] + k, 0)] if len(view_obs) else np.zeros((len(views), W), VIEW_OBSERVATION_DTYPE)
        pt = rec["point"].astype(np.int64)
        known = there & (pt < cap)
        pr = points[np.where(known, pt, 0)] if len(points) else np.zeros((len(views), W), POINT_DTYPE)
        used = known & (pr["status"] == 0)
        X = [np.where(used, pr["X"][..., c], F32(0)) for c in range(3)]
        x, y = np.where(used, rec["x"], F32(0)), np.where(used, rec["y"], F32(0))
        with np.errstate(all="ignore"):
            Q = cameras[views].copy()
            E = evaluate(Q, X, x, y, used)
            nused = used.sum(axis=1)
            too_few = nused < MIN_OBSERVATIONS
            degenerate = ~too_few & (E["bad_w"] | ~np.isfinite(E["s"][:, 0]))
            active = ~too_few & ~degenerate
            cost_start = E["s"][:, 0].copy()
            steps = np.zeros(len(views), U32)
            for it in range(1, nb_steps + 1):
                d, ok = solve_normal(E["s"])
                Qn, fin = step(Q, d)
                can = active & ~E["bad_w"] & ok & fin
                Fv = evaluate(np.where(can[:, None], Qn, Q), X, x, y, used)
                acc = can & (Fv["s"][:, 0] <= E["s"][:, 0])
                Q = np.where(acc[:, None], Qn, Q)
                E = {key: np.where(acc[:, None] if E[key].ndim == 2 else acc, Fv[key], E[key]) for key in E}
                steps[acc] = it
                active = acc
        good = ~too_few & ~degenerate
        max_e2 = np.where(E["max_e2"] > U32(0x7F800000), U32(0x7FC00000), E["max_e2"]).astype(U32).view(F32)
        o = np.zeros(len(views), CAMERA_DTYPE)
        o["P"] = Q
        o["nb_observations"] = nused
        o["cost_start"][good], o["cost"][good], o["max_sq_error"][good], o["steps"][good] = cost_start[good], E["s"][good, 0], max_e2[good], steps[good]
        o["status"] = np.where(too_few, TOO_FEW, np.where(degenerate, DEGENERATE, np.where(E["behind"], BEHIND, 0)))
        out[views] = o
    st = out["status"]
    failed = (st & (TOO_FEW | DEGENERATE)) != 0
    live = (st & ABSENT) == 0
    stats = dict(nb_views=int(live.sum()), nb_refined=int((live & ~failed & (out["steps"] > 0)).sum()),
                 nb_unchanged=int((live & ~failed & (out["steps"] == 0)).sum()), nb_failed=int(failed.sum()))
    return stats, out


# ---- float64 evaluation (what fp32 is measured against; never compared with the GPU) ---------------------------------------------------------------
def cayley_f64(omega):
    a = 0.5 * np.asarray(omega, np.float64)
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return ((1 - a @ a) * np.eye(3) + 2 * np.outer(a, a) + 2 * A) / (1 + a @ a)


def cost_f64(P, X, xy):
    h = np.asarray(X, np.float64) @ np.asarray(P, np.float64).reshape(3, 4)[:, :3].T + np.asarray(P, np.float64).reshape(3, 4)[:, 3]
    return float((((h[:, :2] / h[:, 2:3]) - np.asarray(xy, np.float64)) ** 2).sum())


def refine_f64(P, X, xy, steps=10):
    """Gauss-Newton on the same parametrisation (P <- P [[C(omega), tau], [0, 1]]) in float64, each step by numpy's least squares, kept iff the cost does
    not rise -> (P [3, 4], cost)"""
    P, X, xy = np.asarray(P, np.float64).reshape(3, 4).copy(), np.asarray(X, np.float64), np.asarray(xy, np.float64)
    cost = cost_f64(P, X, xy)
    for _ in range(steps):
        h = X @ P[:, :3].T + P[:, 3]
        px = h[:, :2] / h[:, 2:3]
        J3 = (P[None, :2, :3] - px[:, :, None] * P[None, 2:3, :3]) / h[:, 2, None, None]          # [n, 2, 3]
        J = np.concatenate([np.cross(X[:, None, :], J3), J3], axis=2).reshape(-1, 6)
        d = np.linalg.lstsq(J, -(px - xy).reshape(-1), rcond=None)[0]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = cayley_f64(d[:3]), d[3:]
        Pn = P @ T
        cn = cost_f64(Pn, X, xy)
        if not cn <= cost:
            break
        P, cost = Pn, cn
    return P, cost


def perturbed(cameras, angle, shift, seed=11):
    """every camera P times a rigid motion of the world drawn with rotation parameters of size `angle` and translations of size `shift` -> float32"""
    rng = np.random.RandomState(seed)
    out = []
    for P in np.asarray(cameras, np.float64).reshape(-1, 3, 4):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = cayley_f64(rng.normal(0, angle, 3)), rng.normal(0, shift, 3)
        out.append(P @ T)
    return np.array(out).astype(F32)
