"""Direct access to the launchers of cameras.hip for tests (plain module, no fixtures): vksift_hip_index_views and vksift_hip_refine_cameras.

  * bind(): the ctypes argtypes of the entries
  * IndexViews and RefineCameras turn a case into ONE byte tensor in the manner of tests/hip_triangulate.py (device "cpu" lays out the same bytes
    without a GPU): every input between guard zones of its own, with poisoned words behind the offsets, decoy records behind the last observation, a decoy
    point (status 0) behind the last point and a decoy camera behind the last; then the poisoned outputs with room behind what is written. The index's
    scratch is not compared
  * launch(L, **changes) / expected() / check(): as in hip_records. expected() is tests/np_cameras.py on the case
  * index_cases() / refine_cases(): synthetic tables and views, one builder per shape or status the rules name
"""
import ctypes as C

import numpy as np

import hip_triangulate as HT
import np_cameras as NC
import np_triangulate as NT
from hip_records import HIP_ERROR_INVALID_VALUE  # noqa: F401  (re-exported for the tests)
from hip_two_view import TwoView

u32, f32 = np.uint32, np.float32
TILE = 2048                      # observations per scatter block
VIEW_BYTES, CAMERA_BYTES, POINT_BYTES = NC.VIEW_OBSERVATION_DTYPE.itemsize, NC.CAMERA_DTYPE.itemsize, NT.POINT_DTYPE.itemsize
MAX_BUFFERS = 1024               # the host's largest buffer table


def bind(L):
    vp, w, q, z = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    L.vksift_hip_views_scratch_u32.argtypes = [q]
    L.vksift_hip_views_scratch_u32.restype = z
    L.vksift_hip_index_views.argtypes = [vp, vp, vp, q, q, w, vp, vp, vp, vp, z, vp]
    L.vksift_hip_index_views.restype = C.c_int
    L.vksift_hip_refine_cameras.argtypes = [vp, vp, vp, q, vp, q, vp, w, vp, w, w, vp, vp, vp]
    L.vksift_hip_refine_cameras.restype = C.c_int
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


# ---------------------------------------------------------------------------------------------------------------------- the index
def table(sizes, seed, *, ids=None, per_track=5):
    """an observation table whose view of buffer ids[b] (default b) has sizes[b] observations: tracks of up to per_track members in increasing buffer, rows
    counted per buffer, positions random bit patterns of finite floats -> (offsets, observations)"""
    rng = np.random.RandomState(seed)
    left = np.array(sizes, np.int64)
    ids = list(range(len(sizes))) if ids is None else list(ids)
    rows = np.zeros(len(sizes), np.int64)
    obs, offsets, at = [], [0], 0
    while left.sum():
        have = np.flatnonzero(left)
        take = np.sort(np.roll(have, -(at % len(have)))[:per_track])
        for b in take:
            obs.append((ids[b], rows[b], f32(rng.uniform(-700, 700)), f32(rng.uniform(-500, 500))))
            rows[b] += 1
            left[b] -= 1
        offsets.append(len(obs))
        at += 3
    return np.array(offsets, u32), np.array(obs, NT.OBSERVATION_DTYPE).reshape(-1)


def index_case(name, offsets, obs, nb_cameras, *, nb_tracks=None, nb_observations=None, tracks_cap=None, obs_cap=None):
    """nb_tracks / nb_observations: the table's counts as the device holds them (default: what the arrays are); the caps default to the counts"""
    M = len(offsets) - 1 if nb_tracks is None else nb_tracks
    n = len(obs) if nb_observations is None else nb_observations
    return dict(name=name, offsets=np.asarray(offsets, u32), obs=obs, nb_cameras=nb_cameras, nb_tracks=M, nb_observations=n,
                tracks_cap=max(M, 1) if tracks_cap is None else tracks_cap, obs_cap=max(n, 1) if obs_cap is None else obs_cap)


def index_cases():
    out = [index_case("no observation", [0], np.zeros(0, NT.OBSERVATION_DTYPE), 4, obs_cap=5, tracks_cap=3)]
    out.append(index_case("one observation", *table([0, 1], 1), 3))
    for n in (TILE - 1, TILE, TILE + 1):
        out.append(index_case(f"{n} observations", *table([n // 3, n - 2 * (n // 3), n // 3], n), 3))
    out.append(index_case("views of 0, 1, 255, 256 and 257", *table([0, 1, 255, 256, 257, 0, 3], 2), 7))
    big = [3 + (7 * b) % 5 for b in range(MAX_BUFFERS)]
    for nb in (1, 2, 256, 257, MAX_BUFFERS):
        out.append(index_case(f"{nb} buffers", *table(big[:nb], 10 + nb), nb))
    out.append(index_case("buffer ids that are not contiguous", *table([40, 17, 300, 5], 3, ids=[2, 7, 300, 511]), 600))
    # a conflicting track: two rows of buffer 1 in one track, in increasing row
    offsets, obs = table([6, 6, 6], 4, per_track=3)
    obs = np.insert(obs, 2, np.array([(1, 900, 1.5, 2.5)], NT.OBSERVATION_DTYPE))
    out.append(index_case("a conflicting track with two members in one view", np.concatenate([[0], offsets[1:] + 1]).astype(u32), obs, 3))
    out.append(index_case("buffer ids beyond nb_cameras", *table([9, 8, 7, 6, 5], 5), 3))
    offsets, obs = table([30, 31, 32], 6)
    bad = offsets.copy()
    # observations in front of offsets[0], an extent that ends beyond the table (and swallows the next track's), one that decreases, and — with two
    # tracks fewer on the device than the offsets hold — observations behind the last extent
    bad[0], bad[8], bad[21] = 2, 0xFFFFFFFF, bad[19]
    out.append(index_case("extents that are not the table's", bad, obs, 3, nb_tracks=len(bad) - 3, tracks_cap=len(bad)))
    out.append(index_case("observation count on the device below the table", offsets, obs, 3, nb_observations=int(offsets[7]) + 1, obs_cap=len(obs)))
    out.append(index_case("counts on the device above the capacities", offsets, obs, 3, nb_tracks=len(offsets) + 5, nb_observations=len(obs) + 9,
                          tracks_cap=len(offsets) - 4, obs_cap=len(obs) - 7))
    out.append(index_case("no track on the device", offsets, obs, 3, nb_tracks=0, tracks_cap=4))
    return out


def named(cases, name):
    (c,) = [c for c in cases if c["name"] == name]
    return c


class IndexViews(TwoView):
    entry = "index_views"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c = case
        self.offsets = self.block("offsets", np.concatenate([c["offsets"], np.full(3, 0xA5A5A5A5, u32)]), row_bytes=4)
        decoys = np.array([(0, 0, 100.0, 100.0), (1, 0, 200.0, 200.0)], NT.OBSERVATION_DTYPE)
        self.obs = self.block("observations", np.concatenate([c["obs"], decoys]).view(np.uint8), row_bytes=16)
        self.obs_stats = self.block("observation statistics", np.array([c["nb_tracks"], c["nb_observations"], 77, 78], u32), row_bytes=4)
        self.view_offsets = self.poison("view offsets", 4 * (c["nb_cameras"] + 3), row_bytes=4)
        self.view_obs = self.poison("view observations", VIEW_BYTES * (c["obs_cap"] + 2), row_bytes=VIEW_BYTES)
        self.stats = self.poison("statistics", 4 * 6, row_bytes=4)
        blocks = (c["obs_cap"] + TILE - 1) // TILE
        words = 5 * blocks * TILE + 256 * blocks          # what vksift_hip_views_scratch_u32 must say (checked by the tests against the library)
        self.scratch = self.scratch_block(words)
        self.free = [(self.scratch, 0, 4 * self.scratch_u32)]
        self.build()
        self.args = dict(offsets=self.offsets.ptr, observations=self.obs.ptr, obs_stats=self.obs_stats.ptr, tracks_cap=c["tracks_cap"], obs_cap=c["obs_cap"],
                         nb_cameras=c["nb_cameras"], view_offsets=self.view_offsets.ptr, view_observations=self.view_obs.ptr, stats=self.stats.ptr,
                         scratch=self.scratch.ptr, scratch_u32=self.scratch_u32)

    def restated(self):
        c = self.case
        return NC.index_views(c["offsets"], c["obs"], c["nb_cameras"], nb_tracks=min(c["nb_tracks"], c["tracks_cap"]),
                              nb_observations=min(c["nb_observations"], c["obs_cap"]))

    def expected(self):
        exp = self.host.copy()
        stats, view_offsets, view_obs = self.restated()
        self.put(exp, self.view_offsets, 0, view_offsets)
        self.put(exp, self.view_obs, 0, view_obs)
        self.put(exp, self.stats, 0, np.array([stats[k] for k in NC.VIEW_STATS], u32))
        return exp

    def outputs(self, raw):
        return [self.view(raw, b).copy() for b in (self.view_offsets, self.view_obs, self.stats)]


# ---------------------------------------------------------------------------------------------------------------------- the refinement
CAMERAS = HT.CAMERAS              # the ring of hip_triangulate, its turned camera (CAM_BACK) and its flat one (CAM_FLAT: w = 0 everywhere)
REJECTED = NT.ERROR               # the status of the points a view must not use


def view(nused, seed, *, cam=None, rejected=0, unknown=0, noise=0.3, angle=0.004, shift=0.02, same_point=False):
    """one view: `nused` points with status 0 near the origin seen by camera `cam` of CAMERAS (default: seed % 32) with `noise` px of jitter, `rejected`
    points with a status and `unknown` members whose point number no point has, interleaved; the camera handed in is the true one moved by a small
    rigid motion -> dict(camera float32 [12], X float64 [n, 3], status [n], xy float32 [n, 2], unknown)"""
    rng = np.random.RandomState(5000 + seed)
    cam = seed % HT.NB_RING if cam is None else cam
    n = nused + rejected
    X = rng.uniform(-1.0, 1.0, (n, 3))
    if same_point:
        X[:] = X[0]
    status = np.zeros(n, u32)
    status[rng.choice(n, rejected, replace=False)] = REJECTED
    true = CAMERAS[cam].astype(np.float64)
    with np.errstate(all="ignore"):
        h = X @ true[:, :3].T + true[:, 3]
        px = h[:, :2] / h[:, 2:3]
    px = np.nan_to_num(px, nan=7.0, posinf=7.0, neginf=7.0) + rng.normal(0, noise, (n, 2))
    P = NC.perturbed(CAMERAS[cam:cam + 1], angle, shift, seed=seed)[0].reshape(12) if angle or shift else CAMERAS[cam].reshape(12).copy()
    return dict(camera=P.astype(f32), X=X, status=status, xy=px.astype(f32), unknown=unknown)


def refine_case(name, views, *, nb_steps=4, ids=None, nb_cameras=None, absent=(), nb_indexed=None, obs_cap=None, points_cap=None):
    """views: view() records, view k in gpu_buffer_id ids[k] (default k); buffers of [0, nb_cameras) without a view have an empty range and a camera of
    their own; `absent`: buffers left out of the build's table. nb_indexed: the index's count as the device holds it"""
    ids = list(range(len(views))) if ids is None else list(ids)
    nb_cameras = max(ids) + 1 if nb_cameras is None else nb_cameras
    cams = np.stack([CAMERAS[b % HT.NB_RING].reshape(12) for b in range(nb_cameras)]).astype(f32)
    sizes = np.zeros(nb_cameras, np.int64)
    pts, recs = [], {}
    for b, v in zip(ids, views):
        cams[b] = v["camera"]
        first = len(pts)
        pts += [(tuple(f32(x)), 0.25, 0.5, s, 1, 3) for x, s in zip(v["X"], v["status"])]
        r = [(first + k, 7 * k + b, xy[0], xy[1]) for k, xy in enumerate(v["xy"])]
        for k in range(v["unknown"]):       # members whose point number lies beyond the points
            r.insert(2 * k, (0x40000000 + k, k, 5.0, 6.0))
        recs[b], sizes[b] = r, len(r)
    view_obs = np.array([t for b in sorted(recs) for t in recs[b]], NC.VIEW_OBSERVATION_DTYPE).reshape(-1)
    points = np.array(pts, NT.POINT_DTYPE).reshape(-1)
    n = len(view_obs)
    present = [b for b in range(nb_cameras) if b not in absent]
    return dict(name=name, view_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(u32), view_obs=view_obs, points=points, cameras=cams,
                nb_cameras=nb_cameras, present=present, nb_steps=nb_steps, nb_indexed=n if nb_indexed is None else nb_indexed,
                obs_cap=max(n, 1) if obs_cap is None else obs_cap, points_cap=max(len(points), 1) if points_cap is None else points_cap)


USED = [5, 6, 63, 64, 65, 255, 256, 257, 513]


def status_views():
    """(what, view, status, steps > 0) with nb_steps 4"""
    return [("refined", view(40, 1), 0, True),
            ("TOO_FEW", view(5, 2, rejected=9), NC.TOO_FEW, False),
            ("TOO_FEW: every point rejected", view(0, 3, rejected=12), NC.TOO_FEW, False),
            ("DEGENERATE: w = 0", view(20, 4, cam=HT.CAM_FLAT, angle=0, shift=0), NC.DEGENERATE, False),
            ("BEHIND", view(30, 5, cam=HT.CAM_BACK), NC.BEHIND, True),
            ("all points identical: no solve", view(12, 6, same_point=True), 0, False)]


def refine_cases():
    out = [refine_case("every used count at a boundary", [view(n, n, rejected=n % 7) for n in USED])]
    out.append(refine_case("every status", [v for _, v, _, _ in status_views()], nb_cameras=8, absent=(6,)))
    for steps in (1, 8):
        out.append(refine_case(f"nb_steps {steps}", [view(50, 20 + k, angle=0.01, shift=0.05) for k in range(4)], nb_steps=steps))
    out.append(refine_case("exact projections", [view(30, 30 + k, noise=0.0, angle=0, shift=0) for k in range(3)]))
    out.append(refine_case("buffers that are not contiguous, absent ones between", [view(20 + k, 40 + k) for k in range(4)], ids=[1, 4, 9, 300], nb_cameras=302,
                           absent=tuple(range(10, 300)) + (0,)))
    out.append(refine_case("members without a point", [view(10, 50, unknown=3), view(6, 51, unknown=2, rejected=2)]))
    six = [view(30, 60 + k) for k in range(6)]
    full = refine_case("", six)
    out.append(refine_case("indexed count on the device below the offsets", six, nb_indexed=int(full["view_offsets"][4]) + 9, obs_cap=len(full["view_obs"])))
    out.append(refine_case("indexed count on the device above the capacity", six, nb_indexed=len(full["view_obs"]) + 50, obs_cap=int(full["view_offsets"][5]) - 3))
    out.append(refine_case("points beyond points_cap", six, points_cap=len(full["points"]) - 40))
    return out


class RefineCameras(TwoView):
    entry = "refine_cameras"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c = case
        self.view_offsets = self.block("view offsets", np.concatenate([c["view_offsets"], np.full(3, 0xA5A5A5A5, u32)]), row_bytes=4)
        decoys = np.array([(0, 0, 100.0, 100.0), (1, 0, 200.0, 200.0)], NC.VIEW_OBSERVATION_DTYPE)
        self.view_obs = self.block("view observations", np.concatenate([c["view_obs"], decoys]).view(np.uint8), row_bytes=VIEW_BYTES)
        self.view_stats = self.block("view statistics", np.array([75, c["nb_indexed"], 77, 78], u32), row_bytes=4)
        decoy_point = np.array([((0.5, 0.5, 0.5), 0.1, 0.2, 0, 1, 2)], NT.POINT_DTYPE)
        self.points = self.block("points", np.concatenate([c["points"], decoy_point]).view(np.uint8), row_bytes=POINT_BYTES)
        self.cameras = self.block("cameras", np.concatenate([c["cameras"], np.full((1, 12), 3.0, f32)]), row_bytes=48)
        tab = np.array([[b, 0xA5A50000 + k] for k, b in enumerate(c["present"])], u32)
        self.buf_tab = self.block("buffer table", tab, row_bytes=8)
        self.refined = self.poison("refined cameras", CAMERA_BYTES * (c["nb_cameras"] + 1), row_bytes=CAMERA_BYTES)
        self.stats = self.poison("statistics", 4 * 6, row_bytes=4)
        self.build()
        self.args = dict(view_offsets=self.view_offsets.ptr, view_observations=self.view_obs.ptr, view_stats=self.view_stats.ptr, obs_cap=c["obs_cap"],
                         points=self.points.ptr, points_cap=c["points_cap"], cameras=self.cameras.ptr, nb_cameras=c["nb_cameras"], buf_tab=self.buf_tab.ptr,
                         nbufs=len(c["present"]), nb_steps=c["nb_steps"], refined=self.refined.ptr, stats=self.stats.ptr)

    def restated(self):
        c = self.case
        return NC.refine_cameras(c["view_offsets"], c["view_obs"], c["points"], c["cameras"], c["present"], c["nb_steps"],
                                 nb_indexed=min(c["nb_indexed"], c["obs_cap"]), points_cap=c["points_cap"])

    def expected(self):
        exp = self.host.copy()
        stats, recs = self.restated()
        self.put(exp, self.refined, 0, recs)
        self.put(exp, self.stats, 0, np.array([stats[k] for k in NC.CAMERA_STATS], u32))
        return exp

    def outputs(self, raw):
        return [self.view(raw, b).copy() for b in (self.refined, self.stats)]
