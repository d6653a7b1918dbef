"""Direct access to the triangulation launcher of include/vksift_hip.h for tests (plain module, no fixtures): vksift_hip_triangulate_tracks.

  * bind(): the ctypes argtypes of the entry
  * Triangulate turns a case — an observation table, its two counts as the device holds them, a camera table and the launch's parameters — into ONE byte
    tensor in the manner of tests/hip_two_view.py (device "cpu" lays out the same bytes without a GPU): offsets, observations, the table's statistics
    and the cameras between guard zones of their own, with poisoned words behind offsets[M], decoy observations behind the last one and a decoy camera
    behind the last; then the poisoned outputs — points_cap points and two more, the four statistics words and two more
  * launch(L, **changes) / expected() / check(): as in hip_records. expected() is tests/np_triangulate.py on the table
  * cases(): synthetic tracks over a ring of cameras, one builder per status the rule can give
"""
import ctypes as C

import numpy as np

import np_triangulate as NT
from hip_records import HIP_ERROR_INVALID_VALUE  # noqa: F401  (re-exported for the tests)
from hip_two_view import TwoView

u32, f32 = np.uint32, np.float32
G, TRACKS_PER_WORKGROUP = NT.G, 256 // NT.G
POINT_BYTES = NT.POINT_DTYPE.itemsize


def bind(L):
    vp, w, q, f = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    L.vksift_hip_triangulate_tracks.argtypes = [vp, vp, vp, vp, w, f, f, vp, q, vp, vp]
    L.vksift_hip_triangulate_tracks.restype = C.c_int
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


# ---------------------------------------------------------------------------------------------------------------------- the cameras and the tracks
NB_RING = 32          # cameras 0 .. 31 on a ring around the scene, all looking at it
CAM_BACK = 32         # camera 0 turned by pi: what fits it lies behind it
CAM_ZERO = 33         # all zeros: no bearing
CAM_FLAT = 34         # third row zero: w = 0 everywhere
CAM_NEAR = 35         # 1/1000 of a unit beside camera 0: no parallax with it
NB_CAMERAS = 36


def cameras():
    cams = np.zeros((NB_CAMERAS, 3, 4), np.float64)
    for c in range(NB_RING):
        a = 2.0 * np.pi * c / NB_RING
        centre = np.array([3.0 * np.cos(a), 3.0 * np.sin(a), -8.0 + 0.2 * np.sin(5.0 * a)])
        z = -centre / np.linalg.norm(centre)                       # looks at the origin
        x = np.cross([0.0, 1.0, 0.1], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        f = 500.0 + 3.0 * c
        cams[c] = np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1.0]]) @ np.concatenate([R, (-R @ centre)[:, None]], axis=1)
    cams[CAM_BACK] = np.diag([-1.0, 1.0, -1.0]) @ cams[0]
    cams[CAM_FLAT] = cams[1]
    cams[CAM_FLAT, 2] = 0.0
    cams[CAM_NEAR] = cams[0]
    cams[CAM_NEAR, :, 3] -= cams[0, :, :3] @ np.array([0.001, 0.0, 0.0])
    return cams.astype(f32)


CAMERAS = cameras()


def track(n, seed, *, ids=None, noise=0.05, displaced=None):
    """n members of a point near the origin: cameras `ids` (default: the ring's, in turn from a start that depends on the seed), pixels exact but for
    `noise` px of jitter (several members may share a camera: the jitter tells them apart); displaced: (member, px) moved across the image"""
    rng = np.random.RandomState(1000 + seed)
    X = rng.uniform(-1.0, 1.0, 3)
    ids = [(seed + 5 * k) % NB_RING for k in range(n)] if ids is None else list(ids)
    assert len(ids) == n
    px, _ = NT.project_f64(CAMERAS[ids], X)
    px = np.nan_to_num(px, nan=7.0, posinf=7.0, neginf=7.0) + rng.uniform(-noise, noise, (n, 2))
    if displaced is not None:
        px[displaced[0]] += displaced[1]
    return [(c, f32(p[0]), f32(p[1])) for c, p in zip(ids, px)]


LENGTHS = [2, 3, G - 1, G, G + 1, 2 * G + 1, 64, 65]


def status_tracks():
    """(what, track, the status the rule must give at threshold 0.5 px and cos_min_angle 1)"""
    return [("accepted", track(4, 1), 0),
            ("DEGENERATE: a camera of zeros", track(3, 2, ids=[0, 5, CAM_ZERO]), NT.DEGENERATE),
            ("BEHIND", track(2, 3, ids=[CAM_BACK, 8], noise=0.0), NT.BEHIND),
            ("ERROR", track(5, 4, displaced=(2, 50.0)), NT.ERROR),
            ("BEHIND + ERROR", track(3, 5, ids=[CAM_BACK, 8, 16], displaced=(1, 50.0)), NT.BEHIND | NT.ERROR),
            ("BEHIND + ERROR: w = 0", track(3, 6, ids=[0, 8, CAM_FLAT]), NT.BEHIND | NT.ERROR)]


def case(name, tracks, *, nb_tracks=None, nb_observations=None, points_cap=None, nb_cameras=NB_CAMERAS, threshold=0.5, cos=1.0, offsets=None):
    """tracks: lists of (gpu_buffer_id, x, y). nb_tracks / nb_observations: the table's counts as the device holds them (default: what the tracks are);
    offsets: instead of the tracks' own"""
    obs = np.array([(c, k, x, y) for t in tracks for k, (c, x, y) in enumerate(t)], NT.OBSERVATION_DTYPE).reshape(-1)
    own = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(u32)
    M = len(tracks) if nb_tracks is None else nb_tracks
    return dict(name=name, obs=obs, offsets=own if offsets is None else np.asarray(offsets, u32), nb_tracks=M,
                nb_observations=len(obs) if nb_observations is None else nb_observations, points_cap=max(M, 1) if points_cap is None else points_cap,
                nb_cameras=nb_cameras, t2=float(NT.threshold2(threshold)), cos=cos)


def cases():
    out = [case("every length at a boundary", [track(n, n) for n in LENGTHS])]
    out.append(case("1024 members and 1025 (TOO_LONG)", [track(1024, 7, noise=0.2), track(1025, 8), track(3, 9)]))
    out.append(case("no track", [], points_cap=4))
    for M in (1, TRACKS_PER_WORKGROUP - 1, TRACKS_PER_WORKGROUP, TRACKS_PER_WORKGROUP + 1):
        out.append(case(f"{M} tracks", [track(2 + (3 * k) % 7, 20 + k) for k in range(M)], points_cap=M + 3))
    many = [track(2 + (5 * k) % 9, 40 + k) for k in range(40)]
    out.append(case("track count on the device above points_cap", many, points_cap=21))
    out.append(case("track count on the device above the table", many[:20], nb_tracks=23, points_cap=30,
                    offsets=np.concatenate([case("", many[:20])["offsets"], [5, 3, 0xFFFFFFFF]])))
    out.append(case("observation count on the device below the table", many[:20], nb_observations=int(case("", many[:20])["offsets"][18]) + 1))
    out.append(case("every status", [t for _, t, _ in status_tracks()]))
    out.append(case("cameras beyond nb_cameras", [track(4, 60, ids=[0, 3, 6, 9]), track(4, 61, ids=[0, 3, 10, 9]), track(2, 62, ids=[11, 2])], nb_cameras=10))
    narrow = [track(2, 70, ids=[0, CAM_NEAR], noise=0.0), track(2, 71, ids=[0, 1], noise=0.0), track(3, 72, ids=[0, 8, 16], noise=0.0)]
    out.append(case("angle test off", narrow, cos=1.0))
    out.append(case("angle test that splits the case", narrow, cos=0.9995))
    out.append(case("angle test nothing passes", narrow, cos=-1.0))
    out.append(case("a wide threshold", [t for _, t, _ in status_tracks()], threshold=200.0))
    return out


def case_by_name(name):
    (c,) = [c for c in cases() if c["name"] == name]
    return c


class Triangulate(TwoView):
    entry = "triangulate_tracks"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c = case
        words = np.concatenate([c["offsets"], np.full(3, 0xA5A5A5A5, u32)])
        self.offsets = self.block("offsets", words, row_bytes=4)
        decoys = np.array([(0, 0, 100.0, 100.0), (1, 0, 200.0, 200.0)], NT.OBSERVATION_DTYPE)
        self.obs = self.block("observations", np.concatenate([c["obs"], decoys]).view(np.uint8), row_bytes=16)
        self.obs_stats = self.block("observation statistics", np.array([c["nb_tracks"], c["nb_observations"], 77, 78], u32), row_bytes=4)
        held = np.concatenate([CAMERAS[:c["nb_cameras"]].reshape(-1, 12), np.full((1, 12), 3.0, f32)])      # a decoy camera behind the last
        self.cameras = self.block("cameras", held, row_bytes=48)
        self.points = self.poison("points", POINT_BYTES * (c["points_cap"] + 2), row_bytes=POINT_BYTES)
        self.stats = self.poison("statistics", 4 * 6, row_bytes=4)
        self.build()
        self.args = dict(offsets=self.offsets.ptr, observations=self.obs.ptr, obs_stats=self.obs_stats.ptr, cameras=self.cameras.ptr, nb_cameras=c["nb_cameras"],
                         t2=c["t2"], cos_min_angle=c["cos"], points=self.points.ptr, points_cap=c["points_cap"], stats=self.stats.ptr)

    def restated(self):
        c = self.case
        return NT.triangulate(c["offsets"], c["obs"], CAMERAS[:c["nb_cameras"]], c["t2"], c["cos"], nb_tracks=min(c["nb_tracks"], c["points_cap"]),
                              nb_observations=c["nb_observations"])

    def expected(self):
        exp = self.host.copy()
        stats, pts = self.restated()
        self.put(exp, self.points, 0, pts)
        self.put(exp, self.stats, 0, np.array([stats[k] for k in NT.STATS], u32))
        return exp

    def outputs(self, raw):
        return [self.view(raw, b).copy() for b in (self.points, self.stats)]
