"""tests/np_triangulate.py, the restatement of the triangulation rule (include/vksift_ext.h, vksift_ext_triangulateTracks), on its own (CPU): hand
cases for every status the rule can give, the fixed order of its sums, and a scene of 8 perspective cameras where the fp32 rule is measured against an
independent float64 estimator (numpy.linalg: SVD DLT + Gauss-Newton)."""
import numpy as np
import pytest

import np_triangulate as NT

F32 = np.float32
T2 = NT.threshold2(0.5)


def cam(f=500.0, cx=320.0, cy=240.0, C=(0.0, 0.0, 0.0)):
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    return (K @ np.concatenate([np.eye(3), -np.asarray(C, np.float64)[:, None]], axis=1)).astype(F32)


def table(cams, X, ids, shift=None):
    """one track: the exact projections of X under cameras `ids`, rounded to fp32 (shift: pixels added per member)"""
    px, _ = NT.project_f64(np.asarray(cams)[list(ids)], X)
    px = px + (0.0 if shift is None else np.asarray(shift, np.float64))
    obs = np.array([(c, 0, F32(p[0]), F32(p[1])) for c, p in zip(ids, px)], NT.OBSERVATION_DTYPE)
    return np.array([0, len(ids)], np.uint32), obs


def one(cams, X, ids, cos=1.0, **kw):
    off, obs = table(cams, X, ids, **kw)
    stats, p = NT.triangulate(off, obs, np.asarray(cams, F32), T2, cos)
    assert stats["nb_points"] == 1 and stats["nb_accepted"] + stats["nb_failed"] + stats["nb_rejected"] == 1
    return p[0]


def test_two_members():
    cams = [cam(C=(0, 0, 0)), cam(C=(1, 0, 0))]
    p = one(cams, (0.3, -0.2, 6.0), (0, 1))
    assert p["status"] == 0 and p["nb_observations"] == 2 and p["steps"] <= 2
    assert np.abs(p["X"] - np.array([0.3, -0.2, 6.0])).max() < 1e-3 and p["max_sq_error"] < 1e-4
    # the angle between the two rays, from the geometry: cos = a.b / |a||b|
    a, b = np.array([0.3, -0.2, 6.0]), np.array([-0.7, -0.2, 6.0])
    assert abs(p["min_cos"] - a @ b / np.linalg.norm(a) / np.linalg.norm(b)) < 1e-5
    # the angle test splits at min_cos: a limit just above it accepts, one at or below it rejects
    assert one(cams, (0.3, -0.2, 6.0), (0, 1), cos=float(p["min_cos"]) + 1e-4)["status"] == 0
    assert one(cams, (0.3, -0.2, 6.0), (0, 1), cos=float(p["min_cos"]))["status"] == NT.ANGLE


def test_one_camera_seen_twice_has_no_parallax():
    cams = [cam(), cam(C=(1, 0, 0))]
    p = one(cams, (0.3, -0.2, 6.0), (0, 0), cos=0.9999)
    assert p["status"] & (NT.DEGENERATE | NT.ANGLE)
    if not p["status"] & NT.DEGENERATE:
        assert p["min_cos"] >= F32(0.9999)


def test_point_behind_one_camera():
    """the second camera looks the other way (its left block is diag(-f, f, -1) K-like with positive determinant): the point that fits both lies behind it"""
    back = cam(C=(1, 0, 0))
    back[:, :] = (np.diag([-1.0, 1.0, -1.0]) @ back.astype(np.float64)).astype(F32)         # rotation by pi about y
    assert np.linalg.det(back[:, :3].astype(np.float64)) > 0
    cams = [cam(), back]
    X = (0.3, -0.2, 6.0)
    _, w = NT.project_f64(np.asarray(cams), X)
    assert w[0] > 0 > w[1]
    p = one(cams, X, (0, 1))
    assert p["status"] == NT.BEHIND and p["max_sq_error"] < 1e-4


def test_member_at_w_zero():
    """the point lies in the second camera's principal plane whatever the pixels say: its members are the first camera twice (the solution is that camera's
    centre, where its own w is 0 too)"""
    cams = [cam(C=(0, 0, 0))]
    off = np.array([0, 2], np.uint32)
    obs = np.array([(0, 0, 100.0, 100.0), (0, 1, 500.0, 300.0)], NT.OBSERVATION_DTYPE)
    _, p = NT.triangulate(off, obs, np.asarray(cams), T2, 1.0)
    p = p[0]
    assert not p["status"] & NT.DEGENERATE and np.abs(p["X"]).max() < 1e-3      # the centre of the camera
    assert p["status"] & NT.ERROR and p["steps"] == 0
    # and exactly w = 0: a camera whose third row is zero
    flat = cam(C=(1, 0, 0))
    flat[2] = 0
    off = np.array([0, 3], np.uint32)
    obs = np.array([(0, 0, 345.0, 223.0), (1, 0, 262.0, 223.0), (2, 0, 10.0, 20.0)], NT.OBSERVATION_DTYPE)
    _, p = NT.triangulate(off, obs, np.array([cam(), cam(C=(1, 0, 0)), flat]), T2, 1.0)
    assert p[0]["status"] == NT.BEHIND | NT.ERROR and p[0]["steps"] == 0
    assert p[0]["max_sq_error"].view(np.uint32) in (0x7FC00000, 0x7F800000)      # a division by w = 0: infinity, or the one NaN pattern


def test_camera_with_a_zero_row_and_a_zero_camera():
    zero = np.zeros((3, 4), F32)
    cams = [cam(), cam(C=(1, 0, 0)), zero]
    p = one(cams, (0.3, -0.2, 6.0), (0, 1, 2))
    assert p["status"] == NT.DEGENERATE and p["nb_observations"] == 3
    assert not p["X"].any() and p["max_sq_error"] == 0 and p["min_cos"] == 0 and p["steps"] == 0


def test_lengths_extents_and_cameras_out_of_range():
    cams, _, off, obs = NT.scene(nb_points=8)
    stats, p = NT.triangulate(off, obs, cams, T2, 1.0)
    assert stats == dict(nb_points=8, nb_accepted=8, nb_failed=0, nb_rejected=0)
    # fewer cameras than the table names: the tracks that name one of the missing are DEGENERATE, the others unchanged
    _, q = NT.triangulate(off, obs, cams[:5], T2, 1.0)
    for m in range(8):
        names_missing = (obs[off[m]:off[m + 1]]["gpu_buffer_id"] >= 5).any()
        assert (q[m]["status"] == NT.DEGENERATE) == names_missing and (names_missing or q[m].tobytes() == p[m].tobytes())
    # an extent beyond the table's count, a decreasing one, a track of one and a track of 1025
    stats, q = NT.triangulate(off, obs, cams, T2, 1.0, nb_observations=int(off[7]))
    assert q[7]["status"] == NT.DEGENERATE and q[7]["nb_observations"] == 0 and stats["nb_failed"] == 1 and q[:7].tobytes() == p[:7].tobytes()
    _, q = NT.triangulate(np.array([0, 5, 3, 4], np.uint32), obs, cams, T2, 1.0)
    assert q["status"].tolist()[1:] == [NT.DEGENERATE, NT.DEGENERATE] and q["nb_observations"].tolist()[1:] == [0, 1]
    long = np.zeros(1025, NT.OBSERVATION_DTYPE)
    stats, q = NT.triangulate(np.array([0, 1025], np.uint32), long, cams, T2, 1.0)
    assert q[0]["status"] == NT.TOO_LONG and q[0]["nb_observations"] == 1025 and stats["nb_failed"] == 1


def test_group_sum_order():
    """lane j adds members j, j + 16, ...; then the butterfly 8, 4, 2, 1: restated here with scalars"""
    rng = np.random.RandomState(3)
    v = (rng.standard_normal((3, 48)) * 10.0 ** rng.randint(-3, 4, (3, 48))).astype(F32)
    got = NT.group_sum(v)
    for t in range(3):
        p = [F32(0)] * 16
        for k in range(48):
            p[k % 16] = p[k % 16] + v[t, k]
        for off in (8, 4, 2, 1):
            p = [p[l] + p[l ^ off] for l in range(16)]
        assert all(x.view(np.uint32) == p[0].view(np.uint32) for x in p) and got[t].view(np.uint32) == p[0].view(np.uint32)


def test_solve3_pivots_by_bit_pattern():
    a = np.array([[[0.0, 2.0, 1.0, 5.0], [1.0, 1.0, 1.0, 6.0], [-4.0, 0.0, 1.0, -1.0]]], F32)
    x, ok = NT.solve3(a)
    assert ok[0] and np.allclose(a[0, :, :3] @ x[0], a[0, :, 3])
    with np.errstate(all="ignore"):
        x, ok = NT.solve3(np.array([[[1.0, 2.0, 3.0, 1.0], [2.0, 4.0, 6.0, 2.0], [1.0, 0.0, 1.0, 0.0]]], F32))
    assert not ok[0]


@pytest.fixture(scope="module", params=[(0.0, 0.0, 0.0), (100.0, 0.0, 0.0)], ids=["origin in the rig", "origin 100 units away"])
def world(request):
    cams, pts, off, obs = NT.scene(origin=request.param)
    return cams, pts, off, obs, NT.triangulate(off, obs, cams, T2, 1.0)


def worst_f64_error(cams, off, obs, X):
    worst = 0.0
    for m in range(len(off) - 1):
        o = obs[off[m]:off[m + 1]]
        px, _ = NT.project_f64(cams[o["gpu_buffer_id"]], X[m])
        worst = max(worst, float(np.sqrt(((px - np.stack([o["x"], o["y"]], axis=1).astype(np.float64)) ** 2).sum(axis=1)).max()))
    return worst


def test_scene_noise_free_tracks_are_accepted(world):
    cams, pts, off, obs, (stats, p) = world
    assert stats["nb_accepted"] == stats["nb_points"] == len(pts) and (p["status"] == 0).all()
    assert set(p["nb_observations"].tolist()) == set(range(2, 9))
    # the float64 reprojection error of the fp32 point stays below the threshold (measured: 8.1e-5 px, and 1.2e-3 px with the origin 100 units away)
    worst = worst_f64_error(cams, off, obs, p["X"].astype(np.float64))
    print("worst float64 reprojection error of the fp32 points: %.3g px" % worst)
    assert worst < 0.5
    # ... and agrees with the independent float64 estimator to that extent
    for m in range(len(pts)):
        o = obs[off[m]:off[m + 1]]
        X64 = NT.triangulate_f64(cams[o["gpu_buffer_id"]], np.stack([o["x"], o["y"]], axis=1))
        px32, _ = NT.project_f64(cams[o["gpu_buffer_id"]], p["X"][m])
        px64, _ = NT.project_f64(cams[o["gpu_buffer_id"]], X64)
        assert np.sqrt(((px32 - px64) ** 2).sum(axis=1)).max() < 0.5


def test_scene_displaced_member_gives_error(world):
    cams, pts, off, obs, _ = world
    """50 px across the epipolar lines: along them a displaced member of a two-member track is a point at another depth, which no estimator can tell"""
    moved = obs.copy()
    centre = [-np.linalg.solve(P[:, :3].astype(np.float64), P[:, 3].astype(np.float64)) for P in cams]
    for m in range(len(pts)):
        k = off[m] + m % (off[m + 1] - off[m])
        other = off[m] + (m + 1) % (off[m + 1] - off[m])
        base = (centre[obs["gpu_buffer_id"][other]] - centre[obs["gpu_buffer_id"][k]])[:2]      # (the cameras are nearly parallel: the lines run along it)
        across = np.array([-base[1], base[0]]) / np.linalg.norm(base) * (50.0 if m % 2 else -50.0)
        moved["x"][k] += F32(across[0])
        moved["y"][k] += F32(across[1])
    stats, p = NT.triangulate(off, moved, cams, T2, 1.0)
    assert ((p["status"] & NT.ERROR) != 0).all() and stats["nb_accepted"] == 0
    assert stats["nb_rejected"] + stats["nb_failed"] == len(pts)


def test_launcher_cases_lay_out_and_cover_every_status():
    """the arena of the kernel-level GPU test (tests/hip_triangulate.py) on the CPU: every case lays out, and the restatement gives the statuses the cases
    are named for — each flag alone, BEHIND + ERROR together, TOO_LONG, both sides of the angle limit"""
    import hip_triangulate as HT

    seen = set()
    for c in HT.cases():
        h = HT.Triangulate(c, device="cpu")
        stats, pts = h.restated()
        assert stats["nb_points"] == min(c["nb_tracks"], c["points_cap"]) and h.expected().shape == h.host.shape
        seen |= set(pts["status"].tolist())
    assert {0, NT.DEGENERATE, NT.TOO_LONG, NT.BEHIND, NT.ERROR, NT.ANGLE, NT.BEHIND | NT.ERROR} <= seen
    _, pts = HT.Triangulate(HT.case_by_name("every status"), device="cpu").restated()
    assert pts["status"].tolist() == [s for _, _, s in HT.status_tracks()]
    _, pts = HT.Triangulate(HT.case_by_name("every length at a boundary"), device="cpu").restated()
    assert pts["nb_observations"].tolist() == [2, 3, 15, 16, 17, 33, 64, 65] and not pts["status"].any()
    _, pts = HT.Triangulate(HT.case_by_name("angle test that splits the case"), device="cpu").restated()
    assert pts["status"].tolist() == [NT.ANGLE, 0, 0]
