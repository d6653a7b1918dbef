"""tests/np_cameras.py, the restatement of the per-view index and of the camera refinement (include/vksift_ext.h, vksift_ext_indexObservationsByView and
vksift_ext_refineCameras), on its own (CPU): the index against a plain sort, hand cases for every status the rule can give, the fixed order of its sums,
the scene of tests/np_triangulate.py where the fp32 rule is measured against an independent float64 estimator (Gauss-Newton by numpy.linalg.lstsq on the
same parametrisation), and the alternation with tests/np_triangulate.py."""
import numpy as np
import pytest

import np_cameras as NC
import np_triangulate as NT

F32, U32 = np.float32, np.uint32
T2 = NT.threshold2(2.0)


# ---- the index --------------------------------------------------------------------------------------------------------------------------------------
def test_index_is_the_table_sorted_by_view_with_its_track_numbers():
    cams, _, offsets, obs = NT.scene(120)
    stats, view_offsets, view_obs = NC.index_views(offsets, obs, 8)
    track = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.lexsort((np.arange(len(obs)), obs["gpu_buffer_id"]))              # by view, inside a view in table order
    assert np.array_equal(view_obs["point"], track[order]) and np.array_equal(view_obs["row"], obs["row"][order])
    assert view_obs["x"].tobytes() == obs["x"][order].tobytes() and view_obs["y"].tobytes() == obs["y"][order].tobytes()
    assert np.array_equal(np.diff(view_offsets), np.bincount(obs["gpu_buffer_id"], minlength=8)) and view_offsets[0] == 0
    assert stats == dict(nb_views=8, nb_observations=len(obs), largest_view=int(np.diff(view_offsets).max()), reserved=0)


def test_index_leaves_out_unknown_buffers_and_broken_extents():
    _, _, offsets, obs = NT.scene(40)
    n = len(obs)
    stats, view_offsets, view_obs = NC.index_views(offsets, obs, 5)             # buffers 5, 6, 7 have no view
    assert stats["nb_observations"] == int((obs["gpu_buffer_id"] < 5).sum()) == view_offsets[5] and len(view_offsets) == 6
    cut = int(offsets[30]) + 1                                                    # the table ends inside track 30: its extent is not the table's
    stats, _, view_obs = NC.index_views(offsets, obs, 8, nb_observations=cut)
    assert stats["nb_observations"] == int(offsets[30]) and view_obs["point"].max() == 29
    stats, _, view_obs = NC.index_views(offsets, obs, 8, nb_tracks=10)          # ten tracks only: what lies behind them belongs to none
    assert stats["nb_observations"] == int(offsets[10]) and view_obs["point"].max() == 9
    assert NC.index_views(offsets, obs, 8, nb_tracks=0)[0]["nb_observations"] == 0 and n > 0


# ---- hand cases of the refinement -------------------------------------------------------------------------------------------------------------------
def cam(f=500.0, C=(0.0, 0.0, -6.0)):
    K = np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1.0]])
    return (K @ np.concatenate([np.eye(3), -np.asarray(C, np.float64)[:, None]], axis=1)).astype(F32)


def one_view(P, X, xy, status=None, nb_steps=4, present=(0,), true=None):
    """a single view of buffer 0: camera P, points X with `status` (default 0), pixels xy (default: the exact projections under `true`, default P)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    pts = np.zeros(len(X), NT.POINT_DTYPE)
    pts["X"], pts["status"] = X.astype(F32), 0 if status is None else status
    if xy is None:
        T = np.asarray(P if true is None else true, np.float64).reshape(3, 4)
        with np.errstate(all="ignore"):
            h = pts["X"].astype(np.float64) @ T[:, :3].T + T[:, 3]
            xy = np.nan_to_num(h[:, :2] / h[:, 2:3], nan=7.0, posinf=7.0, neginf=7.0)
    vobs = np.zeros(len(X), NC.VIEW_OBSERVATION_DTYPE)
    vobs["point"], vobs["x"], vobs["y"] = np.arange(len(X)), np.asarray(xy)[:, 0], np.asarray(xy)[:, 1]
    stats, rec = NC.refine_cameras(np.array([0, len(X)], U32), vobs, pts, np.asarray(P, F32).reshape(1, 12), present, nb_steps)
    assert stats["nb_views"] == stats["nb_refined"] + stats["nb_unchanged"] + stats["nb_failed"]
    return stats, rec[0]


def cloud(n, seed=1):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (n, 3))


def test_cayley_of_zero_is_the_identity_exactly_and_a_rotation_otherwise():
    assert NC.cayley(np.zeros((1, 3), F32))[0].tobytes() == np.eye(3, dtype=F32).tobytes()
    C = NC.cayley(np.array([[0.3, -0.2, 0.5]], F32))[0].astype(np.float64)
    assert np.abs(C @ C.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(C) - 1) < 1e-6
    assert np.abs(C - NC.cayley_f64([0.3, -0.2, 0.5])).max() < 1e-6
    P, fin = NC.step(cam().reshape(1, 12), np.zeros((1, 6), F32))
    assert fin[0] and P.tobytes() == cam().tobytes()                                # the step of zero leaves P as it is


def test_exact_projections_leave_the_cost_at_zero():
    stats, r = one_view(cam(), cloud(30), None)
    assert r["status"] == 0 and r["nb_observations"] == 30 and r["cost"] <= r["cost_start"] < 1e-6 and r["max_sq_error"] < 1e-7
    assert r["steps"] == 0 or r["cost"] < 1e-6


def test_a_moved_camera_comes_back():
    true = cam()
    moved = NC.perturbed(true[None], 0.01, 0.05, seed=3)[0]
    stats, r = one_view(moved, cloud(60), None, true=true, nb_steps=8)
    assert r["status"] == 0 and r["steps"] >= 2 and r["cost_start"] > 10.0 and r["cost"] < 1e-4
    assert stats == dict(nb_views=1, nb_refined=1, nb_unchanged=0, nb_failed=0)
    # K [R | t] with the same K: the refined camera differs from the true one by a rigid motion that is close to none
    M = np.linalg.inv(np.vstack([true.astype(np.float64), [0, 0, 0, 1]])) @ np.vstack([r["P"].reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
    assert np.abs(M - np.eye(4)).max() < 1e-3


def test_five_and_six_used_observations():
    X = cloud(9, 2)
    moved = NC.perturbed(cam()[None], 0.01, 0.05, seed=4)[0]
    status = np.array([0, 8, 0, 0, 8, 0, 0, 8, 8], U32)
    stats, r = one_view(moved, X, None, status=status, true=cam())
    assert r["status"] == NC.TOO_FEW and r["nb_observations"] == 5 and r["steps"] == 0 and r["cost_start"] == r["cost"] == r["max_sq_error"] == 0
    assert r["P"].tobytes() == moved.tobytes() and stats["nb_failed"] == 1
    status[8] = 0
    stats, r = one_view(moved, X, None, status=status, true=cam())
    assert r["status"] == 0 and r["nb_observations"] == 6 and r["steps"] > 0 and r["cost"] < r["cost_start"]


def test_every_point_of_a_view_rejected():
    stats, r = one_view(cam(), cloud(20), None, status=np.full(20, NT.ERROR, U32))
    assert r["status"] == NC.TOO_FEW and r["nb_observations"] == 0 and r["P"].tobytes() == cam().tobytes()


def test_identical_points_fail_the_solve_and_leave_the_camera():
    X = np.tile(cloud(1), (12, 1))
    xy = np.random.RandomState(2).uniform(200, 300, (12, 2)).astype(F32)
    stats, r = one_view(cam(), X, xy)
    assert r["status"] == 0 and r["steps"] == 0 and r["nb_observations"] == 12 and r["cost"] == r["cost_start"] > 0
    assert r["P"].tobytes() == cam().tobytes() and stats["nb_unchanged"] == 1


def test_a_point_behind_the_camera():
    back = (np.diag([-1.0, 1.0, -1.0]) @ cam().astype(np.float64)).astype(F32)     # rotation by pi about y: everything it sees lies behind it
    moved = NC.perturbed(back[None], 0.005, 0.02, seed=5)[0]
    stats, r = one_view(moved, cloud(25), None, true=back)
    assert r["status"] == NC.BEHIND and r["steps"] > 0 and r["cost"] < r["cost_start"]
    stats, r = one_view(cam(), np.concatenate([cloud(25), [[0.1, 0.1, -9.0]]]), None)
    assert r["status"] == NC.BEHIND and r["nb_observations"] == 26


def test_a_point_at_w_zero_is_degenerate():
    X = np.concatenate([cloud(10), [[0.25, 0.5, -6.0]]])                             # the last one in the camera's principal plane: w = 0
    stats, r = one_view(cam(), X, None)
    assert r["status"] == NC.DEGENERATE and r["nb_observations"] == 11 and r["steps"] == 0 and r["cost_start"] == r["cost"] == r["max_sq_error"] == 0
    assert r["P"].tobytes() == cam().tobytes() and stats["nb_failed"] == 1


def test_an_absent_buffer():
    stats, r = one_view(cam(), cloud(10), None, present=())
    assert r["status"] == NC.ABSENT and not r.tobytes()[:-4].strip(b"\0")
    assert stats == dict(nb_views=0, nb_refined=0, nb_unchanged=0, nb_failed=0)


def test_the_order_of_the_sums_is_the_rule():
    """257 terms whose sum depends on the order: the rule's order is reproduced by hand, and differs from numpy's own"""
    v = np.random.RandomState(7).uniform(-1, 1, (1, 512)).astype(F32) * np.logspace(-3, 3, 512, dtype=F32)
    v[0, 257:] = 0
    lanes = v[0, :256] + v[0, 256:]
    waves = lanes.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, np.arange(64) ^ off]
    want = ((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]
    assert NC.block_sum(v)[0].tobytes() == F32(want).tobytes()


# ---- fp32 against float64, and the alternation ------------------------------------------------------------------------------------------------------
def noisy_scene(nb_points, origin, seed, noise):
    cams, pts, offsets, obs = NT.scene(nb_points, origin=origin, seed=seed)
    rng = np.random.RandomState(seed)
    obs = obs.copy()
    obs["x"] += rng.normal(0, noise, len(obs)).astype(F32)
    obs["y"] += rng.normal(0, noise, len(obs)).astype(F32)
    return cams, offsets, obs


SCENES = [(400, (0.0, 0.0, 0.0), 5), (400, (3.0, -2.0, 5.0), 6), (300, (0.0, 0.0, 0.0), 7)]
MEASURED_WORST = 2.2e-5  # (2.18e-5: scene 6, a view of 7 used members)
TOLERANCE = 4 * MEASURED_WORST


@pytest.mark.parametrize("nb_points, origin, seed", SCENES)
def test_fp32_cost_against_float64(nb_points, origin, seed):
    """The final cost of the fp32 rule (up to 8 steps) against the float64 estimator's (up to 10 steps, numpy least squares) on the same used members, per
    view with at least MIN_OBSERVATIONS of them: cameras moved by rotation parameters of 0.002 and shifts of 0.01 units, 0.3 px of noise, points from
    np_triangulate under the moved cameras (threshold 2 px). Measured when the file was written, over the three scenes: worst relative difference
    2.18e-5 (MEASURED_WORST; 1.5e-5, 2.2e-5 and 2.0e-5 per scene); asserted: 4 times that."""
    cams, offsets, obs = noisy_scene(nb_points, origin, seed, 0.3)
    P0 = NC.perturbed(cams, 0.002, 0.01, seed=seed)
    _, view_offsets, view_obs = NC.index_views(offsets, obs, 8)
    _, pts = NT.triangulate(offsets, obs, P0.reshape(8, 12), T2, 1.0)
    _, rec = NC.refine_cameras(view_offsets, view_obs, pts, P0.reshape(8, 12), range(8), 8)
    compared, worst = 0, 0.0
    for b in range(8):
        m = view_obs[view_offsets[b]:view_offsets[b + 1]]
        used = pts["status"][m["point"]] == 0
        if rec["status"][b] != 0:
            assert used.sum() < NC.MIN_OBSERVATIONS and rec["status"][b] == NC.TOO_FEW
            continue
        X, xy = pts["X"][m["point"][used]], np.stack([m["x"][used], m["y"][used]], axis=1)
        _, c64 = NC.refine_f64(P0[b], X, xy, 10)
        assert abs(float(rec["cost_start"][b]) - NC.cost_f64(P0[b], X, xy)) <= 1e-4 * float(rec["cost_start"][b])
        rel = abs(float(rec["cost"][b]) - c64) / c64
        print(f"scene {seed} view {b}: {int(used.sum())} used, {rec['steps'][b]} steps, cost {rec['cost_start'][b]:.4f} -> {rec['cost'][b]:.6f}, float64 {c64:.6f}, "
              f"relative difference {rel:.3e}")
        compared, worst = compared + 1, max(worst, rel)
    print("worst relative difference", worst)
    assert compared >= 6
    assert worst <= TOLERANCE


def test_alternation_with_the_triangulation_gains_points():
    """np_triangulate <-> np_cameras for four alternations on scene(400) with 0.3 px of noise, from cameras moved by rotation parameters of 0.004 and
    shifts of 0.02 units, threshold 2 px: fewer than half of the tracks are accepted at the start, the count never falls and ends above its start.
    (86, 110, 152, 200, 306 of 400 when the file was written.)"""
    cams, offsets, obs = noisy_scene(400, (0.0, 0.0, 0.0), 3, 0.3)
    P = NC.perturbed(cams, 0.004, 0.02)
    _, view_offsets, view_obs = NC.index_views(offsets, obs, 8)
    accepted = []
    for _ in range(4):
        stats, pts = NT.triangulate(offsets, obs, P.reshape(8, 12), T2, 1.0)
        accepted.append(stats["nb_accepted"])
        cstats, rec = NC.refine_cameras(view_offsets, view_obs, pts, P.reshape(8, 12), range(8), 4)
        assert (rec["cost"] <= rec["cost_start"]).all()
        P = rec["P"].copy()                                                       # the refined P goes back as it is
    accepted.append(NT.triangulate(offsets, obs, P.reshape(8, 12), T2, 1.0)[0]["nb_accepted"])
    print("accepted over the alternations:", accepted)
    assert accepted[0] < 200
    assert all(b >= a for a, b in zip(accepted, accepted[1:])) and accepted[-1] > accepted[0]
