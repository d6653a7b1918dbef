"""The launchers of cameras.hip called directly — vksift_hip_index_views and vksift_hip_refine_cameras on the cases of tests/hip_cameras.py, not only
through the public entries, which fix the capacities and feed them tables the earlier stages built. Each run: one launch sequence, one synchronisation,
and a BYTE comparison of the whole poisoned arena with the restatement (tests/np_cameras.py): the stated outputs must be there, and every other byte —
guards, the records behind what is written, the words behind the statistics, and the inputs: offsets, observations, counts, points, cameras, the buffer
table — must come back as it went in (the index's scratch excepted, whose contents are unspecified). Nothing is compared with a tolerance."""
import numpy as np
import pytest

import hip_cameras as HC
import np_cameras as NC
from hip_records import Launch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HC.bind(vk.lib())


def run(L, cls, case):
    h = cls(case)
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    after = h.read()
    h.check(after)
    return h, after


@pytest.mark.parametrize("case", HC.index_cases(), ids=lambda c: c["name"])
def test_index_views(L, case):
    h, _ = run(L, HC.IndexViews, case)
    assert L.vksift_hip_views_scratch_u32(case["obs_cap"]) == h.scratch_u32


def test_the_index_leaves_out_what_the_rule_names(L):
    """the fixture's precondition, on what the device wrote"""
    def stats(name):
        h, after = run(L, HC.IndexViews, HC.named(HC.index_cases(), name))
        return h.case, h.view(after, h.stats, np.uint32)[:4].tolist(), h.view(after, h.view_offsets, np.uint32), h.view(after, h.view_obs)

    c, s, _, _ = stats("buffer ids beyond nb_cameras")
    assert s[1] == 9 + 8 + 7 and s[1] < len(c["obs"])
    c, s, _, _ = stats("extents that are not the table's")
    assert 0 < s[1] < len(c["obs"]) - 2
    c, s, vo, recs = stats("a conflicting track with two members in one view")
    view1 = recs[16 * vo[1]:16 * vo[2]].view(NC.VIEW_OBSERVATION_DTYPE)
    assert view1["point"][:2].tolist() == [0, 0] and view1["row"][:2].tolist() == [0, 900]
    c, s, vo, _ = stats("views of 0, 1, 255, 256 and 257")
    assert np.diff(vo[:8]).tolist() == [0, 1, 255, 256, 257, 0, 3] and s == [5, 772, 257, 0]


@pytest.mark.parametrize("case", HC.refine_cases(), ids=lambda c: c["name"])
def test_refine_cameras(L, case):
    run(L, HC.RefineCameras, case)


def test_every_status_and_every_used_count_occur(L):
    """the fixture's precondition, on what the device wrote: each status alone, BEHIND with accepted steps, the failed solve, the boundaries of the sums"""
    h, after = run(L, HC.RefineCameras, HC.named(HC.refine_cases(), "every status"))
    got = h.view(after, h.refined)[:HC.CAMERA_BYTES * 8].view(NC.CAMERA_DTYPE)
    want = HC.status_views()
    assert got["status"][:6].tolist() == [s for _, _, s, _ in want] and got["status"][6:].tolist() == [NC.ABSENT, NC.TOO_FEW]
    assert [bool(s > 0) for s in got["steps"][:6]] == [moved for _, _, _, moved in want]
    assert not got[6].tobytes()[:-4].strip(b"\0")                                        # ABSENT: every other field is 0
    for k in (1, 2, 3):                                                                  # TOO_FEW, DEGENERATE: the input camera, the costs 0
        assert got["P"][k].tobytes() == h.case["cameras"][k].tobytes() and got["cost_start"][k] == got["cost"][k] == got["max_sq_error"][k] == 0
    assert got["cost"][0] < got["cost_start"][0] and got["cost"][4] < got["cost_start"][4]
    h, after = run(L, HC.RefineCameras, HC.named(HC.refine_cases(), "every used count at a boundary"))
    got = h.view(after, h.refined)[:HC.CAMERA_BYTES * len(HC.USED)].view(NC.CAMERA_DTYPE)
    assert got["nb_observations"].tolist() == HC.USED and got["status"].tolist() == [NC.TOO_FEW] + [0] * (len(HC.USED) - 1)
    assert (got["steps"][1:] > 0).all()
    h, after = run(L, HC.RefineCameras, HC.named(HC.refine_cases(), "nb_steps 1"))
    assert h.view(after, h.refined)[:HC.CAMERA_BYTES * 4].view(NC.CAMERA_DTYPE)["steps"].tolist() == [1] * 4
    h, after = run(L, HC.RefineCameras, HC.named(HC.refine_cases(), "exact projections"))
    got = h.view(after, h.refined)[:HC.CAMERA_BYTES * 3].view(NC.CAMERA_DTYPE)
    assert (got["cost"] <= got["cost_start"]).all() and (got["cost"] < 1e-3).all()


def test_second_launch_into_fresh_memory_gives_identical_bytes(L):
    for cls, cases, name in ((HC.IndexViews, HC.index_cases(), "2049 observations"), (HC.RefineCameras, HC.refine_cases(), "every used count at a boundary")):
        h1, a1 = run(L, cls, HC.named(cases, name))
        h2, a2 = run(L, cls, HC.named(cases, name))
        for x, y in zip(h1.outputs(a1), h2.outputs(a2)):
            assert np.array_equal(x, y)


def _ids(d):
    return " ".join(f"{k}={x}" for k, x in d.items())


INDEX_REFUSALS = [dict(offsets=None), dict(observations=None), dict(obs_stats=None), dict(view_offsets=None), dict(view_observations=None), dict(stats=None),
                  dict(scratch=None), dict(nb_cameras=0), dict(nb_cameras=0xFFFFFFFF), dict(tracks_cap=0), dict(tracks_cap=1 << 31), dict(obs_cap=0),
                  dict(obs_cap=(1 << 31) - 2047), {"+scratch_u32": -1}, {"+offsets": 2}, {"+obs_stats": 2}, {"+view_offsets": 2}, {"+stats": 2}, {"+scratch": 2},
                  {"+observations": 4}, {"+view_observations": 4}]


@pytest.mark.parametrize("changes", INDEX_REFUSALS, ids=_ids)
def test_index_refusals(L, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HC.IndexViews(HC.named(HC.index_cases(), "buffer ids beyond nb_cameras"))
    rc = h.launch(L, **changes)
    assert rc == HC.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(Launch.read(h), h.host)


REFINE_REFUSALS = [dict(view_offsets=None), dict(view_observations=None), dict(view_stats=None), dict(points=None), dict(cameras=None), dict(buf_tab=None),
                   dict(refined=None), dict(stats=None), dict(nb_cameras=0), dict(nb_cameras=1 << 31), dict(nbufs=0), dict(obs_cap=0), dict(obs_cap=1 << 31),
                   dict(points_cap=0), dict(points_cap=1 << 31), dict(nb_steps=0), dict(nb_steps=9), {"+view_offsets": 2}, {"+view_stats": 2}, {"+buf_tab": 2},
                   {"+refined": 2}, {"+stats": 2}, {"+view_observations": 4}, {"+points": 4}, {"+cameras": 4}]


@pytest.mark.parametrize("changes", REFINE_REFUSALS, ids=_ids)
def test_refine_refusals(L, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HC.RefineCameras(HC.named(HC.refine_cases(), "every status"))
    rc = h.launch(L, **changes)
    assert rc == HC.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(Launch.read(h), h.host)
