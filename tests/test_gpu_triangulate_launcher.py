"""The triangulation launcher of include/vksift_hip.h called directly — vksift_hip_triangulate_tracks on the cases of tests/hip_triangulate.py, not only
through vksift_ext_triangulateTracks, which fixes the capacities and feeds it a table the selection built. Each run: one launch sequence, one
synchronisation, and a BYTE comparison of the whole poisoned arena with the restatement (tests/np_triangulate.py): the points and the four statistics must
be there, and every other byte — guards, the points at and beyond the track count, the words behind the statistics, and the inputs: offsets, observations,
the table's counts, the cameras — must come back as it went in. Nothing is compared with a tolerance."""
import numpy as np
import pytest

import hip_triangulate as HT
import np_triangulate as NT
from hip_records import Launch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HT.bind(vk.lib())


def run(L, case):
    h = HT.Triangulate(case)
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    after = h.read()
    h.check(after)
    return h, after


@pytest.mark.parametrize("case", HT.cases(), ids=lambda c: c["name"])
def test_triangulate_tracks(L, case):
    run(L, case)


def test_every_status_occurs(L):
    """the fixture's precondition, on what the device wrote: each flag alone, BEHIND + ERROR together, TOO_LONG, and both sides of the angle limit"""
    h, after = run(L, HT.case_by_name("every status"))
    got = h.view(after, h.points)[:HT.POINT_BYTES * len(HT.status_tracks())].view(NT.POINT_DTYPE)
    assert got["status"].tolist() == [s for _, _, s in HT.status_tracks()]
    h, after = run(L, HT.case_by_name("1024 members and 1025 (TOO_LONG)"))
    got = h.view(after, h.points)[:HT.POINT_BYTES * 3].view(NT.POINT_DTYPE)
    assert got["status"].tolist() == [0, NT.TOO_LONG, 0] and got["nb_observations"].tolist() == [1024, 1025, 3]
    h, after = run(L, HT.case_by_name("angle test that splits the case"))
    got = h.view(after, h.points)[:HT.POINT_BYTES * 3].view(NT.POINT_DTYPE)
    assert got["status"].tolist() == [NT.ANGLE, 0, 0]
    h, after = run(L, HT.case_by_name("cameras beyond nb_cameras"))
    got = h.view(after, h.points)[:HT.POINT_BYTES * 3].view(NT.POINT_DTYPE)
    assert got["status"].tolist() == [0, NT.DEGENERATE, NT.DEGENERATE]


def test_second_launch_into_fresh_memory_gives_identical_bytes(L):
    for name in ("every length at a boundary", "1024 members and 1025 (TOO_LONG)"):
        h1, a1 = run(L, HT.case_by_name(name))
        h2, a2 = run(L, HT.case_by_name(name))
        for x, y in zip(h1.outputs(a1), h2.outputs(a2)):
            assert np.array_equal(x, y)


REFUSALS = [dict(offsets=None), dict(observations=None), dict(obs_stats=None), dict(cameras=None), dict(points=None), dict(stats=None), dict(nb_cameras=0),
            dict(points_cap=0), dict(points_cap=1 << 31), dict(t2=0.0), dict(t2=-1.0), dict(t2=float("inf")), dict(t2=float("nan")),
            dict(cos_min_angle=float("nan")), {"+offsets": 2}, {"+obs_stats": 2}, {"+stats": 2}, {"+observations": 4}, {"+cameras": 4}, {"+points": 4}]


@pytest.mark.parametrize("changes", REFUSALS, ids=lambda d: " ".join(f"{k}={x}" for k, x in d.items()))
def test_refusals(L, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HT.Triangulate(HT.case_by_name("every status"))
    rc = h.launch(L, **changes)
    assert rc == HT.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(Launch.read(h), h.host)
