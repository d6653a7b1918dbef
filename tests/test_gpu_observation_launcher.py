"""The observation launcher of include/vksift_hip.h called directly — vksift_hip_build_tracks, then vksift_hip_track_observations on what it left — on the
cases of tests/track_cases.py, not only through vksift_ext_selectTrackObservations, which fixes the strides, the tables and the layouts. Each run: one
launch sequence, one synchronisation, and a BYTE comparison of the whole poisoned arena (tests/hip_observations.py) with the restatement
(tests/np_observations.py): the four statistics, the offsets, the track ids and the observations must be there, and every other byte — guards, the words
behind offsets[nb_tracks], records beyond nb_observations, the SIFT buffers, the tables — must come back as it went in; the arena of the track build
(the launch's inputs) comes back byte for byte too. Nothing is compared with a tolerance. The buffers of a case are dense, sectioned and sectioned with
clamped sections in turn (hip_observations.buffer_layout), every stored record with a float pattern of its own."""
import itertools

import numpy as np
import pytest

import hip_observations as HO
import hip_tracks as HT
import np_observations as NO
from hip_records import Launch
import track_cases as TC

pytestmark = pytest.mark.gpu

# both policies, min_length 2 / 3, max_length 0 / 2 / 3 ((3, 2) is refused by the contract: test_refusals)
GRID = [(mn, mx, c) for mn, mx, c in itertools.product((2, 3), (0, 2, 3), (NO.KEEP_CONFLICTING, NO.DROP_CONFLICTING)) if NO.args_valid(mn, mx, c)]


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HO.bind(HT.bind(vk.lib()))


def built(L, case):
    """the case's tracks on the device, checked against their own restatement"""
    t = HT.Tracks(case)
    rc = t.launch(L)
    assert rc == 0, f"{t.what}: returned {rc}"
    t.check(t.read())
    return t


def run(L, t, *params):
    before = Launch.read(t)
    h = HO.Observations(t, *params)
    assert L.vksift_hip_observations_scratch_u32(h.nbufs, h.stride, h.max_rows) == h.scratch_u32      # exactly the words the library asks for
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    after = h.read()
    h.check(after)
    assert np.array_equal(Launch.read(t), before), f"{h.what}: the launch changed its inputs"
    return h, after


@pytest.mark.parametrize("case", TC.all_cases(), ids=lambda c: c["name"])
def test_track_observations(L, case):
    t = built(L, case)
    for params in GRID:
        run(L, t, *params)


def test_layouts_and_counts_above_max_rows(L):
    """the fixture's precondition: positions come from a dense buffer and from a buffer whose sections are clamped (cap < found), the row count on the
    device exceeds max_rows, and observations of all of them are selected"""
    t = built(L, TC.case_by_name("chain of three"))
    h, after = run(L, t, 2, 0, NO.KEEP_CONFLICTING)
    obs = h.view(after, h.obs)[:16 * 3].view(NO.OBSERVATION_DTYPE)
    assert obs["gpu_buffer_id"].tolist() == [0, 1, 2] and len({(float(o["x"]), float(o["y"])) for o in obs}) == 3
    assert HO.buffer_layout(0, 3)[0] is None and HO.buffer_layout(2, 3)[0][1] < HO.buffer_layout(2, 3)[0][2]       # dense; cap < found
    c = TC.case_by_name("counts above max_n and max_rows")
    assert max(n for _, n in c["bufs"]) > c["max_rows"]
    h, _ = run(L, built(L, c), 2, 0, NO.KEEP_CONFLICTING)
    assert h.restated()[0]["nb_observations"] > 0


def test_contention_two_digit_passes_and_repeat(L):
    """one track of about 32 000 members across every block boundary plus 2 048 short ones (two digit passes); a second launch into fresh memory gives
    identical bytes"""
    case = TC.contention_case()
    rec, _, stats = TC.expected(case)
    assert stats["nb_tracks"] > 2000 and rec["length"].max() > 16 * 2048 * 0.9 and 255 < 16 * 4096 // 2 < 65536
    t = built(L, case)
    h1, a1 = run(L, t, 2, 0, NO.KEEP_CONFLICTING)
    h2, a2 = run(L, t, 2, 0, NO.KEEP_CONFLICTING)
    for x, y in zip(h1.outputs(a1), h2.outputs(a2)):
        assert np.array_equal(x, y)
    run(L, t, 3, 0, NO.DROP_CONFLICTING)           # the giant track is conflicting: dropped, with every two-member track


def test_third_digit(L):
    """70 000 two-member tracks over two buffers of 70 000 rows: new numbers above 65 535"""
    n = 70000
    rows = np.arange(n, dtype=np.uint32)
    case = TC.case("70000 two-member tracks", [(0, n), (1, n)], [TC.pair(0, 1, np.stack([rows, rows[::-1]], axis=1))], rec_extra=0)
    h, _ = run(L, built(L, case), 2, 0, NO.KEEP_CONFLICTING)
    stats = h.restated()[0]
    assert stats["nb_tracks"] == n > 65535 and stats["nb_observations"] == 2 * n


REFUSALS = [dict(nbufs=0), dict(max_rows=0), dict(max_rows=1000), dict(node_stride=0x80000000), dict(min_length=1), dict(min_length=0), dict(min_length=3, max_length=2),
            dict(conflicts=2), {"+tracks": 2}, {"+feats_base": 2}, {"+buf_stride": 2}, {"+observations": 4}, {"+scratch": 4}, {"+tracks_cap": -1}, {"+obs_cap": -1},
            {"+scratch_u32": -1}]


@pytest.mark.parametrize("changes", REFUSALS, ids=lambda d: " ".join(f"{k}={x}" for k, x in d.items()))
def test_refusals(L, changes):
    """hipErrorInvalidValue, and not a byte of either arena changed (the scratch included)"""
    t = built(L, TC.hand_cases()[2])
    before = Launch.read(t)
    h = HO.Observations(t)
    rc = h.launch(L, **changes)
    assert rc == HO.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(Launch.read(h), h.host)
    assert np.array_equal(Launch.read(t), before)
