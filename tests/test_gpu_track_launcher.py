"""The track launcher of include/vksift_hip.h called directly — vksift_hip_build_tracks — on the cases of tests/track_cases.py, not only through
vksift_ext_buildTracks, which fixes the strides, the tables and the counters. Each case: one launch sequence, one synchronisation, and a BYTE comparison
of the whole poisoned arena (tests/hip_tracks.py) with the restatement (tests/np_tracks.py): the four statistics, the track records and the words of the
stored rows must be there, and every other byte — guards, stride padding, the words of rows that are not stored, records beyond nb_tracks, the words
behind the statistics — must come back as it went in. Nothing is compared with a tolerance. Every case runs from records with their own count and from
records with a mask. tests/test_np_tracks.py pins on the CPU what each hand case contains."""
import numpy as np
import pytest

import hip_tracks as HT
from hip_records import Launch
import track_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HT.bind(vk.lib())


def run(L, case):
    h = HT.Tracks(case)
    assert L.vksift_hip_tracks_scratch_u32(h.nbufs, h.stride) == h.scratch_u32      # exactly the words the library asks for
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    after = h.read()
    h.check(after)
    return h, after


@pytest.mark.parametrize("case", TC.all_cases(), ids=lambda c: c["name"])
def test_build_tracks(L, case):
    run(L, case)


@pytest.fixture(scope="module")
def contention():
    c = TC.contention_case()
    return c, TC.as_masked(c)


@pytest.mark.parametrize("form", [0, 1], ids=["own count", "masked"])
def test_contention_and_repeat(L, contention, form):
    """several hundred workgroups race for a few roots; a second launch into fresh memory gives identical bytes"""
    case = contention[form]
    rec, _, stats = TC.expected(case)
    assert stats["nb_tracks"] > 2000 and rec["length"].max() > 16 * 2048 * 0.9 and stats["nb_edges"] == 32 * 4096
    h1, a1 = run(L, case)
    h2, a2 = run(L, case)
    for x, y in zip(h1.outputs(a1), h2.outputs(a2)):
        assert np.array_equal(x, y)


REFUSALS = [dict(nslots=0), dict(nbufs=0), dict(max_n=0), dict(max_rows=0), dict(max_rows=1000), dict(n_stride=0), dict(slot_tab_stride=1), {"+records": 2},
            {"+rec_slot_stride": 2}, {"+tracks": 2}, {"+scratch": 4}, dict(rec_slot_stride=12), dict(tracks_cap=0), {"+scratch_u32": -1}, dict(node_stride=0x80000000)]


@pytest.mark.parametrize("changes", REFUSALS, ids=lambda d: " ".join(f"{k}={x}" for k, x in d.items()))
def test_refusals(L, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed (the scratch included)"""
    h = HT.Tracks(TC.hand_cases()[2])
    rc = h.launch(L, **changes)
    assert rc == HT.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(Launch.read(h), h.host)


def test_masked_refusals(L):
    h = HT.Tracks(TC.as_masked(TC.hand_cases()[2]))
    for changes in (dict(valid_stride=0), dict(mask_slot_stride=1)):
        assert h.launch(L, **changes) == HT.HIP_ERROR_INVALID_VALUE, changes
    h.check(Launch.read(h), h.host)
