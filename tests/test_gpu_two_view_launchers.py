"""The two-view launchers of include/vksift_hip.h called directly — vksift_hip_ransac_homography, _ransac_fundamental, _refit_homography,
_refit_fundamental, _match_guided — on the cases of tests/two_view_cases.py, not only through the three wrappers of vulkansift_amd/api.py, which
fix the strides, the slot table and the counters. Each case: one launch sequence, one synchronisation, and a BYTE comparison of the whole
poisoned arena (tests/hip_two_view.py) with the numpy restatements (np_verify, np_verify_f, np_refine, np_refine_f, np_guided): what the header
says is written must be there, and every other byte — guards, stride padding, rows and decoys beyond n, records beyond nslots, mask bytes at
and beyond n, output rows at and beyond out_n, the key scratch of a guided slot that is not valid — must come back as it went in. All five
launches are specified bit for bit: nothing is compared with a tolerance. Only the scratch payload the header leaves unspecified is not
compared. tests/test_two_view_cases.py pins on the CPU which edge each case reaches."""
import pytest

import hip_two_view as HT
import two_view_cases as T

pytestmark = pytest.mark.gpu

checked = {launch: 0 for launch in T.CASES}
refused = 0


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HT.bind(vk.lib())


def run(L, launch, case):
    h = HT.LAUNCHES[launch](case)
    asks = L.vksift_hip_guided_scratch_u32 if launch == "match_guided" else L.vksift_hip_ransac_scratch_u32 if launch.startswith("ransac") else None
    if asks is not None:    # exactly the words the library asks for
        assert asks(h.ns, case["max_n"] if launch == "match_guided" else case["nb_hyp"]) == h.scratch_u32
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    h.check(h.read())
    checked[launch] += 1


ids = lambda c: c["name"]


@pytest.mark.parametrize("case", T.RANSAC["h"], ids=ids)
def test_ransac_homography(L, case):
    run(L, "ransac_homography", case)


@pytest.mark.parametrize("case", T.RANSAC["f"], ids=ids)
def test_ransac_fundamental(L, case):
    run(L, "ransac_fundamental", case)


@pytest.mark.parametrize("case", T.REFIT["h"], ids=ids)
def test_refit_homography(L, case):
    run(L, "refit_homography", case)


@pytest.mark.parametrize("case", T.REFIT["f"], ids=ids)
def test_refit_fundamental(L, case):
    run(L, "refit_fundamental", case)


@pytest.mark.parametrize("case", T.GUIDED, ids=ids)
def test_match_guided(L, case):
    run(L, "match_guided", case)


@pytest.mark.parametrize("launch,name,changes", T.REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else " ".join(f"{k}={x}" for k, x in v.items()))
def test_refusals(L, launch, name, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed (the scratch included)"""
    global refused
    h = HT.LAUNCHES[launch](T.case_named(T.CASES[launch], name))
    rc = h.launch(L, **changes)
    assert rc == HT.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(HT.Launch.read(h), h.host)
    refused += 1


def test_every_case_was_run(request):
    """no case left out: when the module runs as a whole, every case of every table was launched and compared (a run of a selection, as with
    -k, asserts nothing here)"""
    mine = [i for i in request.session.items if getattr(i, "module", None) is request.module]
    if len(mine) != sum(len(c) for c in T.CASES.values()) + len(T.REFUSALS) + 1:
        assert len(mine) < sum(len(c) for c in T.CASES.values()) + len(T.REFUSALS) + 1
        return
    assert checked == {launch: len(cases) for launch, cases in T.CASES.items()}
    assert refused == len(T.REFUSALS)
