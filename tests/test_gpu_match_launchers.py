"""The matcher launchers of include/vksift_hip.h called directly — vksift_hip_match_2nn_prenormed, vksift_hip_match_2nn_desc,
vksift_hip_match_2nn_async — on the cases of tests/match_cases.py: every size regime of the host planner on its borders, the scratch at
exactly the documented minimum, index bases that wrap, cache entries named in any order, twice or not at all, strides with padding, decoy
rows behind every count, host-side bounds that differ from the device-side counts, more than 16 slots with a large reference set among
them. Each case: one launch, one synchronisation, and a BYTE comparison of the whole poisoned arena (tests/hip_match.py) with the numpy
restatement of the shader (tests/np_match.py): the N_A records and the two count words of every slot must be there, and every other
byte — guards, records at and beyond N_A, stride padding, the other words of a count stride, the cache, all inputs — must come back as it
went in. Scratch is unspecified inside its documented extent only. Everything is exact: nothing is compared with a tolerance.
tests/test_np_match.py pins the reference and asserts on the CPU which edge each case reaches."""
import os
import subprocess
import sys

import pytest

import hip_match as HM
import match_cases as MC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda c: c["name"] if isinstance(c, dict) else f"scratch 0x{c:02x}"
fills = pytest.mark.parametrize("fill", HM.FILLS, ids=ids)   # scratch poisoned and zeroed: each shows what the other hides (hip_match.MatchLaunch)


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HM.bind(vk.lib())


@fills
@pytest.mark.parametrize("case", MC.POINTER, ids=ids)
def test_prenormed(L, case, fill):
    HM.run(L, "match_2nn_prenormed", case, fill=fill)


@fills
@pytest.mark.parametrize("case", MC.POINTER, ids=ids)
def test_desc(L, case, fill):
    HM.run(L, "match_2nn_desc", case, fill=fill)


@fills
@pytest.mark.parametrize("case", MC.SCAN_FORM, ids=ids)
def test_prenormed_other_scan_form(L, case, fill):
    """the cell scan's four-wave form (VKSIFT_TUNE_SCAN_FORM = 1): twice the grid, 256-row blocks, 128-row tiles"""
    before = L.vksift_hip_tune_get(HM.TUNE_SCAN_FORM)
    assert L.vksift_hip_tune(HM.TUNE_SCAN_FORM, 1) == 0
    try:
        HM.run(L, "match_2nn_prenormed", case, fill=fill)
    finally:
        assert L.vksift_hip_tune(HM.TUNE_SCAN_FORM, before) == 0


@fills
@pytest.mark.parametrize("case", MC.ASYNC, ids=ids)
def test_async(L, case, fill):
    HM.run(L, "match_2nn_async", case, fill=fill)


@pytest.mark.parametrize("entry,name,changes", MC.REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else " ".join(f"{k}={x}" for k, x in v.items()))
def test_refusals(L, entry, name, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HM.LAUNCHES[entry](HM.case_named(entry, name))
    rc = h.launch(L, **changes)
    assert rc == HM.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check_untouched(h.read(), "refused")


@pytest.mark.parametrize("entry,name,changes", MC.NOTHING, ids=lambda v: str(v) if not isinstance(v, dict) else " ".join(f"{k}={x}" for k, x in v.items()))
def test_no_query_rows(L, entry, name, changes):
    """na == 0: returns 0, launches nothing, changes not a byte"""
    h = HM.LAUNCHES[entry](HM.case_named(entry, name))
    assert h.launch(L, **changes) == 0
    h.check_untouched(h.read(), "na == 0")


ended_badly = []   # the switch whose child did not end well (a signal, a time limit): no further child is started after it


@pytest.mark.parametrize("switch", list(MC.GROUPS))
def test_switch_group(switch):
    """VKSIFT_MATCH_PK=0 (the B-split and pruning kernels carry the batches) and VKSIFT_MATCH_SCAN=0 (the stream decomposition through the
    pointer entries): the switches are read once per process, so each group runs in a child of its own — one after the other, each under
    its own time limit, and none after one that did not end well (a child that found a difference exits with status 1: that is a result)"""
    assert not ended_badly, f"not started: the child of {ended_badly[0]}=0 did not end well"
    env = dict(os.environ)
    env[switch] = "0"
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hip_match.py"), switch], cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    except subprocess.TimeoutExpired:
        ended_badly.append(switch)
        raise
    if r.returncode not in (0, 1):
        ended_badly.append(switch)
    assert r.returncode == 0, f"{switch}=0: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("ok under") == len(MC.GROUPS[switch]) * len(HM.FILLS) * (1 if switch == "VKSIFT_MATCH_PK" else 2)
