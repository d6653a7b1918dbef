"""The record-moving launchers of include/vksift_hip.h called directly — vksift_hip_gather_descriptors, _shifted_norms, _gather_sections,
_pack_features, _filter_matches, _gather_correspondences, _gather_xy — on the cases of tests/record_cases.py, not only on the section tables,
distances, strides and slot orders a detection or a matching happens to produce. Each case: one launch, one synchronisation, and a BYTE
comparison of the whole poisoned arena (tests/hip_records.py) with the numpy restatement (tests/np_records.py): what the contract says is
written must be there, and every other byte — guards, gaps between buffers, cache entries of buffers not named, rows at and beyond the
written count, stride padding — must come back as it went in. All seven launches are exact: nothing is compared with a tolerance.
tests/test_np_records.py pins the reference and asserts on the CPU which edge each case reaches."""
import pytest

import hip_records as HR
import record_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HR.bind(vk.lib())


def run(L, launch, case):
    h = HR.LAUNCHES[launch](case)
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    h.check(h.read())


ids = lambda c: c["name"]


@pytest.mark.parametrize("case", RC.GATHER_DESC, ids=ids)
def test_gather_descriptors(L, case):
    run(L, "gather_descriptors", case)


@pytest.mark.parametrize("case", RC.NORMS, ids=ids)
def test_shifted_norms(L, case):
    run(L, "shifted_norms", case)


@pytest.mark.parametrize("case", RC.SECTIONS, ids=ids)
def test_gather_sections(L, case):
    run(L, "gather_sections", case)


@pytest.mark.parametrize("case", RC.PACK, ids=ids)
def test_pack_features(L, case):
    run(L, "pack_features", case)


@pytest.mark.parametrize("case", RC.FILTER, ids=ids)
def test_filter_matches(L, case):
    run(L, "filter_matches", case)


@pytest.mark.parametrize("case", RC.CORR, ids=ids)
def test_gather_correspondences(L, case):
    run(L, "gather_correspondences", case)


@pytest.mark.parametrize("case", RC.XY, ids=ids)
def test_gather_xy(L, case):
    run(L, "gather_xy", case)


@pytest.mark.parametrize("launch,name,changes", RC.REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else " ".join(f"{k}={x}" for k, x in v.items()))
def test_refusals(L, launch, name, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HR.LAUNCHES[launch](RC.case_named(launch, name))
    rc = h.launch(L, **changes)
    assert rc == HR.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(h.read(), h.host)
