"""vksift_hip_place_keypoints called directly on the cases of tests/hip_place.py: one launch per case, one synchronisation, and a BYTE comparison
of the whole poisoned arena with what the contract of the header says — words 0..8 of the stored records in input order, the un-clamped
counter of every octave of every image, the placed words, and every other byte as it went in: bytes 36..163 of every record, the canary
records at and beyond every capacity, the gaps between the images' buffers, the words beside the counters, the guards.
tests/test_np_describe.py pins the specification on the CPU."""
import pytest

import hip_place as HPL
import hip_records as HR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HPL.bind(vk.lib())


@pytest.mark.parametrize("case", HPL.CASES, ids=lambda c: c["name"])
def test_place_keypoints(L, case):
    h = HPL.Place(case)
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    h.check(h.read())


@pytest.mark.parametrize("name,changes", HPL.REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else " ".join(f"{k}={x}" for k, x in v.items()))
def test_refusals(L, name, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HPL.Place(HPL.case_named(name))
    rc = h.launch(L, **changes)
    assert rc == HR.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(h.read(), h.host)
