"""vksift_hip_root_descriptors called directly on the cases of tests/hip_rootsift.py: one launch per case, one synchronisation, and a BYTE
comparison of the whole poisoned arena with what the contract of the header says — the descriptor bytes of every stored record of every named
buffer converted (tests/np_rootsift.py), the matcher-cache entry of each as vksift_hip_gather_sections would write it for the converted buffer,
and every other byte as it went in: head words, records at and beyond a section's count, counters, guards, gaps between the buffers, buffers and
cache entries that are not named, stride padding. tests/test_np_rootsift.py pins the specification, tests/test_rootsift_cases.py the case
table, both on the CPU."""
import pytest

import hip_records as HR
import hip_rootsift as HT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(vk):
    import ctypes as C

    import torch

    assert torch.cuda.is_available()
    L = HR.bind(vk.lib())
    vp, hp, w, q = C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64
    L.vksift_hip_root_descriptors.argtypes = [vp, q, hp, w, w, hp, hp, hp, vp, w, w, w, vp, q, vp, q, vp, w, vp]
    L.vksift_hip_root_descriptors.restype = C.c_int
    return L


def _run(L, case):
    h = HT.Root(case)
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    h.check(h.read())


@pytest.mark.parametrize("case", HT.CASES, ids=lambda c: c["name"])
def test_root_descriptors(L, case):
    _run(L, case)


def test_every_reachable_pair(L):
    """every (d, s) pair a row can hold, once at least (the case builder asserts the coverage): an estimate of the square root that is not
    corrected against the two inequalities fails here"""
    _run(L, HT.all_pairs_case())


@pytest.mark.parametrize("name,changes", HT.REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else " ".join(f"{k}={x}" for k, x in v.items()))
def test_refusals(L, name, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HT.Root(HT.case_named(name))
    changes = {k: (HR.host_words([1] * 20) if v == "given" else v) for k, v in changes.items()}
    rc = h.launch(L, **changes)
    assert rc == HR.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(h.read(), h.host)
