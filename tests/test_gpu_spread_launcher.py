"""vksift_hip_keep_grid called directly on the cases of tests/hip_spread.py: one launch per case, one synchronisation, and a BYTE comparison of
the whole poisoned arena with what the contract of the header says — the kept records at the front of their sections, the counters on the
device and in the posted mirror, the matcher-cache entry of every buffer the launch selects from, and every other byte as it went in: guards,
gaps between the buffers, buffers and cache entries that are not named or hold no more than the budget, rows beyond the capacities, stride
padding. The only bytes not compared are the stale records the contract leaves unspecified (hip_spread.Spread.masked).
tests/test_np_spread.py pins the specification and the case table on the CPU."""
import pytest

import hip_records as HR
import hip_spread as HG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(vk):
    import ctypes as C

    import torch

    assert torch.cuda.is_available()
    L = HR.bind(vk.lib())
    vp, hp, fp, w, q = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32, C.c_uint64
    L.vksift_hip_keep_grid.argtypes = [vp, q, hp, w, w, hp, hp, hp, vp, w, vp, w, w, w, fp, fp, w, vp, q, vp, q, vp, w, vp]
    L.vksift_hip_keep_grid.restype = C.c_int
    return L


@pytest.mark.parametrize("case", HG.CASES, ids=lambda c: c["name"])
def test_keep_grid(L, case):
    h = HG.Spread(case)
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    h.check(h.masked(h.read()))


@pytest.mark.parametrize("name,changes", HG.REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else " ".join(f"{k}={x}" for k, x in v.items()))
def test_refusals(L, name, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed"""
    h = HG.Spread(HG.case_named(name))
    changes = {k: (HR.host_words([1] * 20) if v == "given" else v) for k, v in changes.items()}
    rc = h.launch(L, **changes)
    assert rc == HR.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(h.read(), h.host)
