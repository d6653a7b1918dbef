"""A native client of the RootSIFT conversion (tests/native/client_rootsift.c, plain C against the public headers) against the Python mirror."""
import os
import subprocess

import numpy as np
import pytest

import np_rootsift as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIBDIR = os.path.join(ROOT, "vulkansift_amd", "lib")


def _build(src, out):
    cmd = ["gcc", "-O1", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(NATIVE, src), "-o", out, "-L" + LIBDIR, "-lvulkansift",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_rootsift_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_rootsift.c", str(tmp_path / "client_rootsift"))


def _fnv(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.gpu
def test_c_client_prints_the_python_mirrors_bits(vk, tmp_path):
    w, h = 640, 480
    img = vk.gen_synthetic_image(33, w, h)
    img.tofile(str(tmp_path / "a.raw"))
    exe = _build("client_rootsift.c", str(tmp_path / "client_rootsift"))
    r = subprocess.run([exe, str(tmp_path / "a.raw")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    with vk.Instance(vk.default_config(input_image_max_size=w * h)) as inst:
        inst.detectFeatures(img, 0)
        before = np.ascontiguousarray(inst.downloadFeatures(0)).view(np.uint8).reshape(-1, RS.REC)
        inst.convertToRootSift(0, 1)
        after = np.ascontiguousarray(inst.downloadFeatures(0)).view(np.uint8).reshape(-1, RS.REC)
    want = RS.convert_records(before)
    assert len(before) > 100 and after.tobytes() == want.tobytes() and want.tobytes() != before.tobytes()
    assert f[0] == "rootsift" and [int(f[2]), int(f[4]), int(f[6])] == [len(before), len(before), RS.REC]
    assert int(f[8], 16) == _fnv(want.tobytes()) and int(f[10], 16) == _fnv(before.tobytes()) and float(f[12]) == -1.0
