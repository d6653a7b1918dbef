"""A native client of the spatially distributed feature budget (tests/native/client_spread.c, plain C against the public headers) against the
Python mirror."""
import os
import subprocess

import numpy as np
import pytest

import np_spread as NP
import np_strongest as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIBDIR = os.path.join(ROOT, "vulkansift_amd", "lib")


def _build(src, out):
    cmd = ["gcc", "-O1", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(NATIVE, src), "-o", out, "-L" + LIBDIR, "-lvulkansift",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_spread_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_spread.c", str(tmp_path / "client_spread"))


def _fnv(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.gpu
def test_c_client_prints_the_python_mirrors_bits(vk, tmp_path):
    w, h, budget, cols, rows = 640, 480, 300, 8, 6
    img = vk.gen_synthetic_image(33, w, h)
    img.tofile(str(tmp_path / "a.raw"))
    exe = _build("client_spread.c", str(tmp_path / "client_spread"))
    r = subprocess.run([exe, str(tmp_path / "a.raw"), str(budget), str(cols), str(rows)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    with vk.Instance(vk.default_config(input_image_max_size=w * h)) as inst:
        inst.detectFeatures(img, 0)
        before = inst.downloadFeatures(0)
        inst.keepStrongestFeaturesGrid(0, 1, budget, w, h, cols, rows)
        after = inst.downloadFeatures(0)
    want = NP.selected_records(np.ascontiguousarray(before).view(np.uint8).reshape(-1, NS.REC), budget, w, h, cols, rows)
    assert len(before) > budget and np.ascontiguousarray(after).tobytes() == want.tobytes()
    assert want.tobytes() != NS.selected_records(np.ascontiguousarray(before).view(np.uint8).reshape(-1, NS.REC), budget).tobytes()
    assert f[0] == "spread" and [int(f[2]), int(f[4]), int(f[6])] == [len(before), budget, NS.REC]
    assert int(f[8], 16) == _fnv(want.tobytes()) and float(f[10]) == -1.0 and float(f[12]) == -1.0
