"""A native client of the fundamental-matrix refinement entry points (tests/native/client_refine_f.c, plain C against the public headers) against the Python mirror."""
import os
import subprocess

import numpy as np
import pytest

import quality as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIBDIR = os.path.join(ROOT, "vulkansift_amd", "lib")


def _build(src, out):
    cmd = ["gcc", "-O1", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(NATIVE, src), "-o", out, "-L" + LIBDIR, "-lvulkansift",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_refine_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the refinement declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_refine_f.c", str(tmp_path / "client_refine_f"))


def _fnv(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.gpu
def test_c_client_prints_the_python_mirrors_bits(vk, tmp_path):
    w, h = 640, 480
    img1 = vk.gen_synthetic_image(33, w, h)
    img2 = Q.warp(img1, Q.homography(w, h))
    img1.tofile(str(tmp_path / "a.raw"))
    img2.tofile(str(tmp_path / "b.raw"))
    exe = _build("client_refine_f.c", str(tmp_path / "client_refine_f"))
    r = subprocess.run([exe, str(tmp_path / "a.raw"), str(tmp_path / "b.raw")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    with vk.Instance(vk.default_config(input_image_max_size=w * h)) as inst:
        inst.detectFeatures(img1, 0)
        inst.detectFeatures(img2, 1)
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        inst.verifyFundamental(16, 2.5, 42)
        inst.refineFundamental(3, 2.5)
        fun, ref, mask = inst.getFundamental(0), inst.getRefinedFundamental(0), inst.downloadRefinedFundamentalInlierMask(0)
    assert f[0] == "refined" and [int(x, 16) for x in f[1:10]] == [int(x) for x in ref["F"].reshape(9).view(np.uint32)]
    assert int(ref["valid"]) == 1 and int(ref["nb_inliers"]) > 100
    assert [int(f[11]), int(f[12]), int(f[14]), int(f[15]), int(f[17]), int(f[19]), int(f[21])] == [len(mask), int(ref["nb_matches"]), int(ref["nb_inliers"]), int(mask.sum()),
                                                                                                  int(fun["nb_inliers"]), int(ref["rounds"]), 1]
    assert int(f[23], 16) == _fnv(mask.astype(np.uint8).tobytes())
