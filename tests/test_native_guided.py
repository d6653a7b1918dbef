"""A native client of the guided-matching entry points (tests/native/client_guided.c, plain C against the public headers) against the Python mirror."""
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


def test_guided_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the guided-matching declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_guided.c", str(tmp_path / "client_guided"))


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
    exe = _build("client_guided.c", str(tmp_path / "client_guided"))
    r = subprocess.run([exe, str(tmp_path / "a.raw"), str(tmp_path / "b.raw")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    inf = float("inf")
    with vk.Instance(vk.default_config(input_image_max_size=w * h)) as inst:
        inst.detectFeatures(img1, 0)
        inst.detectFeatures(img2, 1)
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        inst.verifyHomography(1024, 2.5, 42)
        inst.verifyFundamental(1024, 2.5, 42)
        nf = len(inst.downloadFilteredMatches(0))
        inst.matchFeaturesGuided(vk.GUIDE_HOMOGRAPHY, None, 2.5, 0.8, inf, True)
        gh = inst.downloadGuidedMatches(0)
        inst.matchFeaturesGuided(vk.GUIDE_FUNDAMENTAL, None, 2.5, 0.8, 250.0, False)
        gf = inst.downloadGuidedMatches(0)
        hom = inst.getHomography(0)
        own = np.asarray(hom["H"], np.float32).reshape(9).copy()
        own[2] += np.float32(0.5)
        inst.matchFeaturesGuided(vk.GUIDE_HOMOGRAPHY, own[None], 3.0, 0.9, inf, True)
        go = inst.downloadGuidedMatches(0)
    # guided filtered n homography n digest fundamental n digest own n digest valid v
    assert f[0] == "guided" and f[1] == "filtered" and int(f[2]) == nf
    for at, name, m in ((3, "homography", gh), (6, "fundamental", gf), (9, "own", go)):
        assert f[at] == name and int(f[at + 1]) == len(m) and int(f[at + 2], 16) == _fnv(m.tobytes()), name
    assert int(f[13]) == int(hom["valid"]) == 1 and len(gh) > 100 and len(gf) > 100
