"""A native client of the view index and camera refinement entry points (tests/native/client_cameras.c, plain C against the public headers) against the
Python mirror."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import track_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIBDIR = os.path.join(ROOT, "vulkansift_amd", "lib")


def _build(src, out):
    cmd = ["gcc", "-O1", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(NATIVE, src), "-o", out, "-L" + LIBDIR, "-lvulkansift",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cameras_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the new declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_cameras.c", str(tmp_path / "client_cameras"))


@pytest.mark.gpu
def test_c_client_prints_the_python_mirrors_bits(vk, tmp_path):
    exe = _build("client_cameras.c", str(tmp_path / "client_cameras"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    cfg = vk.default_config(sift_buffer_count=16, input_image_max_size=192 * 144)
    cameras = np.zeros((16, 3, 4), np.float32)
    for v, (_, _, x0, y0) in enumerate(S.VIEWS):
        cameras[v] = [[256, 0, 0, -256 * (x0 + 0.125 * v)], [0, 256, 0, -256 * (y0 - 0.0625 * v)], [0, 0, 1, 0]]
    with vk.Instance(cfg, batch_capacity=15) as inst:
        for v, img in enumerate(S.images(vk.gen_synthetic_image_family)):
            inst.detectFeatures(img, v)
        inst.matchFeaturesFiltered(S.IDS_A, S.IDS_B, 0.8, True)
        inst.buildTracks(vk.TRACKS_FILTERED)
        inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)
        inst.triangulateTracks(cameras, 2.0, 1.0)
        inst.indexObservationsByView()
        st = inst.getViewStats()
        crc = zlib.crc32(inst.downloadViewObservations().tobytes(), zlib.crc32(inst.downloadViewOffsets().tobytes()))
        want = ["index"] + [str(st[k]) for k in ("nb_views", "nb_observations", "largest_view")] + ["%08x" % crc]
        assert st["nb_views"] == 6 and st["nb_observations"] > 0
        for name, steps in (("first", 4), ("second", 2)):
            if name == "second":
                inst.triangulateTracks(cameras, 2.0, 1.0)
            inst.refineCameras(steps)
            st, rec = inst.getCameraStats(), inst.downloadRefinedCameras()
            want += [name] + [str(st[k]) for k in ("nb_views", "nb_refined", "nb_unchanged", "nb_failed")] + ["%08x" % zlib.crc32(rec.tobytes())]
            assert st["nb_views"] == 6, name
            cameras[:6] = rec["P"][:6].reshape(-1, 3, 4)
    # cameras index nb_views nb_observations largest_view crc first nb_views nb_refined nb_unchanged nb_failed crc second ...
    assert f == ["cameras"] + want
