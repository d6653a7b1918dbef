"""A native client of the track entry points (tests/native/client_tracks.c, plain C against the public headers) against the Python mirror."""
import os
import subprocess
import zlib

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


def test_tracks_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the track declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_tracks.c", str(tmp_path / "client_tracks"))


@pytest.mark.gpu
def test_c_client_prints_the_python_mirrors_bits(vk, tmp_path):
    exe = _build("client_tracks.c", str(tmp_path / "client_tracks"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    want = []
    cfg = vk.default_config(sift_buffer_count=16, input_image_max_size=192 * 144)
    with vk.Instance(cfg, batch_capacity=15) as inst:
        for v, img in enumerate(S.images(vk.gen_synthetic_image_family)):
            inst.detectFeatures(img, v)
        inst.matchFeaturesFiltered(S.IDS_A, S.IDS_B, 0.8, True)
        inst.verifyHomography(1024, 2.5, 42)
        for name, source in (("filtered", vk.TRACKS_FILTERED), ("verified_h", vk.TRACKS_VERIFIED_H)):
            inst.buildTracks(source)
            st = inst.getTrackStats()
            crc = zlib.crc32(inst.downloadTracks().tobytes())
            for b in range(6):
                crc = zlib.crc32(inst.downloadFeatureTracks(b).tobytes(), crc)
            want += [name] + [str(st[k]) for k in ("nb_tracks", "nb_conflicting", "nb_features", "nb_edges")] + ["%08x" % crc]
            assert st["nb_tracks"] > 20 and st["nb_edges"] > 100, name
    # tracks filtered nb_tracks nb_conflicting nb_features nb_edges crc verified_h ...
    assert f == ["tracks"] + want
