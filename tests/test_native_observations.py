"""A native client of the observation entry points (tests/native/client_observations.c, plain C against the public headers) against the Python mirror."""
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


def test_observations_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the observation declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_observations.c", str(tmp_path / "client_observations"))


@pytest.mark.gpu
def test_c_client_prints_the_python_mirrors_bits(vk, tmp_path):
    exe = _build("client_observations.c", str(tmp_path / "client_observations"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    want = []
    cfg = vk.default_config(sift_buffer_count=16, input_image_max_size=192 * 144)
    with vk.Instance(cfg, batch_capacity=15) as inst:
        for v, img in enumerate(S.images(vk.gen_synthetic_image_family)):
            inst.detectFeatures(img, v)
        inst.matchFeaturesFiltered(S.IDS_A, S.IDS_B, 0.8, True)
        inst.buildTracks(vk.TRACKS_FILTERED)
        for name, params in (("all", (2, 0, vk.OBS_KEEP_CONFLICTING)), ("consistent3", (3, 0, vk.OBS_DROP_CONFLICTING))):
            inst.selectTrackObservations(*params)
            st = inst.getObservationStats()
            crc = zlib.crc32(inst.downloadObservationOffsets().tobytes())
            crc = zlib.crc32(inst.downloadObservationTrackIds().tobytes(), crc)
            crc = zlib.crc32(inst.downloadObservations().tobytes(), crc)
            want += [name] + [str(st[k]) for k in ("nb_tracks", "nb_observations", "nb_rejected_length", "nb_rejected_conflicting")] + ["%08x" % crc]
            assert st["nb_tracks"] > 0 and st["nb_observations"] >= params[0] * st["nb_tracks"], name
    # observations all nb_tracks nb_observations nb_rejected_length nb_rejected_conflicting crc consistent3 ...
    assert f == ["observations"] + want
