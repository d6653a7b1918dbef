"""A native client of the edge store entry points (tests/native/client_track_edges.c, plain C against the public headers) against the Python mirror."""
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


def test_track_edges_client_compiles_and_links(vk, tmp_path):
    """gcc accepts the edge store declarations of vksift_ext.h as C11 and libvulkansift.so exports what the client uses (no GPU needed)"""
    _build("client_track_edges.c", str(tmp_path / "client_track_edges"))


def _tracks(inst):
    st = inst.getTrackStats()
    crc = zlib.crc32(inst.downloadTracks().tobytes())
    for b in range(6):
        crc = zlib.crc32(inst.downloadFeatureTracks(b).tobytes(), crc)
    return [str(st[k]) for k in ("nb_tracks", "nb_conflicting", "nb_features", "nb_edges")] + ["%08x" % crc]


@pytest.mark.gpu
def test_c_client_prints_the_python_mirrors_bits(vk, tmp_path):
    exe = _build("client_track_edges.c", str(tmp_path / "client_track_edges"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.strip().splitlines()[-1].split()
    cfg = vk.default_config(sift_buffer_count=16, input_image_max_size=192 * 144)
    with vk.Instance(cfg, batch_capacity=4) as inst:
        for v, img in enumerate(S.images(vk.gen_synthetic_image_family)):
            inst.detectFeatures(img, v)
        inst.beginTrackAccumulation(1 << 16)
        for first in range(0, 15, 4):
            inst.matchFeaturesFiltered(S.IDS_A[first:first + 4], S.IDS_B[first:first + 4], 0.8, True)
            inst.accumulateTrackEdges(vk.TRACKS_FILTERED)
        es = inst.getTrackEdgeStats()
        want = ["edges"] + [str(es[k]) for k in ("nb_edges", "nb_dropped", "nb_calls", "nb_changed_buffers")] + ["%08x" % zlib.crc32(inst.downloadTrackEdges().tobytes())]
        inst.buildTracksAccumulated()
        accumulated = _tracks(inst)
        assert es["nb_calls"] == 4 and es["nb_dropped"] == 0 and es["nb_edges"] > 100 and inst.getTrackStats()["nb_tracks"] > 20
    # edges nb_edges nb_dropped nb_calls nb_changed_buffers crc tracks accumulated nb_tracks nb_conflicting nb_features nb_edges crc
    assert f == want + ["tracks", "accumulated"] + accumulated
    with vk.Instance(cfg, batch_capacity=15) as inst:             # all pairs at once: the plain build gives the bytes the client's chunked one gave
        for v, img in enumerate(S.images(vk.gen_synthetic_image_family)):
            inst.detectFeatures(img, v)
        inst.matchFeaturesFiltered(S.IDS_A, S.IDS_B, 0.8, True)
        inst.buildTracks(vk.TRACKS_FILTERED)
        assert _tracks(inst) == accumulated
