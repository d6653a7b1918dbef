"""The kernels of tracks.hip hold a handful of indices per lane: no scratch memory and no spilled register in any of them (CPU: hipcc cross-compiles).
Resource metadata of the code object only — and the build lists, the headers, the built library and the Python interface carry the new entries."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_tracks_init", "k_tracks_hook", "k_tracks_flatten", "k_tracks_presence", "k_tracks_fold", "k_tracks_scan", "k_tracks_number", "k_tracks_label")
EXT = ("vksift_ext_buildTracks", "vksift_ext_getTrackStats", "vksift_ext_downloadTracks", "vksift_ext_downloadFeatureTracks", "vksift_ext_getTracksTime")
HIP = ("vksift_hip_build_tracks", "vksift_hip_tracks_scratch_u32")


def test_track_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/tracks.hip" in b.HIP_SRCS and "host/vksift_tracks.c" in b.HOST_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "tracks.hip")
    out = str(tmp_path / "tracks.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/tracks.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    assert len(meta) == len(KERNELS), sorted(meta)
    for k in KERNELS:
        hits = [v for name, v in meta.items() if k in name]
        assert len(hits) == 1, (k, sorted(meta))
        lds, scratch, vgpr, spill = hits[0]
        print(k, ": lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
        assert scratch == 0 and spill == 0, (k, scratch, spill)
        # far below the 128 at which a 256-thread workgroup would start to cost occupancy (64 for the scan's single workgroup of 1024)
        assert vgpr <= 64, (k, vgpr)


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(vksift_[A-Za-z0-9_]+)\s*\(", txt))


def test_headers_declare_and_the_library_exports_the_entries(vk):
    assert set(EXT) <= _declared("vksift_ext.h")
    assert set(HIP) <= _declared("vksift_hip.h")
    L = vk.lib()
    for fn in EXT + HIP:
        assert hasattr(L, fn), fn
    assert L.vksift_hip_abi_version() >= 12
    for m in ("buildTracks", "getTrackStats", "downloadTracks", "downloadFeatureTracks", "getTracksTime"):
        assert hasattr(vk.Instance, m), m
    assert vk.NO_TRACK == 0xFFFFFFFF and vk.TRACK_DTYPE.itemsize == 16 and vk.TRACK_STATS_DTYPE.itemsize == 16
    assert (vk.TRACKS_FILTERED, vk.TRACKS_VERIFIED_H, vk.TRACKS_VERIFIED_F, vk.TRACKS_REFINED_H, vk.TRACKS_REFINED_F, vk.TRACKS_GUIDED) == (0, 1, 2, 3, 4, 5)
