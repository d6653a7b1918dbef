"""The kernels of observations.hip hold a few indices per lane: no scratch memory and no spilled register in any of them (CPU: hipcc cross-compiles).
Resource metadata of the code object only — and the build lists, the headers, the built library and the Python interface carry the new entries."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_obs_select", "k_obs_totals", "k_obs_scan", "k_obs_number", "k_obs_xy", "k_obs_keys", "k_obs_hist", "k_obs_scatter", "k_obs_expand")
EXT = ("vksift_ext_selectTrackObservations", "vksift_ext_getObservationStats", "vksift_ext_downloadObservationOffsets", "vksift_ext_downloadObservationTrackIds",
       "vksift_ext_downloadObservations", "vksift_ext_getObservationsTime")
HIP = ("vksift_hip_track_observations", "vksift_hip_observations_scratch_u32")


def test_observation_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/observations.hip" in b.HIP_SRCS and "host/vksift_observations.c" in b.HOST_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "observations.hip")
    out = str(tmp_path / "observations.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/observations.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    assert len(meta) == len(KERNELS), sorted(meta)
    for k in KERNELS:
        hits = [v for name, v in meta.items() if re.search(k + r"E", name)]      # (the mangled name: k_obs_scan is no prefix of another kernel's)
        assert len(hits) == 1, (k, sorted(meta))
        lds, scratch, vgpr, spill = hits[0]
        print(k, ": lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
        assert scratch == 0 and spill == 0, (k, scratch, spill)
        # far below the 128 at which a 256-thread workgroup would start to cost occupancy (64 for the scans' single workgroup of 1024)
        assert vgpr <= 64, (k, vgpr)
        assert lds <= 8192, (k, lds)        # the scatter's four digit tables and the block's bases: 5 KiB


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
    assert L.vksift_hip_abi_version() >= 13
    for m in ("selectTrackObservations", "getObservationStats", "downloadObservationOffsets", "downloadObservationTrackIds", "downloadObservations",
              "getObservationsTime"):
        assert hasattr(vk.Instance, m), m
    assert vk.OBSERVATION_DTYPE.itemsize == 16 and vk.OBSERVATION_STATS_DTYPE.itemsize == 16
    assert vk.OBSERVATION_DTYPE.names == ("gpu_buffer_id", "row", "x", "y") and (vk.OBS_KEEP_CONFLICTING, vk.OBS_DROP_CONFLICTING) == (0, 1)


def test_the_kernels_are_not_in_tracks_hip():
    txt = open(os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "tracks.hip")).read()
    assert "k_obs_" not in txt
