"""The kernels of track_edges.hip hold a handful of indices per lane: no scratch memory and no spilled register in any of them (CPU: hipcc cross-compiles).
Resource metadata of the code object only — and the build lists, the headers, the built library and the Python interface carry the new entries. What the
compile shows for gfx950 (VGPRs / LDS bytes): k_edges_count 6 / 256, k_edges_scan 20 / 144, k_edges_write 30 / 16, k_edges_hook 12 / 256: those are the bounds
below, far under the 128 VGPRs at which a 256-thread workgroup would start to cost occupancy (64 for the scan's single workgroup of 1024)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_edges_count": (6, 256), "k_edges_scan": (20, 144), "k_edges_write": (30, 16), "k_edges_hook": (12, 256)}          # VGPRs, LDS bytes
EXT = ("vksift_ext_beginTrackAccumulation", "vksift_ext_accumulateTrackEdges", "vksift_ext_getTrackEdgeStats", "vksift_ext_downloadTrackEdges",
       "vksift_ext_buildTracksAccumulated", "vksift_ext_getAccumulateTime")
HIP = ("vksift_hip_track_edges_scratch_u32", "vksift_hip_append_track_edges", "vksift_hip_build_tracks_from_edges")


def test_edge_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/track_edges.hip" in b.HIP_SRCS and "host/vksift_track_edges.c" in b.HOST_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "track_edges.hip")
    out = str(tmp_path / "track_edges.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/track_edges.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    assert len(meta) == len(KERNELS), sorted(meta)      # the file holds its own four kernels: init and the tail of a build stay in tracks.hip
    for k, (vgpr_bound, lds_bound) in KERNELS.items():
        hits = [v for name, v in meta.items() if k in name]
        assert len(hits) == 1, (k, sorted(meta))
        lds, scratch, vgpr, spill = hits[0]
        print(k, ": lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
        assert scratch == 0 and spill == 0, (k, scratch, spill)
        assert vgpr <= vgpr_bound and lds <= lds_bound, (k, vgpr, lds)


def test_the_union_find_is_defined_once():
    hip = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip")
    shared = open(os.path.join(hip, "tracks.h")).read()
    for name in ("find_root", "par_load", "par_cas", "buf_rows", "block_node", "union_nodes", "pair_edge"):
        assert len(re.findall(r"__device__ __forceinline__ \w+ " + name + r"\(", shared)) == 1, name
        for f in ("tracks.hip", "track_edges.hip"):
            txt = open(os.path.join(hip, f)).read()
            assert '#include "tracks.h"' in txt and not re.search(r"__device__[^;{]*\b" + name + r"\(", txt), (f, name)
    assert "k_edges_" not in open(os.path.join(hip, "tracks.hip")).read()


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
    assert L.vksift_hip_abi_version() >= 16
    for m in ("beginTrackAccumulation", "accumulateTrackEdges", "getTrackEdgeStats", "downloadTrackEdges", "buildTracksAccumulated", "getAccumulateTime"):
        assert hasattr(vk.Instance, m), m
    assert vk.TRACK_EDGE_DTYPE.itemsize == 16 and vk.TRACK_EDGE_STATS_DTYPE.itemsize == 16
    assert vk.TRACK_EDGE_DTYPE.names == ("gpu_buffer_id_a", "row_a", "gpu_buffer_id_b", "row_b")
    assert vk.TRACK_EDGE_STATS_DTYPE.names == ("nb_edges", "nb_dropped", "nb_calls", "nb_changed_buffers")
