"""The kernels of cameras.hip keep their state in registers: no scratch memory and no spilled register in any of them (CPU: hipcc cross-compiles).
Resource metadata of the code object only — and the build lists, the headers, the built library, the Python interface and the restatement carry the new
entries and agree on names, sizes and constants. Recorded when the file was written (VGPRs, bytes of LDS): k_refine_cameras 116, 576 (the four waves'
28 partial sums, their 28 totals, four words for the integer reductions); k_view_keys 10, 0; k_view_hist 7, 1024; k_view_scan 17, 68; k_view_scatter 36,
5120; k_view_offsets 18, 128; k_view_expand 7, 0; k_cam_stats 15, 256."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (VGPRs: where a workgroup of 256 (1024) would start to cost occupancy; LDS bytes: the recorded figure rounded up to the next power of two)
BOUNDS = {"k_refine_cameras": (128, 1024), "k_view_keys": (128, 0), "k_view_hist": (128, 1024), "k_view_scan": (64, 128), "k_view_scatter": (128, 8192),
          "k_view_offsets": (64, 128), "k_view_expand": (128, 0), "k_cam_stats": (64, 256)}
EXT = ("vksift_ext_indexObservationsByView", "vksift_ext_getViewStats", "vksift_ext_downloadViewOffsets", "vksift_ext_downloadViewObservations",
       "vksift_ext_getIndexViewsTime", "vksift_ext_refineCameras", "vksift_ext_getCameraStats", "vksift_ext_downloadRefinedCameras",
       "vksift_ext_getRefineCamerasTime")
HIP = ("vksift_hip_views_scratch_u32", "vksift_hip_index_views", "vksift_hip_refine_cameras")


def test_camera_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/cameras.hip" in b.HIP_SRCS and "host/vksift_cameras.c" in b.HOST_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "cameras.hip")
    out = str(tmp_path / "cameras.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/cameras.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    assert len(meta) == len(BOUNDS), sorted(meta)
    for k, (max_vgpr, max_lds) in BOUNDS.items():
        hits = [v for name, v in meta.items() if re.search(k + r"E", name)]
        assert len(hits) == 1, (k, sorted(meta))
        lds, scratch, vgpr, spill = hits[0]
        print(k, ": lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
        assert scratch == 0 and spill == 0, (k, scratch, spill)
        assert vgpr <= max_vgpr, (k, vgpr)
        assert lds <= max_lds, (k, lds)
    # nothing here is fused: the rule is written with separate multiplications and additions, and the file asks for no fmaf
    assert "fmaf" not in re.sub(r"//.*", "", open(src).read())


def _header(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_headers_declare_and_the_library_exports_the_entries(vk):
    assert set(EXT) <= set(re.findall(r"\b(vksift_[A-Za-z0-9_]+)\s*\(", _header("vksift_ext.h")))
    assert set(HIP) <= set(re.findall(r"\b(vksift_[A-Za-z0-9_]+)\s*\(", _header("vksift_hip.h")))
    L = vk.lib()
    for fn in EXT + HIP:
        assert hasattr(L, fn), fn
    assert L.vksift_hip_abi_version() >= 15
    for m in ("indexObservationsByView", "getViewStats", "downloadViewOffsets", "downloadViewObservations", "getIndexViewsTime", "refineCameras",
              "getCameraStats", "downloadRefinedCameras", "getRefineCamerasTime"):
        assert hasattr(vk.Instance, m), m
    assert vk.VIEW_OBSERVATION_DTYPE.itemsize == 16 and vk.VIEW_STATS_DTYPE.itemsize == 16
    assert vk.REFINED_CAMERA_DTYPE.itemsize == 72 and vk.CAMERA_STATS_DTYPE.itemsize == 16
    assert vk.REFINED_CAMERA_DTYPE.names == ("P", "cost_start", "cost", "max_sq_error", "nb_observations", "steps", "status")
    # the header's constants, read from the header
    defs = dict(re.findall(r"#define\s+VKSIFT_EXT_CAMERA_(\w+)\s+(\d+)u", _header("vksift_ext.h")))
    assert {k: int(v) for k, v in defs.items()} == dict(ABSENT=vk.CAMERA_ABSENT, TOO_FEW=vk.CAMERA_TOO_FEW, DEGENERATE=vk.CAMERA_DEGENERATE,
                                                        BEHIND=vk.CAMERA_BEHIND, MIN_OBSERVATIONS=vk.CAMERA_MIN_OBSERVATIONS, MAX_STEPS=vk.CAMERA_MAX_STEPS)
    # the scratch the launcher asks for: five lists and a digit table per block of 2048 observations
    for n, blocks in ((1, 1), (2048, 1), (2049, 2), (115024, 57)):
        assert L.vksift_hip_views_scratch_u32(n) == blocks * (5 * 2048 + 256)


def test_the_python_mirror_and_the_restatement_agree_on_the_records():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import np_cameras as NC
    import vulkansift_amd.api as api

    assert NC.VIEW_OBSERVATION_DTYPE == api.VIEW_OBSERVATION_DTYPE and NC.CAMERA_DTYPE == api.REFINED_CAMERA_DTYPE
    assert NC.VIEW_STATS == api.VIEW_STATS_DTYPE.names and NC.CAMERA_STATS == api.CAMERA_STATS_DTYPE.names
    assert (NC.ABSENT, NC.TOO_FEW, NC.DEGENERATE, NC.BEHIND) == (api.CAMERA_ABSENT, api.CAMERA_TOO_FEW, api.CAMERA_DEGENERATE, api.CAMERA_BEHIND)
    assert (NC.MIN_OBSERVATIONS, NC.MAX_STEPS) == (api.CAMERA_MIN_OBSERVATIONS, api.CAMERA_MAX_STEPS)
