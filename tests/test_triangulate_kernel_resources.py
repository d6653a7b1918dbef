"""The kernels of triangulate.hip keep a track's state in registers: no scratch memory and no spilled register in either of them (CPU: hipcc
cross-compiles). Resource metadata of the code object only — and the build lists, the headers, the built library and the Python interface carry the new
entries. Recorded when the file was written: k_triangulate 106 VGPRs, 6144 bytes of LDS (24 bytes per lane that the
compiler places there itself: the source declares none), k_tri_stats 31 VGPRs, 192 bytes of LDS."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_triangulate", "k_tri_stats")
EXT = ("vksift_ext_triangulateTracks", "vksift_ext_getPointStats", "vksift_ext_downloadPoints", "vksift_ext_getTriangulateTime")
HIP = ("vksift_hip_triangulate_tracks",)


def test_triangulation_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/triangulate.hip" in b.HIP_SRCS and "host/vksift_triangulate.c" in b.HOST_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "triangulate.hip")
    out = str(tmp_path / "triangulate.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/triangulate.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    assert len(meta) == len(KERNELS), sorted(meta)
    bounds = {"k_triangulate": (128, 8192), "k_tri_stats": (64, 256)}       # VGPRs: where a workgroup of 256 (1024) would start to cost occupancy; LDS bytes
    for k in KERNELS:
        hits = [v for name, v in meta.items() if re.search(k + r"E", name)]
        assert len(hits) == 1, (k, sorted(meta))
        lds, scratch, vgpr, spill = hits[0]
        print(k, ": lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
        assert scratch == 0 and spill == 0, (k, scratch, spill)
        assert vgpr <= bounds[k][0], (k, vgpr)
        assert lds <= bounds[k][1], (k, lds)
    # nothing here is fused: the rule is written with separate multiplications and additions, and the file asks for no fmaf
    assert "fmaf" not in re.sub(r"//.*", "", open(src).read())


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
    assert L.vksift_hip_abi_version() >= 14
    for m in ("triangulateTracks", "getPointStats", "downloadPoints", "getTriangulateTime"):
        assert hasattr(vk.Instance, m), m
    assert vk.POINT_DTYPE.itemsize == 32 and vk.POINT_STATS_DTYPE.itemsize == 16
    assert vk.POINT_DTYPE.names == ("X", "max_sq_error", "min_cos", "status", "steps", "nb_observations")
    assert (vk.POINT_DEGENERATE, vk.POINT_TOO_LONG, vk.POINT_BEHIND, vk.POINT_ERROR, vk.POINT_ANGLE, vk.TRIANGULATE_MAX_OBSERVATIONS) == (1, 2, 4, 8, 16, 1024)


def test_the_python_mirror_and_the_restatement_agree_on_the_record():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import np_triangulate as NT
    import vulkansift_amd.api as api

    assert NT.POINT_DTYPE == api.POINT_DTYPE and NT.OBSERVATION_DTYPE == api.OBSERVATION_DTYPE
    assert (NT.DEGENERATE, NT.TOO_LONG, NT.BEHIND, NT.ERROR, NT.ANGLE) == (api.POINT_DEGENERATE, api.POINT_TOO_LONG, api.POINT_BEHIND, api.POINT_ERROR, api.POINT_ANGLE)
    assert NT.MAX_OBSERVATIONS == api.TRIANGULATE_MAX_OBSERVATIONS
