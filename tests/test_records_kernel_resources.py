"""The two kernels of records.hip that walk sectioned buffers are streaming kernels: sixteen bytes (gather) or a dword (pack) per lane and step,
no record held in registers (CPU: hipcc cross-compiles). Their sixteen section counts are indexed with compile-time constants only (the walk of
records.h is unrolled); a run-time index would send them to scratch memory. Resource metadata of the code object only, in the manner of
tests/test_rootsift_kernel_resources.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_and_pack_kernels_use_no_scratch(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/records.hip" in b.HIP_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "records.hip")
    out = str(tmp_path / "records.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/records.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    # Before the kernels took their shared steps from records.h the build showed 20 VGPRs for k_gather_sections and 12 for k_pack_features
    # (NOTEBOOK.md): held to that, rounded up to the block of 8.
    for kernel, vgpr_max, lds_free in (("k_gather_sections", 24, True), ("k_pack_features", 16, False)):
        hits = [v for name, v in meta.items() if kernel in name]
        assert len(hits) == 1, sorted(meta)
        lds, scratch, vgpr, spill = hits[0]
        print(kernel, ": lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
        assert scratch == 0 and spill == 0, (kernel, scratch, spill)
        assert vgpr <= vgpr_max, (kernel, vgpr)
        assert lds == 0 or not lds_free, (kernel, lds)
