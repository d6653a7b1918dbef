"""Register budget of the one-launch extraction tail, extract_tail.hip (CPU: hipcc cross-compiles), the mechanism of
tests/test_extrema_kernel_resources.py. k_extract_tail<F16, BUF> runs one workgroup of 512 or 1024 threads per (image, octave): a 1024-thread
workgroup is 16 waves, 4 per SIMD, which a CU holds only while a wave needs at most 128 VGPRs (512 per SIMD lane / 4); scratch memory would put
the refinement's live values into HBM. Read from the code object's metadata: .vgpr_count and .private_segment_fixed_size of every kernel."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VGPR_BUDGET = 128


def test_extract_tail_kernels_fit_a_1024_thread_workgroup(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/extract_tail.hip" in b.HIP_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "extract_tail.hip")
    out = str(tmp_path / "extract_tail.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/extract_tail.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    subprocess.run(cmd, check=True, capture_output=True, cwd=str(tmp_path))
    txt = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)
    names = sorted(name for name, _, _ in meta)
    assert len(meta) == 4 and all("14k_extract_tailI" in n for n in names), names  # <F16, BUF> in {0, 1}^2
    assert len({n for n in names}) == 4
    for name, scratch, vgpr in meta:
        assert int(scratch) == 0, (name, scratch)
        assert int(vgpr) <= VGPR_BUDGET, (name, vgpr)
