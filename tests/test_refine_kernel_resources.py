"""The refit kernel of refine.hip keeps its working set in registers (CPU: hipcc cross-compiles). Every thread carries the 27 accumulators of
the normal equations through the strided sums and then eliminates the 8x9 system, twice per Gauss-Newton step and round; both are fully
unrolled so that every index is a compile-time constant — a run-time index would send the accumulators or the system to scratch memory, and
the solve to memory speed (tests/test_verify_kernel_resources.py has the same concern for the seven-point solve). Resource metadata of the
code object only."""
import os
import re
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refit_kernel_uses_no_scratch(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/refine.hip" in b.HIP_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "refine.hip")
    out = str(tmp_path / "refine.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/refine.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(scratch), int(vgpr))) for name, scratch, vgpr in
                re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt))
    hits = [v for name, v in meta.items() if "k_refit_h" in name]
    assert len(hits) == 1, sorted(meta)
    scratch, vgpr = hits[0]
    print("k_refit_h: scratch", scratch, "vgpr", vgpr)
    assert scratch == 0, scratch
    # The build shows 137 VGPRs (the 72 entries of the system, the 27 sums it is built from and the model carried across the rounds). The occupancy
    # steps of a gfx950 SIMD (512 registers per lane, allocated in blocks of 8) are 128 -> 4, 168 -> 3, 256 -> 2 waves: 137 rounds up to 168, three
    # workgroups of 256 threads resident per CU. The batch is the parallelism (one workgroup per pair), so three per CU is 768 pairs in flight.
    assert vgpr <= 168, vgpr
