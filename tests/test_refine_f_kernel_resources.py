"""The refit kernel of refine_f.hip keeps its working set in registers (CPU: hipcc cross-compiles). Every thread carries the 44 accumulators of
the normal equations through the strided sums and then eliminates the 8x9 system, three times per round; the gauge (which monomial is moved to
the last place, where the 1 goes back) is chosen at run time and applied with selects between compile-time indices — a run-time register index
would send the monomials, the accumulators or the system to scratch memory, and the solve to memory speed
(tests/test_refine_kernel_resources.py has the same concern for the homography's kernel). Resource metadata of the code object only."""
import os
import re
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refit_f_kernel_uses_no_scratch(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/refine_f.hip" in b.HIP_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "refine_f.hip")
    out = str(tmp_path / "refine_f.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/refine_f.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(scratch), int(vgpr))) for name, scratch, vgpr in
                re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt))
    hits = [v for name, v in meta.items() if "k_refit_f" in name]
    assert len(hits) == 1, sorted(meta)
    scratch, vgpr = hits[0]
    print("k_refit_f: scratch", scratch, "vgpr", vgpr)
    assert scratch == 0, scratch
    # The build shows 224 VGPRs (the 72 entries of the system and the 44 sums it is built from, which the scheduler keeps live side by side with the
    # per-match products of the unrolled accumulation, the model and the conditioning carried across the rounds). The occupancy steps of a gfx950
    # SIMD (512 registers per lane, allocated in blocks of 8) are 128 -> 4, 168 -> 3, 256 -> 2 waves: 224 rounds up to 256, two workgroups of 256
    # threads resident per CU — 512 pairs in flight on 256 CUs, one launch wave for the batches the benchmark uses.
    assert vgpr <= 256, vgpr
