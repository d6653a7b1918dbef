"""The RANSAC scoring kernels of verify.hip keep their working set in registers (CPU: hipcc cross-compiles). k_ransac_score_f eliminates a
7x9 system per lane; it is fully unrolled so that every index is a compile-time constant — a run-time index would send the system to scratch
memory, and the solve to memory speed. Resource metadata of the code object only."""
import os
import re
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ransac_kernels_use_no_scratch(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "verify.hip")
    out = str(tmp_path / "verify.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/verify.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(scratch), int(vgpr))) for name, scratch, vgpr in
                re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt))
    seen = 0
    for kernel in ("k_ransac_score_h", "k_ransac_score_f", "k_ransac_final_h", "k_ransac_final_f"):
        hits = [v for name, v in meta.items() if kernel in name]
        assert len(hits) == 1, (kernel, sorted(meta))
        scratch, vgpr = hits[0]
        assert scratch == 0, (kernel, scratch)
        assert vgpr <= 128, (kernel, vgpr)          # 256 lanes per workgroup: four workgroups per CU stay resident at 128 VGPRs
        seen += 1
    assert seen == 4
