"""Register budget of the refinement kernels of extrema.hip (CPU: hipcc cross-compiles), the mechanism of tests/test_kernel_resources.py.
Both forms of the refinement (BUF: one buffer resource per image's octave, otherwise 64-bit pointers) share one body, refine_core(); the
loader decides whether its step loop is unrolled. A change of that body that costs the buffer form registers, or sends either form through
scratch memory, shows up here long before a GPU measures it. Read from the code object's metadata: .vgpr_count and
.private_segment_fixed_size of every kernel."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# VGPRs of the four buffer-form instantiations before the two forms were given one body: <F16, BUF> -> count
BUF_VGPRS = {"k_refine_flagsILb1ELb1EE": 44, "k_refine_flagsILb0ELb1EE": 54, "k_cand_emitILb1ELb1EE": 70, "k_cand_emitILb0ELb1EE": 82}


def test_refinement_kernels_keep_their_registers(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "extrema.hip")
    out = str(tmp_path / "extrema.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/extrema.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    subprocess.run(cmd, check=True, capture_output=True, cwd=str(tmp_path))
    txt = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)
    assert len(meta) == 36, [name for name, _, _ in meta]  # 26 scans, segment scan, candidate list, 2 x 4 refinement kernels
    refine, buf = 0, 0
    for name, scratch, vgpr in meta:
        if "14k_refine_flagsI" not in name and "11k_cand_emitI" not in name:
            continue
        refine += 1
        assert int(scratch) == 0, (name, scratch)
        for inst, limit in BUF_VGPRS.items():
            if inst in name:
                buf += 1
                assert int(vgpr) <= limit, (name, vgpr, limit)
    assert refine == 8 and buf == 4
