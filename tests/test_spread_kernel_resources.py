"""The selection kernel of spread.hip keeps the record it moves in registers and its per-cell state in LDS (CPU: hipcc cross-compiles). The
compaction round is the one of strongest.hip (records.h): every kept row of a round is loaded whole — 41 dwords — before the barrier and stored
after it, with every index a compile-time constant; and the one thread per cell that picks its cell's bin walks its sixteen bins unrolled, so
that no array is indexed at run time. A run-time index would send either to scratch memory. Resource metadata of the code object only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keep_grid_kernel_uses_no_scratch(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/spread.hip" in b.HIP_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "spread.hip")
    out = str(tmp_path / "spread.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/spread.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    hits = [v for name, v in meta.items() if "k_keep_grid" in name]
    assert len(hits) == 1, sorted(meta)
    lds, scratch, vgpr, spill = hits[0]
    print("k_keep_grid: lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
    assert scratch == 0 and spill == 0, (scratch, spill)
    # LDS, by the declarations: 8192 keys (32 768 bytes) and 8192 cells of one byte (8192), 256 cells x 17 histogram words (17 408: sixteen bins and
    # one word of padding), 256 thresholds of 8 bytes (2048), 256 wanted counts (1024), three section arrays, the sixteen wave totals and four words
    # (272) = 61 712. Below the 64 KB a workgroup may declare, and below the 80 KB at which the two 1024-thread workgroups a CU's 2048 thread slots
    # admit still share its 160 KB. The build shows 88 VGPRs — the 41 words of the record, the sixteen section counts, addresses, and the 64-bit
    # composites of the select passes, which are dead by the time the record is loaded. A 1024-thread workgroup is four waves per SIMD: 128 registers
    # each is all there is. Held to what the build gives, registers to their block of 8.
    assert lds == 61712, lds
    assert vgpr <= 88, vgpr
