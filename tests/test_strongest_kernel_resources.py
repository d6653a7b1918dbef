"""The selection kernel of strongest.hip keeps the record it moves in registers (CPU: hipcc cross-compiles). Every kept row of a round is
loaded whole — 41 dwords — before the barrier and stored after it; the loops over the record and over the sixteen sections are fully unrolled
so that every index is a compile-time constant. A run-time index would send the record to scratch memory and the compaction to memory speed
twice over. Resource metadata of the code object only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keep_strongest_kernel_uses_no_scratch(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    assert "hip/strongest.hip" in b.HIP_SRCS
    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "strongest.hip")
    out = str(tmp_path / "strongest.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/strongest.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = dict((name, (int(lds), int(scratch), int(vgpr), int(spill))) for lds, name, scratch, vgpr, spill in
                re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                           r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt))
    hits = [v for name, v in meta.items() if "k_keep_strongest" in name]
    assert len(hits) == 1, sorted(meta)
    lds, scratch, vgpr, spill = hits[0]
    print("k_keep_strongest: lds", lds, "scratch", scratch, "vgpr", vgpr, "vgpr spills", spill)
    assert scratch == 0 and spill == 0, (scratch, spill)
    # The build shows 109 VGPRs (the 41 words of the record, the sixteen section counts, addresses) and 34 064 bytes of LDS (8192 keys, the histogram,
    # the section table). A 1024-thread workgroup is four waves per SIMD: 128 registers each is all there is, and the 160 KB of a CU's LDS hold the
    # two workgroups its 2048 thread slots admit only below 80 KB each. Held to what the build gives (NOTEBOOK.md), registers to their block of 8.
    assert vgpr <= 112, vgpr
    assert lds == 34064, lds
