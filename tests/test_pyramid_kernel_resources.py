"""Resources of every kernel of pyramid.hip (CPU: hipcc cross-compiles). The strip-march kernels are built from shared force-inlined steps
(NOTEBOOK section 16) and the compiler is sensitive to how those are written: a window or tap index that is no compile-time constant, a
value passed by reference, sends a register window to scratch memory and the march to memory speed long before any result changes. The
table is the code object of the commit BEFORE the steps were shared (VGPRs, LDS bytes): the set of instantiations and every LDS size stay
what they were, nothing uses scratch, no kernel needs more registers. Metadata of the code object only."""
import os
import re
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel<template arguments, bools as 0 / 1>: (.vgpr_count, .group_segment_fixed_size)
PARENT = {
    "k_blur_lean<2,0,0>": (92, 4352), "k_blur_lean<2,0,1>": (58, 4352), "k_blur_lean<2,1,0>": (88, 4352), "k_blur_lean<2,1,1>": (65, 4352),
    "k_blur_lean<2,2,0>": (64, 4352), "k_blur_lean<2,2,1>": (41, 4352), "k_blur_lean<3,0,0>": (92, 4352), "k_blur_lean<3,0,1>": (62, 4352),
    "k_blur_lean<3,1,0>": (92, 4352), "k_blur_lean<3,1,1>": (76, 4352), "k_blur_lean<3,2,0>": (64, 4352), "k_blur_lean<3,2,1>": (48, 4352),
    "k_blur_lean<4,0,0>": (100, 4352), "k_blur_lean<4,0,1>": (70, 4352), "k_blur_lean<4,1,0>": (96, 4352), "k_blur_lean<4,1,1>": (80, 4352),
    "k_blur_lean<4,2,0>": (72, 4352), "k_blur_lean<4,2,1>": (56, 4352), "k_blur_lean<5,0,0>": (92, 4352), "k_blur_lean<5,0,1>": (73, 4352),
    "k_blur_lean<5,1,0>": (92, 4352), "k_blur_lean<5,1,1>": (92, 4352), "k_blur_lean<5,2,0>": (64, 4352), "k_blur_lean<5,2,1>": (64, 4352),
    "k_blur_lean<6,0,0>": (102, 4608), "k_blur_lean<6,0,1>": (82, 4608), "k_blur_lean<6,1,0>": (100, 4608), "k_blur_lean<6,1,1>": (96, 4608),
    "k_blur_lean<6,2,0>": (76, 4608), "k_blur_lean<6,2,1>": (72, 4608), "k_blur_lean<7,0,0>": (108, 4608), "k_blur_lean<7,0,1>": (89, 4608),
    "k_blur_lean<7,1,0>": (108, 4608), "k_blur_lean<7,1,1>": (108, 4608), "k_blur_lean<7,2,0>": (80, 4608), "k_blur_lean<7,2,1>": (80, 4608),
    "k_blur_lean<8,0,0>": (118, 4608), "k_blur_lean<8,0,1>": (98, 4608), "k_blur_lean<8,1,0>": (116, 4608), "k_blur_lean<8,1,1>": (112, 4608),
    "k_blur_lean<8,2,0>": (92, 4608), "k_blur_lean<8,2,1>": (88, 4608), "k_blur_lean<9,0,0>": (124, 4608), "k_blur_lean<9,0,1>": (105, 4608),
    "k_blur_lean<9,1,0>": (124, 4608), "k_blur_lean<9,1,1>": (124, 4608), "k_blur_lean<9,2,0>": (96, 4608), "k_blur_lean<9,2,1>": (96, 4608),
    "k_blur_lean<10,0,0>": (134, 4864), "k_blur_lean<10,0,1>": (114, 4864), "k_blur_lean<10,1,0>": (132, 4864), "k_blur_lean<10,1,1>": (128, 4864),
    "k_blur_lean<10,2,0>": (108, 4864), "k_blur_lean<10,2,1>": (104, 4864), "k_blur_lean<11,0,0>": (140, 4864), "k_blur_lean<11,0,1>": (121, 4864),
    "k_blur_lean<11,1,0>": (140, 4864), "k_blur_lean<11,1,1>": (140, 4864), "k_blur_lean<11,2,0>": (112, 4864), "k_blur_lean<11,2,1>": (112, 4864),
    "k_blur_lean<12,0,0>": (150, 4864), "k_blur_lean<12,0,1>": (130, 4864), "k_blur_lean<12,1,0>": (148, 4864), "k_blur_lean<12,1,1>": (144, 4864),
    "k_blur_lean<12,2,0>": (124, 4864), "k_blur_lean<12,2,1>": (120, 4864), "k_blur_lean<13,0,0>": (156, 4864), "k_blur_lean<13,0,1>": (137, 4864),
    "k_blur_lean<14,0,0>": (166, 5120), "k_blur_lean<14,0,1>": (146, 5120), "k_blur_lean<15,0,0>": (172, 5120), "k_blur_lean<15,0,1>": (153, 5120),
    "k_blur_lean<16,0,0>": (182, 5120), "k_blur_lean<16,0,1>": (162, 5120), "k_blur_lean<17,0,0>": (188, 5120), "k_blur_lean<17,0,1>": (169, 5120),
    "k_blur_lean<18,0,0>": (198, 5376), "k_blur_lean<18,0,1>": (178, 5376), "k_blur_lean<19,0,0>": (204, 5376), "k_blur_lean<19,0,1>": (185, 5376),
    "k_blur_lean<20,0,0>": (214, 5376), "k_blur_lean<20,0,1>": (194, 5376), "k_blur_lean_multi<9,0>": (124, 4608),
    "k_blur_lean_multi<9,1>": (105, 4608), "k_blur_lean_multi<11,0>": (140, 4864), "k_blur_lean_multi<11,1>": (121, 4864),
    "k_blur_lean_multi<13,0>": (156, 4864), "k_blur_lean_multi<13,1>": (137, 4864), "k_blur_lean_multi<15,0>": (172, 5120),
    "k_blur_lean_multi<15,1>": (153, 5120), "k_blur_pair<5,7>": (146, 8960), "k_blur_pair_wide<5,7>": (220, 17152), "k_blur_tile<0>": (28, 0),
    "k_blur_tile<1>": (28, 0), "k_blur_wide<5>": (144, 8448), "k_blur_wide<7>": (178, 8704), "k_blur_wide<9>": (178, 8704),
    "k_blur_wide<11>": (210, 8960), "k_blur_wide<13>": (210, 8960), "k_dog_plane<0>": (8, 0), "k_dog_plane<1>": (8, 0), "k_downsample<0>": (13, 0),
    "k_downsample<1>": (13, 0), "k_input_blit<0>": (25, 0), "k_input_blit<1>": (25, 0), "k_input_blit_2x<0>": (24, 0), "k_input_blit_2x<1>": (24, 0),
    "k_octave_chain": (76, 0),
}


def readable(mangled):
    """_ZN12_GLOBAL__N_111k_blur_leanILi5ELi0ELb0EEEvNS_10StreamArgsE -> k_blur_lean<5,0,0>"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    base, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
    args = re.findall(r"L[ib](\d+)E", rest[:rest.index("EE") + 1]) if rest.startswith("I") else []
    return base + ("<" + ",".join(args) + ">" if args else "")


def test_pyramid_kernels_keep_their_resources(tmp_path):
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "pyramid.hip")
    out = str(tmp_path / "pyramid.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/pyramid.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    meta = {}
    for blk in open(out).read().split("\n  - .")[1:]:  # one block of the code-object metadata per kernel
        field = lambda k: re.search(r"^    \.%s:\s+(\S+)" % k, blk, re.M).group(1)
        meta[readable(field("name"))] = (int(field("vgpr_count")), int(field("group_segment_fixed_size")), int(field("private_segment_fixed_size")))
    assert len(meta) == 108 and sorted(meta) == sorted(PARENT), sorted(set(meta) ^ set(PARENT))
    for name, (vgpr, lds, scratch) in sorted(meta.items()):
        assert scratch == 0, (name, scratch)
        assert lds == PARENT[name][1], (name, lds, PARENT[name][1])
        assert vgpr <= PARENT[name][0], (name, vgpr, PARENT[name][0])
