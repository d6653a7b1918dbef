"""The ctypes mirrors of tests/hip_features.py against include/vksift_hip.h: sizeof and every offsetof of vksift_hip_OctaveJob and
vksift_hip_DenseRows, measured by a few lines of C (CPU only)."""
import ctypes as C
import os
import subprocess

import hip_features as HF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_octave_job_and_dense_rows_mirror_the_header(tmp_path):
    structs = {"vksift_hip_OctaveJob": HF.OctaveJob, "vksift_hip_DenseRows": HF.DenseRows}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vksift_hip.h"\nint main(void){\n'
    want = {}
    for cname, mirror in structs.items():
        prog += f'  printf("sizeof({cname})=%zu\\n", sizeof({cname}));\n'
        want[f"sizeof({cname})"] = C.sizeof(mirror)
        for field, ctype in mirror._fields_:
            prog += f'  printf("{cname}.{field}=%zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname} *)0)->{field}));\n'
            want[f"{cname}.{field}"] = (getattr(mirror, field).offset, C.sizeof(ctype))
    prog += "  return 0;\n}\n"
    src = tmp_path / "abi_hip.c"
    src.write_text(prog)
    exe = tmp_path / "abi_hip"
    subprocess.run(["gcc", "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.strip().splitlines():
        k, v = line.split("=")
        nums = tuple(int(x) for x in v.split())
        got[k] = nums[0] if len(nums) == 1 else nums
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    # every member of the header's structs is mirrored: the sizes leave no room for one more
    for mirror in structs.values():
        last, ctype = mirror._fields_[-1]
        end = getattr(mirror, last).offset + C.sizeof(ctype)
        assert C.sizeof(mirror) - end < C.alignment(mirror)
