"""The one build of the simulated-device harness (tests/native/sim_device.c + tests/native/plan_harness.c + every file of csrc/host/) that
tests/test_detect_plan.py and tests/test_pair_plan.py share: compiled once per test process, file by file on a few threads, with gcc's address
and undefined-behaviour sanitizers where their runtimes exist. A stand-alone program: nothing is loaded into Python, nothing is preloaded."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkansift_amd", "csrc")


def host_sources():
    """every host/*.c that vulkansift_amd/build.py names (HOST_SRCS and what is appended to it), read without importing the package's build
    (which needs hipcc)"""
    text = open(os.path.join(ROOT, "vulkansift_amd", "build.py")).read()
    names = list(dict.fromkeys(re.findall(r'"(host/[a-z_]+\.c)"', text)))
    assert "host/vksift_tracks.c" in names and len(names) >= 20, names
    return [os.path.join(CSRC, s) for s in names]


@functools.lru_cache(maxsize=None)
def executable():
    out = tempfile.mkdtemp(prefix="plan_harness_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    san = []
    runtimes = [subprocess.run(["gcc", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libubsan.so")]
    if all(os.path.isabs(p) and os.path.exists(p) for p in runtimes):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    srcs = [os.path.join(ROOT, "tests", "native", f) for f in ("sim_device.c", "plan_harness.c")] + host_sources()
    flags = ["-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror", "-DVKSIFT_BUILD"] + san + \
            ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "host"), "-I" + CSRC]

    def compile_one(src):
        obj = os.path.join(out, os.path.basename(src) + ".o")
        subprocess.run(["gcc"] + flags + ["-c", src, "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        objs = list(pool.map(compile_one, srcs))
    exe = os.path.join(out, "plan_harness")
    subprocess.run(["gcc"] + san + objs + ["-lm", "-lpthread", "-o", exe], check=True)
    return exe
