"""vksift_ext_indexObservationsByView and vksift_ext_refineCameras on the simulated device (tests/native/sim_device.c; CPU), where the launchers of
hip/cameras.hip are absent: the host file's weak references to them are NULL, so either call must report VKSIFT_VULKAN_ERROR through the ordinary failure
path and every refusal above it VKSIFT_INVALID_INPUT_ERROR, serve no accessor, leave the points, the observations and the tracks served and unchanged,
allocate nothing before the launcher check, leave the instance usable, and leave a clean ledger after destroy with no VIOLATION line. A stand-alone C
program of its own (tests/native/cameras_sim.c, which also stands in for the observation and triangulation launchers the device lacks), linked against the
simulated device and every host source as tests/plan_build.py does it, with gcc's address and undefined-behaviour sanitizers in the compile line where
their runtimes exist; nothing is loaded into Python and nothing is preloaded."""
import os
import re
import subprocess

import pytest

import plan_build

ROOT = plan_build.ROOT
INVALID_INPUT, VULKAN_ERROR = 1, 2


@pytest.fixture(scope="module")
def log(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cameras_sim"))
    san = []
    runtimes = [subprocess.run(["gcc", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libubsan.so")]
    if all(os.path.isabs(p) and os.path.exists(p) for p in runtimes):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    srcs = [os.path.join(ROOT, "tests", "native", f) for f in ("sim_device.c", "cameras_sim.c")] + plan_build.host_sources()
    assert any(s.endswith("vksift_cameras.c") for s in srcs)          # the file under test is in the build list, not hidden from it
    flags = ["-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror", "-DVKSIFT_BUILD"] + san + \
            ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(plan_build.CSRC, "host"), "-I" + plan_build.CSRC]
    exe = os.path.join(out, "cameras_sim")
    subprocess.run(["gcc"] + flags + srcs + ["-lm", "-lpthread", "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VKSIFT_")}
    env["VKSIFT_DEFER"] = "0"
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def steps(log):
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^step (\w+) errors=(\d+) last=(-?\d+)$", log, re.M)}


def test_missing_launchers_are_launch_failures(log):
    s = steps(log)
    assert s["detect"] == s["filtered"] == s["tracks"] == s["select"] == s["triangulate"] == s["served_before"] == (0, 0), s
    assert "served tracks=3 observations=3 points=3" in log                  # both stages have their input
    for refused in ("index_before_selection", "refine_before_triangulation", "refine_zero_steps", "refine_nine_steps"):
        assert s[refused] == (1, INVALID_INPUT), refused
    assert s["index"] == (1, VULKAN_ERROR) and s["refine"] == (1, VULKAN_ERROR)
    for accessor in ("vstats", "voffsets", "vobservations", "cstats", "ccameras"):
        assert s[accessor] == (1, INVALID_INPUT), accessor
    assert s["served_after"] == (0, 0) and "served same=1" in log
    assert "times -1 -1" in log
    assert s["filtered_again"] == (0, 0)


def test_nothing_is_left_behind(log):
    assert "VIOLATION" not in log
    (ledger,) = re.findall(r"^ledger blocks=(\d+) streams=(\d+) events=(\d+) execs=(\d+) violations=(\d+)$", log, re.M)
    assert ledger == ("0",) * 5, ledger
    # the failed calls allocated nothing: the blocks of their storage are made behind the launcher check
    allocs_before = log[:log.index("step served_before")].count("alloc ")
    assert log[:log.index("step served_after")].count("alloc ") == allocs_before
