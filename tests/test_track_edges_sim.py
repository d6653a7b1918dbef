"""The edge store of tracks across matching calls on the simulated device (tests/native/sim_device.c; CPU). tests/native/track_edges_sim.c is built twice, each
a stand-alone C program linked against the simulated device and every host source as tests/plan_build.py does it, with gcc's address and undefined-behaviour
sanitizers in the compile line where their runtimes exist; nothing is loaded into Python and nothing is preloaded.
  * as the device is, without the launchers of hip/track_edges.hip: every refusal is VKSIFT_INVALID_INPUT_ERROR and leaves the store untouched, the accumulate
    is VKSIFT_VULKAN_ERROR through the ordinary failure path, the store is refused until the next begin, the instance stays usable
  * with launchers the program defines itself (launches that compute nothing): a new matching leaves the store served and the tracks not, the stages behind an
    accumulated build run over every participating buffer, the first begin releases and re-sizes exactly when 2 batch_cap < sift_buffer_count
Both leave a clean ledger after destroy with no VIOLATION line."""
import os
import re
import subprocess

import pytest

import plan_build

ROOT = plan_build.ROOT
INVALID_INPUT, VULKAN_ERROR = 1, 2


def run(out, name, defines):
    san = []
    runtimes = [subprocess.run(["gcc", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libubsan.so")]
    if all(os.path.isabs(p) and os.path.exists(p) for p in runtimes):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    srcs = [os.path.join(ROOT, "tests", "native", f) for f in ("sim_device.c", "track_edges_sim.c")] + plan_build.host_sources()
    assert any(s.endswith("vksift_track_edges.c") for s in srcs)          # the file under test is in the build list, not hidden from it
    flags = ["-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror", "-DVKSIFT_BUILD"] + defines + san + \
            ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(plan_build.CSRC, "host"), "-I" + plan_build.CSRC]
    exe = os.path.join(out, name)
    subprocess.run(["gcc"] + flags + srcs + ["-lm", "-lpthread", "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VKSIFT_")}
    env["VKSIFT_DEFER"] = "0"
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def bare(tmp_path_factory):
    return run(str(tmp_path_factory.mktemp("track_edges_sim")), "bare", [])


@pytest.fixture(scope="module")
def stubbed(tmp_path_factory):
    return run(str(tmp_path_factory.mktemp("track_edges_sim")), "stubbed", ["-DWITH_LAUNCHERS"])


def steps(log):
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^step (\w+) errors=(\d+) last=(-?\d+)$", log, re.M)}


def between(log, a, b):
    return log[log.index("mark " + a + "\n"):log.index("mark " + b + "\n")]


def clean(log):
    assert "VIOLATION" not in log
    (ledger,) = re.findall(r"^ledger blocks=(\d+) streams=(\d+) events=(\d+) execs=(\d+) violations=(\d+)$", log, re.M)
    assert ledger == ("0",) * 5, ledger


def test_refusals_and_the_missing_launcher(bare):
    s = steps(bare)
    for refused in ("accumulate_before_begin", "build_before_begin", "stats_before_begin", "edges_before_begin", "begin_zero", "stats_after_begin_zero",
                    "accumulate_without_matching", "stats_null", "edges_null", "build_before_accumulate", "accumulate_unknown_source", "accumulate_stage_not_run"):
        assert s[refused] == (1, INVALID_INPUT), refused
    assert "stats untouched=1" in bare
    assert s["detect"] == s["begin"] == s["filtered"] == s["stats_empty"] == (0, 0), s
    assert "stats empty=0 0 0 0" in bare                                    # the refusals queued nothing and left the store as begin made it
    assert s["accumulate"] == (1, VULKAN_ERROR)
    assert "alloc " not in between(bare, "before_failure", "after_failure")  # the launcher is looked for before anything is allocated
    for refused in ("stats_after_failure", "edges_after_failure", "accumulate_after_failure", "build_after_failure"):
        assert s[refused] == (1, INVALID_INPUT), refused
    assert s["begin_again"] == s["stats_after_begin"] == s["plain_build"] == s["plain_stats"] == s["filtered_again"] == (0, 0), s
    assert "times -1" in bare
    clean(bare)


def test_the_store_outlives_matchings_and_builds(stubbed):
    s = steps(stubbed)
    for ok in ("detect", "filtered", "plain_build", "plain_select", "plain_triangulate", "begin", "accumulate_0", "filtered_1", "accumulate_1", "stats", "edges", "build",
               "track_stats", "feature_tracks_first_call", "select", "triangulate", "filtered_2", "stats_after_matching", "build_again", "track_stats_again",
               "plain_build_again", "stats_after_plain_build", "begin_second"):
        assert s[ok] == (0, 0), (ok, s[ok])
    assert "stats served=3 3 3 3" in stubbed
    for refused in ("tracks_after_begin", "track_stats_after_matching", "feature_tracks_outside_pair_list", "build_after_second_begin"):
        assert s[refused] == (1, INVALID_INPUT), refused
    # both calls' buffers take part: 0 1 2 3 of the first, 1 4 5 of the second
    assert stubbed.count("build_from_edges nbufs=6") == 2 and "track_observations nbufs=6" in stubbed and "track_observations nbufs=4" in stubbed
    clean(stubbed)


def test_the_first_begin_resizes_only_a_narrow_instance(stubbed):
    s = steps(stubbed)
    first = between(stubbed, "begin_first", "begin_first_done")
    freed = [int(n) for n in re.findall(r"^free D b\d+ (\d+)$", first, re.M)]
    assert len(freed) >= 8, first                                            # tracks, observations and points allocated for 4 buffers
    node_words_4, node_words_6 = 4 * 4 * 600 + 8, 4 * 6 * 600 + 8
    assert node_words_4 in freed
    after = stubbed[stubbed.index("mark begin_first_done"):stubbed.index("mark begin_second\n")]
    assert f"alloc D b" in after and re.search(rf"^alloc D b\d+ {node_words_6}$", after, re.M) and not re.search(rf"^alloc D b\d+ {node_words_4}$", after, re.M)
    assert "free " not in between(stubbed, "begin_second", "begin_second_done")
    assert s["wide_filtered"] == s["wide_plain_build"] == s["begin_wide"] == s["wide_tracks_after_begin"] == (0, 0)
    assert "free " not in between(stubbed, "begin_wide", "begin_wide_done")
