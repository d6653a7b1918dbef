"""The host scheduler on a simulated device (no GPU): every file of csrc/host/ linked against tests/native/sim_device.c, which records every
launch, copy, event and wait instead of computing, and driven through the public API by tests/native/plan_harness.c. Built with gcc's address
and undefined-behaviour sanitizers where their runtimes exist (a stand-alone program: nothing is preloaded); a sanitizer report, a leak or a
violation of the device's hard checks C1-C3 (sim_device.c) fails a run through its exit status.

What is checked:
  * replay equals direct — a script of calls run with VKSIFT_GRAPH=1 and with VKSIFT_GRAPH=0 issues, call by call, the same operations with
    the same arguments in the same order (a replay flattened to its captured records); only events, waits and the stream may differ. An input
    of plan_detection() that changes the sequence and is missing from the cache key shows up here;
  * the cache policy — captures, replays, evictions and drops of every call are those of tests/plan_model.py, exec by exec;
  * the named scripts of tests/plan_scripts.py (the ones tests/test_gpu_graph_cache.py runs on the GPU) reach their edge: proven with counts
    read from the log;
  * failure paths — every counted call of a capturing detection fails in turn.
"""
import os
import random
import re
import subprocess

import pytest

import plan_build
import plan_scripts as PS
from plan_model import GIVE_UP_AFTER, GRAPH_CACHE, Model

VULKAN_ERROR = 2      # VKSIFT_VULKAN_ERROR


# ---------------------------------------------------------------------------------------------------------------- the log
class Call:
    def __init__(self, cmd):
        self.cmd = tuple(int(t) if t.isdigit() else t for t in cmd.split())
        self.lines, self.ops, self.cache, self.ret, self.errors, self.violations = [], [], [], {}, [], []
        self.counted, self.allocs, self.frees, self.bounds = [], [], [], []

    def close(self):
        """self.cache: the flat cache events ("destroy" | "capture" | "replay", exec); consecutive destroys sorted"""
        out, run, captured = [], [], None
        for kind, x in self.cache:
            if kind == "destroy":
                run.append(x)
                continue
            out += [("destroy", d) for d in sorted(run)]
            run = []
            if kind == "capend":
                captured = x
            elif kind == "launch":
                out.append(("capture" if x == captured else "replay", x))
                captured = None
        self.cache = out + [("destroy", d) for d in sorted(run)]


def parse(stdout):
    calls = []
    for line in stdout.splitlines():
        if line.startswith("> "):
            calls.append(Call(line[2:]))
            continue
        c = calls[-1]
        c.lines.append(line)
        t = line.split()
        if t[0].startswith("#"):
            c.counted.append((int(t[0][1:]), t[1], t[2] if len(t) > 2 else ""))
            t = t[1:]
        if t[0] in ("op", "gop"):
            c.ops.append((t[1], t[3]))
            c.bounds.append((t[1], t[4]))
        elif t[0] == "capend" and len(t) > 2 and t[2].startswith("x"):
            c.cache.append(("capend", int(t[2][1:])))
        elif t[0] == "launch":
            c.cache.append(("launch", int(t[1][1:])))
        elif t[0] == "xdestroy":
            c.cache.append(("destroy", int(t[1][1:])))
        elif t[0] == "alloc":
            c.allocs.append((t[1], t[2], int(t[3])))
        elif t[0] == "free":
            c.frees.append((t[1], t[2], int(t[3])))
        elif t[0] == "error":
            c.errors.append(int(t[1]))
        elif t[0] == "VIOLATION":
            c.violations.append(line)
        elif t[0] == "<":
            c.ret = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}
        elif t[0] == "execs":
            c.live_execs = int(t[1].split("=")[1])
        elif t[0] == "ledger":
            c.ledger = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}
    for c in calls:
        c.close()
    return calls


@pytest.fixture(scope="module")
def harness():
    exe = plan_build.executable()      # one build for this file and tests/test_pair_plan.py
    memo = {}

    def run(script, graph=None, prelude=(), ok=True):
        """the script's calls (create ... destroy, ledger) as parsed Call objects; graph: VKSIFT_GRAPH of this run (None: the script's)"""
        env = {k: v for k, v in os.environ.items() if not k.startswith("VKSIFT_")}
        env.update(script["env"])
        if graph is not None:
            env["VKSIFT_GRAPH"] = graph
        c = script["create"]
        cmds = ["create %d %d %d %d %d %d" % (c["bc"], c["max_px"], c["max_feats"], c["nbuf"], c["ups"], c["fp16"]), "counts 3"] + list(prelude)
        cmds += [" ".join(str(t) for t in op) for op in script["ops"]] + ["destroy", "ledger"]
        key = (tuple(sorted((k, v) for k, v in env.items() if k.startswith("VKSIFT_"))), tuple(cmds))
        if key not in memo:
            r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True, env=env)
            assert not ok or r.returncode == 0, "\n".join(l for l in r.stdout.splitlines() if "VIOLATION" in l)[-3000:] + r.stderr[-4000:]
            memo[key] = (r.returncode, parse(r.stdout))
        return memo[key][1][2 + len(prelude):]      # from the script's first call on
    return run


# ---------------------------------------------------------------------------------------------------------------- the two properties
def check_replay_equals_direct(g, d, busy=False):
    assert [c.cmd for c in g] == [c.cmd for c in d]
    for i, (cg, cd) in enumerate(zip(g, d)):
        # in issue order: captured sequences keep the launch order of the direct ones (the side stream's launches are issued between
        # the trunk's in both), so no case needs a multiset comparison
        assert cg.ops == cd.ops, (i, cg.cmd, [p for p in zip(cg.ops, cd.ops) if p[0] != p[1]][:3], len(cg.ops), len(cd.ops))
        # The host-side bounds of the matcher and the gather pass (sim_device.c: T()) follow which detections the host has seen complete. On
        # a busy GPU the two runs differ in that: a replay's staging event is recorded on the instance stream, so waiting for it tells the
        # host that every earlier detection is done, which the direct run's event on the upload stream does not. Idle, they are equal too.
        assert busy or cg.bounds == cd.bounds, (i, cg.cmd)
        assert cg.ret == cd.ret and cg.errors == cd.errors, (i, cg.cmd)
        assert not cd.cache, (i, cd.cmd)             # VKSIFT_GRAPH=0 captures nothing


def observations(call):
    """per detection with an octave that the call launched on the VKSIFT_GRAPH=0 instance: did it end with the feature posting, and was device memory
    freed in front of it (the scratch re-allocated)"""
    out, freed, i, lines = [], False, 0, call.lines
    while i < len(lines):
        t = lines[i].split()
        freed |= t[0] == "free" and t[1] == "D"
        if len(t) > 2 and t[1] == "op" and t[2] == "extract_keypoints_multi":
            rest = [l.split()[2] for l in lines[i + 1:] if l.startswith("#") and l.split()[1] == "op"]
            k = [j for j, n in enumerate(rest) if n.startswith("descriptors_multi")][0]
            out.append({"post": not (len(rest) > k + 1 and rest[k + 1] == "post_words"), "grew": freed})
            freed = False
        i += 1
    return out


def flat(events):
    out = []
    for e in events:
        if e[0] == "drop":
            out += [("destroy", x) for x in e[1]]
        elif e[0] == "evict":
            out += [("destroy", e[1])] if e[1] is not None else []
        elif e[0] == "capture":
            out += ([("destroy", e[2])] if e[2] is not None else []) + [("capture", e[1])]
        else:
            out.append(e)
    return out


def check_policy(script, g, d):
    """the cache events of every call against the model; returns the model (its launches, its final state)"""
    m = Model(script, graph_env="1" if script["env"].get("VKSIFT_GRAPH") == "1" else None)
    live = set()
    for i, (cg, cd) in enumerate(zip(g, d)):
        if cg.cmd[0] in ("destroy", "ledger"):
            break
        want = flat(m.step(i, cg.cmd, observations(cd)))
        assert cg.cache == want, (i, cg.cmd, cg.cache, want)
        for kind, x in cg.cache:
            assert (x in live) == (kind != "capture"), (i, kind, x)     # replayed and destroyed execs are live ones, a capture makes a new one
            live = live - {x} if kind == "destroy" else live | {x}
        assert cg.live_execs == len(live) <= GRAPH_CACHE, (i, cg.live_execs, live)
    return m


def both(harness, script, prelude=()):
    return harness(script, "1" if script["env"].get("VKSIFT_GRAPH") == "1" else None, prelude), harness(script, "0", prelude)


def clean_end(calls):
    assert calls[-1].cmd[0] == "ledger" and calls[-1].ledger == dict(blocks=0, streams=0, events=0, execs=0, violations=0), calls[-1].lines
    assert not any(c.violations for c in calls)


# ---------------------------------------------------------------------------------------------------------------- named scripts
def events_of(calls, kind):
    return [(i, x) for i, c in enumerate(calls) for k, x in c.cache if k == kind]


def prove_cycle10(s, g, d, m):
    det = [i for i, c in enumerate(g) if c.cmd[0] == "detect"]
    assert len(det) == 90
    caps, destroys = events_of(g, "capture"), events_of(g, "destroy")
    assert len(caps) == GIVE_UP_AFTER and not events_of(g, "replay")
    # captures 9 .. 32 and the miss that gives up evict an exec each: 25 evictions, the last by detection 33, which captures nothing
    evictions = [(i, x) for i, x in destroys if g[i].cmd[0] == "detect"]
    assert len(evictions) >= 25 and evictions[24][0] == det[GIVE_UP_AFTER] and not g[det[GIVE_UP_AFTER]].cache[1:]
    assert [x for _, x in evictions] == list(range(25))                  # least recently used = oldest capture, in order
    assert all(not g[i].cache for i in det[GIVE_UP_AFTER + 1:]) and len(det[GIVE_UP_AFTER + 1:]) >= 50     # 5 more rounds, no capture ever again
    assert not m.use_graphs


def prove_comeback(s, g, d, m):
    det = [c for c in g if c.cmd[0] == "detect"]
    assert [c.cache for c in det[:8]] == [[("capture", i)] for i in range(8)]
    assert det[8].cache == [("destroy", 0), ("capture", 8)]               # the ninth key evicts the first
    assert det[9].cache == [("destroy", 1), ("capture", 9)] and det[9].cmd == det[0].cmd      # the first key again: recaptured
    assert det[10].cache == [("replay", 9)]                               # ... and then replayed


def prove_hit_resets(s, g, d, m, misses=30):
    det = [c for c in g if c.cmd[0] == "detect"]
    kinds = [[k for k, _ in c.cache if k != "destroy"] for c in det]
    assert kinds == ([["capture"]] * misses + [["replay"]]) * 2           # no give-up: the second run of misses still captures
    assert m.use_graphs and m.miss_run == 0


def prove_grow_drop(s, g, d, m):
    det = [c for c in g if c.cmd[0] == "detect"]
    assert det[0].cache == [("capture", 0)] and det[1].cache == [("capture", 1)]
    narrow = det[2]
    assert narrow.cmd[1:3] == PS.NARROW
    # the allocation log: scale-space and extraction scratch freed and re-allocated larger, every exec destroyed
    assert len(narrow.frees) >= 5 and sum(b for _, _, b in narrow.allocs) > sum(b for _, _, b in narrow.frees)
    assert narrow.cache == [("destroy", 0), ("destroy", 1), ("capture", 2)]
    assert det[3].cache == [("capture", 3)] and det[3].cmd == det[0].cmd  # recaptured (C1 silent: the run's exit status)
    assert det[4].cache == [("replay", 3)]
    assert det[5].cache == [("capture", 4)] and det[5].cmd == det[1].cmd


def prove_defer_grow(s, g, d, m):
    assert m.det_cap >= 8 and m.pingpong and m.overlap_min == 8
    counts = [n for _, n, _ in m.launches]
    assert counts == [1, 1, 1, 2, 4, 5, 1, 1, 1, 1], counts                 # the run of 12: one direct, batches of 2 and 4 that fill the capacity, the rest
    drops = [c for c in g if c.cmd[0] == "detect" and any(k == "destroy" for k, _ in c.cache)]
    assert len(drops) == 3                                                # capacity 2, 4, 8: each re-allocation drops the cache
    tail = [c for c in g if c.cache and c.cmd[0] != "destroy"][-4:]
    assert [k for c in tail for k, _ in c.cache] == ["capture", "replay", "replay", "capture"]   # single detections afterwards: recaptured and replayed


def prove_dense_flip(s, g, d, m):
    cached = [c for c in g if c.cache and c.cmd[0] == "detect"]
    assert [c.cache for c in cached] == [[("capture", 0)], [("capture", 1)], [("capture", 2)], [("replay", 2)], [("capture", 3)]]
    first_match = [i for i, c in enumerate(g) if c.cmd[0] == "match"][0]
    assert len(g[first_match].allocs) >= 2                                # the first matching creates the cache blocks
    names = lambda c: [n for n, _ in c.ops]
    assert cached[2].cmd == cached[0].cmd and names(cached[2]) == names(cached[0]) and cached[2].ops != cached[0].ops   # same launches, dense rows in the arguments
    second_match = [c for c in g if c.cmd[0] == "match"][1]
    assert "gather_sections" not in names(second_match) and "gather_sections" in names(g[first_match])   # the detection left the rows behind itself


def prove_post_flip(s, g, d, m):
    det = [c for c in g if c.cmd[0] == "detect"]
    posted = [o["post"] for c in d if c.cmd[0] == "detect" for o in observations(c)]
    assert posted == [True] * (PS.POST_IDLE + 1) + [False] * 2 + [True]     # the 17th unfetched posting switches it off, the download on again
    assert [c.cache for c in det] == [[("capture", 0)]] + [[("replay", 0)]] * PS.POST_IDLE + [[("capture", 1)], [("replay", 1)], [("replay", 0)]]


def prove_two_pointers(s, g, d, m):
    det = [c for c in g if c.cmd[0] == "batchdev"]
    assert [c.cache for c in det] == [[("capture", 0)], [("capture", 1)], [("replay", 0)], [("replay", 1)], [("replay", 0)], [("replay", 1)]]
    assert det[0].ops != det[1].ops and det[2].ops == det[0].ops and det[3].ops == det[1].ops


def prove_describe_table(s, g, d, m):
    det = [c for c in g if c.cmd[0] == "detect"]
    desc = [c for c in g if c.cmd[0] == "describe"]
    assert det[0].cache == [("capture", 0)] and det[1].cache == [("replay", 0)]
    assert desc[0].cache == [("destroy", 0)] and not desc[1].cache         # the first describe call extends the table and drops the cache, once
    assert det[2].cache == [("capture", 1)] and det[3].cache == [("replay", 1)] and det[4].cache == [("replay", 1)]
    assert [n for n, _ in det[2].ops] == [n for n, _ in det[0].ops] and det[2].ops != det[0].ops   # the same launches, the new table length in them


def prove_batch_profile(s, g, d, m):
    import api_model as A
    p = A.PROFILES["batch"]
    assert s["env"] == p["env"] and (s["create"]["bc"], s["create"]["nbuf"]) == (p["bc"], p["nbuf"])
    assert s["create"]["max_px"] == max(w * h for w, h in A.SIZES) and {c.cmd[1:3] for c in g if c.cmd[0] in ("detect", "batch")} == set(A.SIZES)
    # what the library does under this profile: every detection with an octave overlaps (batch capacity 8: one scale-space stream of its
    # own from the first image on), an overlapped detection is never captured, so NOTHING is ever captured or replayed
    assert len(m.launches) >= 10 and not any(e for _, _, e in m.launches)
    assert not any(c.cache for c in g) and not any("capbegin" in l for c in g for l in c.lines)


def prove_cycle10_device(s, g, d, m):
    det = [c for c in g if c.cmd[0] == "batchdev"]
    assert [c.cache for c in det] == [[("capture", i)] for i in range(8)] + [[("destroy", i - 8), ("capture", i)] for i in range(8, 20)]
    assert not any(k in ("sync", "esync") for c in det for _, k, _ in c.counted if c.cache[0][0] != "destroy")   # the host waits for nothing but evictions


def detections(g):
    return [c for c in g if c.cmd[0] in ("detect", "batch", "batchdev")]


def touches_cache(c):
    return bool(c.cache) or any("capbegin" in l or "launch x" in l for l in c.lines)


def prove_above_limit(s, g, d, m):
    limit = PS.LIMIT[0] * PS.LIMIT[1]
    assert s["create"]["max_px"] > limit and "VKSIFT_GRAPH" not in s["env"]
    pixels = lambda c: c.cmd[1] * c.cmd[2] * (c.cmd[4] if c.cmd[0] == "batch" else 1)
    over = [c for c in detections(g) if pixels(c) > limit]
    under = [c for c in detections(g) if pixels(c) <= limit]
    assert len(over) == 5 and not any(touches_cache(c) for c in over)      # a single image and a batch above the limit: queued directly, every time
    assert {pixels(c) for c in over} == {800 * 600, 2 * 480 * 360} and limit in {pixels(c) for c in under}
    assert [c.cache for c in under] == [[("capture", 0)], [("replay", 0)], [("capture", 1)], [("replay", 1)], [("replay", 0)]]   # at the limit and below: cached
    assert m.miss_run == 0


def prove_two_buffers(s, g, d, m):
    assert s["env"]["VKSIFT_PYR_PINGPONG"] == "2" and len(detections(g)) == 5 and not any(touches_cache(c) for c in g)
    # the image without an octave does not overlap (the same calls on the one-buffer instance capture it: one_buffer_overlap), so it is the
    # two-buffer clause of replay_ok that decides; the allocation log shows the second scale-space buffer
    assert s["ops"] == PS.SCRIPTS["one_buffer_overlap"]["ops"] and s["create"] == PS.SCRIPTS["one_buffer_overlap"]["create"]
    assert not any(e for _, _, e in m.launches) and m.miss_run == 0


def prove_one_buffer_overlap(s, g, d, m):
    tiny = [c for c in detections(g) if c.cmd[1:3] == PS.TINY]
    assert [c.cache for c in tiny] == [[("capture", 0)], [("replay", 0)], [("replay", 0)]]
    assert not any(touches_cache(c) for c in detections(g) if c.cmd[1:3] != PS.TINY) and len(detections(g)) == 5


def prove_miss_run(s, g, d, m, overlap=False):
    shape = PS.TINY if overlap else PS.BIG
    prof, misses, others = 0, [], []
    for c in g:
        prof = c.cmd[1] if c.cmd[0] == "prof" else prof
        if c.cmd[0] == "detect":
            (misses if c.cmd[1:3] == shape and c.cmd[3] < 10 and not prof else others).append(c)
    assert len(misses) == 36 and len(others) == (4 if overlap else 5)
    assert not any(touches_cache(c) for c in others)                       # profiled / above the limit / overlapped: no lookup, no capture
    if not overlap:
        assert {(c.cmd[1:3] == PS.OVER) for c in others} == {True, False} and any(c.cmd[0] == "describe" for c in g)
    first_other, last_other = g.index(others[0]), g.index(others[-1])
    assert g.index(misses[19]) < first_other and last_other < g.index(misses[20])       # 20 misses in front of them, the rest behind
    captured = [any(k == "capture" for k, _ in c.cache) for c in misses]
    # had one of the ineligible calls counted as a miss, the give-up would come that many detections early
    assert captured == [True] * GIVE_UP_AFTER + [False] * 4 and not any(k == "replay" for c in misses for k, _ in c.cache)
    assert not any(touches_cache(c) for c in misses[GIVE_UP_AFTER + 1:]) and not m.use_graphs


PROOFS = {"above_limit": prove_above_limit, "two_buffers": prove_two_buffers, "one_buffer_overlap": prove_one_buffer_overlap, "miss_run": prove_miss_run,
          "miss_run_overlap": lambda s, g, d, m: prove_miss_run(s, g, d, m, True), "cycle10": prove_cycle10, "cycle10_device": prove_cycle10_device, "cycle10_unsync": prove_cycle10, "comeback": prove_comeback, "hit_resets": prove_hit_resets,
          "hit_resets_short": lambda s, g, d, m: prove_hit_resets(s, g, d, m, 10), "grow_drop": prove_grow_drop, "defer_grow": prove_defer_grow,
          "dense_flip": prove_dense_flip, "post_flip": prove_post_flip, "two_pointers": prove_two_pointers, "batch_profile": prove_batch_profile,
          "describe_table": prove_describe_table}


@pytest.mark.parametrize("name", sorted(PS.SCRIPTS))
def test_named_script_reaches_its_edge(harness, name):
    s = PS.SCRIPTS[name]
    g, d = both(harness, s)
    check_replay_equals_direct(g, d)
    m = check_policy(s, g, d)
    clean_end(g), clean_end(d)
    PROOFS[name](s, g, d, m)


@pytest.mark.parametrize("name", ["cycle10_unsync", "cycle10_device", "comeback", "hit_resets_short"])
def test_no_exec_is_destroyed_in_flight(harness, name):
    """busy GPU: nothing completes unless the host waits for it. An eviction must not destroy an exec whose last launch the host has not seen
    complete (C3). A detection of host images waits for the staging buffer, which the previous replay released on the instance stream;
    cycle10_device has no such wait: nothing at all lies between the launch of an exec and its eviction eight detections later"""
    s = PS.SCRIPTS[name]
    g, d = both(harness, s, ["busy 1"])
    check_replay_equals_direct(g, d, busy=True)
    check_policy(s, g, d)
    clean_end(g), clean_end(d)
    assert len([1 for i, _ in events_of(g, "destroy") if g[i].cmd[0] in ("detect", "batchdev")]) >= 2


def test_every_gpu_script_is_proven_here():
    assert set(PS.GPU_SCRIPTS) <= set(PROOFS) and set(PS.SCRIPTS) == set(PROOFS)


# ---------------------------------------------------------------------------------------------------------------- the matrix
def matrix_ops(ups):
    shapes = [PS.BIG, PS.SMALL, (120, 160), PS.NARROW] + ([] if ups else [(64, 24)])      # (64, 24) without up-sampling: below a single octave
    ops = []
    for w, h in shapes:
        for rep in range(2):
            ops += [("detect", w, h, 0), ("download", 0)]
        # a run of plain detections with nothing asked in between: under VKSIFT_DEFER=1 the second and third are staged and launched as one batch
        ops += [("detect", w, h, 4), ("detect", w, h, 5), ("detect", w, h, 6), ("download", 4), ("download", 6)]
        for count in (2, 7, 1):
            for rep in range(2):
                ops += [("batch", w, h, 1, count), ("download", 1), ("num", count)]
        for which in (0, 1, 0):
            ops += [("batchdev", w, h, 3, 1, which), ("download", 3)]
        ops += [("batchdev", w, h, 2, 7, 1), ("num", 8), ("batchdev", w, h, 2, 7, 1), ("download", 2), ("match", 2, 3)]
    return ops


BASE = dict(ups=1, fp16=0, busy=0, covered=1, env={"VKSIFT_DEFER": "0"})
MATRIX = {
    "base": {},
    "no_upsampling": dict(ups=0),
    "fp16": dict(fp16=1),
    "busy": dict(busy=1),
    "not_covered": dict(covered=0),
    "no_fork": dict(env={"VKSIFT_DEFER": "0", "VKSIFT_FORK_SCALES": "0"}),
    "no_lds_chain": dict(env={"VKSIFT_DEFER": "0", "VKSIFT_LDS_CHAIN": "0"}),
    "chain_refuses_busy_fp16": dict(env={"VKSIFT_DEFER": "0", "VKSIFT_LDS_CHAIN": "refuse"}, busy=1),
    "deferred": dict(env={"VKSIFT_DEFER": "1"}),
    "deferred_no_fork_not_covered": dict(env={"VKSIFT_DEFER": "1", "VKSIFT_FORK_SCALES": "0", "VKSIFT_LDS_CHAIN": "0"}, covered=0, ups=0),
    "graph_always_no_posting": dict(env={"VKSIFT_DEFER": "0", "VKSIFT_GRAPH": "1", "VKSIFT_POST_FEATURES": "0"}),
}


def variant(v, ops=None, bc=7):
    v = dict(BASE, **v)
    script = dict(env=v["env"], create=PS.create(bc=bc, nbuf=12, ups=v["ups"], fp16=v["fp16"]), ops=ops if ops is not None else matrix_ops(v["ups"]))
    return script, ["busy %d" % v["busy"], "covered %d" % v["covered"]]


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_replay_equals_direct_and_policy_over_the_switch_matrix(harness, name):
    script, prelude = variant(MATRIX[name])
    g, d = both(harness, script, prelude)
    check_replay_equals_direct(g, d, busy="busy 1" in prelude)
    m = check_policy(script, g, d)
    clean_end(g), clean_end(d)
    # the matrix means something: captures and replays both happened, at every batch size, and the narrow shape grew the scratch
    eligible = {n for _, n, e in m.launches if e}
    assert eligible >= {1, 2, 7} and len(events_of(g, "replay")) >= 15 and len(events_of(g, "capture")) >= 15
    assert any(o["grew"] for c in d for o in observations(c)) == bool(script["create"]["ups"])    # (without up-sampling no shape of this area outgrows it)
    # deferred submission: batches that no batch entry point asked for exist exactly under VKSIFT_DEFER=1, one per shape at least
    staged = [(call, n) for call, n, _ in m.launches if n > 1 and g[call].cmd[0] not in ("batch", "batchdev")]
    assert (len(staged) >= 4) == (script["env"]["VKSIFT_DEFER"] == "1") and (staged or script["env"]["VKSIFT_DEFER"] == "0"), staged
    assert all(g[call].cmd[0] in ("detect", "download") for call, _ in staged)


def random_script(seed):
    r = random.Random(seed)
    v = dict(ups=r.choice((1, 1, 0)), fp16=r.choice((0, 0, 1)), busy=r.choice((0, 1)), covered=r.choice((1, 1, 0)),
             env={"VKSIFT_DEFER": r.choice("01"), "VKSIFT_FORK_SCALES": r.choice("11" "0"), "VKSIFT_LDS_CHAIN": r.choice(("1", "1", "0", "refuse"))})
    bc = r.choice((1, 7))
    shapes = [PS.BIG, PS.BIG, PS.SMALL, PS.SMALL, (120, 160), PS.NARROW] + ([] if v["ups"] else [(64, 24)])
    ops, prof = [], 0
    home = [(r.choice(shapes[:5]), r.randrange(12)) for _ in range(3)]    # most detections come back to a few (shape, buffer) pairs: replays
    while len(ops) < 60:
        (w, h), b = r.choice(home) if r.random() < 0.7 else (r.choice(shapes), r.randrange(12))
        k = r.random()
        if k < 0.45:
            for i in range(r.choice((1, 1, 1, 2, 3, 5))):              # runs of plain detections: staged and launched as batches when deferred
                ops.append(("detect", w, h, (b + i) % 12) if b + i < 12 else ("detect", w, h, i))
            if r.random() < 0.7:
                ops.append((r.choice(("download", "download", "num", "avail")), ops[-1][3]))
        elif k < 0.6 and bc > 1:
            n = r.choice((1, 2, 7))
            ops.append(("batch", w, h, min(b, 12 - n), n))
        elif k < 0.7:
            n = r.choice((1, 2, 7)) if bc > 1 else 1
            ops.append(("batchdev", w, h, min(b, 12 - n), n, r.randrange(2)))
        elif k < 0.78:
            ops.append(("match", r.randrange(12), r.randrange(12)))
        elif k < 0.84:
            prof ^= 1
            ops.append(("prof", prof))
        elif k < 0.9:
            # (shapes inside the reservation: the model does not tell a describe call's scratch growth from that of its keypoint staging)
            dw, dh = r.choice((PS.BIG, PS.SMALL))
            ops.append(("describe", dw, dh, r.randrange(12), r.choice((0, 5, 40))))
        elif k < 0.95 and v["busy"]:
            ops.append(("drain",))
        else:
            ops.append((r.choice(("download", "num", "avail")), r.randrange(12)))
    script, prelude = variant(v, ops, bc)
    return script, prelude


@pytest.mark.parametrize("seed", range(24))
def test_random_scripts_replay_equals_direct_and_follow_the_policy(harness, seed):
    script, prelude = random_script(seed)
    assert len(script["ops"]) >= 60
    g, d = both(harness, script, prelude)
    check_replay_equals_direct(g, d, busy="busy 1" in prelude)
    check_policy(script, g, d)
    clean_end(g), clean_end(d)


def test_random_scripts_reach_the_cache():
    """(no harness: the model alone) the random scripts together capture, replay, evict and drop; kept apart so that a seed change cannot empty them"""
    # the observations are the model's defaults here (no posting, no growth): enough to count what the walks reach
    kinds = {}
    for seed in range(24):
        script, _ = random_script(seed)
        m = Model(script)
        for i, op in enumerate(script["ops"]):
            for e in m.step(i, op, []):
                kinds[e[0]] = kinds.get(e[0], 0) + 1
    assert kinds.get("capture", 0) > 100 and kinds.get("replay", 0) > 50 and kinds.get("drop", 0) >= 3, kinds


# ---------------------------------------------------------------------------------------------------------------- failure paths
def failure_script(k, warm):
    """the k-th counted call of the TARGET detection fails. Buffer 0 holds features of another shape when it comes (so "empty" and "unchanged" can be
    told apart; the device reports other counts from the target on, so that they differ from the target's own), the posting slots exist (the failing call is all launches). warm: the target's key has been captured: the target is a replay"""
    big, small = ("detect", 160, 120, 0), ("detect", 96, 64, 0)
    ops = [big, ("download", 0)] if warm else [("detect", 160, 120, 1), ("download", 1)]
    ops += [small, ("download", 0), ("counts", 5), ("failin", k), big, ("avail", 0), ("num", 0), big, ("download", 0), big, ("download", 0)]
    return dict(env={"VKSIFT_DEFER": "0"}, create=PS.create(), ops=ops)


@pytest.mark.parametrize("graph,warm", [("1", False), ("1", True), ("0", False)])
def test_every_call_of_a_detection_fails_in_turn(harness, graph, warm):
    """a capturing detection, a replay and a directly queued detection; every counted call of each fails in turn"""
    clean = harness(failure_script(0, warm), graph)
    t = [i for i, c in enumerate(clean) if c.cmd[0] == "failin"][0] + 1
    target, before = clean[t], clean[t - 3]
    want = {("1", False): ["capture"], ("1", True): ["replay"], ("0", False): []}[(graph, warm)]
    assert target.cmd[0] == "detect" and [k for k, _ in target.cache] == want
    assert before.cmd[0] == "download" and before.ret["n"] > 0 and clean[t + 2].ret["n"] > 0 and clean[t + 2].ret["n"] != before.ret["n"]
    kinds = [(kind, name) for _, kind, name in target.counted]
    n_calls, reported, failed_kinds = len(kinds), 0, set()
    assert n_calls >= (4 if warm else 15)
    for k in range(1, n_calls + 1):
        calls = harness(failure_script(k, warm), graph)
        det, avail, num, again, third = calls[t], calls[t + 1], calls[t + 2], calls[t + 3], calls[t + 5]
        assert any("FAIL" in l for l in det.lines), k
        clean_end(calls)                                                   # C2: no capture left open; C3: destroy leaves a clean ledger
        if not det.errors:
            assert kinds[k - 1][0] == "capbegin", (k, kinds[k - 1])         # a capture that cannot start is no failure: the sequence is queued directly
            continue
        reported += 1
        failed_kinds.add(kinds[k - 1])
        assert det.errors == [VULKAN_ERROR] and det.ret["errors"] == 1, k
        assert avail.ret["ok"] == 1, k                                     # complete ...
        early = all(kind == "esync" for kind, _ in kinds[:k])
        if early:
            # the wait for the staging buffer, in front of everything: nothing was queued, marked or captured (detect_failed with no context).
            # Nothing changed: the buffer holds what it held, and the next detection does what this one would have done
            assert num.ret["n"] == before.ret["n"], k
        else:
            assert num.ret["n"] == 0, k                                    # ... and empty: the features it held are gone, none of the call's arrived
        assert not again.errors and again.ret["errors"] == 0, k
        if graph == "1":
            # captured afresh, whatever failed once the call had touched the instance
            assert [kind for kind, _ in again.cache if kind != "destroy"] == (want if early else ["capture"]), (k, again.cache)
            assert [kind for kind, _ in third.cache] == ["replay"], (k, third.cache)
            assert again.ops == clean[t + 3].ops                           # ... the whole sequence again
    assert reported >= n_calls - 1
    if graph == "1" and not warm:
        assert {("cop", "seed_upsampled"), ("capend", "s0")} <= failed_kinds and any(k == "launch" for k, _ in failed_kinds), failed_kinds
    if warm:
        assert any(k == "launch" for k, _ in failed_kinds), failed_kinds     # the replay's own launch


def test_a_failed_eviction_wait_fails_the_detection_and_destroys_nothing_in_flight(harness):
    """busy GPU, device input over nine buffers: the ninth detection evicts the first exec and waits for its last launch first. If that wait fails
    the exec must not be destroyed while it may be executing (C3, through the run's exit status): the detection fails, the streams are drained,
    the cache is dropped behind them, and the next detection captures afresh"""
    def script(k):
        ops = [("batchdev", 160, 120, b, 1, 0) for b in range(8)] + [("failin", k), ("batchdev", 160, 120, 8, 1, 0), ("avail", 8), ("num", 8),
                                                                     ("batchdev", 160, 120, 8, 1, 0), ("batchdev", 160, 120, 8, 1, 0), ("download", 8)]
        return dict(env={"VKSIFT_DEFER": "0"}, create=PS.create(), ops=ops)
    clean = harness(script(0), None, ["busy 1"])
    target = clean[9]
    assert target.cache == [("destroy", 0), ("capture", 8)]
    waits = [i for i, (_, kind, _) in enumerate(target.counted) if kind == "esync"]
    assert waits == [0]                                                    # the eviction's wait, in front of the destruction; the host waits for nothing else
    calls = harness(script(1), None, ["busy 1"])
    det, avail, num, again, third = calls[9:14]
    assert det.errors == [VULKAN_ERROR] and avail.ret["ok"] == 1 and num.ret["n"] == 0
    assert det.cache == [("destroy", x) for x in range(8)] and any(" sync s0" in l for l in det.lines)     # dropped, behind a drained stream
    assert det.lines.index([l for l in det.lines if " sync s0" in l][0]) < det.lines.index("xdestroy x0")
    assert again.cache == [("capture", 8)] and third.cache == [("replay", 8)] and not again.errors
    clean_end(calls)
