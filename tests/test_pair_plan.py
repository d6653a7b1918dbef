"""The stages behind a matching on the simulated device (no GPU): the batch and filtered matchings, the verifications, the refits, guided matching,
the tracks, the in-place passes, upload and export, driven through the public API by tests/native/plan_harness.c over tests/native/sim_device.c —
the harness of tests/test_detect_plan.py, one build for both files (tests/plan_build.py), address and undefined-behaviour sanitizers included.
Provoking a device error on a GPU is off limits, so the ~1 500 lines of host code behind HIP_CHECK / goto gpu_error can be tested here only.

What is checked:
  * named scripts — every stage behind a filtered matching of 1, 2 and batch_cap pairs, idle and on a busy device whose postings arrive late, with
    repeated buffers, a list longer than VKSIFT_HIP_MATCH_SLOTS, stage pairs that share a pinned table with no accessor in between, an in-place
    pass between matching and stage, a staged detection run: no VIOLATION (C1-C5), no poison served, a repeated call logs what the first did, a
    clean ledger;
  * the invalidation table — after every step every accessor is served or refused as tests/api_model.py's sets say (ACCESSORS and SETS are
    imported; which step drops which set is api_model.Model's rule, restated in Table below in five lines: any matching drops every set, a filtered
    one brings "filtered" back, a verification of m drops "refined m"). Tracks are not in that model; include/vksift_ext.h: dropped by any matching,
    kept across a new verification or refit;
  * failure paths — every counted call (allocations and event creations included) of every entry fails in turn, on an instance that never ran the
    entry and on one that did: assertions (a)-(g) of check_failure;
  * 24 seeded random scripts over the whole command set, held to the table, the hard checks and the ledger.
"""
import random
from concurrent.futures import ThreadPoolExecutor
import os
import re
import subprocess

import pytest

import plan_build
from api_model import ACCESSORS, INVALID_INPUT, SETS
from test_detect_plan import VULKAN_ERROR, parse

ACC = list(ACCESSORS)                    # `acc K PAIR` of the harness takes the index
W, H = 160, 120
DL_BATCH_MIN, MATCH_SLOTS = 8, 256       # VKSIFT_DL_BATCH_MIN, VKSIFT_HIP_MATCH_SLOTS
# which argument of which launcher is which result's device storage (the roles of include/vksift_hip.h, as the device logs them)
WRITES = {("filter_matches", "out"): "filtered", ("filter_matches", "out_n"): "filtered", ("ransac_homography", "results"): "H", ("ransac_homography", "masks"): "H",
          ("ransac_fundamental", "results"): "F", ("ransac_fundamental", "masks"): "F", ("refit_homography", "results"): "refined H",
          ("refit_homography", "masks_out"): "refined H", ("refit_fundamental", "results"): "refined F", ("refit_fundamental", "masks_out"): "refined F",
          ("match_guided", "out"): "guided", ("match_guided", "out_n"): "guided", ("build_tracks", "node_words"): "tracks", ("build_tracks", "tracks"): "tracks",
          ("build_tracks", "stats"): "tracks"}
DERIVED = {"H": ["refined H"], "F": ["refined F"], "plain": list(SETS) + ["tracks"], "filtered": [s for s in SETS if s != "filtered"] + ["tracks", "plain"]}
READS_BUFFERS = ("feats_base", "cache_desc")     # an operation that names the SIFT buffers' records or their matcher cache entries


# ---------------------------------------------------------------------------------------------------------------- running
class Run:
    def __init__(self, r):
        self.rc, self.err, self.calls = r.returncode, r.stderr, parse(r.stdout)
        for c in self.calls:
            annotate(c)

    def clean(self):
        assert self.rc == 0, "\n".join(l for c in self.calls for l in c.violations)[-3000:] + self.err[-3000:]
        last = self.calls[-1]
        assert last.cmd[0] == "ledger" and last.ledger == dict(blocks=0, streams=0, events=0, execs=0, violations=0), last.lines
        served_poison = [c.cmd for c in self.calls if c.ret.get("poison") and not c.errors]     # (what a call that reported an error left behind is nobody's result)
        assert not served_poison, served_poison


def annotate(c):
    """c.issued: the operations the call issued, [(line index, name, {argument: (block, offset, role, extent)})]; c.waits: line indices of host waits"""
    c.issued, c.waits = [], []
    for i, line in enumerate(c.lines):
        t = line.split()
        if t[0].startswith("#") and t[1] == "op":
            c.issued.append((i, t[2], {}))
        elif t[0] == "args":
            for a in t[2:]:
                m = re.match(r"(\w+)=([^:]+):([rw]):(\d+)$", a)
                if not m:       # (the log of a run the sanitizer ended: its exit status fails the test)
                    continue
                name, blk, role, ext = m.groups()
                b, _, off = blk.partition("+")
                c.issued[-1][2][name] = (b, int(off or 0), role, int(ext))
        elif t[0].startswith("#") and t[1] in ("sync", "esync"):
            c.waits.append(i)


@pytest.fixture(scope="module")
def sim():
    exe = plan_build.executable()
    memo = {}

    def run(ops, bc=4, nbuf=12, env=(("VKSIFT_DEFER", "0"),), busy=0, late=0, allocs=0):
        cmds = ["create %d %d 600 %d 1 0" % (bc, W * H, nbuf), "counts 3", "roles 1", "late %d" % late, "busy %d" % busy, "countallocs %d" % allocs]
        cmds += [" ".join(str(t) for t in op) for op in ops] + ["destroy", "ledger"]
        key = (tuple(env), tuple(cmds))
        if key not in memo:
            e = {k: v for k, v in os.environ.items() if not k.startswith("VKSIFT_")}
            e.update(dict(env))
            memo[key] = Run(subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True, env=e))
        r = memo[key]
        return r, r.calls[6:]
    return run


def detections(bc, nbuf=6):
    return ([("batch", W, H, 0, min(bc, nbuf))] if bc > 1 else []) + [("detect", W, H, b) for b in range(min(bc, nbuf) if bc > 1 else 0, nbuf)]


def pairs(n, ids=((0, 1), (2, 3), (1, 1), (4, 0), (0, 1), (5, 2))):
    """n pairs over six buffers: repeated buffers, a repeated pair, a pair of a buffer with itself"""
    return [x for i in range(n) for x in ids[i % len(ids)]]


def filtered(n, cross=1):
    return ("filtered", cross, n, *pairs(n))


def probes(table, at=(0,)):
    """every accessor, at the pairs of `at` (-1: the last pair that has results, -2: the first that has none)"""
    ops = []
    for p in at:
        for i, name in enumerate(ACC):
            n = table.sets[ACCESSORS[name]]
            ops.append(("acc", i, p if p >= 0 else (max((n or 1) - 1, 0) if p == -1 else (n or 0))))
        n = table.plain
        ops += [("mnum", p if p >= 0 else (max((n or 1) - 1, 0) if p == -1 else (n or 0)))]
    return ops + [("mdl", 1), ("tstats",), ("tdl",), ("tfeat", table.pairs[0] if table.pairs else 0)]


# ---------------------------------------------------------------------------------------------------------------- the table
class Table:
    """which accessor is served: the six sets of tests/api_model.py (a count of pairs, or None: refused), the plain matching's pairs, the tracks"""

    def __init__(self):
        self.sets, self.plain, self.tracks, self.pairs = {s: None for s in SETS}, None, False, None

    def step(self, op):
        """applies a stage or matching command; False: the call must be refused with VKSIFT_INVALID_INPUT_ERROR and change nothing"""
        k, n = op[0], self.sets["filtered"]
        if k in ("bmatch", "filtered", "pmatch", "match"):
            count = {"bmatch": op[1], "filtered": op[2], "pmatch": 1, "match": 1}[k]
            self.sets, self.tracks, self.plain, self.pairs = {s: None for s in SETS}, False, count, None
            if k == "filtered":
                self.sets["filtered"], self.pairs = count, list(op[3:])
        elif k == "verify":
            if n is None:
                return False
            self.sets["HF"[op[1]]], self.sets["refined " + "HF"[op[1]]] = n, None
        elif k == "refine":
            if self.sets["HF"[op[1]]] is None:
                return False
            self.sets["refined " + "HF"[op[1]]] = n
        elif k == "guided":
            if n is None or (not op[2] and self.sets["HF"[op[1]]] is None):
                return False
            self.sets["guided"] = n
        elif k == "tracks":
            need = [["filtered"], ["filtered", "H"], ["filtered", "F"], ["filtered", "refined H"], ["filtered", "refined F"], ["guided"]][op[1]]
            if n is None or any(self.sets[s] is None for s in need):
                return False
            self.tracks = True
        return True

    def served(self, c):
        k = c.cmd[0]
        if k == "acc":
            n = self.sets[ACCESSORS[ACC[c.cmd[1]]]]
            return n is not None and c.cmd[2] < n
        if k == "mnum":
            return self.plain is not None and c.cmd[1] < self.plain
        if k == "mdl":
            return self.plain is not None and c.cmd[1] < self.plain
        if k in ("tstats", "tdl"):
            return self.tracks
        if k == "tfeat":
            return self.tracks and c.cmd[1] in self.pairs
        return None


def check_probe(table, c):
    want = table.served(c)
    if want is None:
        return
    assert c.ret["served"] == int(want) and c.errors == ([] if want else [INVALID_INPUT]), (c.cmd, want, c.ret, c.errors)
    assert not c.ret["poison"], c.cmd


def table_of(ops):
    table = Table()
    for op in ops:
        table.step(op)
    return table


def follow(calls, table=None):
    """walks the calls of a script: stage calls against Table.step, accessors against Table.served; returns the table"""
    table = table or Table()
    for c in calls:
        if c.cmd[0] in STAGES:
            ok = table.step(c.cmd)
            assert c.errors == ([] if ok else [INVALID_INPUT]), (c.cmd, c.errors)
            assert ok or not c.issued, c.cmd
        else:
            check_probe(table, c)
            assert c.cmd[0] in ("acc", "mnum", "mdl", "tstats", "tdl", "tfeat") or not c.errors, (c.cmd, c.errors)
    return table


def test_the_harness_names_the_accessors_as_the_model_does(sim):
    _, calls = sim([("accnames",)])
    assert [l.split(" ", 2)[2] for l in calls[0].lines if l.startswith("accname")] == ACC


# ---------------------------------------------------------------------------------------------------------------- named scripts
def all_stages():
    """every stage once, consecutive ones sharing their pinned tables (h_vtab: verify -> refine -> verify; h_gtab: guided -> guided; the tracks'
    table: every source in turn), repeated calls side by side, no accessor anywhere"""
    ops = [("verify", 0, 128, 7), ("refine", 0, 2), ("verify", 0, 128, 7), ("verify", 0, 128, 7), ("verify", 1, 128, 7), ("refine", 1, 2), ("refine", 1, 2),
           ("refine", 0, 2), ("guided", 0, 0, 1), ("guided", 1, 1, 0), ("guided", 1, 1, 0), ("guided", 0, 0, 1)]
    return ops + [("tracks", s) for s in (0, 1, 2, 3, 4, 5, 5, 0)]


def without_gathers(c):
    return [o for o in c.ops if o[0] != "gather_sections"]


def check_repeats(calls):
    """a call that repeats the one in front of it issues the same operations with the same arguments (a matching's first call also fills the cache)"""
    seen = 0
    for a, b in zip(calls, calls[1:]):
        if a.cmd == b.cmd and a.cmd[0] in ("filtered", "bmatch", "verify", "refine", "guided", "tracks", "budget", "grid", "rootsift"):
            assert without_gathers(a) == b.ops and not b.errors, (a.cmd, a.ops, b.ops)
            seen += 1
    return seen


@pytest.mark.parametrize("busy", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_every_stage_behind_a_filtered_matching(sim, n, busy):
    ops = detections(4) + [filtered(n), filtered(n), filtered(n)] + all_stages()
    table = table_of(ops)
    ops += probes(table, at=(0, -1, -2)) + [("bmatch", n, *pairs(n)), ("bmatch", n, *pairs(n))]
    r, calls = sim(ops, busy=busy, late=busy)
    r.clean()
    t = follow(calls[:-2])
    assert t.plain == n and not t.tracks
    assert check_repeats(calls) == 7
    # the tables are shared: one block each, whoever reads them
    tabs = {name: {a[arg][0] for c in calls for _, op, a in c.issued if op == name} for name, arg in (("gather_correspondences", "slot_tab"), ("gather_xy", "slot_tab"))}
    assert all(len(v) == 1 for v in tabs.values()), tabs


def test_the_busy_device_means_something(sim):
    """the script above, busy: the host waited for its tables (and for nothing else) between the stages, and every posting arrived late"""
    _, calls = sim(detections(4) + [filtered(2), filtered(2), filtered(2)] + all_stages(), busy=1, late=1)
    stages = [c for c in calls if c.cmd[0] in ("verify", "guided", "tracks")]
    assert {k: sum(1 for c in stages if c.cmd[0] == k and c.waits) for k in ("verify", "guided", "tracks")} == dict(verify=3, guided=3, tracks=7)     # every call but the first
    assert all(len(c.waits) <= 1 for c in stages)
    assert not any(c.waits for c in calls if c.cmd[0] == "refine")


def test_a_table_is_not_rewritten_under_the_launch_that_reads_it(sim):
    """busy, and nothing waits between the calls: each stage runs again behind a matching of OTHER pairs, so the pinned table it fills differs from
    the one its previous launch may still be reading (C5 hashes the bytes; a table rewritten with the same bytes would pass unseen)"""
    other = ("filtered", 1, 2, 3, 2, 5, 4)
    stages = [("verify", 0, 128, 7), ("guided", 1, 1, 0), ("tracks", 0)]
    ops = detections(4) + [filtered(2)] + stages + [other] + stages + [filtered(4)] + stages + [("refine", 0, 2), ("guided", 0, 0, 1), ("tracks", 3), other, ("verify", 1, 128, 7),
                                                                                              ("guided", 1, 0, 1), ("tracks", 2)]
    r, calls = sim(ops, busy=1, late=1)
    r.clean()
    follow(calls[:-2])
    tabs = [a[arg] for c in calls for _, op, a in c.issued for arg in ("slot_tab", "src") if arg in a and op in ("gather_correspondences", "gather_xy", "memcpy_h2d") and c.cmd[0] in STAGES]
    assert len(tabs) >= 12 and all(blk != "-" and ext > 0 for blk, _, _, ext in tabs)         # pinned, and hashed over their whole extent


@pytest.mark.parametrize("busy", [0, 1])
def test_batches_on_both_sides_of_the_packed_download(sim, busy):
    """VKSIFT_DL_BATCH_MIN pairs and more are fetched by one packed copy from the second download on; fewer never"""
    for n, packed in ((DL_BATCH_MIN - 1, False), (DL_BATCH_MIN, True)):
        ops = detections(8) + [("bmatch", n, *pairs(n))] + [("mnum", p) for p in range(n)] + [("mdl", p) for p in range(n)] + [("mnum", n), ("mdl", n)]
        ops += [filtered(n, 0), ("mdl", 0), ("mdl", n - 1), ("acc", 1, n - 1), ("mdl0",), ("mnum0",)]
        r, calls = sim(ops, bc=8, busy=busy, late=busy)
        r.clean()
        follow(calls[:-2])
        copies = [name for c in calls if c.cmd[0] == "mdl" for _, name, _ in c.issued]
        assert ("memcpy2d_d2h" in copies) == packed and copies.count("memcpy2d_d2h") == (2 if packed else 0), copies


def test_a_pair_list_longer_than_one_launch_sequence(sim):
    n = MATCH_SLOTS + 4
    ops = detections(4) + [filtered(n), ("verify", 0, 64, 1), ("refine", 0, 1), ("guided", 0, 0, 1), ("tracks", 3), ("tracks", 5)]
    r, calls = sim(ops + probes(table_of(ops), at=(0, -1, -2)), bc=n, nbuf=n, busy=1, late=1)
    r.clean()
    follow(calls[:-2])
    assert [name for _, name, _ in calls[len(detections(4))].issued].count("filter_matches") == 2      # two runs of launches, the second into the slots behind the first


@pytest.mark.parametrize("busy", [0, 1])
def test_an_in_place_pass_between_matching_and_stage(sim, busy):
    ops = detections(4) + [filtered(2), ("budget", 0, 2, 100), ("budget", 0, 2, 100), ("verify", 0, 128, 7), ("grid", 1, 3, 100, W, H, 4, 4), ("refine", 0, 2), ("rootsift", 0, 6),
                           ("rootsift", 0, 6), ("guided", 0, 0, 1), ("tracks", 5), ("upload", 5, 10), ("tracks", 0), ("export", 5), ("export", 0), ("verify", 1, 128, 7)]
    r, calls = sim(ops + probes(table_of(ops), at=(0, -1, -2)) + [("avail", b) for b in range(6)], busy=busy, late=busy)
    r.clean()
    follow(calls[:-2])
    assert check_repeats(calls) == 2


def test_a_staged_detection_run_is_launched_by_the_stage(sim):
    """VKSIFT_DEFER=1: plain detections staged when the stage arrives are launched by it, in front of its own launches"""
    run = [("detect", W, H, b) for b in (6, 7, 8)]
    ops = detections(4) + [("num", 5), filtered(2)] + run + [("verify", 0, 128, 7)] + run + [("guided", 0, 0, 1)] + run + [("tracks", 1)] + run + [("budget", 6, 3, 50)]
    r, calls = sim(ops + probes(table_of(ops)), env=(("VKSIFT_DEFER", "1"),), busy=1, late=1)
    r.clean()
    follow(calls[:-2])
    for c in calls:
        if c.cmd[0] in ("verify", "guided", "tracks", "budget"):
            names = [name for name, _ in c.ops]       # (issued or replayed from a captured graph)
            assert "extract_keypoints_multi" in names and names.index("extract_keypoints_multi") < len(names) - 2, (c.cmd, names)


# ---------------------------------------------------------------------------------------------------------------- the invalidation table
TABLE_SCRIPT = [("verify", 0, 128, 7), ("tracks", 0), filtered(2), ("refine", 0, 2), ("guided", 0, 0, 1), ("tracks", 1), ("verify", 0, 128, 7), ("tracks", 3), ("refine", 0, 2),
                ("tracks", 3), ("verify", 0, 128, 9), ("tracks", 3), ("guided", 0, 0, 1), ("guided", 1, 0, 0), ("verify", 1, 128, 7), ("refine", 1, 2), ("tracks", 4),
                ("guided", 1, 0, 1), ("tracks", 5), ("verify", 1, 128, 7), ("refine", 0, 2), ("bmatch", 3, *pairs(3)), ("tracks", 0), ("verify", 0, 128, 7),
                filtered(4, 0), ("guided", 1, 1, 1), ("tracks", 5), ("tracks", 2), ("pmatch", 0, 1), ("refine", 0, 2), filtered(1), ("verify", 0, 128, 7), ("verify", 1, 128, 7),
                ("refine", 0, 2), ("refine", 1, 2), ("guided", 0, 0, 0), ("tracks", 4), filtered(3)]


@pytest.mark.parametrize("busy", [0, 1])
def test_the_invalidation_table_after_every_step(sim, busy):
    ops, table = detections(4), Table()
    for op in TABLE_SCRIPT:
        table.step(op)
        ops += [op] + probes(table, at=(0, -1, -2))
    r, calls = sim(ops, busy=busy, late=busy)
    r.clean()
    t = follow(calls[:-2])
    refused = sum(1 for c in calls if c.errors == [INVALID_INPUT])
    assert refused > 200 and sum(1 for c in calls if c.cmd[0] == "acc" and c.ret["served"]) > 200
    # the tracks' rule, stated here: a verification or a refit keeps them (steps 7-12 above), any matching drops them
    assert t.sets["filtered"] == 3 and not t.tracks


# ---------------------------------------------------------------------------------------------------------------- failure paths
FULL = [filtered(2), ("verify", 0, 128, 7), ("verify", 1, 128, 7), ("refine", 0, 2), ("refine", 1, 2), ("guided", 0, 0, 1), ("tracks", 1)]
# entry: (the call, what an instance needs before its FIRST such call, batch capacity)
ENTRIES = {
    "bmatch": (("bmatch", 2, *pairs(2)), [], 4),
    "filtered cross": (filtered(2), [], 4),
    "filtered": (filtered(2, 0), [], 4),
    "pmatch": (("pmatch", 2, 3), [], 4),
    "verify H": (("verify", 0, 128, 7), [filtered(2)], 4),
    "verify F": (("verify", 1, 128, 7), [filtered(2)], 4),
    "refine H": (("refine", 0, 2), [filtered(2), ("verify", 0, 128, 7)], 4),
    "refine F": (("refine", 1, 2), [filtered(2), ("verify", 1, 128, 7)], 4),
    "guided verified": (("guided", 0, 0, 1), [filtered(2), ("verify", 0, 128, 7)], 4),
    "guided supplied": (("guided", 1, 1, 0), [filtered(2)], 4),
    "tracks filtered": (("tracks", 0), [filtered(2)], 4),
    "tracks H": (("tracks", 1), [filtered(2), ("verify", 0, 128, 7)], 4),
    "tracks F": (("tracks", 2), [filtered(2), ("verify", 1, 128, 7)], 4),
    "tracks refined H": (("tracks", 3), [filtered(2), ("verify", 0, 128, 7), ("refine", 0, 2)], 4),
    "tracks refined F": (("tracks", 4), [filtered(2), ("verify", 1, 128, 7), ("refine", 1, 2)], 4),
    "tracks guided": (("tracks", 5), [filtered(2), ("guided", 0, 1, 1)], 4),
    "budget": (("budget", 0, 3, 100), [], 4),
    "grid": (("grid", 0, 3, 100, W, H, 4, 4), [], 4),
    "rootsift": (("rootsift", 0, 3), [], 4),
    "upload": (("upload", 1, 10), [], 4),
    # caller-supplied keypoints, both modes; the first call comes before any matching (no dense rows), the later one behind one (dense rows)
    "describe orient": (("describe", W, H, 1, 20, 0), [], 4),
    "describe given": (("describe", W, H, 1, 20, 1), [], 4),
    "profiled budget": (("budget", 0, 3, 100), [("prof", 1)], 4),
    "profiled grid": (("grid", 0, 3, 100, W, H, 4, 4), [("prof", 1)], 4),
    "profiled rootsift": (("rootsift", 0, 3), [("prof", 1)], 4),
    "export": (("export", 1), [], 4),
    "profiled verify": (("verify", 0, 128, 7), [("prof", 1), filtered(2)], 4),
    "times": (("times",), [("prof", 1), filtered(2), ("verify", 0, 128, 7)], 4),
    "avail": (("avail", 1), [filtered(2)], 4),
    "filtered number": (("acc", 0, 1), [filtered(2)], 4),
    "filtered download": (("acc", 1, 1), [filtered(2)], 4),
    "mask download": (("acc", 3, 1), [filtered(2), ("verify", 0, 128, 7)], 4),
    "match download": (("mdl", 1), [("bmatch", 2, *pairs(2))], 4),
    # (the packed copy is made by the second download after a matching: the first is the one among the accessors read in front of the call)
    "packed match download": (("mdl", 2), [("bmatch", 8, *pairs(8))], 8),
    "tracks download": (("tdl",), [filtered(2), ("tracks", 0)], 4),
    "feature tracks": (("tfeat", 1), [filtered(2), ("tracks", 0)], 4),
}
# a failure the library absorbs by design: the packed copy of all pairs falls back to the copy of the one pair asked for
ABSORBED = {"packed match download": ("alloc", "memcpy2d_d2h", "sync")}
STAGES = ("bmatch", "filtered", "pmatch", "verify", "refine", "guided", "tracks")
FIRST_CALL_ALLOCATES = ("bmatch", "filtered", "filtered cross", "pmatch", "verify H", "verify F", "refine H", "refine F", "guided verified", "guided supplied", "tracks filtered",
                        "tracks guided", "export", "packed match download", "profiled verify")


def failure_ops(name, warm, k, then=0):
    call, needs, bc = ENTRIES[name]
    table = Table()
    # a later call: the instance has run the entry, then every stage (every set is there to be kept or dropped), then what the entry needs beside them
    setup = needs + [call] + FULL + [op for op in needs if op[0] == "bmatch"] if warm else needs
    for op in setup:
        table.step(op)
    snap = probes(table) + [("num", 1)]
    # (failin K J: the J-th counted call behind the failure fails too; disarmed behind the call, so that it never reaches the accessors)
    ops = detections(bc) + setup + snap + [("counts", 5), ("failin", k, then), call, ("failin", 0)] + [("avail", b) for b in range(6)] + snap + [call] + [("drain",)] + snap
    at = len(detections(bc)) + len(setup) + len(snap) + 2
    return ops, at, len(snap), table, bc


def written_sets(r, target):
    """the result sets whose device storage an operation issued inside `target` names as written, and what derives from them"""
    owner = {}
    for c in r.calls:
        for _, name, args in c.issued:
            for arg, (blk, _, role, _) in args.items():
                if (name, arg) in WRITES and role == "w":
                    owner[blk] = WRITES[(name, arg)]
                if (name == "match_2nn_async" and arg in ("n_dev", "matches") and c.cmd[0] in ("bmatch", "pmatch")) or (name, arg) in (("filter_matches", "fwd"), ("filter_matches", "n_fwd")):
                    owner[blk] = "plain"        # (the forward matching's slots; a filtered matching's reverse pass has scratch of its own)
    hit = {owner[blk] for _, _, args in target.issued for blk, _, role, _ in args.values() if role == "w" and blk in owner}
    return hit | {d for s in hit for d in DERIVED.get(s, ())}


def set_of(c):
    k = c.cmd[0]
    return ACCESSORS[ACC[c.cmd[1]]] if k == "acc" else "plain" if k in ("mnum", "mdl") else "tracks" if k in ("tstats", "tdl", "tfeat") else None


def canon(c):
    """the call's operations modulo addresses: names and roles, blocks numbered in order of appearance (equal digests imply this)"""
    ids, out = {}, []
    for _, name, args in c.issued:
        if name != "gather_sections":
            out.append((name, tuple((a, ids.setdefault(b, len(ids)) if b != "-" else -1, off, role, ext) for a, (b, off, role, ext) in args.items())))
    return out


def check_failure(name, warm, k, r, clean, at, nsnap, table):
    calls, ref = r.calls[6:], clean.calls[6:]
    r.clean()       # (b) no VIOLATION, ranges balanced, sanitizers silent, and (g) a clean ledger after destroy
    target, kind = calls[at], ref[at].counted[k - 1][1:]
    snap0, avail, snap1, again, snap2 = calls[at - 2 - nsnap:at - 2], calls[at + 2:at + 8], calls[at + 8:at + 8 + nsnap], calls[at + 8 + nsnap], calls[at + 10 + nsnap:at + 10 + 2 * nsnap]
    what = (name, warm, k, kind)
    assert any("FAIL" in l for l in target.lines), what
    # (a) the error callback fired exactly once, with VKSIFT_VULKAN_ERROR
    if not target.errors and (kind[0] in ABSORBED.get(name, ()) or kind[1] in ABSORBED.get(name, ())):
        assert target.ret == ref[at].ret, what
    else:
        assert target.errors == [VULKAN_ERROR], (what, target.errors)
    # (c) a set that an issued launch wrote is refused by all its accessors; (d) every other set is served, unchanged
    hit = written_sets(r, target)
    for a, b in zip(snap0, snap1):
        s = set_of(a)
        if s in hit:
            assert b.errors == [INVALID_INPUT] or (a.errors == [INVALID_INPUT] and b.errors == a.errors), (what, "wrote", s, "yet served", b.cmd)
        elif s is not None:
            assert (a.ret, a.errors) == (b.ret, b.errors), (what, s, a.cmd, a.ret, b.ret)
    # (e) a buffer the call names is not reported available before the host has seen the stream pass an operation that reads it
    op = ENTRIES[name][0]
    named = set(op[3:]) if op[0] == "filtered" else set(op[2:]) if op[0] == "bmatch" else set(op[1:3]) if op[0] == "pmatch" else \
        set(range(op[1], op[1] + op[2])) if op[0] in ("budget", "grid", "rootsift") else {op[1]} if op[0] in ("upload", "export") else {op[3]} if op[0] == "describe" else \
        set(table.pairs or ())
    readers = [i for i, _, args in target.issued if any(a in READS_BUFFERS for a in args)]
    if readers and not any(w > readers[-1] for w in target.waits):
        for c in avail:
            assert c.ret["ok"] == 0 or c.cmd[1] not in named, (what, "buffer", c.cmd[1], "reported available behind", target.issued[-1][1])
    # an upload that fails behind its copy leaves the buffer complete and empty (never new bytes under the old section table); in front of it, unchanged
    if op[0] == "upload":
        copied = "memcpy_h2d" in [n for _, n, _ in target.issued]
        assert snap1[-1].cmd == ("num", op[1]) and snap1[-1].ret["n"] == (0 if copied else snap0[-1].ret["n"]) and snap0[-1].ret["n"] > 0, (what, snap1[-1].ret)
        assert snap2[-1].ret["n"] == op[2], (what, snap2[-1].ret)
    # (f) the same call again succeeds, and logs what it logs on an instance that never failed
    assert not again.errors, (what, again.errors)
    same_blocks = [(a[0], a[2]) for c in calls[:at + 9 + nsnap] for a in c.allocs] == [(a[0], a[2]) for c in ref[:at + 9 + nsnap] for a in c.allocs]
    want = ref[at + 8 + nsnap]
    if op[0] == "describe" and canon(again) != canon(want):
        # a describe call that failed in front of its once-per-instance work (the descriptor scale table, its staging) leaves it to the next one:
        # that one logs what the FIRST call of an instance that never failed logs
        want = ref[at]
    assert canon(again) == canon(want) and (not same_blocks or without_gathers(again) == without_gathers(want)), (what, again.ops, want.ops)
    assert again.ret.get("served", 1) == 1 and again.ret == want.ret, (what, again.ret, want.ret)
    for a, b in zip(ref[at + 10 + nsnap:at + 10 + 2 * nsnap], snap2):
        assert (a.ret, a.errors) == (b.ret, b.errors) and not b.ret.get("poison"), (what, a.cmd, a.ret, b.ret)


@pytest.mark.parametrize("warm", [False, True], ids=["first call", "later call"])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_call_of_an_entry_fails_in_turn(sim, name, warm):
    ops, at, nsnap, table, bc = failure_ops(name, warm, 0)
    clean, calls = sim(ops, bc=bc, busy=1, late=1, allocs=1)
    clean.clean()
    n = len(calls[at].counted)
    assert calls[at].cmd == ENTRIES[name][0] and not calls[at].errors and (n >= 1 or name in ("avail", "filtered number")), (name, n)
    assert name != "packed match download" or "memcpy2d_d2h" in [op for _, op, _ in calls[at].issued]
    with ThreadPoolExecutor(max_workers=8) as pool:
        runs = list(pool.map(lambda k: sim(failure_ops(name, warm, k)[0], bc=bc, busy=1, late=1, allocs=1)[0], range(1, n + 1)))
    for k, r in enumerate(runs, 1):
        check_failure(name, warm, k, r, clean, at, nsnap, table)
    if not warm and name in FIRST_CALL_ALLOCATES:
        assert any(kind in ("alloc", "evcreate") for _, kind, _ in calls[at].counted), name      # a first call allocates: refused allocations are among the failures


DOUBLE = ("bmatch", "filtered cross", "verify H", "refine F", "guided verified", "tracks H", "budget", "grid", "rootsift", "profiled budget")


@pytest.mark.parametrize("name", DOUBLE)
def test_the_error_exit_s_own_device_call_fails_too(sim, name):
    """every counted call fails in turn AND the next counted call behind it fails as well: where that is the record an error exit ends the sequence
    with (match_follow, the ring event), the exit falls back to a drained stream — assertions (a)-(g) hold all the same"""
    ops, at, nsnap, table, bc = failure_ops(name, True, 0)
    clean, calls = sim(ops, bc=bc, busy=1, late=1, allocs=1)
    n = len(calls[at].counted)
    with ThreadPoolExecutor(max_workers=8) as pool:
        runs = list(pool.map(lambda k: sim(failure_ops(name, True, k, 1)[0], bc=bc, busy=1, late=1, allocs=1)[0], range(1, n + 1)))
    drained = 0
    for k, r in enumerate(runs, 1):
        check_failure(name, True, k, r, clean, at, nsnap, table)
        lines = r.calls[6 + at].lines
        fails = [i for i, l in enumerate(lines) if " FAIL " in l]
        drained += len(fails) == 2 and any(" sync s" in l for l in lines[fails[1]:])
    assert drained >= 1, name            # the second failure did hit an error exit's own call, and the exit drained the stream


# ---------------------------------------------------------------------------------------------------------------- random scripts
def random_ops(seed):
    r = random.Random(seed)
    bc = r.choice((1, 2, 4, 8))
    busy = r.randrange(2)
    ops, table = detections(bc), Table()
    while len(ops) < 70:
        x = r.random()
        n = r.randint(1, bc)
        if x < 0.12:
            op = filtered(n, r.randrange(2))
        elif x < 0.17:
            op = ("bmatch", n, *pairs(n))
        elif x < 0.2:
            op = ("pmatch", r.randrange(6), r.randrange(6))
        elif x < 0.32:
            op = ("verify", r.randrange(2), r.choice((1, 128)), r.randrange(99))
        elif x < 0.42:
            op = ("refine", r.randrange(2), r.choice((1, 8)))
        elif x < 0.52:
            op = ("guided", r.randrange(2), r.randrange(2), r.randrange(2))
        elif x < 0.64:
            op = ("tracks", r.randrange(6))
        elif x < 0.7:
            first = r.randrange(6)
            op = r.choice([("budget", first, r.randint(1, 6 - first), r.choice((1, 100, 1000))), ("grid", first, r.randint(1, 6 - first), 50, W, H, r.randint(1, 16), r.randint(1, 16)),
                           ("rootsift", first, r.randint(1, 6 - first))])
        elif x < 0.74:
            op = r.choice([("upload", r.randrange(6), r.choice((0, 1, 600))), ("export", r.randrange(6)), ("detect", W, H, r.randrange(6)), ("prof", r.randrange(2)), ("times",)])
        elif x < 0.78 and busy:
            op = ("drain",)
        elif x < 0.82:
            op = r.choice([("avail", r.randrange(6)), ("num", r.randrange(6)), ("download", r.randrange(6)), ("mnum0",), ("mdl0",)])
        else:
            ops += r.sample(probes(table, at=(r.choice((0, -1, -2)),)), 4)
            continue
        table.step(op)
        ops.append(op)
    return ops + probes(table, at=(0, -2)), bc, busy


@pytest.mark.parametrize("seed", range(24))
def test_random_scripts_follow_the_table(sim, seed):
    ops, bc, busy = random_ops(seed)
    r, calls = sim(ops, bc=bc, busy=busy, late=busy, env=(("VKSIFT_DEFER", str(seed & 1)),))
    r.clean()
    follow(calls[:-2])


def test_random_scripts_reach_every_stage():
    """(no harness) kept apart so that a seed change cannot empty the walks"""
    done = {}
    for seed in range(24):
        table = Table()
        for op in random_ops(seed)[0]:
            if op[0] in ("verify", "refine", "guided", "tracks"):
                k = (op[0], table.step(op))
                done[k] = done.get(k, 0) + 1
            else:
                table.step(op)
    assert all(done.get((s, ok), 0) >= 8 for s in ("verify", "refine", "guided", "tracks") for ok in (True, False)), done


def random_failure_ops(seed):
    """a random script, then a stretch of calls somewhere in which one counted call fails: failures behind states no fixed setup has (an in-place
    pass, a half-built table, an upload in the pair list)"""
    ops, bc, busy = random_ops(seed)
    r = random.Random(1000 + seed)
    n, m, first = r.randint(1, bc), r.randrange(2), r.randrange(5)
    tail = [filtered(n, r.randrange(2)), r.choice([("budget", first, 2, 50), ("grid", first, 2, 50, W, H, 3, 3), ("rootsift", first, 2), ("upload", first, 7)]), ("verify", m, 64, seed),
            ("refine", m, 2), ("guided", m, r.randrange(2), 1), ("tracks", r.choice((0, 1 + m, 3 + m, 5))), ("export", r.randrange(6)), ("tracks", 0), ("times",)]
    r.shuffle(tail)
    return ops, [("counts", 5), ("failin", r.randint(1, 45))] + tail + [("failin", 0)], bc, busy


def test_random_scripts_with_a_failure_somewhere(sim):
    """(a) the call in which the failure falls reports VKSIFT_VULKAN_ERROR exactly once, every other call of the stretch is served or refused, never
    failed; (b) no VIOLATION, ranges balanced, sanitizers silent, no poison served; (g) a clean ledger — on whatever state the walk had reached"""
    def one(seed):
        ops, tail, bc, busy = random_failure_ops(seed)
        return sim(ops + tail, bc=bc, busy=busy, late=busy, allocs=1, env=(("VKSIFT_DEFER", str(seed & 1)),))[0], len(ops), len(tail)
    with ThreadPoolExecutor(max_workers=8) as pool:
        runs = list(pool.map(one, range(24)))
    failed_in = {}
    for seed, (r, n_ops, n_tail) in enumerate(runs):
        r.clean()
        calls = r.calls[6:]
        follow(calls[:n_ops])
        for c in calls[n_ops:n_ops + n_tail]:
            if any(" FAIL " in l for l in c.lines):
                assert c.errors == [VULKAN_ERROR], (seed, c.cmd, c.errors)
                failed_in[c.cmd[0]] = failed_in.get(c.cmd[0], 0) + 1
            else:
                assert c.errors in ([], [INVALID_INPUT]), (seed, c.cmd, c.errors)
    assert sum(failed_in.values()) >= 16 and len(failed_in) >= 5, failed_in
