"""How results come back to the caller, on the simulated device (no GPU): the strategies of vksift_downloadFeatures and of the plain matching's
download, read from the operation log of tests/native/sim_device.c — the harness and the build of tests/test_pair_plan.py (tests/plan_build.py).

What is checked:
  * strategy choice — which of the posted records, the one-buffer packed copy, the packed copy of a whole batch (staged through pinned memory in
    chunks, or read by DMA into a page-locked destination) and the per-section copies serves a download, for every situation of SCRIPTS;
  * the drain — an in-place pass behind a direct packed download begins with a wait on the download stream, behind a staged one it does not;
  * failure paths — every counted call of a download of each strategy fails in turn, on an instance that never took the strategy and on one
    that did: conditions (1)-(4) of check_failure.
The scripts are data (SCRIPTS, failure_ops): a refactoring of the download path is held to the log they produce, byte for byte.
"""
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_detect_plan import VULKAN_ERROR
from test_pair_plan import DL_BATCH_MIN, H, W, detections, pairs, sim  # noqa: F401  (sim: the fixture)

FEAT_BYTES = 164
N = DL_BATCH_MIN
NO_POSTING = (("VKSIFT_DEFER", "0"), ("VKSIFT_POST_FEATURES", "0"))


def batch(n=N, first=0):
    return ("batch", W, H, first, n)


def walk(cmd, n=N, first=0):
    return [(cmd, b) for b in range(first, first + n)]


def in_place(kind, n=N):
    return {"budget": ("budget", 0, n, 100), "grid": ("grid", 0, n, 100, W, H, 4, 4), "rootsift": ("rootsift", 0, n)}[kind]


# name: (operations, how the instance is made and the device behaves)
SCRIPTS = {
    "posted": ([("detect", W, H, 0), ("download", 0), ("detect", W, H, 1), ("downloadp", 1)], {}),
    "not posted": ([("detect", W, H, 0), ("download", 0), ("detect", W, H, 1), ("downloadp", 1)], dict(env=NO_POSTING)),
    "batch of 7": ([batch(N - 1)] + 2 * walk("download", N - 1) + [batch(N - 1)] + 2 * walk("downloadp", N - 1), {}),
    "pageable walk": ([batch()] + 2 * walk("download"), {}),
    # 64 buffers of 600 records: 6.3 MB, two chunks of the staged copy
    "pageable walk in chunks": ([("counts", 1000), ("batch", W, H, 0, 64)] + walk("download", 64), dict(bc=64, nbuf=64)),
    "page-locked walk": ([batch()] + 2 * walk("downloadp") + walk("download", 2), {}),
    # (busy alone says nothing: the download has waited for the batch, the device is idle as far as the library knows. A detection queued behind it is not)
    "page-locked walk, busy": ([batch()] + walk("downloadp"), dict(busy=1, late=1)),
    "page-locked walk, detection queued": ([batch(), ("num", 0), ("detect", W, H, 9)] + walk("downloadp"), dict(busy=1, late=1)),
    "uploaded buffer": ([batch(), ("upload", 3, 10)] + walk("download"), {}),
    "refilled buffer": ([batch(), ("detect", W, H, 5)] + walk("download"), dict(env=NO_POSTING)),
    "left the ring": ([batch()] + [("detect", W, H, b) for b in (8, 9, 10, 11)] + walk("download"), dict(env=NO_POSTING)),
    "second batch": ([batch()] + walk("download", 3) + [batch()] + walk("download", 3, 2), {}),
    # what else takes the records away from a copy that exists: the one-buffer copy of another buffer goes through the same staging pair; a batch refills a posted buffer
    "one-buffer copy in between": ([batch()] + walk("download", 2) + [("detect", W, H, 9), ("download", 9), ("download", 2), ("download", 3)], dict(env=NO_POSTING)),
    "posted, then refilled": ([("detect", W, H, 0), ("download", 0), batch(), ("download", 0), ("download", 1), ("download", 2)], {}),
    "pairs, page-locked": (detections(8) + [("bmatch", N, *pairs(N))] + 2 * [("mdlp", p) for p in range(N)], dict(bc=8)),
    "drain, direct": ([op for k in ("budget", "grid", "rootsift") for op in [batch()] + walk("downloadp", 2) + [in_place(k)]] + walk("download"), {}),
    "drain, staged": ([op for k in ("budget", "grid", "rootsift") for op in [batch()] + walk("download", 2) + [in_place(k)]] + walk("download"), {}),
}


def script(sim, name):
    ops, how = SCRIPTS[name]
    r, calls = sim(ops, **dict(dict(bc=8, nbuf=12), **how))
    r.clean()
    return [c for c in calls if c.cmd[0] in ("download", "downloadp", "mdl", "mdlp")], calls


# ---------------------------------------------------------------------------------------------------------------- reading a download's log
def names(c):
    return [name for _, name, _ in c.issued]


def counted(c, kind):
    return sum(1 for _, k, _ in c.counted if k == kind)


def own_blocks(c):
    """the blocks the harness made for the call: allocated and released inside it (the page-locked destination)"""
    return {b for _, b, _ in c.allocs} & {b for _, b, _ in c.frees}


def copies(c):
    """(destination is the caller's page-locked block, bytes) of every device-to-host copy"""
    return [(a["dst"][0] in own_blocks(c), a["dst"][3]) for _, name, a in c.issued if name == "memcpy_d2h"]


def nothing_issued(c):
    return not c.issued and not c.counted and not [a for a in c.allocs if a[1] not in own_blocks(c)]


def one_buffer_packed(c):
    """one pack launch into the staging pair, one copy of this buffer's records into pinned staging, one wait for the stream"""
    return names(c) == ["pack_features", "memcpy_d2h"] and copies(c) == [(False, c.ret["n"] * FEAT_BYTES)] and counted(c, "sync") == 1 and counted(c, "rec") == 0


def builds_batch_copy(c):
    return counted(c, "rec") > 0


def per_section(c):
    return names(c) and set(names(c)) == {"memcpy_d2h"} and sum(b for _, b in copies(c)) == c.ret["n"] * FEAT_BYTES and counted(c, "sync") == 1 and not counted(c, "rec")


def all_served(dl):
    assert all(c.ret["n"] == 9 or c.cmd[0][0] == "m" for c in dl) and not any(c.errors or c.ret["poison"] for c in dl)


# ---------------------------------------------------------------------------------------------------------------- strategy choice
def test_a_posted_detection_is_downloaded_without_the_device(sim):
    dl, _ = script(sim, "posted")
    all_served(dl)
    for c in dl:
        assert not c.issued and not [a for a in c.allocs if a[1] not in own_blocks(c)] and [k for _, k, _ in c.counted] == ["esync"], c.lines      # the wait for the detection, nothing else


def test_without_posting_one_pack_one_copy_one_wait(sim):
    dl, _ = script(sim, "not posted")
    all_served(dl)
    assert all(one_buffer_packed(c) for c in dl), [c.lines for c in dl]


def test_seven_images_never_get_a_packed_batch_copy(sim):
    dl, _ = script(sim, "batch of 7")
    all_served(dl)
    assert len(dl) == 4 * (N - 1) and all(one_buffer_packed(c) for c in dl)


def test_a_pageable_walk_of_eight(sim):
    dl, _ = script(sim, "pageable walk")
    all_served(dl)
    assert one_buffer_packed(dl[0])
    total = N * 9 * FEAT_BYTES
    assert names(dl[1]) == ["pack_features", "memcpy_d2h"] and copies(dl[1]) == [(False, total)] and counted(dl[1], "rec") == 1 and counted(dl[1], "esync") == 1 and not counted(dl[1], "sync")
    assert all(nothing_issued(c) for c in dl[2:]), [c.lines for c in dl[2:]]


def test_a_pageable_walk_in_chunks(sim):
    dl, _ = script(sim, "pageable walk in chunks")
    assert not any(c.errors or c.ret["poison"] for c in dl)
    total = sum(c.ret["n"] for c in dl) * FEAT_BYTES
    assert 4 << 20 < total <= 8 << 20
    assert one_buffer_packed(dl[0])
    # one launch packs all 64 buffers; the copy goes in two pieces with an event each; the second download waits for the first piece only
    assert names(dl[1]) == ["pack_features", "memcpy_d2h", "memcpy_d2h"] and [b for _, b in copies(dl[1])] == [total // 2, total - total // 2]
    assert counted(dl[1], "rec") == 2 and counted(dl[1], "esync") == 1
    waits = [i for i, c in enumerate(dl) if i > 1 and c.counted]
    assert len(waits) == 1 and [k for _, k, _ in dl[waits[0]].counted] == ["esync"] and not dl[waits[0]].issued        # the first buffer whose records end in the second piece
    assert sum(c.ret["n"] for c in dl[:waits[0] + 1]) * FEAT_BYTES > total // 2 >= sum(c.ret["n"] for c in dl[:waits[0]]) * FEAT_BYTES


def test_a_page_locked_walk_of_eight_on_an_idle_device(sim):
    dl, _ = script(sim, "page-locked walk")
    all_served(dl)
    assert one_buffer_packed(dl[0])
    one = 9 * FEAT_BYTES
    # pack launches and the event behind them; no copy into the staging block, this buffer's records straight into the caller's
    assert names(dl[1]) == ["pack_features", "memcpy_d2h"] and copies(dl[1]) == [(True, one)] and counted(dl[1], "rec") == 1 and counted(dl[1], "sync") == 1
    for c in dl[2:2 * N]:
        assert names(c) == ["memcpy_d2h"] and copies(c) == [(True, one)] and [k for _, k, _ in c.counted] == ["op", "sync"], c.lines
    # a pageable destination of the same detection: a plain copy out of the device block
    for c in dl[2 * N:]:
        assert names(c) == ["memcpy_d2h"] and copies(c) == [(False, one)] and counted(c, "sync") == 1


def test_a_page_locked_walk_behind_a_queued_detection_is_staged(sim):
    dl, _ = script(sim, "page-locked walk, detection queued")
    all_served(dl)
    assert one_buffer_packed(dl[0])
    assert names(dl[1]) == ["pack_features", "memcpy_d2h"] and copies(dl[1]) == [(False, N * 9 * FEAT_BYTES)] and counted(dl[1], "rec") == 1 and counted(dl[1], "esync") == 1
    assert all(nothing_issued(c) for c in dl[2:])
    # busy, but nothing queued behind the batch: the library has seen it complete, the copy is direct
    dl, _ = script(sim, "page-locked walk, busy")
    all_served(dl)
    assert copies(dl[1]) == [(True, 9 * FEAT_BYTES)] and all(copies(c) == [(True, 9 * FEAT_BYTES)] for c in dl[2:])


def test_buffers_outside_their_batch_take_the_per_buffer_paths(sim):
    dl, _ = script(sim, "uploaded buffer")
    assert not any(c.errors or c.ret["poison"] for c in dl)
    # the second download finds a buffer of the range refilled (the upload): no packed batch copy for this detection, ever
    assert not any(builds_batch_copy(c) for c in dl)
    assert dl[3].ret["n"] == 10 and per_section(dl[3]) and len(names(dl[3])) == 1
    assert all(one_buffer_packed(c) for i, c in enumerate(dl) if i != 3)
    dl, _ = script(sim, "refilled buffer")
    all_served(dl)
    assert not any(builds_batch_copy(c) for c in dl) and all(one_buffer_packed(c) for c in dl)
    dl, _ = script(sim, "left the ring")
    all_served(dl)
    assert not any(builds_batch_copy(c) for c in dl) and all(one_buffer_packed(c) for c in dl)


def test_a_second_batch_is_not_served_the_first_one_s_copy(sim):
    dl, _ = script(sim, "second batch")
    all_served(dl)
    assert one_buffer_packed(dl[0]) and builds_batch_copy(dl[1]) and nothing_issued(dl[2])
    # buffer 2 is in the cached copy of the first batch: the second batch's records are fetched anew
    assert [k for _, k, _ in dl[3].counted][0] == "esync" and one_buffer_packed(dl[3])
    assert builds_batch_copy(dl[4]) and nothing_issued(dl[5])


def test_a_copy_is_not_served_once_its_records_are_gone(sim):
    dl, _ = script(sim, "one-buffer copy in between")
    all_served(dl)
    assert builds_batch_copy(dl[1]) and one_buffer_packed(dl[2])
    assert builds_batch_copy(dl[3]) and nothing_issued(dl[4])             # the staging pair held buffer 9's records: packed again
    dl, _ = script(sim, "posted, then refilled")
    all_served(dl)
    assert not dl[0].issued and one_buffer_packed(dl[1]) and builds_batch_copy(dl[2]) and nothing_issued(dl[3])    # slot 0 still holds the single detection's records


def test_pairs_into_a_page_locked_destination_are_never_packed(sim):
    dl, _ = script(sim, "pairs, page-locked")
    assert len(dl) == 2 * N and not any(c.errors or c.ret["poison"] for c in dl)
    for c in dl:
        assert names(c) == ["memcpy_d2h"] and copies(c)[0][0] and counted(c, "sync") == 1, c.lines


# ---------------------------------------------------------------------------------------------------------------- the drain
@pytest.mark.parametrize("how", ["direct", "staged"])
def test_an_in_place_pass_waits_for_a_direct_packed_download_only(sim, how):
    dl, calls = script(sim, "drain, " + how)
    all_served(dl)
    dl_stream = {l.split()[3] for c in dl for l in c.lines if " op memcpy_d2h " in l}
    assert len(dl_stream) == 1
    passes = [c for c in calls if c.cmd[0] in ("budget", "grid", "rootsift")]
    assert [c.cmd[0] for c in passes] == ["budget", "grid", "rootsift"] and not any(c.errors for c in passes)
    for c in passes:
        first = c.lines[0].split()[1:]
        assert (first == ["sync", dl_stream.copy().pop()]) == (how == "direct"), (c.cmd, c.lines[:2])
        assert counted(c, "sync") == (1 if how == "direct" else 0)


# ---------------------------------------------------------------------------------------------------------------- failure paths
# entry: (what the instance has done before, the download that fails, the downloads behind it, how the instance is made)
ENTRIES = {
    "posted": ([("detect", W, H, 0)], ("download", 0), [], {}),
    "one-buffer packed": ([("detect", W, H, 0)], ("download", 0), [], dict(env=NO_POSTING)),
    "batch packed, pageable": ([batch(), ("download", 0)], ("download", 1), walk("download", 3, 2), {}),
    "batch packed, page-locked": ([batch(), ("downloadp", 0)], ("downloadp", 1), walk("downloadp", 3, 2), {}),
    "batch packed, page-locked, later buffer": ([batch(), ("downloadp", 0), ("downloadp", 1)], ("downloadp", 2), walk("downloadp", 3, 3), {}),
    "per-section": ([("upload", 0, 10)], ("download", 0), [], {}),
}
# the failures the library absorbs by design, by the counted call that fails: every step of a packed copy falls back to the next strategy down
# (batch -> one buffer -> per section), which serves the same records. What is reported: a failure of the last strategy's own copy or wait.
ABSORBED = {
    # (what the library does today, not a design: wait_for_buffer() drops the error code of its wait for the detection, so the failed wait is neither
    # reported nor repeated and the records are served as if it had passed — NOTEBOOK.md, "Result downloads")
    "posted": ("esync",),
    "one-buffer packed": ("alloc", "pack_features", "memcpy_d2h", "sync"),
    "batch packed, pageable": ("alloc", "pack_features", "memcpy_d2h", "evcreate", "rec", "esync"),
    "batch packed, page-locked": ("alloc", "pack_features", "memcpy_d2h", "evcreate", "rec", "sync"),
    "batch packed, page-locked, later buffer": ("memcpy_d2h", "sync"),
    "per-section": (),
}


def failure_ops(name, warm, k):
    before, call, behind, how = ENTRIES[name]
    # a later call: the instance has taken the strategy once (its staging, rows and events exist) and produced the same state again
    # (the wait for the detection belongs to the count in front of the download: only the posted download, which has no other counted call, keeps it)
    ops = (before + [call] + behind if warm else []) + before + [("num", call[1])] * (name != "posted") + [("failin", k), call, ("failin", 0), call] + behind + walk("download", 1, call[1])
    return ops, len(ops) - len(behind) - 4, how


def check_failure(name, warm, k, r, clean, at):
    calls, ref = r.calls[6:], clean.calls[6:]
    what = (name, warm, k, ref[at].counted[k - 1][1:])
    r.clean()                                                       # (4) no violation, no poison served, a clean ledger after destroy
    target, again, behind = calls[at], calls[at + 2], calls[at + 3:-2]
    assert any("FAIL" in l for l in target.lines), what
    # (1) absorbed by the fallback — the same record count, no poison — or reported exactly once with VKSIFT_VULKAN_ERROR
    if target.errors:
        assert target.errors == [VULKAN_ERROR], (what, target.errors)
    else:
        assert target.ret == ref[at].ret and not target.ret["poison"], (what, target.ret)
    kind = ref[at].counted[k - 1][1:]
    assert (not target.errors) == (kind[0] in ABSORBED[name] or kind[1] in ABSORBED[name]), (what, target.errors, target.lines)
    # (2) the same download again succeeds and serves no poison
    assert not again.errors and again.ret == ref[at + 2].ret and not again.ret["poison"], (what, again.ret)
    # (3) a packed copy whose build (or serve) failed is never served afterwards: the next download of the batch fetches its records anew
    if behind and "batch" in name:
        assert builds_batch_copy(again), (what, again.lines)
    for c, want in zip(behind, ref[at + 3:-2]):
        assert not c.errors and c.ret == want.ret and not c.ret["poison"], (what, c.cmd, c.ret)


@pytest.mark.parametrize("warm", [False, True], ids=["first call", "later call"])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_call_of_a_download_fails_in_turn(sim, name, warm):
    ops, at, how = failure_ops(name, warm, 0)
    kw = dict(dict(bc=8, nbuf=12, busy=1, late=1, allocs=1), **how)
    clean, calls = sim(ops, **kw)
    clean.clean()
    n = len(calls[at].counted)
    assert calls[at].cmd == ENTRIES[name][1] and not calls[at].errors and n >= 1, (name, n)
    with ThreadPoolExecutor(max_workers=8) as pool:
        runs = list(pool.map(lambda k: sim(failure_ops(name, warm, k)[0], **kw)[0], range(1, n + 1)))
    for k, r in enumerate(runs, 1):
        check_failure(name, warm, k, r, clean, at)
    if not warm and "packed" in name and "later" not in name:
        assert any(kind == "alloc" for _, kind, _ in calls[at].counted), name      # a first call allocates: refused allocations are among the failures
