"""The edge store launchers of include/vksift_hip.h called directly — vksift_hip_append_track_edges and vksift_hip_build_tracks_from_edges — not only
through the vksift_ext_* entries, which fix the strides, the tables and the counters. Each case: the launches, one synchronisation per comparison, and a
BYTE comparison of the whole poisoned arena (tests/hip_track_edges.py) with the restatement (tests/np_track_edges.py): the edges, the four statistics words,
the row table, and for a build the track records, the words of the stored rows and the track statistics must be there; every other byte — guards, stride
padding, edge records at and beyond nb_edges, the words behind the statistics, the rows that are not stored — must come back as it went in. Nothing is
compared with a tolerance. The equivalence tests compare append + build with vksift_hip_build_tracks on the same input, byte for byte.
tests/test_np_track_edges.py pins on the CPU what the restatement says."""
import numpy as np
import pytest

import hip_track_edges as HE
import hip_tracks as HT
import track_cases as TC
from hip_records import Launch

pytestmark = pytest.mark.gpu
u32 = np.uint32


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HE.bind(vk.lib())


def random_call(name, rows, slots, n, seed, **kw):
    """`slots` pairs of n records each between buffers drawn from rows {id: count}; every record names stored rows"""
    rng = np.random.default_rng(seed)
    ids = sorted(rows)
    pairs = []
    for _ in range(slots):
        a, b = (int(x) for x in rng.choice(ids, 2))
        pairs.append(TC.pair(a, b, np.stack([rng.integers(0, max(rows[a], 1), n), rng.integers(0, max(rows[b], 1), n)], axis=1)))
    return TC.case(name, [(b, rows[b]) for b in ids], pairs, **kw)


def store_case(name, calls, *, max_edges=None, nb_buffers=None, build=None, **kw):
    total = sum(len(p["recs"]) for c in calls for p in c["pairs"])
    top = max(b for c in calls for b, _ in c["bufs"])
    return dict(name=name, calls=calls, max_edges=total + 3 if max_edges is None else max_edges, nb_buffers=top + 2 if nb_buffers is None else nb_buffers, build=build, **kw)


def appended(L, case, check_each=True):
    h = HE.Store(case)
    for k, c in enumerate(case["calls"]):
        assert L.vksift_hip_track_edges_scratch_u32(len(c["pairs"]), c["max_n"]) == h.append_args[k]["scratch_u32"]    # exactly the words the library asks for
        rc = h.append(L, k)
        assert rc == 0, f"{h.what} call {k}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
        if check_each or k + 1 == len(case["calls"]):
            h.check(h.read(), h.expected(calls=k + 1, built=False))
    return h


ROWS = {2: 300, 3: 1, 5: 700, 9: 41}


# ------------------------------------------------------------------------------------------------------------------------ append: one call
@pytest.mark.parametrize("masked", [False, True], ids=["own count", "masked"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_append_one_call(L, n, masked):
    """1, 2 and 3 slots of n records: below, at and above one block of 256 and two"""
    for slots in (1, 2, 3):
        c = random_call(f"{slots} slots of {n}", ROWS, slots, n, seed=100 * slots + n)
        h = appended(L, store_case(c["name"], [TC.as_masked(c) if masked else c]))
        want = sum(min(p["n_dev"], c["max_n"]) for p in c["pairs"])
        assert h.restated()["nb_calls"] == 1 and len(h.restated()["edges"]) == want


def test_append_skips_a_pair_that_is_not_valid_between_two_that_are(L):
    c = TC.as_masked(random_call("valid 1 0 1", ROWS, 3, 300, seed=7))
    c["pairs"][1]["valid"] = 0
    h = appended(L, store_case(c["name"], [c]))
    s = h.restated()
    assert len(s["edges"]) == 600 and {e[0] for e in s["edges"]} | {e[2] for e in s["edges"]} <= set(ROWS)


@pytest.mark.parametrize("case", TC.masked_only_cases() + [TC.case_by_name("counts above max_n and max_rows"), TC.case_by_name("no edges")], ids=lambda c: c["name"])
def test_append_hand_cases(L, case):
    """mask bytes all 0, a pair whose model is not valid, record and row counts on the device above max_n and max_rows, a record that names a row that is not
    stored, pairs without records"""
    appended(L, store_case(case["name"], [case]))


# ------------------------------------------------------------------------------------------------------------------------ append: the store
def three_calls():
    return [random_call("first", {0: 50, 1: 60, 4: 70}, 3, 200, seed=1), random_call("second", {1: 60, 2: 300, 7: 10}, 2, 257, seed=2),
            random_call("third", {0: 50, 7: 10}, 4, 31, seed=3)]


def test_second_and_third_append_go_behind_what_the_store_holds(L):
    h = appended(L, store_case("three calls", three_calls()))
    s = h.restated()
    assert len(s["edges"]) == 600 + 514 + 124 and s["nb_calls"] == 3 and s["nb_changed_buffers"] == 0 and sorted(s["table"]) == [0, 1, 2, 4, 7]


@pytest.mark.parametrize("room", [0, -1, -124, -700], ids=["exactly met", "exceeded by one", "already full at the third call", "full within the second"])
def test_capacity(L, room):
    total = 600 + 514 + 124
    h = appended(L, store_case("capacity", three_calls(), max_edges=total + room))
    s = h.restated()
    assert len(s["edges"]) == total + room and s["nb_dropped"] == -room


def test_a_store_count_above_the_capacity_is_clamped(L):
    c = random_call("onto a count above the capacity", ROWS, 1, 3, seed=4)
    case = store_case(c["name"], [c], max_edges=10, preset_stats=(17, 2, 1, 5))
    h = HE.Store(case)
    assert h.append(L, 0) == 0
    exp = h.host.copy()
    h.put(exp, h.stats, 0, np.array([10, 5, 2, 5], u32))        # held = min(17, 10): full, three more dropped
    table = np.full(case["nb_buffers"], HE.UNSET, u32)
    table[sorted(ROWS)] = [ROWS[b] for b in sorted(ROWS)]
    h.put(exp, h.table, 0, table)
    h.check(h.read(), exp)


def test_a_row_count_that_changes_is_counted_and_the_table_kept(L):
    first = random_call("first", {0: 50, 1: 60}, 2, 40, seed=5)
    second = random_call("second", {0: 20, 1: 60, 3: 9}, 2, 40, seed=6)
    third = random_call("third", {0: 20, 1: 61}, 1, 5, seed=8)
    h = appended(L, store_case("changed rows", [first, second, third]))
    s = h.restated()
    assert s["table"] == {0: 50, 1: 60, 3: 9} and s["nb_changed_buffers"] == 3


def test_buffers_at_or_beyond_nb_buffers_are_not_recorded(L):
    c = random_call("ids beyond the table", {1: 30, 6: 30}, 2, 20, seed=9)
    h = appended(L, store_case(c["name"], [c], nb_buffers=4))
    assert h.restated()["table"] == {1: 30}


APPEND_REFUSALS = [dict(nslots=0), dict(nbufs=0), dict(max_n=0), dict(max_rows=0), dict(nb_buffers=0), dict(max_edges=0), dict(n_stride=0), dict(slot_tab_stride=1),
                   {"+records": 2}, {"+rec_slot_stride": 2}, {"+edges": 8}, {"+scratch": 2}, dict(rec_slot_stride=12), {"+scratch_u32": -1}]


@pytest.mark.parametrize("changes", APPEND_REFUSALS, ids=lambda d: " ".join(f"{k}={x}" for k, x in d.items()))
def test_append_refusals(L, changes):
    """hipErrorInvalidValue, and not a byte of the arena changed (the scratch included)"""
    h = HE.Store(store_case("refused", [random_call("refused", ROWS, 2, 300, seed=11)]))
    rc = h.append(L, 0, **changes)
    assert rc == HE.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(Launch.read(h), h.host)


def test_append_masked_refusals(L):
    h = HE.Store(store_case("refused", [TC.as_masked(random_call("refused", ROWS, 2, 30, seed=12))]))
    for changes in (dict(valid_stride=0), dict(mask_slot_stride=1)):
        assert h.append(L, 0, **changes) == HE.HIP_ERROR_INVALID_VALUE, changes
    h.check(Launch.read(h), h.host)


# ------------------------------------------------------------------------------------------------------------------------ build from edges
def build_case(name, bufs, edges, *, count=None, max_edges=None, nb_buffers=None, node_stride=None, max_rows=None, absent=()):
    edges = np.asarray(edges, u32).reshape(-1, 4)
    max_rows = max([n for _, n in bufs] + [1]) if max_rows is None else max_rows
    return dict(name=name, bufs=list(bufs), edges=edges, count=len(edges) if count is None else count, max_edges=max(len(edges), 1) if max_edges is None else max_edges,
                nb_buffers=max([b for b, _ in list(bufs) + list(absent)]) + 2 if nb_buffers is None else nb_buffers,
                node_stride=max_rows + 2 if node_stride is None else node_stride, max_rows=max_rows, absent=list(absent))


def chain_case(nbufs):
    """a chain through every buffer in a shuffled order, one edge beside it: crosses the presence group of 64 at 65 and 129"""
    ids = [3 + 2 * i for i in range(nbufs)]
    order = np.random.default_rng(nbufs).permutation(max(nbufs - 1, 0))
    edges = [(ids[i], i % 2, ids[i + 1], (i + 1) % 2) for i in order] + [(ids[0], 2, ids[-1], 2)]
    return build_case(f"{nbufs} buffers", [(b, 3) for b in ids], edges)


def build_cases():
    two = [(1, 5), (4, 4)]
    return [
        build_case("no edges", two, []),
        build_case("one edge", two, [(1, 2, 4, 3)]),
        build_case("self and duplicate edges", two, [(1, 1, 4, 1), (1, 1, 4, 1), (4, 1, 1, 1), (1, 3, 1, 3), (4, 0, 4, 2)]),
        build_case("ids at and beyond nb_buffers", two, [(1, 0, 4, 0), (6, 0, 4, 1), (1, 1, 7, 1), (0xFFFFFFFF, 0, 1, 2), (1, 4, 4, 3)], nb_buffers=6),
        build_case("absent buffers", two, [(1, 0, 4, 0), (2, 0, 4, 1), (1, 1, 3, 0), (0, 0, 1, 3), (1, 4, 4, 3)], absent=[(2, 9), (3, 1)]),
        build_case("rows not stored", two, [(1, 5, 4, 0), (1, 4, 4, 4), (1, 4, 4, 3), (1, 0xFFFFFFFF, 4, 0)]),
        build_case("a table row at 0 and one at max_rows", [(0, 0), (2, 6), (5, 9)], [(0, 0, 2, 0), (2, 5, 5, 5), (2, 0, 5, 6), (5, 8, 2, 1)], max_rows=6, node_stride=8),
        build_case("a count above the capacity", two, [(1, 0, 4, 0), (1, 1, 4, 1), (1, 2, 4, 2), (1, 3, 4, 3)], count=9, max_edges=2),
        build_case("a count below the records held", two, [(1, 0, 4, 0), (1, 1, 4, 1), (1, 2, 4, 2)], count=1, max_edges=3),
        build_case("257 edges", [(0, 300), (1, 300)], [(0, i, 1, (7 * i) % 300) for i in range(257)]),
    ] + [chain_case(n) for n in (1, 2, 64, 65, 129)]


@pytest.mark.parametrize("case", build_cases(), ids=lambda c: c["name"])
def test_build_from_edges(L, case):
    h = HE.BuildOnly(case)
    assert L.vksift_hip_tracks_scratch_u32(h.nbufs, h.stride) == h.build_scratch_u32
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    h.check(h.read())


BUILD_REFUSALS = [dict(max_edges=0), dict(nb_buffers=0), dict(nbufs=0), dict(max_rows=0), dict(max_rows=1000), {"+edges": 8}, {"+tracks": 2}, {"+scratch": 4},
                  dict(tracks_cap=0), {"+scratch_u32": -1}, dict(node_stride=0x80000000)]


@pytest.mark.parametrize("changes", BUILD_REFUSALS, ids=lambda d: " ".join(f"{k}={x}" for k, x in d.items()))
def test_build_refusals(L, changes):
    h = HE.BuildOnly(build_cases()[2])
    rc = h.launch(L, **changes)
    assert rc == HE.HIP_ERROR_INVALID_VALUE, f"{h.what} with {changes}: returned {rc}"
    h.check(Launch.read(h), h.host)


# ------------------------------------------------------------------------------------------------------------------------ append + build
def accumulated(L, case, calls):
    top = max(b for c in calls for b, _ in c["bufs"])
    h = HE.Store(store_case(case["name"], calls, nb_buffers=top + 1, build=dict(node_stride=case["node_stride"], max_rows=case["max_rows"])))
    for k in range(len(calls)):
        assert h.append(L, k) == 0
    assert h.run_build(L) == 0
    return h, h.read()


@pytest.mark.parametrize("case", TC.all_cases(), ids=lambda c: c["name"])
def test_one_append_and_a_build_equal_the_plain_build(L, case):
    h, after = accumulated(L, case, [case])
    h.check(after)
    p = HT.Tracks(case)
    assert p.launch(L) == 0
    for x, y in zip(h.outputs(after), p.outputs(p.read())):
        assert np.array_equal(x, y)


def test_contention_equals_the_plain_build_and_repeats(L):
    """several hundred workgroups race for a few roots: the same bytes as the plain build, and as a second run into fresh memory"""
    case = TC.contention_case()
    h1, a1 = accumulated(L, case, [case])
    h2, a2 = accumulated(L, case, [case])
    p = HT.Tracks(case)
    assert p.launch(L) == 0
    plain = p.outputs(p.read())
    assert int(plain[2].view(u32)[3]) == 32 * 4096
    for x, y, z in zip(h1.outputs(a1), h2.outputs(a2), plain):
        assert np.array_equal(x, z) and np.array_equal(y, z)
    assert np.array_equal(h1.view(a1, h1.edges), h2.view(a2, h2.edges))


def test_a_chain_through_three_calls_is_one_track_after_the_third(L):
    rows = {0: 2, 1: 2, 2: 2, 3: 2}
    calls = [TC.case("a", [(0, 2), (1, 2)], [TC.pair(0, 1, [(0, 1)])]), TC.case("b", [(2, 2), (3, 2)], [TC.pair(2, 3, [(1, 0)])]),
             TC.case("c", [(1, 2), (2, 2)], [TC.pair(1, 2, [(1, 1)])])]
    shape = dict(name="chain", node_stride=4, max_rows=2)
    h, after = accumulated(L, shape, calls[:2])
    h.check(after)
    assert h.view(after, h.track_stats, u32)[:4].tolist() == [2, 0, 4, 2]
    h, after = accumulated(L, shape, calls)
    h.check(after)
    assert h.view(after, h.track_stats, u32)[:4].tolist() == [1, 0, 4, 3] and len(rows) == h.nbufs
