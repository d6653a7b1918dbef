"""The restatement of the edge store (tests/np_track_edges.py; CPU) on cases small enough to check by hand: what the GPU tests compare the library with."""
import numpy as np

import np_track_edges as NE
import np_tracks as NT


def e(*pairs):
    return np.array(pairs, np.int64).reshape(-1, 2)


def test_empty_calls_count_as_calls_and_record_rows():
    s = NE.begin(8)
    NE.accumulate(s, {0: 3, 1: 2}, [(0, 1, e())])
    NE.accumulate(s, {1: 2, 2: 5}, [(1, 2, e()), (2, 1, e())])
    assert NE.stats(s) == dict(nb_edges=0, nb_dropped=0, nb_calls=2, nb_changed_buffers=0)
    assert s["table"] == {0: 3, 1: 2, 2: 5} and len(NE.edge_records(s)) == 0
    rec, words, st = NE.build(s, 100)
    assert len(rec) == 0 and st["nb_edges"] == 0 and all((words[b] == NT.NO_TRACK).all() for b in (0, 1, 2)) and len(words[2]) == 5


def test_mask_of_zeros_and_invalid_pair_give_no_edge():
    recs = e((0, 0), (1, 1), (2, 2))
    s = NE.begin(8)
    NE.accumulate(s, {0: 3, 1: 3}, [(0, 1, NT.pair_edges(recs, np.zeros(3, np.uint8), True)), (1, 0, NT.pair_edges(recs, np.ones(3, np.uint8), False))])
    assert NE.stats(s)["nb_edges"] == 0 and s["table"] == {0: 3, 1: 3}
    NE.accumulate(s, {0: 3, 1: 3}, [(0, 1, NT.pair_edges(recs, np.array([0, 1, 2], np.uint8), True))])       # only a byte equal to 1 selects
    assert s["edges"] == [(0, 1, 1, 1)]


def test_order_is_slot_then_record_and_the_capacity_clamps():
    s = NE.begin(4)
    NE.accumulate(s, {0: 9, 1: 9, 2: 9}, [(2, 0, e((5, 1), (4, 2))), (0, 1, e((3, 3)))])
    assert s["edges"] == [(2, 5, 0, 1), (2, 4, 0, 2), (0, 3, 1, 3)]
    NE.accumulate(s, {0: 9, 1: 9}, [(1, 0, e((8, 8), (7, 7)))])                                       # overflow by one
    assert s["edges"][3] == (1, 8, 0, 8) and NE.stats(s) == dict(nb_edges=4, nb_dropped=1, nb_calls=2, nb_changed_buffers=0)
    NE.accumulate(s, {0: 9, 1: 9}, [(1, 0, e((1, 1)))])                                               # already full
    assert NE.stats(s) == dict(nb_edges=4, nb_dropped=2, nb_calls=3, nb_changed_buffers=0)
    assert NE.edge_records(s)["row_a"].tolist() == [5, 4, 3, 8]


def test_rows_not_stored_are_no_edge_and_max_rows_clamps():
    s = NE.begin(8)
    NE.accumulate(s, {0: 9, 1: 2}, [(0, 1, e((0, 0), (5, 1), (7, 1), (1, 2)))], max_rows=6)
    assert s["edges"] == [(0, 0, 1, 0), (0, 5, 1, 1)] and s["table"] == {0: 9, 1: 2}                  # the table keeps the raw count
    rec, words, st = NE.build(s, 6)
    assert len(words[0]) == 6 and st["nb_edges"] == 2 and len(rec) == 2


def test_a_changed_row_count_is_counted_and_the_table_kept():
    s = NE.begin(8)
    NE.accumulate(s, {0: 4, 1: 4}, [(0, 1, e((3, 3)))])
    NE.accumulate(s, {0: 2, 1: 4, 2: 1}, [(0, 2, e((1, 0)))])
    assert s["table"] == {0: 4, 1: 4, 2: 1} and NE.stats(s)["nb_changed_buffers"] == 1
    NE.accumulate(s, {0: 2, 1: 5}, [(0, 1, e())])
    assert s["table"] == {0: 4, 1: 4, 2: 1} and NE.stats(s)["nb_changed_buffers"] == 3
    # an edge the smaller count let through names a stored row of the table; one beyond the table's count is no edge at the build
    s["edges"].append((0, 7, 1, 0))
    assert NE.build(s, 100)[2]["nb_edges"] == 2


def test_duplicate_and_self_edges_are_kept_and_counted():
    s = NE.begin(8)
    NE.accumulate(s, {0: 3, 1: 3}, [(0, 1, e((1, 1), (1, 1))), (0, 0, e((2, 2), (0, 2)))])
    assert NE.stats(s)["nb_edges"] == 4
    rec, words, st = NE.build(s, 3)
    assert st == dict(nb_tracks=2, nb_conflicting=1, nb_features=4, nb_edges=4)
    assert rec.tolist() == [(0, 0, 2, 1), (0, 1, 2, 2)] and words[0].tolist() == [0, 1, 0] and words[1].tolist() == [NT.NO_TRACK, 1, NT.NO_TRACK]


def test_a_chain_through_three_calls_is_one_track_only_after_the_third():
    s = NE.begin(16)
    NE.accumulate(s, {0: 2, 1: 2}, [(0, 1, e((0, 1)))])
    NE.accumulate(s, {2: 2, 3: 2}, [(2, 3, e((1, 0)))])
    rec, _, st = NE.build(s, 2)
    assert st["nb_tracks"] == 2 and rec["length"].tolist() == [2, 2]
    NE.accumulate(s, {1: 2, 2: 2}, [(1, 2, e((1, 1)))])
    rec, words, st = NE.build(s, 2)
    assert st == dict(nb_tracks=1, nb_conflicting=0, nb_features=4, nb_edges=3) and rec.tolist() == [(0, 0, 4, 4)]
    assert [words[b].tolist() for b in range(4)] == [[0, NT.NO_TRACK], [NT.NO_TRACK, 0], [NT.NO_TRACK, 0], [0, NT.NO_TRACK]]


def test_one_call_builds_what_the_plain_build_builds():
    rng = np.random.default_rng(3)
    rows = {1: 40, 4: 33, 6: 25}
    pairs = [(a, b, np.stack([rng.integers(0, rows[a], 30), rng.integers(0, rows[b], 30)], axis=1)) for a, b in ((1, 4), (6, 4), (1, 6), (4, 4))]
    s = NE.accumulate(NE.begin(1000), rows, pairs)
    got, want = NE.build(s, 64), NT.build(rows, pairs)
    assert np.array_equal(got[0], want[0]) and got[2] == want[2] and all(np.array_equal(got[1][b], want[1][b]) for b in rows)


def test_buffers_at_or_beyond_nb_buffers_are_not_recorded():
    s = NE.begin(8)
    NE.accumulate(s, {0: 2, 9: 2}, [(0, 9, e((1, 1)))], nb_buffers=4)
    assert s["table"] == {0: 2} and s["edges"] == [(0, 1, 9, 1)]
    assert NE.build(s, 2)[2] == dict(nb_tracks=0, nb_conflicting=0, nb_features=0, nb_edges=0)
