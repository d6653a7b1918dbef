"""tests/np_observations.py (the restatement of vksift_ext_selectTrackObservations) against a brute-force grouping — a dictionary of member lists built row
by row, no sort — on the hand cases of tests/track_cases.py, under both conflict policies, min_length 2 / 3 and max_length 0 / 2 / 3 (CPU)."""
import itertools

import numpy as np
import pytest

import np_observations as NO
import np_tracks as NT
import track_cases as TC

GRID = [(mn, mx, c) for mn, mx, c in itertools.product((2, 3), (0, 2, 3), (NO.KEEP_CONFLICTING, NO.DROP_CONFLICTING)) if NO.args_valid(mn, mx, c)]


def positions(rows, seed=3):
    """a distinct float pair per (buffer, row)"""
    rng = np.random.default_rng(seed)
    return {b: (rng.random((n, 2), np.float32) * 1000 + np.float32(b)).astype(np.float32) for b, n in rows.items()}


def brute_force(records, words, xy, min_length, max_length, conflicts):
    members = {}
    for b in sorted(words):
        for row, w in enumerate(words[b]):
            if int(w) != NT.NO_TRACK:
                members.setdefault(int(w), []).append((b, row))
    stats = dict(nb_tracks=0, nb_observations=0, nb_rejected_length=0, nb_rejected_conflicting=0)
    offsets, ids, obs = [0], [], []
    for t, r in enumerate(records):
        m = sorted(members[t])
        assert len(m) == int(r["length"])
        if len(m) < min_length or (max_length and len(m) > max_length):
            stats["nb_rejected_length"] += 1
        elif conflicts == NO.DROP_CONFLICTING and len({b for b, _ in m}) < len(m):
            stats["nb_rejected_conflicting"] += 1
        else:
            ids.append(t)
            obs += [(b, row, xy[b][row, 0], xy[b][row, 1]) for b, row in m]
            offsets.append(len(obs))
    stats["nb_tracks"], stats["nb_observations"] = len(ids), len(obs)
    return stats, np.array(offsets, np.uint32), np.array(ids, np.uint32), np.array(obs, NO.OBSERVATION_DTYPE) if obs else np.zeros(0, NO.OBSERVATION_DTYPE)


@pytest.mark.parametrize("case", TC.hand_cases(), ids=lambda c: c["name"])
def test_restatement_equals_brute_force(case):
    rows, _ = TC.read_by_contract(case)
    records, words, track_stats = TC.expected(case)
    xy = positions(rows)
    for mn, mx, c in GRID:
        got, want = NO.select(records, words, xy, mn, mx, c), brute_force(records, words, xy, mn, mx, c)
        assert got[0] == want[0], (mn, mx, c)
        for g, w in zip(got[1:], want[1:]):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (mn, mx, c)
        stats, offsets = got[0], got[1]
        assert stats["nb_tracks"] + stats["nb_rejected_length"] + stats["nb_rejected_conflicting"] == track_stats["nb_tracks"]
        assert offsets[0] == 0 and offsets[-1] == stats["nb_observations"] and len(offsets) == stats["nb_tracks"] + 1


def test_the_grid_selects_and_rejects_something():
    """the fixture's precondition: over the hand cases every count of the statistics is non-zero for some parameters, and the policies differ"""
    seen = dict.fromkeys(NO.STATS, 0)
    differ = False
    for case in TC.hand_cases():
        rows, _ = TC.read_by_contract(case)
        records, words, _ = TC.expected(case)
        xy = positions(rows)
        for mn, mx, c in GRID:
            stats = NO.select(records, words, xy, mn, mx, c)[0]
            for k in NO.STATS:
                seen[k] += stats[k]
        differ |= NO.select(records, words, xy, 2, 0, 0)[0] != NO.select(records, words, xy, 2, 0, 1)[0]
    assert all(seen.values()) and differ, seen


def test_no_tracks_is_the_single_offset_zero():
    case = TC.case_by_name("no edges")
    rows, _ = TC.read_by_contract(case)
    records, words, _ = TC.expected(case)
    stats, offsets, ids, obs = NO.select(records, words, positions(rows), 2, 0, NO.KEEP_CONFLICTING)
    assert stats == dict.fromkeys(NO.STATS, 0) and offsets.tolist() == [0] and len(ids) == 0 and len(obs) == 0


def test_argument_rule():
    assert NO.args_valid(2, 0, 0) and NO.args_valid(3, 3, 1) and NO.args_valid(2, 7, 1)
    assert not NO.args_valid(1, 0, 0) and not NO.args_valid(3, 2, 0) and not NO.args_valid(2, 0, 2)
