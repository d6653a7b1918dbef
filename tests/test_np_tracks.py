"""tests/np_tracks.py (the restatement of vksift_ext_buildTracks) against an independent breadth-first labelling on seeded random graphs, and the hand
cases of tests/track_cases.py against their written-out answers. CPU only."""
from collections import deque

import numpy as np
import pytest

import hip_tracks as HT
import np_tracks as NT
import track_cases as TC


def bfs_tracks(rows, pairs):
    """components by breadth-first search over adjacency lists, visited in the order (gpu_buffer_id, row): the first node of a component met is its
    smallest member, so the tracks come out in their numbering order"""
    adj, nb_edges = {}, 0
    for a, b, edges in pairs:
        for ia, ib in np.asarray(edges).reshape(-1, 2).tolist():
            if ia < rows[a] and ib < rows[b]:
                nb_edges += 1
                adj.setdefault((a, ia), []).append((b, ib))
                adj.setdefault((b, ib), []).append((a, ia))
    label, records = {}, []
    for b in sorted(rows):
        for r in range(rows[b]):
            if (b, r) in label:
                continue
            seen, queue = {(b, r)}, deque([(b, r)])
            while queue:
                for v in adj.get(queue.popleft(), []):
                    if v not in seen:
                        seen.add(v)
                        queue.append(v)
            t = len(records) if len(seen) >= 2 else NT.NO_TRACK
            if len(seen) >= 2:
                records.append((b, r, len(seen), len({x[0] for x in seen})))
            for v in seen:
                label[v] = t
    words = {b: np.array([label[(b, r)] for r in range(rows[b])], np.uint32).reshape(-1) for b in rows}
    return records, words, nb_edges


@pytest.mark.parametrize("seed", range(12))
def test_union_find_equals_breadth_first_labelling(seed):
    rng = np.random.default_rng(seed)
    ids = sorted(rng.choice(40, rng.integers(1, 8), replace=False).tolist())
    rows = {b: int(rng.integers(0, 30)) for b in ids}
    pairs = []
    for _ in range(int(rng.integers(1, 12))):
        a, b = (int(x) for x in rng.choice(ids, 2))      # A == B happens
        n = int(rng.integers(0, 25))
        # indices one beyond the rows now and then: no edge
        pairs.append((a, b, np.stack([rng.integers(0, rows[a] + 2, n), rng.integers(0, rows[b] + 2, n)], axis=1)))
    rec, words, stats = NT.build(rows, pairs)
    want_rec, want_words, want_edges = bfs_tracks(rows, pairs)
    assert [tuple(int(x) for x in r) for r in rec] == want_rec
    for b in ids:
        assert np.array_equal(words[b], want_words[b])
    assert stats == dict(nb_tracks=len(want_rec), nb_conflicting=sum(r[2] > r[3] for r in want_rec), nb_features=sum(r[2] for r in want_rec), nb_edges=want_edges)


# name -> (records, {buffer: words}, nb_edges), written out by hand
N = NT.NO_TRACK
ANSWERS = {
    "no edges": ([], {0: [N] * 4, 1: [N] * 3, 2: [N] * 5}, 0),
    "one edge": ([(0, 2, 2, 2)], {0: [N, N, 0, N, N], 1: [N, N, N, 0]}, 1),
    "chain of three": ([(0, 1, 3, 3)], {0: [N, 0, N], 1: [N, 0, N], 2: [0, N, N]}, 2),
    "cycle closing on another row": ([(0, 0, 4, 3)], {0: [0, N, N, 0], 1: [0, N], 2: [0, N]}, 3),
    "two rows of A on one of B": ([(0, 0, 3, 2)], {0: [0, 0, N], 1: [N, N, 0]}, 2),
    "pair of a buffer with itself": ([(3, 2, 2, 1)], {3: [N, N, 0, N, 0, N]}, 3),
    "idle buffer": ([(0, 0, 2, 2)], {0: [0, N], 1: [0, N], 5: [N] * 7}, 1),
    "counts above max_n and max_rows": ([(0, 0, 3, 2), (0, 5, 2, 2)], {0: [0, 0, N, N, N, 1], 1: [0, N, N, N, 1]}, 3),
    "no edges: every mask byte 0": ([], {0: [N] * 4, 1: [N] * 3}, 0),
    "pair whose model is not valid": ([(1, 3, 2, 2)], {0: [N] * 4, 1: [N, N, N, 0], 2: [N, N, N, 0]}, 1),
}


@pytest.mark.parametrize("case", TC.all_cases(), ids=lambda c: c["name"])
def test_hand_cases(case):
    rec, words, stats = TC.expected(case)
    name = case["name"].replace(" (masked)", "")
    if name in ANSWERS:
        want_rec, want_words, want_edges = ANSWERS[name]
        assert [tuple(int(x) for x in r) for r in rec] == want_rec
        assert {b: w.tolist() for b, w in words.items()} == want_words
        assert stats["nb_edges"] == want_edges
    elif name.startswith("chain over 64"):
        assert [tuple(int(x) for x in r) for r in rec] == [(1, 0, 64, 64)] and all(w.tolist() == [0] for w in words.values()) and stats["nb_edges"] == 63
    else:
        assert name.startswith("131 buffers")
        assert [tuple(int(x) for x in r) for r in rec] == [(3, 0, 131, 131), (3, 1, 2, 2)] and stats["nb_edges"] == 131
    assert stats["nb_conflicting"] == int((rec["length"] > rec["nb_buffers"]).sum()) and stats["nb_features"] == int(rec["length"].sum())
    # a masked case is the same graph as the case it was derived from
    if case["name"].endswith(" (masked)"):
        base = TC.expected(TC.case_by_name(name))
        assert np.array_equal(rec, base[0]) and stats == base[2]


def test_arena_layout_without_a_gpu():
    """the launcher harness lays out the same bytes on the CPU; the expected arena differs from the initial one exactly in the output blocks"""
    for case in TC.all_cases()[:4] + TC.masked_only_cases():
        h = HT.Tracks(case, device="cpu")
        exp = h.expected()
        changed = np.flatnonzero(exp != h.host)
        lo = min(b.off for b in (h.node_words, h.tracks, h.stats))
        assert len(changed) and changed.min() >= lo and changed.max() < h.stats.off + 16
        assert h.scratch_u32 == HT.scratch_words(h.nbufs, h.stride)
