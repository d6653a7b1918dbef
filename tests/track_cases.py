"""The cases of the track launcher's tests (tests/test_gpu_track_launcher.py; plain module, no GPU).

A case: name; bufs = [(gpu_buffer_id, raw row count on the device)] in increasing id; node_stride, max_rows, max_n; pairs = [dict(a, b, recs, n_dev, mask,
valid)] — recs: every (idx_a, idx_b) record the slot HOLDS (those at and beyond min(n_dev, max_n) are decoys), mask: one byte per held record or None, valid: the
pair's valid word. A case is launched in the form it is written in: `masked` False hands over records with their own count (sources FILTERED, GUIDED),
True records with a mask and valid words (the four mask sources). as_masked() derives the second form from a case of the first: the same graph, with
decoy records whose mask byte is 0 shuffled between the edges. expected() is tests/np_tracks.py on what the contract says the launch reads.
"""
import numpy as np

import np_tracks as NT

JUNK_COUNTER = 0x00ABCDEF


def pair(a, b, recs, n_dev=None, mask=None, valid=1):
    recs = np.asarray(recs, np.uint32).reshape(-1, 2)
    return dict(a=a, b=b, recs=recs, n_dev=len(recs) if n_dev is None else n_dev, mask=None if mask is None else np.asarray(mask, np.uint8), valid=valid)


def case(name, bufs, pairs, *, masked=False, node_stride=None, max_rows=None, max_n=None, rec_extra=1, mask_extra=3, n_stride=3, valid_stride=2, tab_stride=3):
    rows = max(n for _, n in bufs)
    max_rows = max(rows, 1) if max_rows is None else max_rows
    held = max([len(p["recs"]) for p in pairs] + [1])
    return dict(name=name, bufs=list(bufs), pairs=pairs, masked=masked, node_stride=max_rows + 2 if node_stride is None else node_stride, max_rows=max_rows,
                max_n=held if max_n is None else max_n, rec_extra=rec_extra, mask_extra=mask_extra, n_stride=n_stride, valid_stride=valid_stride, tab_stride=tab_stride)


def as_masked(c, seed=5):
    """the same graph from records with a mask: every second held record a decoy (rows that exist, mask byte 0)"""
    rng = np.random.default_rng(seed)
    rows = dict(c["bufs"])
    pairs = []
    for p in c["pairs"]:
        n = min(p["n_dev"], c["max_n"])
        real = p["recs"][:n]
        k = len(real) + 1
        ra, rb = max(min(rows[p["a"]], c["max_rows"]), 1), max(min(rows[p["b"]], c["max_rows"]), 1)
        decoys = np.stack([rng.integers(0, ra, k), rng.integers(0, rb, k)], axis=1).astype(np.uint32)
        recs = np.zeros((len(real) + k, 2), np.uint32)
        mask = np.zeros(len(recs), np.uint8)
        recs[0::2][:k], recs[1::2][:len(real)], mask[1::2][:len(real)] = decoys, real, 1
        pairs.append(dict(a=p["a"], b=p["b"], recs=recs, n_dev=len(recs), mask=mask, valid=1))
    out = dict(c, name=c["name"] + " (masked)", pairs=pairs, masked=True, max_n=2 * c["max_n"] + 1)
    return out


def read_by_contract(c):
    """rows {id: stored rows} and the [(a, b, edges)] the launch takes"""
    rows = {b: min(n, c["max_rows"]) for b, n in c["bufs"]}
    pairs = []
    for p in c["pairs"]:
        n = min(p["n_dev"], c["max_n"])
        assert n <= len(p["recs"])
        mask = p["mask"][:n] if c["masked"] else None
        pairs.append((p["a"], p["b"], NT.pair_edges(p["recs"][:n], mask, bool(p["valid"]) or not c["masked"])))
    return rows, pairs


_memo = {}


def expected(c):
    if c["name"] not in _memo:
        _memo[c["name"]] = NT.build(*read_by_contract(c))
    return _memo[c["name"]]


# ------------------------------------------------------------------------------------------------------------------------ the hand cases
def hand_cases():
    out = []
    out.append(case("no edges", [(0, 4), (1, 3), (2, 5)], [pair(0, 1, []), pair(1, 2, [])]))
    out.append(case("one edge", [(0, 5), (1, 4)], [pair(0, 1, [(2, 3)])]))
    out.append(case("chain of three", [(0, 3), (1, 3), (2, 3)], [pair(0, 1, [(1, 1)]), pair(1, 2, [(1, 0)])]))
    out.append(case("cycle closing on another row", [(0, 4), (1, 2), (2, 2)], [pair(0, 1, [(0, 0)]), pair(1, 2, [(0, 0)]), pair(2, 0, [(0, 3)])]))
    out.append(case("two rows of A on one of B", [(0, 3), (1, 3)], [pair(0, 1, [(0, 2), (1, 2)])]))
    out.append(case("pair of a buffer with itself", [(3, 6)], [pair(3, 3, [(1, 1), (2, 4), (0, 0)])]))
    out.append(case("idle buffer", [(0, 2), (1, 2), (5, 7)], [pair(0, 1, [(0, 0)]), pair(0, 5, [])]))
    # the longest find paths: every link goes under a root that the next pair in the list links again
    ids = [2 * i + 1 for i in range(64)]
    out.append(case("chain over 64 buffers, decreasing", [(b, 1) for b in ids], [pair(ids[i], ids[i + 1], [(0, 0)]) for i in reversed(range(63))]))
    # more buffers than one presence word has bits: three groups, the chain in a shuffled order, one pair beside it
    ids = list(range(3, 3 + 131))
    order = np.random.default_rng(11).permutation(129)
    out.append(case("131 buffers, three presence groups", [(b, 2) for b in ids], [pair(ids[i], ids[i + 1], [(0, 1)] if i % 2 == 0 else [(1, 0)]) for i in order] +
                    [pair(ids[129], ids[130], [(1, 1)]), pair(ids[0], ids[130], [(1, 0)])]))
    # counts above the bounds: 9 rows on the device against max_rows 6, 7 records against max_n 4; record 2 names a row that is not stored
    out.append(case("counts above max_n and max_rows", [(0, 9), (1, 5)], [pair(0, 1, [(0, 0), (5, 4), (7, 1), (1, 0), (2, 2), (3, 3), (4, 4)], n_dev=7)], max_rows=6,
                    node_stride=8, max_n=4))
    return out


def masked_only_cases():
    junk = np.ones(3, np.uint8)
    return [
        case("no edges: every mask byte 0", [(0, 4), (1, 3)], [pair(0, 1, [(0, 0), (1, 1), (2, 2)], mask=[0, 0, 0]), pair(1, 0, [(0, 1)], mask=[0])], masked=True),
        case("pair whose model is not valid", [(0, 4), (1, 4), (2, 4)], [pair(0, 1, [(0, 0), (1, 1), (2, 2)], mask=junk, valid=0), pair(1, 2, [(3, 3), (0, 1)], mask=[1, 0])],
             masked=True),
    ]


# ------------------------------------------------------------------------------------------------------------------------ the contention case
def contention_case(seed=2024):
    """16 buffers x 4096 rows, 32 pairs of about 4096 edges: rows [0, 2048) of every buffer are joined at random (one component takes nearly all of them,
    about half of all edges), row r of [2048, 4096) forms one track over the two or three neighbouring buffers its hash picks, its edges repeated many times"""
    rng = np.random.default_rng(seed)
    nb, rows, half = 16, 4096, 2048
    first = rng.integers(0, nb, rows)       # S_r = {first, first + 1 [, first + 2]} mod 16
    triple = rng.integers(0, 2, rows).astype(bool)
    pairs = []
    for d in (1, 2):
        for a in range(nb):
            b = (a + d) % nb
            r = np.arange(half, rows)
            off = (a - first[r]) % nb
            ok = (off == 0) & (triple[r] | (d == 1)) if d == 2 else ((off == 0) | ((off == 1) & triple[r]))
            small = rng.choice(r[ok], half)
            giant = np.stack([rng.integers(0, half, half), rng.integers(0, half, half)], axis=1)
            recs = np.concatenate([giant, np.stack([small, small], axis=1)])
            pairs.append(pair(a, b, rng.permutation(recs)))
    return case("contention: 16 x 4096 rows, 32 pairs", [(b, rows) for b in range(nb)], pairs, node_stride=rows + 64, rec_extra=0)


def all_cases():
    plain = hand_cases()
    return plain + [as_masked(c) for c in plain] + masked_only_cases()


def case_by_name(name):
    (c,) = [c for c in all_cases() if c["name"] == name]
    return c
