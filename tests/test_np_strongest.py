"""tests/np_strongest.py — the specification of the feature budget — against a second, independent statement: a stable argsort on
(-key, row) whose first min(total, N) rows, sorted again, are the kept rows. Random section tables, the special bit patterns, idempotence,
the identity at N >= total and the key mapping; and, without a GPU, that the case table of tests/hip_strongest.py reaches the edges it is
there for and lays out its arenas. CPU only."""
import numpy as np
import pytest

import hip_strongest as HS
import np_strongest as NS
from test_section_walk import TABLES, stored_rows

u32 = np.uint32


def kept_by_sort(keys, n):
    order = np.argsort(-(np.asarray(keys, u32).astype(np.int64)), kind="stable")   # key descending, row ascending among equals
    return np.sort(order[:min(len(keys), n)])


def random_table(rng):
    nsec = int(rng.integers(1, 17))
    cap = [int(v) for v in rng.integers(0, 40, nsec)]
    gap = [int(v) for v in rng.integers(0, 4, nsec)]
    off, at = [], 0
    for o in range(nsec):
        off.append(at + gap[o])
        at = off[-1] + cap[o]
    found = [int(rng.integers(0, cap[o] + 4)) for o in range(nsec)]
    pad = 16 - nsec
    return nsec, off + [7] * pad, cap + [9] * pad, found + [11] * pad


def random_buffer(rng, table, kind):
    nsec, off, cap, found = table
    extent = max([off[o] + cap[o] for o in range(nsec)] + [1]) + 2
    buf = rng.integers(0, 256, (extent, NS.REC), dtype=np.uint8)
    rows = stored_rows(nsec, off, cap, found)
    buf[rows, NS.KEY_AT:NS.KEY_AT + 4] = HS.make_keys(kind, len(rows), rng).astype("<u4").view(np.uint8).reshape(-1, 4)
    return buf


def test_key_mapping():
    """the intensity word with the sign bit cleared, as an unsigned integer: |x| for finite x, -0 == +0 < denormals < normals < inf < NaN patterns"""
    vals = np.array([0.0, -0.0, 1e-45, -1e-39, 1.17549435e-38, 0.03, -0.03, -1.5, 3e38, np.inf, -np.inf], np.float32)
    rec = np.zeros((len(vals) + 2, NS.REC), np.uint8)
    rec[:len(vals), NS.KEY_AT:NS.KEY_AT + 4] = vals.view(np.uint8).reshape(-1, 4)
    rec[len(vals):, NS.KEY_AT:NS.KEY_AT + 4] = np.array([0x7FC00001, 0xFF800001], "<u4").view(np.uint8).reshape(-1, 4)
    k = NS.keys_of(rec)
    assert k.dtype == u32 and np.array_equal(k[:len(vals)], np.abs(vals).view(u32))
    assert k[0] == k[1] == 0 and k[5] == k[6]
    assert k[0] < k[2] < k[3] < k[4] < k[5] < k[7] < k[8] < k[9] == k[10] < k[12] < k[11]
    rec[:, :NS.KEY_AT] = 0xFF
    rec[:, NS.KEY_AT + 4:] = 0xFF
    assert np.array_equal(NS.keys_of(rec), k)   # no other byte of the record takes part


@pytest.mark.parametrize("kind", ["random", "all equal", "low byte", "high byte", "each byte once", "special", "ties"])
def test_keep_mask_is_the_sorted_prefix(kind):
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 64, 257, 1500):
        keys = HS.make_keys(kind, n, rng) & u32(0x7FFFFFFF)
        for budget in sorted({1, 2, n // 3 + 1, max(n - 1, 1), n, n + 1}):
            assert np.array_equal(np.flatnonzero(NS.keep_mask(keys, budget)), kept_by_sort(keys, budget)), (kind, n, budget)


@pytest.mark.parametrize("seed", range(12))
def test_random_tables(seed):
    rng = np.random.default_rng(100 + seed)
    table = random_table(rng)
    nsec, off, cap, found = table
    kind = ["random", "special", "ties", "low byte"][seed % 4]
    buf = random_buffer(rng, table, kind)
    rows = stored_rows(nsec, off, cap, found)
    total = len(rows)
    for budget in sorted({1, max(total // 2, 1), max(total - 1, 1), max(total, 1), total + 1}):
        out, found_out, stale, kept = NS.keep_strongest(buf, nsec, off, cap, found, budget)
        want = kept_by_sort(NS.keys_of(buf[rows]), budget)
        assert np.array_equal(kept, want)
        if total <= budget:     # identity: the records, and the raw counters even where they exceed the capacity
            assert np.array_equal(out, buf) and found_out == list(found) and not stale.any()
            continue
        new_rows = stored_rows(nsec, off, cap, found_out)
        assert len(new_rows) == budget and found_out[nsec:] == list(found[nsec:])
        assert np.array_equal(out[new_rows], buf[rows[want]])                       # the kept records, in download order
        assert np.array_equal(NS.selected_records(buf[rows], budget), out[new_rows])
        # a kept row stays in its section; the stale records are exactly the section's old rows from its new count on; nothing else changed
        base = 0
        changed = np.zeros(len(buf), bool)
        for o in range(nsec):
            n = min(found[o], cap[o])
            assert found_out[o] == int(((want >= base) & (want < base + n)).sum())
            assert stale[off[o]:off[o] + n].tolist() == [False] * found_out[o] + [True] * (n - found_out[o])
            changed[off[o]:off[o] + n] = True
            base += n
        assert not stale[~changed].any() and np.array_equal(out[~changed], buf[~changed]) and np.array_equal(out[stale], buf[stale])
        # idempotence
        again, found_again, stale_again, _ = NS.keep_strongest(out, nsec, off, cap, found_out, budget)
        assert np.array_equal(again, out) and found_again == found_out and not stale_again.any()


def test_case_table_reaches_its_edges():
    cs = HS.CASES
    one_sec = [c for c in cs if c["table"][0] == 1 and len(c["buf_ids"]) == 1]
    for t in (0, 1, 2, HS.ROUND - 1, HS.ROUND, HS.ROUND + 1, 2 * HS.ROUND + 1):
        budgets = {c["N"] for c in one_sec if c["totals"][0] == t}
        assert budgets >= {n for n in (1, t - 1, t, t + 1) if n >= 1}, t
    assert any(max(c["totals"]) > HS.LDS_KEYS for c in cs)
    assert {c["keys"] for c in cs} >= {"all equal", "low byte", "high byte", "special", "ties", "random"}
    assert any(c["table"][0] == 16 for c in cs) and any(c["fixed"] for c in cs) and any(c["cache"] for c in cs) and any(not c["cache"] for c in cs)
    assert any(len(c["buf_ids"]) == 3 and any(c["totals"][b] <= c["N"] for b in c["buf_ids"]) and sorted(c["buf_ids"]) != list(range(3)) for c in cs)
    assert any(any(f > k for f, k in zip(c["counts"][b], c["table"][2])) and c["totals"][b] <= c["N"] for c in cs for b in c["buf_ids"])   # above its capacity, unchanged
    assert any(any(f > k for f, k in zip(c["counts"][b], c["table"][2])) and c["totals"][b] > c["N"] for c in cs for b in c["buf_ids"])
    for name, sec_kept in (("N empties every section but the last", [0, 0, 3]), ("N keeps only rows of the first section", [28, 0, 0])):
        c = HS.case_named(name)
        _, found_out, _, _ = NS.keep_strongest(HS.case_buffers(c)[0], *c["table"][:3], c["counts"][0], c["N"])
        assert found_out[:3] == sec_kept
    # the ties cases: the kept rows at the threshold lie on both sides of the section boundary (row 1000) and of the round boundary (row 1024)
    c = HS.case_named("ties across the section and the round boundary, N 1500")
    buf = HS.case_buffers(c)[0]
    rows = stored_rows(*c["table"][:3], c["counts"][0])
    keys = NS.keys_of(buf[rows])
    kept = np.flatnonzero(NS.keep_mask(keys, c["N"]))
    at = kept[keys[kept] == keys[kept].min()]
    assert (keys == keys[kept].min()).sum() > len(at) and at.min() < 1000 and at.max() > HS.ROUND and (keys[~NS.keep_mask(keys, c["N"])] == keys[kept].min()).any()
    c = HS.case_named("ties, the quota ends with the last row of round 0")
    keys = NS.keys_of(HS.case_buffers(c)[0][stored_rows(*c["table"][:3], c["counts"][0])])
    kept = np.flatnonzero(NS.keep_mask(keys, c["N"]))
    assert kept[keys[kept] == keys[kept].min()].max() in (HS.ROUND - 1, HS.ROUND - 2, HS.ROUND - 3)


@pytest.mark.parametrize("case", [c for c in HS.CASES if max(c["totals"]) <= 2 * HS.ROUND + 1 and c["nbuf"] <= 8], ids=lambda c: c["name"])
def test_arena_states_the_contract(case):
    """the arena of a case on the CPU: what is expected differs from what goes in exactly where the contract writes"""
    h = HS.Strongest(case, device="cpu")
    exp, loose = h._state()
    diff = exp != h.host
    changed = [b for b in case["buf_ids"] if case["totals"][b] > case["N"]]
    assert diff.any() == bool(changed) or not diff.any()
    assert not loose[~((np.arange(len(exp)) >= h.feats.off) & (np.arange(len(exp)) < h.feats.off + len(h.feats.payload)))].any()
    for b in case["buf_ids"]:
        if b not in changed:
            lo = h.feats.off + b * h.buf_stride
            assert not diff[lo:lo + h.buf_stride].any() and not loose[lo:lo + h.buf_stride].any()
    assert np.array_equal(h.masked(h.host)[~loose], h.host[~loose])
