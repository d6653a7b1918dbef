"""tests/np_spread.py — the specification of the spatially distributed feature budget — against a second, independent statement: a stable
argsort on (-key, row) per cell whose first min(n_cell, q) rows are kept, and another over the rows that leaves. Random section tables, the key
kinds of hip_strongest.make_keys, the identities (a 1x1 grid and N < C are the plain budget, total <= N, idempotence), the per-cell guarantee and
the cell mapping on the coordinates a float comparison can get wrong; and, without a GPU, that the case table of tests/hip_spread.py reaches the
edges it is there for and lays out its arenas. CPU only."""
import numpy as np
import pytest

import hip_spread as HG
import hip_strongest as HS
import np_spread as NP
import np_strongest as NS
from test_np_strongest import kept_by_sort, random_buffer, random_table
from test_section_walk import stored_rows

u32 = np.uint32


def kept_by_sorts(keys, cells, ncell, n):
    """the second statement"""
    keys = np.asarray(keys, u32)
    if len(keys) <= n:
        return np.arange(len(keys))
    q, kept = n // ncell, []
    for c in range(ncell):
        idx = np.flatnonzero(cells == c)
        kept += list(idx[kept_by_sort(keys[idx], q)]) if q else []
    rest = np.setdiff1d(np.arange(len(keys)), kept)
    kept += list(rest[kept_by_sort(keys[rest], n - len(kept))]) if n > len(kept) else []
    return np.sort(np.array(kept, np.int64))


def records_at(x, y):
    rec = np.zeros((len(x), NS.REC), np.uint8)
    rec[:, 0:4] = np.asarray(x, "<f4").view(np.uint8).reshape(-1, 4)
    rec[:, 4:8] = np.asarray(y, "<f4").view(np.uint8).reshape(-1, 4)
    return rec


def test_bounds_formula():
    assert NP.bounds(640, 1).shape == (0,) and NP.bounds(640, 8).tolist() == [80.0 * j for j in range(1, 8)]
    b = NP.bounds(100, 3)
    assert b.dtype == np.float32 and b.tolist() == [float(np.float32(100 / 3)), float(np.float32(200 / 3))]
    assert NP.bounds(0xFFFFFFFF, 16)[-1] == np.float32(15.0 * 0xFFFFFFFF / 16)


def test_cell_mapping():
    """4 x 3 cells over 160 x 120: column bounds 40, 80, 120, row bounds 40, 80"""
    bx, by = NP.bounds(160, 4), NP.bounds(120, 3)
    below = float(np.nextafter(np.float32(40), np.float32(0)))
    x = [0.0, -0.0, 39.9, below, 40.0, 79.99, 80.0, 120.0, 159.9, 160.0, 1e30, np.inf, -np.inf, -1.0, np.nan, -1e-45, 1e-45]
    cx = [0, 0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 3, 0, 0, 0, 0, 0]
    assert NP.cells_of(records_at(x, np.zeros(len(x))), 4, bx, by).tolist() == cx
    cy = [0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 0, 0, 0, 0, 0]
    assert NP.cells_of(records_at(np.zeros(len(x)), x), 4, bx, by).tolist() == [4 * v for v in cy]
    assert NP.cells_of(records_at(x, x), 4, bx, by).tolist() == [4 * r + c for r, c in zip(cy, cx)]
    # a NaN with the sign bit set, and one with a payload
    rec = records_at([0.0, 0.0], [0.0, 0.0])
    rec[:, 0:4] = np.array([0xFFC00000, 0x7F800001], "<u4").view(np.uint8).reshape(-1, 4)
    assert NP.cells_of(rec, 4, bx, by).tolist() == [0, 0]
    # -0.0 behaves as 0.0 on either side of the comparison; bounds in any order: the count of satisfied comparisons
    assert NP.cells_of(records_at([-0.0, 0.0, -1.0], [0, 0, 0]), 2, [0.0], []).tolist() == [1, 1, 0]
    assert NP.cells_of(records_at([-0.0, 0.0], [0, 0]), 2, [-0.0], []).tolist() == [1, 1]
    assert NP.cells_of(records_at([50.0, 150.0, 450.0], [0, 0, 0]), 4, [400.0, 100.0, 400.0], [-5.0, np.nan]).tolist() == [4, 5, 7]
    # no byte of the record but the first eight takes part
    rec = records_at(x, x[::-1])
    noisy = rec.copy()
    noisy[:, 8:] = 0xFF
    assert np.array_equal(NP.cells_of(noisy, 4, bx, by), NP.cells_of(rec, 4, bx, by))


@pytest.mark.parametrize("kind", ["random", "all equal", "low byte", "high byte", "each byte once", "special", "ties"])
def test_keep_mask_is_the_two_sorts(kind):
    rng = np.random.default_rng(6)
    for n in (0, 1, 2, 3, 64, 257, 1500):
        keys = HS.make_keys(kind, n, rng) & u32(0x7FFFFFFF)
        for ncell in (1, 2, 15, 256):
            cells = rng.integers(0, ncell, n) if ncell < 256 else rng.choice([0, 3, 200, 255], n)
            for budget in sorted({1, ncell - 1, ncell, 2 * ncell + 1, n // 3 + 1, max(n - 1, 1), n, n + 1} - {0}):
                keep = NP.keep_mask_grid(keys, cells, ncell, budget)
                assert np.array_equal(np.flatnonzero(keep), kept_by_sorts(keys, cells, ncell, budget)), (kind, n, ncell, budget)
                assert keep.sum() == min(n, budget)
                if ncell == 1 or budget < ncell:    # the plain budget
                    assert np.array_equal(keep, NS.keep_mask(keys, budget))
                if n > budget:                      # every cell that held at least q rows keeps at least q
                    q, had, has = budget // ncell, np.bincount(cells, minlength=ncell), np.bincount(cells[keep], minlength=ncell)
                    assert (has >= np.minimum(had, q)).all()
                    # idempotence on the kept rows
                    assert NP.keep_mask_grid(keys[keep], cells[keep], ncell, budget).all()


@pytest.mark.parametrize("seed", range(12))
def test_random_tables(seed):
    rng = np.random.default_rng(300 + seed)
    table = random_table(rng)
    nsec, off, cap, found = table
    buf = random_buffer(rng, table, ["random", "special", "ties", "all equal"][seed % 4])
    rows = stored_rows(nsec, off, cap, found)
    total = len(rows)
    cols, grows = [(1, 1), (2, 1), (1, 2), (3, 5), (16, 16), (16, 1)][seed % 6]
    w, h = 160, 120
    if seed % 3:    # coordinates inside the frame; else the buffer's random bytes
        buf[rows, 0:4] = rng.uniform(0, w, total).astype("<f4").view(np.uint8).reshape(-1, 4)
        buf[rows, 4:8] = rng.uniform(0, h, total).astype("<f4").view(np.uint8).reshape(-1, 4)
    bx, by = NP.bounds(w, cols), NP.bounds(h, grows)
    cells = NP.cells_of(buf[rows], cols, bx, by)
    assert total == 0 or (0 <= cells.min() and cells.max() < cols * grows)
    for budget in sorted({1, max(total // 2, 1), max(total - 1, 1), max(total, 1), total + 1}):
        out, found_out, stale, kept = NP.keep_grid(buf, nsec, off, cap, found, budget, cols, grows, bx, by)
        want = kept_by_sorts(NS.keys_of(buf[rows]), cells, cols * grows, budget)
        assert np.array_equal(kept, want)
        if total <= budget:     # identity: the records, and the raw counters even where they exceed the capacity
            assert np.array_equal(out, buf) and found_out == list(found) and not stale.any()
            continue
        new_rows = stored_rows(nsec, off, cap, found_out)
        assert len(new_rows) == budget and found_out[nsec:] == list(found[nsec:])
        assert np.array_equal(out[new_rows], buf[rows[want]])                       # the kept records, in download order
        assert np.array_equal(NP.selected_records(buf[rows], budget, w, h, cols, grows), out[new_rows])
        if cols * grows == 1 or budget < cols * grows:      # the plain budget, byte for byte
            plain = NS.keep_strongest(buf, nsec, off, cap, found, budget)
            assert np.array_equal(plain[0], out) and plain[1] == found_out and np.array_equal(plain[2], stale)
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
        again, found_again, stale_again, _ = NP.keep_grid(out, nsec, off, cap, found_out, budget, cols, grows, bx, by)
        assert np.array_equal(again, out) and found_again == found_out and not stale_again.any()


def _rows_keys_cells(c, b=None):
    b = c["buf_ids"][0] if b is None else b
    buf = HG.case_buffers(c)[b]
    rows = stored_rows(*c["table"][:3], c["counts"][b])
    return NS.keys_of(buf[rows]), NP.cells_of(buf[rows], c["grid"][0], *c["bounds"])


def _kept(c):
    keys, cells = _rows_keys_cells(c)
    return keys, cells, NP.keep_mask_grid(keys, cells, c["grid"][0] * c["grid"][1], c["N"])


def test_case_table_reaches_its_edges():
    cs = HG.CASES
    changed = [c for c in cs if any(c["totals"][b] > c["N"] for b in c["buf_ids"])]
    assert {c["totals"][0] for c in cs if len(c["buf_ids"]) == 1} >= {0, 1, HG.ROUND - 1, HG.ROUND, HG.ROUND + 1, 2 * HG.ROUND + 1}
    assert any(max(c["totals"]) > HG.LDS_ROWS for c in changed)
    assert {c["grid"] for c in changed} >= {(1, 1), (2, 1), (1, 2), (3, 5), (16, 16), (16, 1)}
    cells_of_case = lambda c: c["grid"][0] * c["grid"][1]
    assert any(c["N"] < cells_of_case(c) and cells_of_case(c) > 1 for c in changed) and any(c["N"] == cells_of_case(c) > 1 for c in changed)
    assert any(c["N"] > cells_of_case(c) > 1 and c["N"] % cells_of_case(c) for c in changed)
    assert {c["keys"] for c in changed} >= {"all equal", "special", "ties", "random"}
    assert {c["place"] for c in changed if isinstance(c["place"], str)} == {"bytes", "uniform"} and any(callable(c["place"]) for c in changed)
    assert any(c["table"][0] == 16 for c in changed) and any(c["fixed"] for c in changed) and any(c["cache"] for c in changed) and any(not c["cache"] for c in changed)
    assert {c["pad"] for c in changed if c["cache"]} >= {0, 2}
    assert any(any(f > k for f, k in zip(c["counts"][b], c["table"][2])) and c["totals"][b] > c["N"] for c in cs for b in c["buf_ids"])       # clamped, selected
    assert any(any(f > k for f, k in zip(c["counts"][b], c["table"][2])) and c["totals"][b] <= c["N"] for c in cs for b in c["buf_ids"])      # clamped, unchanged
    assert any(len(c["buf_ids"]) == 3 and any(c["totals"][b] <= c["N"] for b in c["buf_ids"]) and sorted(c["buf_ids"]) != list(range(3)) for c in cs)
    assert any(len(c["buf_ids"]) == HG.GATHER_SLOTS for c in cs)
    # random bytes reach NaNs, negatives and values beyond the frame; bounds that are not monotone, NaN or infinite
    c = HG.case_named("grid (3, 5), 2049 rows as random bytes, N 301")
    x, y = NP.coords_of(HG.case_buffers(c)[0][stored_rows(*c["table"][:3], c["counts"][0])])
    assert np.isnan(x).any() and (x < 0).any() and (x > 640).any() and np.isnan(y).any() and len(np.unique(_rows_keys_cells(c)[1])) > 3
    assert any((np.diff(c["bounds"][0]) < 0).any() for c in changed) and any(np.isnan(c["bounds"][0]).any() for c in changed)
    # every row in one cell
    for name in ("every row in one cell (the last) of 3x5", "every row in one cell, all equal keys"):
        assert len(np.unique(_rows_keys_cells(HG.case_named(name))[1])) == 1
    # cells of q - 1, q and q + 1 rows, an empty one; the guarantee
    for c in [c for c in cs if c["name"].startswith("cells of q - 1, q, q + 1 rows")]:
        keys, cells, keep = _kept(c)
        q, had, has = c["N"] // 6, np.bincount(cells, minlength=6), np.bincount(cells[keep], minlength=6)
        assert sorted(had.tolist()) == [0, q - 1, q, q, q + 1, 40] and (has >= np.minimum(had, q)).all() and has.sum() == c["N"] and has.max() > q
    c = HG.case_named("empty cells: 2049 rows in cells 0 and 7 of 16x16")
    assert sorted(np.unique(_rows_keys_cells(c)[1]).tolist()) == [0, 7]
    # a tie at a cell's threshold whose kept rows lie on both sides of the section boundary (row 1000) and of the round boundary (row 1024), with rows
    # of the cell at that key left out behind them
    for name in ("all equal: the kept ties of a cell cross row 1000 and row 1024, N 1201", "ties: the kept ties of a cell cross row 1000 and row 1024, N 1500"):
        c = HG.case_named(name)
        keys, cells, keep = _kept(c)
        q = c["N"] // 2
        in0 = np.flatnonzero(cells == 0)
        first = in0[NS.keep_mask(keys[in0], q)]      # phase 1 of cell 0
        t = keys[first].min()
        at = first[keys[first] == t]
        assert at.min() < 1000 and ((at > 1000) & (at < HG.ROUND)).any() and at.max() > HG.ROUND and (keys[in0[in0 > at.max()]] == t).any(), name
    # the same key at a cell's threshold and at the threshold of phase 2: phase 2 has to pass over rows at its threshold that phase 1 kept
    for name in ("all equal: the kept ties of a cell cross row 1000 and row 1024, N 1201", "ties: cell and phase 2 thresholds share a key, 1x2, N 901"):
        c = HG.case_named(name)
        keys, cells, keep = _kept(c)
        q, ncell = c["N"] // 2, 2
        p1 = np.zeros(len(keys), bool)
        for k in range(ncell):
            idx = np.flatnonzero(cells == k)
            p1[idx[NS.keep_mask(keys[idx], q)]] = True
        p2 = keep & ~p1
        assert p2.any() and (keep & p1).sum() == p1.sum()
        t2 = keys[p2].min()
        assert any(keys[p1 & (cells == k)].min() == t2 for k in range(ncell)), name
        assert (p1 & (keys == t2) & (np.arange(len(keys)) > np.flatnonzero(p2 & (keys == t2)).min())).any() or (p1 & (keys == t2)).any()
        assert (~keep & (keys == t2)).any()      # and rows at that key are left out: the threshold is a tie
    c = HG.case_named("all equal, three cells, the kept ties end with the last row of round 0")
    keys, cells, keep = _kept(c)
    assert np.flatnonzero(keep).max() in (HG.ROUND - 1, HG.ROUND)


@pytest.mark.parametrize("case", [c for c in HG.CASES if max(c["totals"]) <= 2 * HG.ROUND + 1 and c["nbuf"] <= 8], ids=lambda c: c["name"])
def test_arena_states_the_contract(case):
    """the arena of a case on the CPU: what is expected differs from what goes in exactly where the contract writes"""
    h = HG.Spread(case, device="cpu")
    exp, loose = h._state()
    diff = exp != h.host
    changed = [b for b in case["buf_ids"] if case["totals"][b] > case["N"]]
    assert diff.any() == bool(changed) or not diff.any()
    inside = (np.arange(len(exp)) >= h.feats.off) & (np.arange(len(exp)) < h.feats.off + len(h.feats.payload))
    assert not loose[~inside].any()
    for b in case["buf_ids"]:
        if b not in changed:
            lo = h.feats.off + b * h.buf_stride
            assert not diff[lo:lo + h.buf_stride].any() and not loose[lo:lo + h.buf_stride].any()
    assert np.array_equal(h.masked(h.host)[~loose], h.host[~loose])
    # a 1x1 grid and N < C state the plain budget's arena
    if case["grid"] == (1, 1) or case["N"] < case["grid"][0] * case["grid"][1]:
        for b in changed:
            plain = NS.keep_strongest(h.bufs[b], h.nsec, h.off, h.cap, case["counts"][b], case["N"])
            mine = h.select(b)
            assert np.array_equal(plain[0], mine[0]) and plain[1] == mine[1] and np.array_equal(plain[2], mine[2])
