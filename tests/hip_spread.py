"""vksift_hip_keep_grid called directly, in the manner of tests/hip_strongest.py (plain module, no fixtures): the case table, and a Launch that
turns a case into ONE poisoned arena — the SIFT buffers with poisoned gaps, their counters, the host mirror the kernel posts the counters to,
and the matcher-cache blocks — and states the whole arena as the contract expects it afterwards, from tests/np_spread.py (records, counters)
and np_records.gather_sections of the selected buffer (cache entry). The only bytes not compared are the stale records the contract leaves
unspecified (Spread.masked).

A case is small: the smallest shapes at which the kernel can go wrong — totals around the round size of 1024 rows, one beyond the 8192 rows
whose key and cell the kernel holds in LDS, every grid shape that changes the cell arithmetic, budgets below, at and not divisible by the
number of cells, cells that hold one row fewer, exactly as many and one more than their share, ties at a cell's threshold across a round and
a section boundary, and a key that is both a cell's threshold and the threshold of the second phase.

Coordinates: "bytes" makes the x and y words random bytes (every bit pattern: NaNs, negatives, denormals, values far outside the frame; the
harness's own records name their buffer and row there);
"uniform" scatters the rows over the frame; a list or function gives every row its cell and puts the row exactly ON the cell's lower bounds
(the >= edge), or at 0 where the cell has none."""
import ctypes as C
import functools

import numpy as np

import hip_records as HR
import hip_strongest as HS
import np_spread as NP
import np_strongest as NS
import record_cases as RC
from test_section_walk import stored_rows

REC = NS.REC
u32 = np.uint32
ROUND = 1024          # rows per round of the ordered pass
LDS_ROWS = 8192       # GRID_LDS_ROWS of spread.hip
GATHER_SLOTS = HR.GATHER_SLOTS
one, two = HR.one, HS.two


def case(name, table, max_features, grid, *, size=(640, 480), bounds=None, place="uniform", keys="random", post=True, fixed=False, **shared):
    """grid: (cols, rows); bounds: (column bounds, row bounds) in place of those of `size`; shared: hip_records.sectioned_case"""
    c = HR.sectioned_case(name, table, fixed=fixed, keys=keys, post=post and not fixed, **shared)
    c["N"] = max_features([c["totals"][b] for b in c["buf_ids"]]) if callable(max_features) else max_features
    c["grid"], c["size"], c["place"] = tuple(grid), tuple(size), place
    bx, by = bounds if bounds is not None else (NP.bounds(size[0], grid[0]), NP.bounds(size[1], grid[1]))
    c["bounds"] = np.asarray(bx, np.float32), np.asarray(by, np.float32)
    assert len(c["bounds"][0]) == grid[0] - 1 and len(c["bounds"][1]) == grid[1] - 1
    return c


def _cells_with_counts(counts):
    """row -> cell such that cell k holds counts[k] rows, interleaved (row r goes to the next cell that still wants one)"""
    def place(total, rng):
        left, out, k = list(counts), [], 0
        assert sum(left) == total, (sum(left), total)
        while len(out) < total:
            if left[k % len(left)]:
                left[k % len(left)] -= 1
                out.append(k % len(left))
            k += 1
        return np.array(out)
    return place


def _alternate(ncell):
    return lambda total, rng: np.arange(total) % ncell


def _one_cell(cell):
    return lambda total, rng: np.full(total, cell)


CASES = []
# totals around the round size and every grid shape; alternately without and with the cache block, coordinates scattered or random bytes
_GRIDS = [(1, 1), (2, 1), (1, 2), (3, 5), (16, 16), (16, 1)]
for _i, _t in enumerate((0, 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1)):
    for _j, _n in enumerate(sorted({1, _t // 3, _t - 1, _t} - {0, -1})):
        CASES.append(case(f"total {_t}, N {_n}, grid {_GRIDS[(_i + _j) % 6]}", one(_t), _n, _GRIDS[(_i + _j) % 6], cache=len(CASES) % 2 == 1, seed=10 + len(CASES),
                          place="bytes" if len(CASES) % 3 == 0 else "uniform"))
CASES.append(case(f"total {LDS_ROWS + 9}, N 1000, grid 8x6 (rows beyond the LDS copy)", two(5000, LDS_ROWS + 9 - 5000), 1000, (8, 6), cache=True, seed=50))
CASES.append(case(f"total {LDS_ROWS + 9}, N total - 1, ties, random bytes", two(5000, LDS_ROWS + 9 - 5000), LDS_ROWS + 8, (3, 5), keys="ties", place="bytes", seed=51))
# grids and budgets: N < C, N == C, N not divisible by C
for _g in _GRIDS:
    _c = _g[0] * _g[1]
    CASES.append(case(f"grid {_g}, 2049 rows in two sections, N 700", two(1000, 1049), 700, _g, cache=_c % 2 == 1, seed=60 + len(CASES)))
    CASES.append(case(f"grid {_g}, 2049 rows as random bytes, N 301", two(1000, 1049), 301, _g, place="bytes", cache=_c % 2 == 0, seed=60 + len(CASES)))
CASES += [
    case("N < C: 255 of 300 rows, grid 16x16", one(300), 255, (16, 16), cache=True, seed=90),
    case("N == C: 256 of 300 rows, grid 16x16", one(300), 256, (16, 16), seed=91),
    case("N == C: 15 of 54 rows, grid 3x5", "three sections", 15, (3, 5), cache=True, seed=92),
    case("N < C: 14 of 54 rows, grid 3x5", "three sections", 14, (3, 5), seed=93),
    case("N = 2 C + 7, grid 3x5", one(400), 37, (3, 5), cache=True, seed=94),
]
# keys
for _k in ("all equal", "ties", "special", "low byte"):
    CASES.append(case(f"keys: {_k}, 2049 rows in two sections, grid 3x5, N 700", two(1000, 1049), 700, (3, 5), keys=_k, cache=True, seed=100 + len(CASES)))
    CASES.append(case(f"keys: {_k}, three sections, grid 2x1, N 17, random bytes", "three sections", 17, (2, 1), keys=_k, place="bytes", seed=100 + len(CASES)))
# cells
CASES += [
    case("every row in one cell (the last) of 3x5", two(1000, 1049), 700, (3, 5), place=_one_cell(14), cache=True, seed=120),
    case("every row in one cell, all equal keys", one(ROUND + 77), 100, (16, 1), place=_one_cell(5), keys="all equal", seed=121),
    # N 60, grid 3x2: q = 10; cells of 9, 10 and 11 rows, an empty one, one of 40: the cell of 9 and the empty one hand 11 rows on
    case("cells of q - 1, q, q + 1 rows and an empty cell", one(80), 60, (3, 2), place=_cells_with_counts([9, 10, 0, 11, 40, 10]), cache=True, seed=122),
    case("cells of q - 1, q, q + 1 rows, ties", one(80), 60, (3, 2), place=_cells_with_counts([9, 10, 0, 11, 40, 10]), keys="ties", seed=123),
    case("cells of q - 1, q, q + 1 rows, all equal keys", one(80), 60, (3, 2), place=_cells_with_counts([9, 10, 0, 11, 40, 10]), keys="all equal", cache=True, seed=124),
    case("empty cells: 2049 rows in cells 0 and 7 of 16x16", two(1000, 1049), 1000, (16, 16), place=lambda t, r: np.where(np.arange(t) % 3 == 0, 0, 7), seed=125),
    # 2049 equal keys, rows alternate between the two cells: q = 600 — cell 0 keeps rows 0, 2, .. 1198, across the section boundary (row 1000) and the
    # round boundary (row 1024), and not its rows behind them; the one row of phase 2 has the key of both thresholds: it is row 1200, the first not kept
    case("all equal: the kept ties of a cell cross row 1000 and row 1024, N 1201", two(1000, 1049), 1201, (2, 1), place=_alternate(2), keys="all equal", cache=True, seed=3),
    case("ties: the kept ties of a cell cross row 1000 and row 1024, N 1500", two(1000, 1049), 1500, (2, 1), place=_alternate(2), keys="ties", seed=4),
    case("ties: cell and phase 2 thresholds share a key, 1x2, N 901", two(1000, 1049), 901, (1, 2), place=_alternate(2), keys="ties", cache=True, seed=5),
    case("all equal, three cells, the kept ties end with the last row of round 0", one(ROUND + 500), 3 * 341 + 1, (3, 1), place=_alternate(3), keys="all equal", seed=6),
    # bounds that are no partition of anything: descending, repeated, negative, infinite, NaN (never satisfied), -0.0
    case("non-monotone bounds, 4x3", two(1000, 1049), 500, (4, 3), bounds=([400.0, 100.0, 400.0], [-5.0, 1e30]), cache=True, seed=7),
    case("bounds NaN, inf, -0.0, random bytes", one(700), 200, (4, 3), bounds=([np.nan, np.inf, -0.0], [-np.inf, 0.0]), place="bytes", seed=8),
    case("bounds of a 1x1 frame, random bytes", one(700), 200, (3, 5), size=(1, 1), place="bytes", cache=True, seed=9),
]
# tables
CASES += [
    case("sixteen sections, grid 3x5, N 100", "sixteen sections", 100, (3, 5), cache=True, fbs=17, seed=130),
    case("sixteen sections, grid 16x16, N total - 1, random bytes", "sixteen sections", lambda t: t[0] - 1, (16, 16), place="bytes", seed=131),
    case("sixteen, every one clamped, grid 2x1, N 60", "sixteen, every one clamped", 60, (2, 1), cache=True, seed=132),
    case("an empty section between two others, grid 1x2, N 20", "three, an empty section between two others", 20, (1, 2), cache=True, seed=133),
    case("gaps between the sections, grid 2x1, N 7", "three, gaps between the sections", 7, (2, 1), cache=True, seed=134),
    case("a counter above its capacity, grid 3x5, N 40", "three, found > cap in the middle", 40, (3, 5), cache=True, seed=135),
    case("a counter above its capacity, unchanged (N = total)", "three, found > cap in the middle", lambda t: t[0], (3, 5), cache=True, seed=136),
    case("dense layout (fixed counts), 1500 rows, grid 8x6, N 1000", one(1500, cap=1500), 1000, (8, 6), fixed=True, cache=True, seed=137),
    case("dense layout (fixed counts), unchanged", one(300, cap=300), 300, (8, 6), fixed=True, cache=True, seed=138),
    case("fixed counts, three sections, grid 2x1, N 11", "three sections", 11, (2, 1), fixed=True, seed=139),
    case("not posted, found_buf_stride 3", "three sections", 30, (3, 5), post=False, fbs=3, seed=140),
    case("posted, found_buf_stride 256", "three sections", 30, (3, 5), fbs=256, cache=True, desc_extra=3, norm_extra=5, n_stride=3, seed=141),
    case("N 1 of 54 with the cache block: one padding row", "three sections", 1, (2, 1), cache=True, seed=142),
    case("N 1, pad 0", "three sections", 1, (2, 1), cache=True, pad=0, seed=143),
    case("N 30, grid 3x5, pad 0", "three sections", 30, (3, 5), cache=True, pad=0, seed=144),
    # slots: buffers 5, 0, 3 of 8 with different totals; buffer 0 holds 9 rows and is left alone, the unnamed ones hold rows too
    case("three slots {5, 0, 3} of 8, one unchanged", "three sections", 25, (3, 2), nbuf=8, buf_ids=[5, 0, 3], cache=True, desc_extra=1, norm_extra=3, n_stride=2, seed=145,
         counts=[[4, 3, 2], [50, 20, 8], [31, 20, 3], [0, 20, 9], [7, 7, 7], [50, 0, 8], [1, 1, 1], [31, 77, 3]]),
    case("three slots {5, 0, 3} of 8, no cache", "three sections", 25, (3, 2), nbuf=8, buf_ids=[5, 0, 3], seed=146,
         counts=[[4, 3, 2], [50, 20, 8], [31, 20, 3], [0, 20, 9], [7, 7, 7], [50, 0, 8], [1, 1, 1], [31, 77, 3]]),
    case("512 slots", one(40, cap=40), 13, (3, 2), size=(160, 120), nbuf=512, buf_ids=[(37 * i + 5) % 512 for i in range(512)], cache=True, seed=147,
         counts=[[(11 * b) % 43] for b in range(512)]),
]
assert len({c["name"] for c in CASES}) == len(CASES)

case_named = functools.partial(HR.case_named, CASES)


def _f32_bytes(v):
    return np.asarray(v, "<f4").view(np.uint8).reshape(-1, 4)


def case_buffers(c):
    """(nbuf, extent, 164) record bytes of the case: random records whose intensity words are the case's keys and whose x and y words follow the
    case's placement, in download order; the records outside the stored rows keep random bytes"""
    nsec, off, cap, _ = c["table"]
    bufs = RC.buffer_bytes(c["nbuf"], RC.extent_of(off, cap, nsec), c["seed"])
    rng = np.random.default_rng(2000 + c["seed"])
    (cols, _), (w, h), (bx, by) = c["grid"], c["size"], c["bounds"]
    lo_x, lo_y = np.concatenate([[0.0], bx]).astype(np.float32), np.concatenate([[0.0], by]).astype(np.float32)
    for b in range(c["nbuf"]):
        rows = stored_rows(nsec, off, cap, c["counts"][b])
        n = len(rows)
        bufs[b, rows, NS.KEY_AT:NS.KEY_AT + 4] = HS.make_keys(c["keys"], n, rng).astype("<u4").view(np.uint8).reshape(-1, 4)
        if c["place"] == "bytes":       # of every record of the buffer, stored or not
            bufs[b, :, 0:8] = rng.integers(0, 256, (bufs.shape[1], 8), dtype=np.uint8)
        if c["place"] == "bytes" or n == 0:
            continue
        if c["place"] == "uniform":
            x, y = rng.uniform(0, w, n), rng.uniform(0, h, n)
        else:
            cells = np.asarray(c["place"](n, rng) if callable(c["place"]) else c["place"])
            x, y = lo_x[cells % cols], lo_y[cells // cols]
        bufs[b, rows, 0:4], bufs[b, rows, 4:8] = _f32_bytes(x), _f32_bytes(y)
    return bufs


def float_words(values):
    """a host array of floats the launcher reads"""
    values = [float(v) for v in np.asarray(values, np.float32)]
    return (C.c_float * max(len(values), 1))(*values)


class Spread(HR.Sectioned):
    entry = "keep_grid"

    def __init__(self, c, device="cuda"):
        super().__init__(c, device)
        self.sift_blocks(case_buffers(c))
        self.post = self.poison("found_post", c["nbuf"] * c["fbs"] * 4, slot_bytes=4 * c["fbs"], row_bytes=4) if c["post"] else None
        self.cache_blocks(max(min(max(c["totals"]), c["N"]), c["pad"]), c["cache"])
        self.finish(found_post=self.post, max_features=c["N"], grid_cols=c["grid"][0], grid_rows=c["grid"][1], col_bounds=float_words(c["bounds"][0]),
                    row_bounds=float_words(c["bounds"][1]))
        self._expected = None

    def select(self, b):
        """np_spread.keep_grid of buffer b"""
        c = self.case
        return NP.keep_grid(self.bufs[b], self.nsec, self.off, self.cap, c["counts"][b], c["N"], *c["grid"], *c["bounds"])

    def _state(self):
        """(expected arena, bool mask of the arena bytes the contract leaves unspecified)"""
        if self._expected is None:
            c = self.case
            exp, loose = self.host.copy(), np.zeros(len(self.host), bool)
            extent = self.bufs.shape[1]
            for b in c["buf_ids"]:
                if c["totals"][b] <= c["N"]:
                    continue    # nothing of this buffer is written
                out, found_out, stale, _ = self.select(b)
                lo = self.feats.off + b * self.buf_stride
                exp[lo:lo + extent * REC] = out.reshape(-1)
                loose[lo:lo + extent * REC] = np.repeat(stale, REC)
                if not c["fixed"]:
                    self.view(exp, self.found, u32)[b * c["fbs"]:][:self.nsec] = found_out[:self.nsec]
                    if c["post"]:
                        self.view(exp, self.post, u32)[b * c["fbs"]:][:self.nsec] = found_out[:self.nsec]
                if c["cache"]:
                    total = self.expect_entry(exp, b, out, found_out)
                    assert total == c["N"]
            self._expected = exp, loose
        return self._expected

    def expected(self):
        return self._state()[0]

    def masked(self, after):
        """`after` with the expected bytes in place of the unspecified ones"""
        exp, loose = self._state()
        out = np.array(after, copy=True)
        out[loose] = exp[loose]
        return out


# (a case of the table, the arguments changed): hipErrorInvalidValue, and the arena as it was. "+name": added to a pointer or a stride.
_R = "three slots {5, 0, 3} of 8, one unchanged"
REFUSALS = [
    (_R, {"nslots": 0}),
    (_R, {"nslots": GATHER_SLOTS + 1}),
    (_R, {"nsec": 17}),
    (_R, {"max_features": 0}),
    (_R, {"+feats_base": 2}),
    (_R, {"+buf_stride": 2}),
    (_R, {"+desc": 8}),
    (_R, {"+desc_stride": 8}),
    (_R, {"norms": None}),
    (_R, {"found_base": None}),                                              # no counter source at all (and a mirror without device counters)
    ("posted, found_buf_stride 256", {"found_buf_stride": 257}),
    (_R, {"fixed_counts": "given"}),                                        # fixed_counts and found_base both given
    ("dense layout (fixed counts), 1500 rows, grid 8x6, N 1000", {"fixed_counts": None}),   # ... and both NULL
    ("dense layout (fixed counts), 1500 rows, grid 8x6, N 1000", {"found_post": "given"}),     # a mirror without device counters
    (_R, {"grid_cols": 0}),
    (_R, {"grid_cols": 17}),
    (_R, {"grid_rows": 0}),
    (_R, {"grid_rows": 17}),
    (_R, {"grid_cols": 0xFFFFFFFF}),
    (_R, {"col_bounds": None}),                                             # three columns, no bounds
    (_R, {"row_bounds": None}),
]
