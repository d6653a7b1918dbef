"""vksift_hip_root_descriptors called directly, in the manner of tests/hip_records.py and tests/hip_strongest.py (plain module, no fixtures): the
case table, and a Launch that turns a case into ONE poisoned arena — the SIFT buffers with poisoned gaps, their counters, and the matcher-cache
blocks — and states the whole arena as the contract expects it afterwards: tests/np_rootsift.py on the stored rows of every named buffer, and
np_records.gather_sections of the converted buffer for its cache entry. Every byte is compared; the contract leaves none unspecified.

A case is small: the smallest shapes at which the kernel can go wrong — totals around the eight rows of a wave, the 32 of a workgroup and the
stride of a grid of one, two, eight (512 slots) and 256 workgroups; rows of every shape the arithmetic treats differently; and ONE large case,
all_pairs_rows(): every (d, s) pair a 128-bin row can hold, which is what fails an implementation without the integer correction step."""
import functools

import numpy as np

import hip_records as HR
import np_rootsift as RS
import record_cases as RC
from test_section_walk import _table, stored_rows

REC = RS.REC
u32 = np.uint32
ROWS_PER_WAVE, ROWS_PER_BLOCK = 8, 32     # rootsift.hip: eight lanes per row, 256 threads
MAX_BLOCKS, MIN_BLOCKS = 256, 8           # ... and the grid of one buffer alone; 8 per buffer with 512 slots
GATHER_SLOTS = HR.GATHER_SLOTS
REST_MAX = 127 * 255                      # what the other 127 bins of a row can add to one bin


# ---------------------------------------------------------------------------------------------------------------------- rows
def reachable_pairs():
    """(S_MAX + 1, 256) bool: [s, d] — a row of 128 bytes can hold a bin d and sum to s >= 1"""
    s, d = np.arange(RS.S_MAX + 1)[:, None], np.arange(256)[None, :]
    return (s >= 1) & (d <= s) & (s - d <= REST_MAX)


@functools.lru_cache(maxsize=None)
def all_pairs_rows():
    """(n, 128) uint8 rows in which every reachable (d, s) pair occurs at least once (asserted). For each s the bins it needs, from the largest
    down, go into rows in runs c, c - 1, .. of as many as fit — at most 128, their sum at most s, and the rest of the row able to hold what is
    missing to s —, the rest is topped up with 255s and one remainder; all s at once, one run per round. The bins of a row are then permuted.
    Some 3.7e5 rows (60 MB of records), and no table is much smaller: the bins a row of sum s shows sum to at most s, and what they lack to 255
    each sums to at most 32640 - s, while the 256 bins to be shown sum to 32640 either way — at least 32640 / min(s, 32640 - s) rows for every s."""
    s_all = np.arange(1, RS.S_MAX + 1, dtype=np.int64)
    lo, cur = np.maximum(0, s_all - REST_MAX), np.minimum(255, s_all)
    runs, active = [], np.arange(len(s_all))
    while len(active):
        s, c = s_all[active], cur[active]
        # the longest run c, c - 1, .. of k bins that fits: k = 1 always does, and each condition holds for a prefix of the run lengths (bisection)
        fits = lambda k: (k * c - k * (k - 1) // 2 <= s) & (s - (k * c - k * (k - 1) // 2) <= 255 * (128 - k))
        k, over = np.ones_like(c), np.minimum(128, c - lo[active] + 1) + 1
        assert fits(k).all()
        while (over - k > 1).any():
            mid = (k + over) // 2
            ok = fits(mid) & (over - k > 1)
            k, over = np.where(ok, mid, k), np.where(ok | (over - k <= 1), over, mid)
        runs.append((s, c, k))
        cur[active] -= k
        active = active[cur[active] >= lo[active]]
    s, c, k = (np.concatenate(v)[:, None] for v in zip(*runs))
    i = np.arange(128, dtype=np.int64)[None, :]
    rows = np.where(i < k, c - i, 0)
    rest = s - rows.sum(1, keepdims=True)
    full, part, at = rest // 255, rest % 255, i - k
    rows += np.where((at >= 0) & (at < full), 255, 0) + np.where(at == full, part, 0)
    assert rows.min() >= 0 and rows.max() <= 255 and np.array_equal(rows.sum(1, keepdims=True), s)
    rows = np.random.default_rng(12).permuted(rows.astype(np.uint8), axis=1)
    seen = np.zeros((RS.S_MAX + 1, 256), bool)
    seen[np.broadcast_to(s, rows.shape), rows] = True
    assert np.array_equal(seen, reachable_pairs()), "every reachable (d, s) pair, and no other"
    return rows


def shape_rows():
    """the rows the arithmetic treats differently, once each"""
    def row(*bins, fill=0):
        r = np.full(128, fill, np.uint8)
        for at, v in bins:
            r[at] = v
        return r
    out = [row(), row((5, 1)), row((127, 1)), row((0, 255)), row((66, 255)), row(fill=255), row(fill=1), row((3, 2), fill=1)]
    # d = 255 in rows of s = 1021 .. 1034: r goes from 256 (cut to 255) at s <= 1023 through 255 to 254 at s = 1033 (512 sqrt(255 / s) = 254.5 at 1032.1)
    out += [row((9, 255), (10, 255), (77, 255), (120, 255), (121, extra)) for extra in range(1, 15)]
    out += [row((0, 255), (1, 1)), row((0, 254), (64, 1), (127, 1)), row((31, 128), (32, 127))]
    return np.stack(out)


def make_rows(kind, n, rng):
    """n descriptor rows in download order"""
    if kind == "all pairs":
        rows = all_pairs_rows()
        assert n == len(rows)
        return rows
    if kind == "shapes":
        return shape_rows()[np.arange(n) % len(shape_rows())]
    if kind == "random":      # every scale of s: the largest bin of a row is 1, 3, 15, 63 or 255, a third of the rows sparse
        top = np.array([1, 3, 15, 63, 255])[rng.integers(0, 5, n)][:, None]
        rows = rng.integers(0, 256, (n, 128)) % (top + 1)
        rows[rng.random((n, 128)) < 0.8 * (rng.random(n) < 0.33)[:, None]] = 0
        return rows.astype(np.uint8)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------------- cases
def case(name, table, *, rows="random", max_rows="exact", **shared):
    """max_rows: "exact" = the largest total of the named buffers; shared: hip_records.sectioned_case"""
    return HR.sectioned_case(name, table, rows=rows, max_rows=max_rows, **shared)


one = HR.one


_EIGHT = [[4, 3, 2], [50, 20, 8], [31, 20, 3], [0, 20, 9], [7, 7, 7], [50, 0, 8], [1, 1, 1], [31, 77, 3]]
_WAVE, _BLOCK = ROWS_PER_WAVE, ROWS_PER_BLOCK
CASES = []
# row totals: 0, 1, 2; around a wave (8 rows), a workgroup (32), and the stride of a grid of one workgroup (max_rows 0: 32 rows), of two (max_rows 64:
# 64 rows) and of the 256 a buffer alone gets (8192 rows); alternately without and with the cache block
for _t, _mr in [(0, "exact"), (1, "exact"), (2, "exact"), (_WAVE - 1, "exact"), (_WAVE, "exact"), (_WAVE + 1, "exact"), (_BLOCK - 1, "exact"), (_BLOCK, "exact"),
                (_BLOCK + 1, "exact"), (_BLOCK - 1, 0), (_BLOCK, 0), (_BLOCK + 1, 0), (2 * _BLOCK + 1, 0), (2 * _BLOCK - 1, 2 * _BLOCK), (2 * _BLOCK, 2 * _BLOCK),
                (2 * _BLOCK + 1, 2 * _BLOCK), (4 * _BLOCK + 1, 2 * _BLOCK),
                (MAX_BLOCKS * _BLOCK - 1, "exact"), (MAX_BLOCKS * _BLOCK, "exact"), (MAX_BLOCKS * _BLOCK + 1, "exact")]:
    CASES.append(case(f"total {_t}, max_rows {_mr}", one(_t), max_rows=_mr, cache=len(CASES) % 2 == 1, seed=10 + len(CASES)))
CASES += [
    # max_rows sizes the grid and nothing else
    case("54 rows, max_rows 0", "three sections", max_rows=0, cache=True, seed=40),
    case("54 rows, max_rows 4000000000", "three sections", max_rows=4000000000, cache=True, seed=40),
    case("54 rows, max_rows 0, no cache", "three sections", max_rows=0, seed=41),
    # row shapes
    case("row shapes", one(2 * len(shape_rows()) + 1), rows="shapes", cache=True, seed=42),
    case("row shapes in three sections, no cache", "three sections", rows="shapes", seed=43),
    # tables
    case("sixteen sections", "sixteen sections", cache=True, fbs=17, seed=44),
    case("sixteen sections, no cache", "sixteen sections", seed=45),
    case("sixteen, every one clamped", "sixteen, every one clamped", cache=True, seed=46),
    case("an empty section between two others", "three, an empty section between two others", cache=True, seed=47),
    case("first empty, last found == cap", "three, first empty, last found == cap", seed=48),
    case("gaps between the sections", "three, gaps between the sections", cache=True, seed=49),
    case("gaps between the sections, no cache", "three, gaps between the sections", seed=50),
    case("a capacity of zero", "a capacity of zero", cache=True, seed=51),
    case("a counter above its capacity", "three, found > cap in the middle", cache=True, seed=52),
    case("one section, found > cap", "one section, found > cap", seed=53),
    case("no section", _table(0, [], [], off=[]), cache=True, seed=54),
    # counters
    case("dense layout (fixed counts), 300 rows", one(300, cap=300), fixed=True, cache=True, seed=55),
    case("dense layout (fixed counts), no cache", one(77, cap=77), fixed=True, seed=56),
    case("fixed counts, three sections", "three sections", fixed=True, cache=True, seed=57),
    case("found_buf_stride 3", "three sections", fbs=3, seed=58),
    case("found_buf_stride 256", "three sections", fbs=256, cache=True, seed=59),
    # cache
    case("total 0, pad 0", one(0), cache=True, pad=0, seed=60),
    case("total 1, pad 0", one(1), cache=True, pad=0, seed=61),
    case("total 0, pad 2", one(0), cache=True, pad=2, seed=62),
    case("total 1, pad 2", one(1), cache=True, pad=2, seed=63),
    case("total 1, pad 2, no cache: pad_rows_to is not looked at", one(1), pad=2, seed=64),
    case("strides with extra room", "three sections", cache=True, desc_extra=3, norm_extra=5, n_stride=3, seed=65),
    # slots: buffers 5, 0, 3 of 8 with different totals, the unnamed ones full of rows
    case("three slots {5, 0, 3} of 8", "three sections", nbuf=8, buf_ids=[5, 0, 3], cache=True, desc_extra=1, norm_extra=3, n_stride=2, seed=66, counts=_EIGHT),
    case("three slots {5, 0, 3} of 8, no cache", "three sections", nbuf=8, buf_ids=[5, 0, 3], seed=67, counts=_EIGHT),
    # 512 slots get 8 workgroups each: a stride of 256 rows, totals up to 260
    case("512 slots", one(260, cap=260), nbuf=512, buf_ids=[(37 * i + 5) % 512 for i in range(512)], cache=True, seed=68, counts=[[(11 * b) % 261] for b in range(512)]),
]
# (the large case is laid out when it is asked for: building its rows takes a second)
ALL_PAIRS = "every reachable (d, s) pair"


def all_pairs_case():
    n = len(all_pairs_rows())
    return case(ALL_PAIRS, one(n, cap=n), rows="all pairs", seed=69)   # (no cache block: the entry is a copy of the same dwords, and as large again)


assert len({c["name"] for c in CASES}) == len(CASES)


case_named = functools.partial(HR.case_named, CASES)


def case_buffers(c):
    """(nbuf, extent, 164) record bytes of the case: random records whose stored rows carry the case's descriptor rows, in download order; the
    records outside the stored rows keep random bytes"""
    nsec, off, cap, _ = c["table"]
    bufs = RC.buffer_bytes(c["nbuf"], RC.extent_of(off, cap, nsec), c["seed"])
    rng = np.random.default_rng(2000 + c["seed"])
    for b in range(c["nbuf"]):
        rows = stored_rows(nsec, off, cap, c["counts"][b])
        bufs[b, rows, RS.DESC_AT:] = make_rows(c["rows"], len(rows), rng)
    return bufs


class Root(HR.Sectioned):
    entry = "root_descriptors"

    def __init__(self, c, device="cuda"):
        super().__init__(c, device)
        self.sift_blocks(case_buffers(c))
        self.cache_blocks(max(max(self.named), c["pad"]), c["cache"])
        self.finish(max_rows=self.max_rows())
        self._expected = None

    def expected(self):
        if self._expected is None:
            c = self.case
            exp = self.host.copy()
            extent = self.bufs.shape[1]
            for b in c["buf_ids"]:
                out = RS.convert_buffer(self.bufs[b], stored_rows(self.nsec, self.off, self.cap, c["counts"][b]))
                lo = self.feats.off + b * self.buf_stride
                exp[lo:lo + extent * REC] = out.reshape(-1)
                if c["cache"]:
                    self.expect_entry(exp, b, out, c["counts"][b])
            self._expected = exp
        return self._expected


# (a case of the table, the arguments changed): hipErrorInvalidValue, and the arena as it was. "+name": added to a pointer or a stride.
_R = "three slots {5, 0, 3} of 8"
REFUSALS = [
    (_R, {"nslots": 0}),
    (_R, {"nslots": GATHER_SLOTS + 1}),
    (_R, {"nsec": 17}),
    (_R, {"+feats_base": 2}),
    (_R, {"+feats_base": 1}),
    (_R, {"+buf_stride": 2}),
    (_R, {"+desc": 4}),
    (_R, {"+desc": 8}),
    (_R, {"+desc_stride": 8}),
    (_R, {"norms": None}),
    (_R, {"n_out": None}),
    (_R, {"fixed_counts": "given"}),                                   # fixed_counts and found_base both given
    ("dense layout (fixed counts), 300 rows", {"fixed_counts": None}),    # ... and both NULL
]
