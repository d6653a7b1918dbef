"""vksift_hip_keep_strongest called directly, in the manner of tests/hip_records.py (plain module, no fixtures): the case table, and a
Launch that turns a case into ONE poisoned arena — the SIFT buffers with poisoned gaps, their counters, the host mirror the kernel posts the
counters to, and the matcher-cache blocks — and states the whole arena as the contract expects it afterwards, from tests/np_strongest.py
(records, counters) and np_records.gather_sections of the selected buffer (cache entry).

The only bytes that are not compared are the ones the contract leaves unspecified: of a buffer the launch selects from, the records of a
section from its new count up to its old stored count (Strongest.masked puts the expected bytes there before the comparison).

A case is small: the smallest shapes at which the kernel can go wrong — totals around the round size of 1024 rows, one total beyond the
8192 keys the kernel holds in LDS (it reads the others from the records again), budgets around the total, ties at the threshold across a
section and a round boundary, keys that differ in one byte only, and the bit patterns a float comparison would get wrong."""
import functools

import numpy as np

import hip_records as HR
import np_strongest as NS
import record_cases as RC
from test_section_walk import _table, stored_rows

REC = NS.REC
u32 = np.uint32
ROUND = 1024          # rows per round of the ordered pass
LDS_KEYS = 8192       # STRONGEST_LDS_KEYS of strongest.hip
GATHER_SLOTS = HR.GATHER_SLOTS


def _bits(v):
    return int(np.array(v, np.float32).view(u32))


SPECIAL_KEYS = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00000, 0x7F800001, _bits(-0.03), _bits(0.03),
                _bits(-1.5), _bits(1e-38), _bits(3.0e38), _bits(-0.02999), 0x00800000]


def make_keys(kind, n, rng):
    """the intensity words (sign bit and all) of n download-order rows"""
    i = np.arange(n)
    if kind == "random":          # |response| of a detection: small positive and negative normals
        return (rng.uniform(0.005, 0.2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32).view(u32)
    if kind == "all equal":
        return np.full(n, _bits(-0.04), u32)
    if kind == "low byte":        # one radix pass decides: the last
        return (u32(0x3D000000) | rng.integers(0, 256, n).astype(u32)) ^ (rng.integers(0, 2, n).astype(u32) << 31)
    if kind == "high byte":       # ... the first
        return (rng.integers(0, 128, n).astype(u32) << 24) | u32(0x00345678) | (rng.integers(0, 2, n).astype(u32) << 31)
    if kind == "each byte once":  # distinct in every byte: every pass narrows the set
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(u32)
    if kind == "special":
        return np.array(SPECIAL_KEYS, u32)[rng.integers(0, len(SPECIAL_KEYS), n)]
    if kind == "ties":            # every fifth row above the threshold, a few below, the rest AT it
        k = np.full(n, _bits(0.05), u32)
        k[i % 5 == 0] = _bits(-0.07)
        k[i % 11 == 3] = _bits(0.01)
        return k
    if kind == "last section strongest" or kind == "first section strongest":
        return (rng.uniform(0.005, 0.01, n)).astype(np.float32).view(u32)   # the section's rows are raised by case()
    raise KeyError(kind)


def _ties_budget(total, upto):
    """the budget with which the last kept row of `total` rows of kind "ties" is the last row at the threshold below row `upto`"""
    k = make_keys("ties", total, None) & u32(0x7FFFFFFF)
    return int((k > _bits(0.05)).sum() + (k[:upto] == _bits(0.05)).sum())


def case(name, table, max_features, *, keys="random", post=True, fixed=False, **shared):
    """max_features: a number, or a function of the totals of the named buffers (a list) that returns one; shared: hip_records.sectioned_case"""
    c = HR.sectioned_case(name, table, fixed=fixed, keys=keys, post=post and not fixed, **shared)
    c["N"] = max_features([c["totals"][b] for b in c["buf_ids"]]) if callable(max_features) else max_features
    return c


one = HR.one


def two(a, b):
    return _table(2, [a + 2, b + 1], [a, b])


CASES = []
# totals around the round size, budgets around the total; alternately without and with the cache block
for _t in (0, 1, 2, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1):
    for _n in sorted({1, _t - 1, _t, _t + 1} - {0, -1}):
        CASES.append(case(f"total {_t}, N {_n}", one(_t), _n, cache=len(CASES) % 2 == 1, seed=10 + len(CASES)))
CASES.append(case(f"total {LDS_KEYS + 9}, N 1000 (keys beyond the LDS copy)", two(5000, LDS_KEYS + 9 - 5000), 1000, cache=True, seed=50))
CASES.append(case(f"total {LDS_KEYS + 9}, N total - 1, ties", two(5000, LDS_KEYS + 9 - 5000), LDS_KEYS + 8, keys="ties", seed=51))
# keys
for _k in ("all equal", "low byte", "high byte", "each byte once", "special"):
    CASES.append(case(f"keys: {_k}, total 2049 in two sections, N 700", two(1000, 1049), 700, keys=_k, cache=True, seed=60 + len(CASES)))
    CASES.append(case(f"keys: {_k}, three sections, N 17", "three sections", 17, keys=_k, seed=80 + len(CASES)))
CASES.append(case("keys: special, N 5 of 16 rows, every pattern once", one(16), 5, keys="special", cache=True, seed=99))
# 2049 rows, sections of 1000 and 1049: 373 rows above the threshold, 1490 at it (727 of them in the first section). N 1500: the kept ties run across the section boundary (row 1000)
# and the round boundary (row 1024), and end in the second round; N 700: they end in the first round, in front of both
CASES.append(case("ties across the section and the round boundary, N 1500", two(1000, 1049), 1500, keys="ties", cache=True, seed=3))
CASES.append(case("ties that end in the first round, N 700", two(1000, 1049), 700, keys="ties", seed=4))
CASES.append(case("ties, the quota ends with the last row of round 0", one(ROUND + 500), _ties_budget(ROUND + 500, ROUND), keys="ties", seed=5))
# tables
CASES += [
    case("sixteen sections, N 100", "sixteen sections", 100, cache=True, fbs=17, seed=6),
    case("sixteen sections, N total - 1", "sixteen sections", lambda t: t[0] - 1, seed=7),
    case("sixteen, every one clamped, N 60", "sixteen, every one clamped", 60, cache=True, seed=8),
    case("an empty section between two others, N 20", "three, an empty section between two others", 20, cache=True, seed=9),
    case("first empty, last found == cap, N 4", "three, first empty, last found == cap", 4, seed=10),
    case("gaps between the sections, N 7", "three, gaps between the sections", 7, cache=True, seed=11),
    case("a capacity of zero, N 3", "a capacity of zero", 3, seed=12),
    case("a counter above its capacity, N 40", "three, found > cap in the middle", 40, cache=True, seed=13),
    case("a counter above its capacity, unchanged (N = total)", "three, found > cap in the middle", lambda t: t[0], cache=True, seed=14),
    case("one section, found > cap, unchanged (N above)", "one section, found > cap", 41, seed=15),
    case("N empties every section but the last", "three sections", 3, keys="last section strongest", cache=True, seed=16),
    case("N keeps only rows of the first section", "three sections", 28, keys="first section strongest", seed=17),
    case("dense layout (fixed counts), 1500 rows, N 1000", one(1500, cap=1500), 1000, fixed=True, cache=True, seed=18),
    case("dense layout (fixed counts), unchanged", one(300, cap=300), 300, fixed=True, cache=True, seed=19),
    case("fixed counts, three sections, N 11", "three sections", 11, fixed=True, seed=20),
    case("not posted, found_buf_stride 3", "three sections", 30, post=False, fbs=3, seed=21),
    case("posted, found_buf_stride 256", "three sections", 30, fbs=256, cache=True, desc_extra=3, norm_extra=5, n_stride=3, seed=22),
    case("N 1 of 54 with the cache block: one padding row", "three sections", 1, cache=True, seed=23),
    case("N 1, pad 0", "three sections", 1, cache=True, pad=0, seed=24),
    # slots: buffers 5, 0, 3 of 8 with different totals; buffer 0 holds 9 rows and is left alone, the unnamed ones hold rows too
    case("three slots {5, 0, 3} of 8, one unchanged", "three sections", 25, nbuf=8, buf_ids=[5, 0, 3], cache=True, desc_extra=1, norm_extra=3, n_stride=2, seed=25,
         counts=[[4, 3, 2], [50, 20, 8], [31, 20, 3], [0, 20, 9], [7, 7, 7], [50, 0, 8], [1, 1, 1], [31, 77, 3]]),
    case("three slots {5, 0, 3} of 8, no cache", "three sections", 25, nbuf=8, buf_ids=[5, 0, 3], seed=26,
         counts=[[4, 3, 2], [50, 20, 8], [31, 20, 3], [0, 20, 9], [7, 7, 7], [50, 0, 8], [1, 1, 1], [31, 77, 3]]),
    case("512 slots", one(40, cap=40), 13, nbuf=512, buf_ids=[(37 * i + 5) % 512 for i in range(512)], cache=True, seed=27,
         counts=[[(11 * b) % 43] for b in range(512)]),
]
assert len({c["name"] for c in CASES}) == len(CASES)


case_named = functools.partial(HR.case_named, CASES)


def case_buffers(c):
    """(nbuf, extent, 164) record bytes of the case: random records whose intensity words are the case's keys, in download order; the records
    outside the stored rows keep random intensity words"""
    nsec, off, cap, _ = c["table"]
    extent = RC.extent_of(off, cap, nsec)
    bufs = RC.buffer_bytes(c["nbuf"], extent, c["seed"])
    rng = np.random.default_rng(1000 + c["seed"])
    for b in range(c["nbuf"]):
        rows = stored_rows(nsec, off, cap, c["counts"][b])
        keys = make_keys(c["keys"], len(rows), rng).copy()
        strong = {"last section strongest": nsec - 1, "first section strongest": 0}.get(c["keys"])
        if strong is not None:
            sel = (rows >= off[strong]) & (rows < off[strong] + cap[strong])
            keys[sel] = rng.uniform(0.05, 0.2, int(sel.sum())).astype(np.float32).view(u32) | u32(0x80000000)
        bufs[b, rows, NS.KEY_AT:NS.KEY_AT + 4] = keys.astype("<u4").view(np.uint8).reshape(-1, 4)
    return bufs


class Strongest(HR.Sectioned):
    entry = "keep_strongest"

    def __init__(self, c, device="cuda"):
        super().__init__(c, device)
        self.sift_blocks(case_buffers(c))
        self.post = self.poison("found_post", c["nbuf"] * c["fbs"] * 4, slot_bytes=4 * c["fbs"], row_bytes=4) if c["post"] else None
        self.cache_blocks(max(min(max(c["totals"]), c["N"]), c["pad"]), c["cache"])
        self.finish(found_post=self.post, max_features=c["N"])
        self._expected = None

    def _state(self):
        """(expected arena, bool mask of the arena bytes the contract leaves unspecified)"""
        if self._expected is None:
            c = self.case
            exp, loose = self.host.copy(), np.zeros(len(self.host), bool)
            extent = self.bufs.shape[1]
            for b in c["buf_ids"]:
                if c["totals"][b] <= c["N"]:
                    continue    # nothing of this buffer is written
                out, found_out, stale, _ = NS.keep_strongest(self.bufs[b], self.nsec, self.off, self.cap, c["counts"][b], c["N"])
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
    (_R, {"+feats_base": 1}),
    (_R, {"+buf_stride": 2}),
    (_R, {"+desc": 4}),
    (_R, {"+desc": 8}),
    (_R, {"+desc_stride": 8}),
    ("posted, found_buf_stride 256", {"found_buf_stride": 257}),
    (_R, {"fixed_counts": "given"}),                                        # fixed_counts and found_base both given
    ("dense layout (fixed counts), 1500 rows, N 1000", {"fixed_counts": None}),   # ... and both NULL
]
