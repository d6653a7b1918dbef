"""The case table of the record-moving launchers (vksift_hip_gather_descriptors, _shifted_norms, _gather_sections, _pack_features,
_filter_matches, _gather_correspondences, _gather_xy): plain data and seeded numpy, imported by tests/test_np_records.py (CPU: pins the
reference and asserts that the table reaches every edge) and tests/test_gpu_record_launchers.py (one launch per case). tests/hip_records.py
turns a case into a poisoned arena and the bytes the contract expects.

Every case is tiny: a few hundred records per buffer, a few thousand 2-NN records per slot."""
import numpy as np

import np_records as NR
from test_section_walk import MAX_SECTIONS, TABLES, _table, stored_rows

f32 = np.float32
REC = NR.REC
DENSE = NR.LAYOUT_DENSE
JUNK_COUNTER = 11   # what a counter beyond a buffer's sections holds: never to be read


def buffer_bytes(nbuf, extent, seed):
    """(nbuf, extent, 164) random record bytes; x, y are finite floats that name (buffer, record): x = 4096 * buffer + record, y = -record - 0.5"""
    out = np.random.default_rng(seed).integers(0, 256, (nbuf, extent, REC), dtype=np.uint8)
    xy = np.empty((nbuf, extent, 2), f32)
    xy[..., 0] = 4096.0 * np.arange(nbuf)[:, None] + np.arange(extent)[None, :]
    xy[..., 1] = -np.arange(extent)[None, :] - 0.5
    out[..., :8] = xy.view(np.uint8).reshape(nbuf, extent, 8)
    return out


def extent_of(off, cap, nsec):
    return max([off[o] + cap[o] for o in range(nsec)] + [1]) + 2


def buffer_counts(table, nbuf, seed):
    """raw counters of nbuf buffers that share one section table: buffer 0 has the table's own, the others random ones from 0 to cap + 2
    (so some sections are clamped, some empty)"""
    nsec, off, cap, found = table
    rng = np.random.default_rng(seed)
    out = [list(found[:nsec])]
    for _ in range(1, nbuf):
        out.append([int(rng.integers(0, cap[o] + 3)) for o in range(nsec)])
    return out


def one(total, cap=40):
    return _table(1, [cap], [total])


LOCAL_TABLES = {
    "no section": _table(0, [], [], off=[]),
    "three, found > cap in the first": _table(3, [50, 20, 8], [51, 4, 3]),
    "three, found > cap in the last": _table(3, [50, 20, 8], [6, 4, 4000000000]),
    "one section of 300, 290 stored": _table(1, [300], [290]),
}
ALL_TABLES = {**TABLES, **LOCAL_TABLES}

# ====================================================================================================================== gather_descriptors
GATHER_DESC = [dict(name=f"n={n}", n=n, base_off=0) for n in (0, 1, 7, 8, 9, 257)] + [dict(name="n=9, base 4 mod 16", n=9, base_off=4),
                                                                                       dict(name="n=257, base 12 mod 16", n=257, base_off=12)]

# ====================================================================================================================== shifted_norms
NORM_PATTERNS = ("zeros", "all 128", "all 255", "one byte", "random")


def norm_rows(n, shift, seed=5):
    """row i holds NORM_PATTERNS[(i + shift) % 5]"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    for i in range(n):
        k = (i + shift) % 5
        if k == 0:
            rows[i] = 0
        elif k == 1:
            rows[i] = 128
        elif k == 2:
            rows[i] = 255
        elif k == 3:
            rows[i] = 0
            rows[i, (7 * i) % 128] = 1 + (i % 255)
    return rows


NORMS = [dict(name=f"n={n}, first row {NORM_PATTERNS[s]}", n=n, shift=s) for n, s in ((0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (255, 0), (256, 1), (257, 2))]


# ====================================================================================================================== gather_sections
def sec_case(name, table, *, nbuf=1, buf_ids=None, fixed=False, pad=0, max_rows="exact", fbs=16, desc_extra=0, norm_extra=0, n_stride=1, seed=1):
    """max_rows: "exact" = the largest total of the named buffers. fbs: found_buf_stride. desc_extra: 16-byte units of a cache entry behind
    its rows, norm_extra: words behind its norms (entries are always two rows longer than the payload; the slack must stay poisoned)"""
    table = ALL_TABLES[table] if isinstance(table, str) else table
    nsec = table[0]
    assert fbs >= nsec or fixed
    counts = [list(table[3][:nsec])] * nbuf if fixed else buffer_counts(table, nbuf, seed)
    return dict(name=name, table=table, nbuf=nbuf, buf_ids=list(buf_ids if buf_ids is not None else range(nbuf)), fixed=fixed, pad=pad, max_rows=max_rows,
                fbs=fbs, desc_extra=desc_extra, norm_extra=norm_extra, n_stride=n_stride, counts=counts, seed=seed)


def sec_totals(case):
    nsec, off, cap, _ = case["table"]
    return [len(stored_rows(nsec, off, cap, c)) for c in case["counts"]]


SECTIONS = []
for _name in TABLES:
    SECTIONS.append(sec_case(f"{_name} / found", _name, nbuf=2, pad=2, fbs=TABLES[_name][0] + 1 if (len(SECTIONS) // 2) % 2 else 16, seed=len(SECTIONS)))
    SECTIONS.append(sec_case(f"{_name} / fixed counts", _name, fixed=True, pad=2))
for _t in (0, 1, 2, 7, 9, 31, 33):
    SECTIONS.append(sec_case(f"total {_t}, pad 0", one(_t), pad=0))
    SECTIONS.append(sec_case(f"total {_t}, pad 2", one(_t), pad=2, desc_extra=3, norm_extra=5, n_stride=3))
for _mr in (0, 1, 100000):
    SECTIONS.append(sec_case(f"total 33, max_rows {_mr}", one(33), pad=2, max_rows=_mr))
    SECTIONS.append(sec_case(f"total 0, pad 2, max_rows {_mr}", one(0), pad=2, max_rows=_mr))
    SECTIONS.append(sec_case(f"sixteen sections, max_rows {_mr}", "sixteen sections", pad=2, max_rows=_mr, fbs=17))
SECTIONS += [
    sec_case("no section, pad 0", "no section", pad=0, fbs=1),
    sec_case("no section, pad 2", "no section", pad=2, fbs=1, nbuf=2),
    sec_case("no section, fixed", "no section", pad=2, fixed=True),
    sec_case("identity, 4 buffers", "three sections", nbuf=4, pad=2, desc_extra=1, norm_extra=1, n_stride=2, seed=21),
    sec_case("reversed, 4 buffers", "three sections", nbuf=4, buf_ids=[3, 2, 1, 0], pad=2, desc_extra=2, n_stride=2, seed=22),
    sec_case("sparse {5, 0, 3} of 8", "three, found > cap in the middle", nbuf=8, buf_ids=[5, 0, 3], pad=2, desc_extra=5, norm_extra=7, n_stride=4, seed=23),
    sec_case("a buffer named twice", "three, gaps between the sections", nbuf=3, buf_ids=[2, 0, 2], pad=2, seed=24),
    sec_case("one slot of 8 buffers", "sixteen sections", nbuf=8, buf_ids=[6], pad=2, fbs=17, seed=25),
    # 512 slots get 8 workgroups of 32 rows each: 290 rows need a second sweep of the grid-stride loop. 16 buffers, each named 32 times.
    sec_case("512 slots, second sweep", "one section of 300, 290 stored", nbuf=16, buf_ids=[(7 * i + 3) % 16 for i in range(512)], pad=2, n_stride=2, seed=26),
    sec_case("512 slots, second sweep, max_rows 0", "one section of 300, 290 stored", nbuf=16, buf_ids=[(5 * i + 1) % 16 for i in range(512)], pad=2,
             max_rows=0, fbs=2, seed=27),
]


# ====================================================================================================================== pack_features
def pack_case(name, table, *, nbuf=1, buf_ids=None, out_rows="back to back", max_rows="exact", fbs=16, post=False, seed=1):
    """out_rows: "back to back" | "holes" (three records between consecutive slots) | "non-increasing" (the slots' runs laid out from the back)"""
    table = ALL_TABLES[table] if isinstance(table, str) else table
    assert fbs >= table[0]
    buf_ids = list(buf_ids if buf_ids is not None else range(nbuf))
    assert len(set(buf_ids)) == len(buf_ids)
    c = dict(name=name, table=table, nbuf=nbuf, buf_ids=buf_ids, max_rows=max_rows, fbs=fbs, post=post, counts=buffer_counts(table, nbuf, seed), seed=seed,
             mode=out_rows)
    totals = [sec_totals(c)[b] for b in buf_ids]
    gap = 3 if out_rows == "holes" else 0
    starts = [int(v) for v in np.cumsum([0] + [t + gap for t in totals[:-1]])]
    if out_rows == "non-increasing":
        order = list(range(len(buf_ids)))[::-1]
        pos, starts = 0, [0] * len(buf_ids)
        for i in order:
            starts[i] = pos
            pos += totals[i]
    c["out_rows"] = starts
    c["out_records"] = sum(totals) + gap * len(totals) + 2
    return c


PACK = []
for _name in ALL_TABLES:
    PACK.append(pack_case(f"{_name}", _name, nbuf=3, out_rows=("back to back", "holes", "non-increasing")[len(PACK) % 3], fbs=16, post=len(PACK) % 2 == 1,
                          seed=40 + len(PACK)))
PACK += [
    pack_case("one slot, max_rows 0", "sixteen sections", max_rows=0),
    pack_case("one slot, max_rows 20 of 290", "one section of 300, 290 stored", max_rows=20),
    pack_case("three slots of 6 buffers, holes, max_rows 3", "three, found > cap in the middle", nbuf=6, buf_ids=[4, 1, 5], out_rows="holes", max_rows=3, seed=61),
    pack_case("64 slots", "three sections", nbuf=64, buf_ids=list(range(63, -1, -1)), out_rows="holes", seed=62),
    pack_case("64 slots, non-increasing, posted", "three, found > cap in the first", nbuf=64, out_rows="non-increasing", post=True, seed=63),
    pack_case("posted, found_buf_stride 1", "one section, found > cap", nbuf=5, buf_ids=[3, 0], fbs=1, post=True, seed=64),
    pack_case("posted, found_buf_stride 16", "sixteen sections", nbuf=4, buf_ids=[2, 1], fbs=16, post=True, seed=65),
    pack_case("posted, found_buf_stride 256", "three sections", nbuf=4, buf_ids=[3, 1, 0], fbs=256, post=True, out_rows="holes", seed=66),
    pack_case("not posted, found_buf_stride 256", "three sections", nbuf=2, fbs=256, seed=67),
]

# ====================================================================================================================== filter_matches
FILTER_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
FILTER_PATTERNS = ("all", "none", "alternating", "one per wave", "thread 1023 of round 0", "thread 0 of round 1", "a third")
REV_REASONS = ("own ratio", "j >= nb", "names another row", "reverse ratio")


def pattern_mask(pattern, na, rng):
    i = np.arange(na)
    return {"all": i >= 0, "none": i < 0, "alternating": i % 2 == 0, "one per wave": i % 64 == 37, "thread 1023 of round 0": i == 1023,
            "thread 0 of round 1": i == 1024, "a third": rng.random(na) < 1 / 3}[pattern]


def _dists(rng, n, below):
    """n (d1, d2) bit pairs, d2 the square root of an integer, d1 / d2 clearly below 0.6 (below) or above 0.9"""
    d2 = np.sqrt(rng.integers(1, 200000, n)).astype(f32)
    u = np.where(below, rng.uniform(0.0, 0.6, n), rng.uniform(0.9, 1.0, n))
    d1 = (d2 * u).astype(f32)
    return d1.view(np.uint32), d2.view(np.uint32)


def filter_slot(na, pattern, rev, seed, *, idx_base=0, nb=None):
    """One slot whose survivors at ratios 0.75 and 0.8 are exactly pattern_mask(pattern). Without rev, idx_b1 is arbitrary. With rev, a
    row that is dropped is dropped for ONE reason, the reasons taking turns (REV_REASONS): its own quotient; an idx_b1 of nb, nb + 1 (the
    reverse table holds, BEHIND its nb rows, two records that name such rows and pass: only the j < nb guard drops them) or 0xFFFFFFFF;
    a reverse record that names the next row; a reverse record that fails its own ratio."""
    rng = np.random.default_rng(seed)
    keep = pattern_mask(pattern, na, rng)
    nb = na + 3 if nb is None else nb
    fwd = np.zeros((na, 5), np.uint32)
    fwd[:, 0] = idx_base + np.arange(na)
    fwd[:, 1] = rng.integers(0, 1 << 32, na, dtype=np.uint64)
    fwd[:, 2] = rng.integers(0, 1 << 32, na, dtype=np.uint64)
    slot = dict(na=na, nb=nb, intent=keep, pattern=pattern, reasons=np.full(na, -1))
    if not rev:
        fwd[:, 3], fwd[:, 4] = _dists(rng, na, keep)
        slot.update(fwd=fwd, rev=None)
        return slot
    reason = np.where(keep, -1, np.arange(na) % 4)
    free = [int(v) for v in rng.permutation(nb)]
    table = np.zeros((nb + 2, 5), np.uint32)
    table[:, 0] = np.arange(nb + 2)
    table[:, 1] = 0xFFFFFFF0           # names no row
    table[:, 2] = rng.integers(0, 1 << 32, nb + 2, dtype=np.uint64)
    table[:, 3], table[:, 4] = _dists(rng, nb + 2, np.ones(nb + 2, bool))
    decoys = [nb, nb + 1]
    for i in range(na):
        r = int(reason[i])
        if r == 1 or not free:
            assert not keep[i], "more survivors than reference rows"
            reason[i] = 1
            if decoys:
                j = decoys.pop(0)
                table[j, 1] = i
            else:
                j = (0xFFFFFFFF, 0x80000000 + i, nb + 2 + i)[i % 3]
            fwd[i, 1] = j
            continue
        j = free.pop()
        fwd[i, 1] = j
        table[j, 1] = i + 1 if r == 2 else i
        if r == 3:
            table[j, 3:5] = np.stack(_dists(rng, 1, np.zeros(1, bool)), 1)[0]
    fwd[:, 3], fwd[:, 4] = _dists(rng, na, reason != 0)
    slot.update(fwd=fwd, rev=table, reasons=reason)
    return slot


def filter_case(name, slots, *, ratio=0.75, n_stride=2, fwd_extra=0, out_extra=0):
    """fwd_extra: records of slack behind the largest table of a slot, out_extra: words of slack behind a slot's output"""
    return dict(name=name, slots=slots, ratio=float(f32(ratio)), n_stride=n_stride, fwd_extra=fwd_extra, out_extra=out_extra)


_bits = lambda v: int(np.array(v, f32).view(np.uint32))
INF, NAN = 0x7F800000, 0x7FC00001
SPECIAL_PAIRS = [
    (0, 0), (_bits(3.0), 0), (0, _bits(3.0)), (INF, INF), (NAN, _bits(2.0)), (_bits(2.0), NAN), (NAN, NAN), (_bits(2.0), INF), (INF, _bits(2.0)),
    (1, 2), (3, 4), (0x007FFFFF, 0x007FFFFF), (5, 0x007FFFFF), (0x00000003, _bits(1e-38)), (_bits(1.0), 1), (1, _bits(1.0)),
    (0x80000000, _bits(3.0)), (_bits(-1.0), _bits(4.0)), (_bits(3.0), _bits(4.0)), (_bits(2.9999998), _bits(4.0)), (0x00600000, 0x00800000),
    (0x005FFFFF, 0x00800000), (0x80000000, 0), (_bits(1.0), 0x80000000),
]


def special_slot(rev):
    """every pair of SPECIAL_PAIRS as a forward record; with rev every forward record passes plainly and its reverse record carries the pair"""
    n = len(SPECIAL_PAIRS)
    rng = np.random.default_rng(3)
    pairs = np.array(SPECIAL_PAIRS, np.uint32)
    fwd = np.zeros((n, 5), np.uint32)
    fwd[:, 0] = np.arange(n)
    fwd[:, 1] = rng.permutation(n)
    fwd[:, 3:5] = pairs
    table = None
    if rev:
        fwd[:, 3], fwd[:, 4] = _dists(rng, n, np.ones(n, bool))
        table = np.zeros((n + 2, 5), np.uint32)
        table[:, 1] = 0xFFFFFFF0
        table[fwd[:, 1], 1] = np.arange(n)
        table[fwd[:, 1], 3:5] = pairs
    return dict(na=n, nb=n, fwd=fwd, rev=table, intent=None, pattern=None, reasons=np.full(n, -1))


def small_nb_slot(nb):
    """N_B of 0 or 1: five forward records that pass, idx_b1 = 0, 1, nb, 0, 0xFFFFFFFF; reverse rows 0 and 1 name rows 0 and 1 and pass"""
    rng = np.random.default_rng(9)
    fwd = np.zeros((5, 5), np.uint32)
    fwd[:, 0] = np.arange(5)
    fwd[:, 1] = [0, 1, nb, 0, 0xFFFFFFFF]
    fwd[:, 3], fwd[:, 4] = _dists(rng, 5, np.ones(5, bool))
    table = np.zeros((3, 5), np.uint32)
    table[:, 1] = [0, 1, 2]
    table[:, 3], table[:, 4] = _dists(rng, 3, np.ones(3, bool))
    return dict(na=5, nb=nb, fwd=fwd, rev=table, intent=np.array([nb >= 1, False, False, False, False]), pattern=None, reasons=np.full(5, -1))


def _alt_mul(d1, d2, r):
    """d1 < fl32(ratio * d2): a comparison a rewrite might put in the division's place"""
    return d1 < (f32(r) * d2).astype(f32)


def _alt_rcp(d1, d2, r):
    """fl32(d1 * fl32(1 / d2)) < ratio: the other one"""
    return (d1 * (f32(1) / d2).astype(f32)).astype(f32) < f32(r)


def boundary_pairs():
    """(d1, d2, ratio, kind) with ratio = fl32(d1 / d2) or the float above it, on which an alternative comparison decides differently from
    the division: the first pair found of each (alternative, side)"""
    rng = np.random.default_rng(7)
    d2 = np.sqrt(rng.integers(1, 200000, 20000)).astype(f32)
    d1 = (d2 * rng.uniform(0.5, 0.95, 20000)).astype(f32)
    q = (d1 / d2).astype(f32)
    qn = np.nextafter(q, f32(np.inf))
    out = []
    for alt, fn in (("mul", _alt_mul), ("rcp", _alt_rcp)):
        for side, r, div_keeps in (("at", q, False), ("above", qn, True)):
            dis = fn(d1, d2, r) != div_keeps
            if dis.any():
                k = int(np.flatnonzero(dis)[0])
                out.append((d1[k], d2[k], r[k], f"{alt} {side}"))
    return out


BOUNDARY = boundary_pairs()


def boundary_slot(rev):
    n = len(BOUNDARY)
    rng = np.random.default_rng(4)
    fwd = np.zeros((n, 5), np.uint32)
    fwd[:, 0] = np.arange(n)
    fwd[:, 1] = np.arange(n)[::-1]
    fwd[:, 3] = np.array([p[0] for p in BOUNDARY], f32).view(np.uint32)
    fwd[:, 4] = np.array([p[1] for p in BOUNDARY], f32).view(np.uint32)
    table = None
    if rev:   # the reverse record of row i carries pair i, the forward record passes plainly
        table = np.zeros((n + 2, 5), np.uint32)
        table[:, 1] = 0xFFFFFFF0
        table[:, 3], table[:, 4] = _dists(rng, n + 2, np.ones(n + 2, bool))
        table[fwd[:, 1], 1] = np.arange(n)
        table[fwd[:, 1], 3:5] = fwd[:, 3:5]
        fwd[:, 3], fwd[:, 4] = _dists(rng, n, np.ones(n, bool))
    return dict(na=n, nb=n, fwd=fwd, rev=table, intent=None, pattern=None, reasons=np.full(n, -1))


FILTER = []
for _rev in (False, True):
    _r = "rev" if _rev else "no rev"
    for _na in FILTER_SIZES:
        FILTER.append(filter_case(f"N_A {_na}, a third, {_r}", [filter_slot(_na, "a third", _rev, 100 + _na)], ratio=0.8 if _na % 2 else 0.75))
    for _p in FILTER_PATTERNS:
        FILTER.append(filter_case(f"{_p}, three slots, {_r}", [filter_slot(na, _p, _rev, 200 + na, idx_base=1000 * k) for k, na in enumerate((2049, 1025, 1024))],
                                  n_stride=5 if _rev else 2, fwd_extra=2, out_extra=4))
    FILTER.append(filter_case(f"70 slots, {_r}", [filter_slot(FILTER_SIZES[k % 9], FILTER_PATTERNS[(k // 9 + k) % 7], _rev, 300 + k, idx_base=7 * k) for k in range(70)],
                              n_stride=2 if _rev else 5, fwd_extra=1, out_extra=8, ratio=0.8))
    FILTER.append(filter_case(f"special distances, {_r}", [special_slot(_rev)]))
    for _d1, _d2, _ratio, _kind in BOUNDARY:
        FILTER.append(filter_case(f"ratio boundary ({_kind}), {_r}", [boundary_slot(_rev)], ratio=_ratio))
FILTER += [filter_case(f"N_B {nb}", [small_nb_slot(nb)]) for nb in (0, 1)]
FILTER.append(filter_case("N_B 0 beside N_B 1 and an ordinary slot", [small_nb_slot(0), small_nb_slot(1), filter_slot(65, "alternating", True, 77)], n_stride=5))


# ====================================================================================================================== correspondences, xy
def world(layout_names, buf_tables, *, fbs=16, seed=1, dense_extent=300):
    """layouts: the section tables a slot may name; buffer b holds the raw counters of table buf_tables[b] (found_buf_stride words of them:
    a stride below 16 cuts the list, and a buffer's next counter is then its neighbour's first)"""
    layouts = [ALL_TABLES[n][:3] for n in layout_names]
    founds = [list(ALL_TABLES[n][3][:fbs]) + [JUNK_COUNTER] * max(0, fbs - MAX_SECTIONS) for n in buf_tables]
    extent = max([extent_of(off, cap, nsec) for nsec, off, cap in layouts] + [dense_extent + 2])
    return dict(layouts=layouts, layout_names=list(layout_names), founds=founds, fbs=fbs, extent=extent, seed=seed, nbuf=len(buf_tables))


def world_layout_words(w):
    out = []
    for nsec, off, cap in w["layouts"]:
        out += [nsec] + list(off) + list(cap)
    return np.array(out, np.uint32)


def world_found_words(w):
    return np.array([v for f in w["founds"] for v in f], np.uint32)


def side_rows(w, buf, word):
    """stored rows of buffer `buf` named with layout word `word`"""
    return NR.layout_rows(word, world_layout_words(w), world_found_words(w)[buf * w["fbs"]:], w["fbs"])


def corr_case(name, w, slots, max_n, *, extra=0, seed=1):
    """slots: (buffer A, buffer B, layout word A, layout word B, filtered_n). The filtered table of a slot has max_n + 3 records with rows below
    the totals; where the count allows, record 0 names row total_A of A (B present), record 1 row total_B of B (A present), record 2 row
    0xFFFFFFFF of A, record 3 a missing row on both sides, record 4 row total_A - 1 / total_B - 1 (the last ones present)."""
    rng = np.random.default_rng(seed)
    out = []
    for ba, bb, wa, wb, fn in slots:
        ta, tb = len(side_rows(w, ba, wa)), len(side_rows(w, bb, wb))
        f = np.zeros((max_n + 3, 4), np.uint32)
        f[:, 0] = rng.integers(0, max(ta, 1), max_n + 3)
        f[:, 1] = rng.integers(0, max(tb, 1), max_n + 3)
        f[:, 2:] = rng.integers(0, 1 << 32, (max_n + 3, 2), dtype=np.uint64)
        special = [(ta, f[0, 1]), (f[1, 0], tb), (0xFFFFFFFF, f[2, 1]), (ta + 5, 0xFFFFFFFF), (max(ta, 1) - 1, max(tb, 1) - 1)]
        for k, (a, b) in enumerate(special[:len(f)]):
            f[k, 0], f[k, 1] = a, b
        out.append(dict(buf=(ba, bb), word=(wa, wb), filtered=f, filtered_n=fn, totals=(ta, tb)))
    return dict(name=name, world=w, slots=out, max_n=max_n, extra=extra)


def xy_case(name, w, slots, max_n, *, extra=0):
    """slots: (buffer A, buffer B, layout word A, layout word B); extra: float2 of a side behind max_n (xy_side_stride = max_n + extra)"""
    return dict(name=name, world=w, slots=[dict(buf=(a, b), word=(wa, wb), totals=(len(side_rows(w, a, wa)), len(side_rows(w, b, wb)))) for a, b, wa, wb in slots],
                max_n=max_n, extra=extra)


_NAMES = ["three sections", "three, found > cap in the middle", "three, an empty section between two others", "sixteen sections",
          "three, gaps between the sections", "sixteen, every one clamped", "one section, empty", "three, found > cap in the last"]
W_SECTIONS = world(_NAMES, _NAMES, seed=11)                         # buffer b holds the counters of table b
W_SHORT = world(_NAMES, _NAMES, fbs=5, seed=12)                     # found_buf_stride 5 < nsec 16: sections 5 .. 15 of tables 3 and 5 count as empty
W_STRIDE2 = world(_NAMES[:3], _NAMES[:3], fbs=2, seed=13)           # ... and 2 < 3
_D = lambda n: DENSE | n

_SLOTS_SECTIONS = [(0, 1, 0, 1), (0, 3, 4, 3), (2, 0, 2, 0), (5, 4, 5, 4), (3, 7, 3, 7), (6, 2, 6, 2)]   # slots 0, 1, 2 share buffer 0: layouts 0 and 4
_SLOTS_DENSE = [(0, 1, _D(120), 1), (3, 1, 3, _D(300)), (2, 5, _D(7), _D(1)), (4, 0, _D(0), 0), (1, 2, _D(0), _D(0)), (2, 2, _D(257), 2)]
CORR = [
    corr_case("sections, six slots", W_SECTIONS, [s + (n,) for s, n in zip(_SLOTS_SECTIONS, (0, 1, 255, 256, 257, 300))], 260, seed=1),
    corr_case("sections, counts above max_n", W_SECTIONS, [s + (n,) for s, n in zip(_SLOTS_SECTIONS, (9, 8, 7, 1000, 0xFFFFFFFF, 6))], 7, extra=2, seed=2),
    corr_case("dense layouts", W_SECTIONS, [s + (n,) for s, n in zip(_SLOTS_DENSE, (5, 257, 40, 7, 7, 256))], 257, extra=1, seed=3),
    corr_case("found_buf_stride 5 below nsec 16", W_SHORT, [s + (n,) for s, n in zip(_SLOTS_SECTIONS, (30, 257, 12, 40, 40, 5))], 257, seed=4),
    corr_case("found_buf_stride 2 below nsec 3", W_STRIDE2, [(0, 1, 0, 1, 40), (2, 0, 2, _D(3), 9)], 64, seed=5),
    corr_case("one slot", W_SECTIONS, [(3, 4, 3, 4, 255)], 255, seed=6),
    corr_case("one slot, nothing filtered", W_SECTIONS, [(3, 4, 3, 4, 0)], 16, seed=7),
]
XY = [
    xy_case("sections, five slots, max_n above most totals", W_SECTIONS, _SLOTS_SECTIONS[:5], 300, extra=3),
    xy_case("sections, five slots, max_n 54 = the total of a side", W_SECTIONS, _SLOTS_SECTIONS[:5], 54),
    xy_case("sections, five slots, max_n 14", W_SECTIONS, _SLOTS_SECTIONS[1:], 14, extra=1),
    xy_case("dense layouts, five slots", W_SECTIONS, _SLOTS_DENSE[:5], 257, extra=2),
    xy_case("dense layouts, max_n 256", W_SECTIONS, _SLOTS_DENSE[1:], 256),
    xy_case("found_buf_stride 5 below nsec 16", W_SHORT, _SLOTS_SECTIONS[:5], 600, extra=3),
    xy_case("found_buf_stride 2 below nsec 3", W_STRIDE2, [(0, 1, 0, 1)], 64, extra=3),
    xy_case("one slot, sixteen sections, 1003 rows", W_SECTIONS, [(3, 5, 3, 5)], 1100, extra=5),
    xy_case("one slot, max_n 1", W_SECTIONS, [(3, 5, 3, 5)], 1),
]

# ====================================================================================================================== refusals
# (launch, a case of that launch, the arguments changed): every one must return hipErrorInvalidValue and leave the arena as it was.
# "+name": bytes added to a pointer argument.
REFUSALS = [
    ("gather_sections", "identity, 4 buffers", {"nslots": 0}),
    ("gather_sections", "identity, 4 buffers", {"nslots": 513}),
    ("gather_sections", "identity, 4 buffers", {"nsec": 17}),
    ("gather_sections", "identity, 4 buffers", {"+feats_base": 2}),      # the alignment refusals are new with these tests
    ("gather_sections", "identity, 4 buffers", {"+buf_stride": 2}),
    ("gather_sections", "identity, 4 buffers", {"+desc": 4}),
    ("gather_sections", "identity, 4 buffers", {"+desc": 8}),
    ("gather_sections", "identity, 4 buffers", {"+desc_stride": 4}),
    ("gather_sections", "identity, 4 buffers", {"+desc_stride": 8}),
    ("pack_features", "three sections", {"nslots": 0}),
    ("pack_features", "three sections", {"nslots": 65}),
    ("pack_features", "three sections", {"nsec": 17}),
    ("pack_features", "posted, found_buf_stride 256", {"found_buf_stride": 257}),
    ("pack_features", "three sections", {"+feats_base": 1}),
    ("pack_features", "three sections", {"+buf_stride": 2}),
    ("pack_features", "three sections", {"+out": 2}),
    ("filter_matches", "all, three slots, rev", {"nslots": 0}),
    ("filter_matches", "all, three slots, rev", {"+fwd": 2}),
    ("filter_matches", "all, three slots, rev", {"+fwd_slot_stride": 2}),
    ("filter_matches", "all, three slots, rev", {"+rev": 1}),
    ("filter_matches", "all, three slots, rev", {"+rev_slot_stride": 2}),
    ("filter_matches", "all, three slots, rev", {"+out": 2}),
    ("filter_matches", "all, three slots, rev", {"+out_slot_stride": 2}),
    ("gather_correspondences", "sections, six slots", {"nslots": 0}),
    ("gather_correspondences", "sections, six slots", {"+filtered_slot_stride": 2}),
    ("gather_correspondences", "sections, six slots", {"+corr_slot_stride": 8}),
    ("gather_correspondences", "sections, six slots", {"+corr": 8}),
    ("gather_xy", "sections, five slots, max_n 14", {"nslots": 0}),
    ("gather_xy", "sections, five slots, max_n 14", {"xy_side_stride": 13}),
    ("gather_xy", "sections, five slots, max_n 14", {"+xy": 4}),
]
CASES = {"gather_descriptors": GATHER_DESC, "shifted_norms": NORMS, "gather_sections": SECTIONS, "pack_features": PACK, "filter_matches": FILTER,
         "gather_correspondences": CORR, "gather_xy": XY}


def case_named(launch, name):
    (c,) = [c for c in CASES[launch] if c["name"] == name]
    return c


for _launch, _cases in CASES.items():
    assert len({c["name"] for c in _cases}) == len(_cases), f"{_launch}: case names repeat"
