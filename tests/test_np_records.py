"""Pins, on the CPU, the reference and the case table that tests/test_gpu_record_launchers.py holds the record-moving kernels to:

  * tests/np_records.py against the CPU oracle (orc_filter_matches, orc_match_2nn on FEATURE_DTYPE records) and against int64 arithmetic
  * every case of tests/record_cases.py laid out by tests/hip_records.py on the CPU: the expected arena changes output blocks only
  * test_cases_cover_the_domain: the table really holds every edge the kernels can go wrong at, and for each of the five steps whose
    removal must be noticed — the j < nb guard, the zero fill below pad_rows_to, the per-buffer output addressing, the carry between
    1024-row rounds, the one-sided NaN — a case whose EXPECTED BYTES differ from what the kernel without that step would write
No GPU, nothing sampled: every case is compared in full."""
import numpy as np
import pytest

import hip_records as HR
import np_records as NR
import record_cases as RC
from test_section_walk import stored_rows

f32 = np.float32
POISON = 0xA5


def ordinary(slot):
    """distances a CPU filter written with plain float division handles like the GPU: finite, positive, normal"""
    d = np.concatenate([slot["fwd"][:, 3:5].reshape(-1)] + ([slot["rev"][:, 3:5].reshape(-1)] if slot["rev"] is not None else [])).view(f32)
    return bool(np.all(np.isfinite(d) & (d >= f32(1.2e-38))))


# ====================================================================================================================== the reference
@pytest.mark.parametrize("case", RC.FILTER, ids=lambda c: c["name"])
def test_filter_against_the_oracle(oracle, case):
    n_ordinary = 0
    for s in case["slots"]:
        kept = NR.filter_matches(s["fwd"], s["rev"], s["nb"], case["ratio"])
        assert np.array_equal(kept[:, 2:], s["fwd"][np.isin(s["fwd"][:, 0], kept[:, 0])][:, 3:5])   # the distances travel with their record
        assert np.all(np.diff(kept[:, 0].astype(np.int64)) > 0)
        if s["intent"] is not None:
            assert np.array_equal(np.isin(np.arange(s["na"]), kept[:, 0].astype(np.int64) - int(s["fwd"][0, 0]) if s["na"] else []), s["intent"])
        if not ordinary(s):
            continue
        n_ordinary += 1
        m12 = np.ascontiguousarray(s["fwd"]).view(oracle.MATCH_DTYPE).reshape(-1)
        if s["rev"] is None:
            a, b = oracle.filter_matches(m12, None, ratio=case["ratio"], cross_check=False)
        else:
            m21 = np.ascontiguousarray(s["rev"][:s["nb"]]).view(oracle.MATCH_DTYPE).reshape(-1)
            a, b = oracle.filter_matches(m12, m21, ratio=case["ratio"], cross_check=True)
        assert np.array_equal(a, kept[:, 0]) and np.array_equal(b, kept[:, 1])
    assert n_ordinary or "special" in case["name"]


def test_patterns_hold_at_both_ratios():
    """a pattern slot keeps exactly its pattern at 0.75 and at 0.8"""
    for rev in (False, True):
        for p in RC.FILTER_PATTERNS:
            s = RC.filter_slot(1025, p, rev, 5)
            for ratio in (0.75, 0.8):
                assert np.array_equal(np.isin(np.arange(1025), NR.filter_matches(s["fwd"], s["rev"], s["nb"], ratio)[:, 0]), s["intent"])


def test_gather_against_feature_records(oracle):
    """the dense rows, the packed records and the coordinates are the fields of FEATURE_DTYPE records; matching the dense rows is matching
    the records"""
    nsec, off, cap, found = RC.ALL_TABLES["three, found > cap in the middle"]
    bufs = RC.buffer_bytes(2, RC.extent_of(off, cap, nsec), 3)
    recs = [np.ascontiguousarray(b).reshape(-1).view(oracle.FEATURE_DTYPE) for b in bufs]
    rows = stored_rows(nsec, off, cap, found)
    dense = []
    for b in range(2):
        d, norms, total = NR.gather_sections(bufs[b], nsec, off, cap, found, 2)
        assert total == len(rows) == 31 + 20 + 3 and np.array_equal(d, recs[b][rows]["descriptor"])
        assert norms.dtype == np.uint32 and [int(v) for v in norms] == [sum((int(x) - 128) ** 2 for x in row) for row in d]
        packed = NR.pack_features(bufs[b], nsec, off, cap, found)
        assert packed.tobytes() == recs[b][rows].tobytes()   # (bytes: the random fields hold NaNs)
        xy = NR.gather_xy(bufs[b], rows, 1 << 20).view(f32)
        assert np.array_equal(xy[:, 0], recs[b][rows]["x"]) and np.array_equal(xy[:, 1], recs[b][rows]["y"])
        assert np.array_equal(NR.gather_descriptors(bufs[b], 9), recs[b][:9]["descriptor"])
        dense.append(d)
    m_rows = oracle.match_2nn(dense[0], dense[1])
    m_recs = oracle.match_2nn(np.ascontiguousarray(recs[0][rows]), np.ascontiguousarray(recs[1][rows]))
    assert np.array_equal(m_rows.view(np.uint8), m_recs.view(np.uint8))


def test_norms_in_int64():
    """the kernels form sum b^2 - 256 sum b + 128^3 in uint32: the same number as sum (b - 128)^2, which never leaves 32 bits"""
    rows = RC.norm_rows(257, 0)
    want = NR.shifted_norms(rows)
    b = rows.astype(np.int64)
    assert np.array_equal((b * b).sum(1) - 256 * b.sum(1) + 128 ** 3, want)
    assert want.min() == 0 and want.max() == NR.ZERO_ROW_NORM < 2 ** 32 and int(want[2]) == 128 * 127 ** 2
    assert [int(v) for v in want[:4]] == [128 ** 3, 0, 128 * 127 ** 2, 128 ** 3 - 128 ** 2 + (128 - 4) ** 2]


def test_layout_rows():
    """the decode of a layout word: dense, a table, and sections at or beyond found_buf_stride"""
    w = RC.W_SHORT
    assert np.array_equal(NR.layout_rows(RC.DENSE | 5, RC.world_layout_words(w), [], 5), np.arange(5))
    nsec, off, cap, found = RC.ALL_TABLES["sixteen sections"]
    assert np.array_equal(RC.side_rows(RC.W_SECTIONS, 3, 3), stored_rows(16, off, cap, found))
    assert np.array_equal(RC.side_rows(w, 3, 3), stored_rows(5, off, cap, found))
    assert 0 < len(RC.side_rows(w, 3, 3)) < len(RC.side_rows(RC.W_SECTIONS, 3, 3))


# ====================================================================================================================== the harness, on the CPU
ALL = [(launch, c) for launch, cases in RC.CASES.items() for c in cases]


@pytest.fixture(scope="module")
def laid_out():
    """every case as hip_records lays it out (on the CPU) with its expected arena, built once"""
    out = {}
    for launch, c in ALL:
        h = HR.LAUNCHES[launch](c, device="cpu")
        out[launch, c["name"]] = (h, h.expected())
    return out


def test_expected_arenas_change_outputs_only(laid_out):
    """guards, inputs, gaps: the contract leaves them alone; the base pointers have the alignment the header asks for"""
    outputs = {"dense rows", "norms", "cache rows", "cache norms", "cache n", "packed records", "found_post", "filtered records", "filtered counts",
               "correspondences", "coordinates"}
    for (launch, name), (h, exp) in laid_out.items():
        changed = np.flatnonzero(exp != h.host)
        inside = np.zeros(len(exp), bool)
        for blk in h.blocks:
            is_out = blk.name in outputs and not (launch == "shifted_norms" and blk.name == "dense rows") and \
                not (launch == "gather_correspondences" and blk.name in ("filtered records", "filtered counts"))
            if is_out:
                inside[blk.off:blk.off + len(blk.payload)] = True
                assert np.all(h.view(h.host, blk) == POISON), (launch, name, blk.name)
        assert inside[changed].all(), (launch, name)
        assert h.read().tobytes() == h.host.tobytes()
        for k, v in h.args.items():
            if k in ("desc", "corr") and launch != "gather_descriptors":
                assert v % 16 == 0
            if k == "xy":
                assert v % 8 == 0


def _exp_block(laid_out, launch, name, attr, dtype=np.uint8):
    h, exp = laid_out[launch, name]
    return h, h.view(exp, getattr(h, attr), dtype)


def test_cases_cover_the_domain(laid_out):
    """each edge the issue of these tests names is in the table"""
    # ---- gather_descriptors, shifted_norms
    assert {c["n"] for c in RC.GATHER_DESC} >= {0, 1, 7, 8, 9, 257}
    assert any(c["base_off"] % 16 and c["base_off"] % 4 == 0 for c in RC.GATHER_DESC)
    h, _ = laid_out["gather_descriptors", "n=9, base 4 mod 16"]
    assert h.args["feats"] % 16 == 4
    assert {c["n"] for c in RC.NORMS} >= {0, 1, 255, 256, 257}
    assert {c["shift"] for c in RC.NORMS if c["n"] == 1} == set(range(5))

    # ---- gather_sections
    S = RC.SECTIONS
    tot = lambda c: [RC.sec_totals(c)[b] for b in c["buf_ids"]]
    for name in RC.TABLES:
        assert any(c["table"] is RC.TABLES[name] and c["fixed"] for c in S) and any(c["table"] is RC.TABLES[name] and not c["fixed"] for c in S)
    assert {tot(c)[0] for c in S if len(c["buf_ids"]) == 1} >= {0, 1, 2, 7, 9, 31, 33}
    sweep = [c for c in S if len(c["buf_ids"]) == 512]
    assert sweep and all(max(tot(c)) > 256 and 4096 // 512 == 8 for c in sweep)        # 8 workgroups x 32 rows < the rows of a buffer
    assert any(c["pad"] == 0 for c in S)
    assert any(c["pad"] == 2 and tot(c) == [0] for c in S) and any(c["pad"] == 2 and tot(c) == [1] for c in S) and any(c["pad"] == 2 and min(tot(c)) >= 2 for c in S)
    assert {c["max_rows"] for c in S} >= {"exact", 0, 1, 100000}
    assert any(c["max_rows"] == 0 and max(tot(c)) > 32 for c in S)                     # one workgroup: a second sweep at 33 rows
    assert any(c["buf_ids"] == list(range(c["nbuf"])) and c["nbuf"] > 1 for c in S)
    assert any(c["buf_ids"] == list(range(c["nbuf"]))[::-1] and c["nbuf"] > 1 for c in S)
    assert any(c["buf_ids"] == [5, 0, 3] and c["nbuf"] == 8 for c in S)
    assert any(len(set(c["buf_ids"])) < len(c["buf_ids"]) <= 3 for c in S)
    assert any(c["desc_extra"] and c["norm_extra"] and c["n_stride"] > 1 for c in S)
    assert {len(c["buf_ids"]) for c in S} >= {1, 2, 512}
    assert {c["table"][0] for c in S} >= {0, 16}
    assert any(c["fbs"] == 16 for c in S) and any(c["fbs"] == c["table"][0] + 1 and not c["fixed"] for c in S)
    # the zero fill: rows [total, 2) of the expected cache entry are zeros with norm 128^3, over the poison
    h, rows = _exp_block(laid_out, "gather_sections", "total 1, pad 2", "desc")
    _, norms = _exp_block(laid_out, "gather_sections", "total 1, pad 2", "norms", np.uint32)
    assert not rows[128:256].any() and norms[1] == 128 ** 3 and rows[256] == POISON
    h, rows = _exp_block(laid_out, "gather_sections", "total 0, pad 2, max_rows 0", "desc")
    assert not rows[:256].any() and rows[256] == POISON
    # per-buffer addressing: slots 0, 1, 2 name buffers 5, 0, 3 — entries 1 and 2, which per-slot addressing would fill, stay poisoned,
    # entries 5 and 3 are written, and entry 0 holds buffer 0's rows, not buffer 5's
    h, rows = _exp_block(laid_out, "gather_sections", "sparse {5, 0, 3} of 8", "desc")
    _, n = _exp_block(laid_out, "gather_sections", "sparse {5, 0, 3} of 8", "n", np.uint32)
    st, ns = h.desc_stride, h.case["n_stride"]
    assert all((rows[b * st:(b + 1) * st] == POISON).all() and n[b * ns] == 0xA5A5A5A5 for b in (1, 2, 4, 6, 7))
    assert all(n[b * ns] == h.totals[b] for b in (5, 0, 3)) and len({h.totals[b] for b in (5, 0, 3)}) == 3
    assert np.array_equal(rows[:128], NR.descriptors(h.bufs[0])[0]) and not np.array_equal(rows[:128], NR.descriptors(h.bufs[5])[0])
    # max_rows does not reach the bytes: the cases that differ in max_rows alone expect the same cache entries
    for stem in ("total 33", "total 0, pad 2", "sixteen sections"):
        a, b, c = (laid_out["gather_sections", f"{stem}, max_rows {m}"] for m in (0, 1, 100000))
        assert a[1].tobytes() == b[1].tobytes() == c[1].tobytes()

    # ---- pack_features
    P = RC.PACK
    clamped = lambda c, o: any(cnt[o] > c["table"][2][o] for cnt in (c["counts"][b] for b in c["buf_ids"]))
    assert any(c["table"][0] == 3 and clamped(c, 0) for c in P) and any(c["table"][0] == 3 and clamped(c, 1) for c in P)
    assert any(c["table"][0] == 3 and clamped(c, 2) for c in P)
    assert {c["mode"] for c in P} == {"back to back", "holes", "non-increasing"}
    assert any(c["mode"] == "non-increasing" and len(c["buf_ids"]) > 1 and all(np.diff(c["out_rows"]) <= 0) and c["out_rows"][0] > 0 for c in P)
    assert {len(c["buf_ids"]) for c in P} >= {1, 3, 64}
    ptot = lambda c: [RC.sec_totals(c)[b] for b in c["buf_ids"]]
    assert any(c["max_rows"] == 0 and max(ptot(c)) * 41 > 256 for c in P)
    assert any(c["max_rows"] not in (0, "exact") and c["max_rows"] * 41 + 1023 < max(ptot(c)) * 41 for c in P)
    assert any((t * 41) % 256 for c in P for t in ptot(c))
    assert {c["fbs"] for c in P if c["post"]} >= {1, 16, 256} and any(not c["post"] for c in P)
    h, recs = _exp_block(laid_out, "pack_features", "three slots of 6 buffers, holes, max_rows 3", "out")
    t0 = ptot(h.case)[0]
    assert t0 > 0 and (recs[t0 * 164:(t0 + 3) * 164] == POISON).all() and (recs[(t0 + 3) * 164:(t0 + 4) * 164] != POISON).any()   # a hole between two runs
    h, post = _exp_block(laid_out, "pack_features", "posted, found_buf_stride 256", "post", np.uint32)
    named = set(h.case["buf_ids"])
    for b in range(h.case["nbuf"]):
        assert (post[b * 256:(b + 1) * 256] == 0xA5A5A5A5).all() == (b not in named)
    assert list(post[3 * 256:3 * 256 + 4]) == h.case["counts"][3] + [RC.JUNK_COUNTER]

    # ---- filter_matches
    F = RC.FILTER
    slots = [(c, s) for c in F for s in c["slots"]]
    for rev in (False, True):
        mine = [(c, s) for c, s in slots if (s["rev"] is not None) == rev]
        assert {s["na"] for _, s in mine} >= set(RC.FILTER_SIZES)
        assert {s["pattern"] for _, s in mine if s["na"] >= 1025} >= set(RC.FILTER_PATTERNS)
    assert {len(c["slots"]) for c in F} >= {1, 3, 70} and {c["n_stride"] for c in F} == {2, 5}
    assert any(len({s["na"] for s in c["slots"]}) > 1 for c in F) and any(c["fwd_extra"] and c["out_extra"] for c in F)
    assert any(s["na"] and s["fwd"][0, 0] != 0 for _, s in slots)
    assert {c["ratio"] for c in F} >= {float(f32(0.75)), float(f32(0.8))}
    # a round boundary with the only survivor on either side
    for p, i in (("thread 1023 of round 0", 1023), ("thread 0 of round 1", 1024)):
        for rev in (False, True):
            s = RC.filter_slot(2049, p, rev, 1)
            assert list(NR.filter_matches(s["fwd"], s["rev"], s["nb"], 0.75)[:, 0]) == [i]
    # the carry: survivors in rounds 0, 1 and 2 of one slot — without it round 1 would overwrite round 0's records from record 0 on
    h, exp = laid_out["filter_matches", "all, three slots, no rev"]
    assert [len(k) for k in h.kept()] == [2049, 1025, 1024]
    # every reason a cross-checked record is dropped for, and the guard: the reverse table holds two decoys BEHIND its nb rows that name
    # their forward rows and pass, so a filter without `j < nb` keeps rows this one drops
    for c, s in slots:
        if s["rev"] is not None and s["pattern"] == "none" and s["na"] >= 63:
            assert set(s["reasons"].tolist()) == {0, 1, 2, 3}
            without_guard = NR.filter_matches(s["fwd"][s["fwd"][:, 1] < len(s["rev"])], s["rev"], len(s["rev"]), c["ratio"])
            assert len(without_guard) == 2 and len(NR.filter_matches(s["fwd"], s["rev"], s["nb"], c["ratio"])) == 0
    assert {s["nb"] for _, s in slots if s["rev"] is not None} >= {0, 1}
    for nb in (0, 1):
        s = RC.small_nb_slot(nb)
        assert len(NR.filter_matches(s["fwd"], s["rev"], nb, 0.75)) == nb and len(NR.filter_matches(s["fwd"], s["rev"], 3, 0.75)) > nb
    # special distances: each class is there and decides as IEEE division does
    got = dict(zip(RC.SPECIAL_PAIRS, NR.quotient_below(*np.array(RC.SPECIAL_PAIRS, np.uint32).T, 0.75)))
    assert not got[0, 0] and not got[RC._bits(3.0), 0] and got[0, RC._bits(3.0)] and not got[RC.INF, RC.INF] and not got[RC.NAN, RC._bits(2.0)]
    assert got[1, 2] and not got[3, 4] and not got[RC._bits(3.0), RC._bits(4.0)] and got[RC._bits(2.9999998), RC._bits(4.0)]
    assert not got[0x00600000, 0x00800000] and got[0x005FFFFF, 0x00800000] and got[RC._bits(2.0), RC.INF]
    # the ratio boundary: at ratio = fl32(d1 / d2) the pair is dropped, one float above it is kept — and on the chosen pairs a product
    # or a reciprocal in the division's place decides differently
    kinds = {k for _, _, _, k in RC.BOUNDARY}
    assert any(k.startswith("mul") for k in kinds) and any(k.startswith("rcp") for k in kinds)
    for d1, d2, r, kind in RC.BOUNDARY:
        bits = (np.array([d1], f32).view(np.uint32), np.array([d2], f32).view(np.uint32))
        q = f32(d1) / f32(d2)
        division = bool(NR.quotient_below(*bits, r)[0])
        assert division == (kind.endswith("above")) and r == (np.nextafter(q, f32(np.inf)) if division else q)
        alt = RC._alt_mul if kind.startswith("mul") else RC._alt_rcp
        assert bool(alt(np.array([d1], f32), np.array([d2], f32), r)[0]) != division
        assert any(c["ratio"] == float(r) and "boundary" in c["name"] for c in F)
    # records at and beyond out_n stay poisoned
    h, exp = laid_out["filter_matches", "alternating, three slots, rev"]
    out = h.view(exp, h.out)
    k0 = len(h.kept()[0])
    assert 0 < k0 < 2049 and (out[16 * k0:h.out_stride] == POISON).all() and (out[:16 * k0] != POISON).any()

    # ---- gather_correspondences
    Cc = RC.CORR
    assert {s["filtered_n"] for c in Cc for s in c["slots"]} >= {0, 1, 255, 256, 257}
    assert any(s["filtered_n"] > c["max_n"] for c in Cc for s in c["slots"]) and {len(c["slots"]) for c in Cc} >= {1, 6}
    words = [(s["word"], s["totals"]) for c in Cc for s in c["slots"]]
    dense = lambda w: bool(w & RC.DENSE)
    assert any(dense(a) and not dense(b) for (a, b), _ in words) and any(dense(b) and not dense(a) for (a, b), _ in words)
    assert any(dense(a) and dense(b) for (a, b), _ in words)
    assert any(dense(a) and (a & 0x7FFFFFFF) == 0 for (a, b), _ in words) and any(dense(a) and (a & 0x7FFFFFFF) > 0 for (a, b), _ in words)
    used = {RC.W_SECTIONS["layout_names"][w] for c in Cc for s in c["slots"] for w in s["word"] if not dense(w)}
    assert used >= {"sixteen sections", "three, found > cap in the middle", "three, an empty section between two others", "three, gaps between the sections"}
    assert any(c["world"]["fbs"] < max(t[0] for t in c["world"]["layouts"]) for c in Cc)
    # two slots share a buffer under different layout entries, and see different rows of it
    c = RC.case_named("gather_correspondences", "sections, six slots")
    s0, s1 = c["slots"][0], c["slots"][1]
    assert s0["buf"][0] == s1["buf"][0] and s0["word"][0] != s1["word"][0] and s0["totals"][0] != s1["totals"][0]
    # the one-sided NaN: records whose A row alone, whose B row alone and whose rows both are missing; idx == total and 0xFFFFFFFF
    h, _ = laid_out["gather_correspondences", "sections, six slots"]
    r = h.rows()[3]
    nan = r == NR.QUIET_NAN
    assert list(nan[0]) == [True, True, False, False] and list(nan[1]) == [False, False, True, True] and list(nan[2]) == [True, True, False, False]
    assert nan[3].all() and not nan[4].any() and not nan[5:].any()
    f = c["slots"][3]["filtered"]
    assert f[0, 0] == c["slots"][3]["totals"][0] and f[1, 1] == c["slots"][3]["totals"][1] and f[2, 0] == 0xFFFFFFFF
    # rows beyond min(filtered_n, max_n) stay poisoned
    h, exp = laid_out["gather_correspondences", "sections, counts above max_n"]
    out = h.view(exp, h.corr)
    assert (out[3 * h.c_stride + 16 * 7:4 * h.c_stride] == POISON).all() and (out[3 * h.c_stride:3 * h.c_stride + 16 * 7] != POISON).any()

    # ---- gather_xy
    X = RC.XY
    sides = [(c["max_n"], t) for c in X for s in c["slots"] for t in s["totals"]]
    assert any(t < m for m, t in sides) and any(t == m > 0 for m, t in sides) and any(t > m for m, t in sides) and any(t == 0 for m, t in sides)
    assert {len(c["slots"]) for c in X} >= {1, 5} and any(c["extra"] for c in X) and any(not c["extra"] for c in X)
    assert any(t > 256 and m > 256 for m, t in sides)                                   # a second pass of the 256-thread loop
    assert any(dense(w) for c in X for s in c["slots"] for w in s["word"]) and any(c["world"]["fbs"] < 16 for c in X)
    h, exp = laid_out["gather_xy", "sections, five slots, max_n above most totals"]
    out = h.view(exp, h.xy)
    t = h.case["slots"][0]["totals"][0]
    assert (out[8 * t:8 * h.side_stride] == POISON).all() and (out[:8 * t] != POISON).any()

    # ---- refusals
    want = {"gather_sections": [{"nslots": 0}, {"nslots": 513}, {"nsec": 17}],
            "pack_features": [{"nslots": 0}, {"nslots": 65}, {"nsec": 17}, {"found_buf_stride": 257}],
            "filter_matches": [{"nslots": 0}],
            "gather_correspondences": [{"nslots": 0}, {"+filtered_slot_stride": 2}, {"+corr_slot_stride": 8}, {"+corr": 8}],
            "gather_xy": [{"nslots": 0}, {"xy_side_stride": 13}, {"+xy": 4}]}
    for launch, changes in want.items():
        for ch in changes:
            assert any(l == launch and c == ch for l, _, c in RC.REFUSALS), (launch, ch)
    for launch, name, ch in RC.REFUSALS:
        h, _ = laid_out[launch, name]
        assert all(k.lstrip("+") in h.args for k in ch)
    h, _ = laid_out["pack_features", "posted, found_buf_stride 256"]
    assert h.args["found_post"] is not None
    h, _ = laid_out["gather_xy", "sections, five slots, max_n 14"]
    assert h.args["max_n"] == 14
