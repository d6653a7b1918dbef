"""What the cases of tests/test_gpu_extract_launcher.py reach, asserted on the CPU (the oracle, numpy): every GPU case is known to hit its target
before a GPU is asked, and every plateau case is known to tell the 26 STRICT comparisons from `>=`.

  * the builders of tests/extract_planes.py: the DoG stack comes back bit for bit from the Gaussian layers (gauss_from_dog asserts it for every
    case built here), in fp32 and through the binary16 rounding
  * the numpy restatement of the stage (candidates / refine_trace) accepts exactly the oracle's keypoints, with the oracle's scale_x, scale_y
    and intensity bits — so its reports of where a candidate walks and which clamp it meets are about the oracle's own computation
  * plateaus: tests/np_features.py::extract_keypoints with strict=False (a tie passes) yields a DIFFERENT record set than the oracle on every
    plateau case, i.e. the refinement accepts the tied texels; a plateau it rejected either way would test nothing
  * the arena of tests/hip_features.py on the host: layout of the scratch blocks, expected_extraction, and that check() sees a stray byte"""
import numpy as np
import pytest

import extract_planes as EP
import hip_features as HF
import np_features as NF

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _agree(oracle, case, b=0):
    """the restatement against the oracle: same keypoints in the same order, same bits; returns (traces, records)"""
    tr = case.traces(b)
    recs, n = case.oracle_records(oracle, b)
    acc = [t for *_, t in tr if t["ok"]]
    assert len(acc) == n == len(recs), (case.name, len(acc), n)
    assert np.array_equal(_bits([t["sx"] for t in acc]), _bits(recs["scale_x"])) and np.array_equal(_bits([t["sy"] for t in acc]), _bits(recs["scale_y"]))
    assert np.array_equal(_bits([t["nv"] for t in acc]), _bits(recs["intensity"]))
    return tr, recs


def _nonstrict_differs(oracle, case, n_plateaus):
    """the wrong comparison yields more records than the oracle: at least one per plateau"""
    recs, n = case.oracle_records(oracle)
    dog = case.dogs[0]
    strict = NF.extract_keypoints(dog, case.S, 0, case.seed_sigma, case.it, case.et)
    loose = NF.extract_keypoints(dog, case.S, 0, case.seed_sigma, case.it, case.et, strict=False)
    key = lambda r: sorted((int(k["scale_idx"]), round(float(k["scale_y"]), 3), round(float(k["scale_x"]), 3)) for k in r)
    assert key(strict) == key(recs), case.name                       # the restatement in its right form is the oracle
    assert len(loose) >= n + n_plateaus and key(loose) != key(recs), (case.name, len(loose), n)
    # ... and it is the plateau texels that make the difference: none of them is a candidate of the strict test, all are of the loose one
    cs = {(y, x) for s, y, x in EP.candidates(dog, case.S, case.thr)}
    cl = {(y, x) for s, y, x, t in case.traces(0, strict=False) if t["ok"]}
    for (x, y) in case.marks["plateaus"]:
        assert (y, x) not in cs and (y, x) in cl, (case.name, x, y)


# =================================================================================================================== builders
def test_builders_are_exact_and_refuse_what_is_not():
    D = np.zeros((3, 9, 9), f32)
    EP.bump(D, 4, 4, 1, 1)
    for fp16 in (False, True):
        G = EP.gauss_from_dog(D, fp16=fp16)
        assert G.shape == (4, 9, 9) and np.array_equal(_bits(G[2] - G[1]), _bits(D[1])) and G[0].min() != G[0].max()
    with pytest.raises(AssertionError):
        EP.gauss_from_dog(D * f32(1.0 / 3), fp16=True)                # not binary16 values
    with pytest.raises(AssertionError):
        EP.gauss_from_dog(D + f32(2.0 ** -30))                        # 2^-30 is lost beside a base of 2^-5: the stack does not come back
    with pytest.raises(AssertionError):
        EP.bump(D, 5, 5, 1, -1)                                       # overlapping peaks
    assert D[1, 4, 4] == 64 * EP.Q and D[1, 4, 5] == 56 * EP.Q and D[0, 4, 4] == 48 * EP.Q and D[1, 4, 7] == 0
    E = np.zeros((4, 9, 9), f32)
    EP.bump(E, 3, 4, 1, -1, plateau=(1, 1, 0))
    assert E[1, 4, 3] == E[1, 5, 4] == -64 * EP.Q and (E[1] >= -64 * EP.Q).all()
    p = EP.periodic(1, 8, 8)
    assert len(EP.candidates(p, 1, 0.04)) == 2 * 3 * 3                # the bound of tests/test_extraction_limits.py for 8 x 8
    assert np.array_equal(EP.noise(2, 5, 7, 3), EP.noise(2, 5, 7, 3)) and not np.array_equal(EP.noise(2, 5, 7, 3), EP.noise(2, 5, 7, 4))


def test_octave_scaling_is_exact(oracle):
    """expected_extraction scales the oracle's octave-0 records by 2^octave_idx; for octave -1 the oracle can say so itself"""
    case = EP.moves_case()
    r0, n0 = case.oracle_records(oracle)
    rm, nm = case.pyramids(oracle, use_input_upsampling=1)[0].extract_keypoints(0, cap=1 << 20)
    assert n0 == nm > 100 and (rm["octave_idx"] == -1).all()
    for name in ("x", "y", "sigma"):
        assert np.array_equal(_bits(r0[name] * f32(0.5)), _bits(rm[name])), name
    for name in ("scale_x", "scale_y", "intensity"):
        assert np.array_equal(_bits(r0[name]), _bits(rm[name])), name


# =================================================================================================================== columns, rows, scales
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_columns_cases(oracle, fp16):
    seen, plateau_kinds = set(), set()
    for w in EP.WIDTHS:
        case = EP.columns_case(w, fp16)
        tr, recs = _agree(oracle, case)
        got = [(s, y, x) for s, y, x, t in tr if t["ok"]]
        assert sorted(got) == sorted(case.marks["want"]), w         # exactly the placed peaks, and each on its own column
        cols = {x for _, _, x in got}
        assert cols == {c for c in EP.COLS + [w - 3, w - 2] if 1 <= c <= w - 2}
        assert {float(np.sign(v)) for v in recs["intensity"]} == ({1.0, -1.0} if w > 3 else {1.0})
        seen |= cols
        if case.marks["plateaus"]:
            _nonstrict_differs(oracle, case, len(case.marks["plateaus"]))
            plateau_kinds |= {x for x, _ in case.marks["plateaus"]}
    assert seen >= set(EP.COLS) and plateau_kinds == {10, 21, 63, 127}   # one lane's pair, two lanes, the two segments of a wave, the two halos
    assert 10 % 2 == 0 and 21 % 2 == 1


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_rows_cases(oracle, fp16):
    seen, edges = set(), set()
    for h in (3, 17, 33, 48, 49, 257, 300):
        case = EP.rows_case(h, fp16)
        tr, recs = _agree(oracle, case)
        got = [(s, y, x) for s, y, x, t in tr if t["ok"]]
        assert sorted(got) == sorted(case.marks["want"]), h
        rows = {y for _, y, _ in got}
        assert rows == {r for r in EP.ROWS + [h - 2] if 1 <= r <= h - 2}
        seen |= rows
        if case.marks["plateaus"]:
            _nonstrict_differs(oracle, case, len(case.marks["plateaus"]))
            edges |= {y for _, y in case.marks["plateaus"]}
        bands = -(-h // 16)
        if h in (33, 257, 300):
            assert bands % 4 != 0                                      # a band count that is no multiple of the four waves of a workgroup
    assert seen >= set(EP.ROWS) and edges == {15, 31, 47}             # the plateaus lie across rows 15/16, 31/32, 47/48: band edges of 16, 32, 48 rows
    assert {h for h in (33, 48, 49) if EP.rows_case(h).marks["plateaus"]} == {33, 48, 49}


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("S", range(1, 14))
def test_scales_cases(oracle, S, fp16):
    case = EP.scales_case(S, fp16)
    tr, recs = _agree(oracle, case)
    got = {(s, y, x) for s, y, x, t in tr if t["ok"]}
    assert got >= set(case.marks["want"]) and {s for s, _, _ in case.marks["want"]} == set(range(1, S + 1))   # a keypoint on every scale
    _nonstrict_differs(oracle, case, 2)                               # the two plateaus across layers
    q1 = recs[(recs["scale_idx"] == S + 1)]
    walked = [t for *_, t in tr if t["ok"] and t["rs"] == S + 1 and t["ss"] > S + 0.6]
    assert len(walked) >= 1 and len(q1) >= 1                          # quirk Q1: the refinement read DoG layer S + 2 as 0 and the record was kept
    assert case.planes.shape[1] == S + 3


# =================================================================================================================== values
def test_value_cases(oracle):
    case = EP.threshold_case()
    tr, recs = _agree(oracle, case)
    cand = {(x, y) for s, y, x, t in tr}
    acc = {(x, y) for s, y, x, t in tr if t["ok"]}
    pre = EP.pre_for(case.thr)
    D = case.dogs[0][1]
    for (x, y) in case.marks["at"]:
        assert abs(D[y, x]) == pre and (x, y) not in cand            # |c| == 0.8f * dog_threshold exactly: `>` fails
    for (x, y) in case.marks["above"]:
        assert abs(D[y, x]) == np.nextafter(pre, f32(1)) and (x, y) in acc
    for (x, y) in case.marks["below"]:
        assert abs(D[y, x]) == np.nextafter(pre, f32(0)) and (x, y) not in cand
    assert {float(np.sign(D[y, x])) for x, y in case.marks["above"]} == {1.0, -1.0}
    for fp16 in (False, True):
        case = EP.tiny_case(fp16)
        tr, recs = _agree(oracle, case)
        assert case.thr == 0 and {(x, y) for s, y, x, t in tr if t["ok"]} >= set(case.marks["tiny"])
        tiny = np.sort(np.abs(recs["intensity"]))[:2]
        if fp16:
            assert (tiny < 2.0 ** -14).all() and (tiny > 0).all()    # binary16 subnormals
        else:
            assert (tiny < 2.0 ** -126).all() and (tiny > 0).all()   # fp32 denormals
    finite, infinite = EP.edge_case(False), EP.edge_case(True)
    assert np.isinf(infinite.edge_limit) and infinite.edge_limit > 0 and abs(float(finite.edge_limit) - 12.1) < 1e-5
    assert np.array_equal(finite.planes, infinite.planes)
    a = {(x, y) for s, y, x, t in _agree(oracle, finite)[0] if t["ok"]}
    b = {(x, y) for s, y, x, t in _agree(oracle, infinite)[0] if t["ok"]}
    assert not a & set(finite.marks["ridges"]) and b - a == set(finite.marks["ridges"])
    for batch in (1, 3):
        case = EP.constant_case(batch)
        counts = [case.oracle_records(oracle, b)[1] for b in range(batch)]
        assert counts == ([0] if batch == 1 else [2, 0, 2])


# =================================================================================================================== compaction, capacity
def test_compaction_cases(oracle):
    big = EP.noise_case(3, 300, 330, 5)
    nseg = (330 + 63) // 64
    assert 3 * 300 * nseg > HF.SEG_CHUNK                               # two scan chunks
    ncand = len(EP.candidates(big.dogs[0], 3, big.thr))
    recs, n = big.oracle_records(oracle)
    assert ncand > 40 * HF.CAND_CHUNK and n > 10000                    # dozens of refinement chunks
    assert (recs["scale_idx"] == 4).any()
    per = EP.periodic_case(66, 130)
    tr, recs = _agree(oracle, per)
    assert len(tr) == 2 * 64 * 32 == len(recs)                         # the bound, all accepted
    assert len(tr) // HF.CAND_CHUNK > EP.refine_grid_rows(1, 130, 66)  # 16 chunks on 9 workgroup rows: the stride loops of both refinement kernels run
    small = EP.moves_case()
    tr, recs = _agree(oracle, small)
    assert any(t["moved_x"] for *_, t in tr) and any(t["moved_y"] for *_, t in tr) and any(t["moved_s"] for *_, t in tr)
    clamps = set().union(*[t["clamps"] for *_, t in tr])
    assert clamps & {"x1", "xw", "s1", "y1", "yh"}, clamps
    assert any(t["ok"] and t["rs"] == small.S + 1 and t["ss"] > small.S + 0.6 for *_, t in tr)
    assert len(recs) > 5 and len(tr) > len(recs)                       # cap around found, cand_cap around the candidate count: both exist
    for fp16 in (False, True):
        b8 = EP.noise_case(2, 24, 70, 40, fp16, 8)
        assert all(b8.oracle_records(oracle, b)[1] > 50 for b in range(8))


def test_many_chunks_case(oracle):
    case = EP.many_chunks_case()
    nsegs = case.S * case.h * ((case.w + 63) // 64)
    assert -(-nsegs // HF.SEG_CHUNK) == 130
    recs, n = case.oracle_records(oracle)
    assert n == len(case.marks["want"]) == 6
    chunks = [EP.seg_chunk(case, *k) for k in case.marks["want"]]
    assert chunks[0] == 0 and any(64 < c <= 128 for c in chunks) and any(c > 128 for c in chunks), chunks
    assert [int(round(float(k["scale_y"]))) for k in recs] == [y for _, y, _ in case.marks["want"]]


# =================================================================================================================== the harness on the host
def test_extraction_arena_on_the_host(oracle):
    case = EP.noise_case(2, 24, 70, 40, True, 3)
    pyr = case.pyramids(oracle)
    fa = HF.FeatureArena(case.planes, None, None, 40, fp16=True, device="cpu", scratch=True, pitch=72, img_gap=6, base_offset=2, feat_gap=3,
                         found_img_stride=4, sec_index=1, nsec=3, front=[[5, 0, 9]] * 3, cand_cap=900, cand_img_stride=1000, seg_extra=17)
    job = fa.job(octave_idx=2, **case.job_kw())
    base = fa.arena.dev.data_ptr()
    assert job.seg_img_stride == 2 * 24 * 2 == fa.nsegs and job.cand_cap == 900 and job.cand_img_stride == 1000
    assert job.pitch % 2 == 0 and job.plane_stride % 2 == 0 and job.img_stride % 2 == 0 and job.gauss % 4 == 0   # what the contract asks of binary16
    for blk, es in ((fa.seg_mask, 8), (fa.seg_off, 4)):
        assert len(blk.payload) == es * (fa.nsegs * 3 + 17) and (blk.payload == HF.POISON_BYTE).all()
    assert job.seg_mask - base == fa.seg_mask.off and job.seg_mask % 8 == 0
    assert (fa.words(fa.host, fa.found)[[1, 5, 9]] == HF.POISON_WORD).all() and fa.words(fa.host, fa.found)[[0, 2]].tolist() == [5, 9]
    exp, free, counts = fa.expected_extraction(pyr, octave_idx=2)
    assert all(c > 40 for c in counts)                                   # found above cap: the records are clipped, the counter is not
    for b in range(3):
        assert fa.found_after(exp, b) == counts[b]
        r = fa.records(exp, b)
        assert (r["octave_idx"] == 2).all() and (r["orientation"] == 0).all() and (r["descriptor"] == HF.POISON_BYTE).all()
        ref, _ = pyr[b].extract_keypoints(0, cap=40)
        assert np.array_equal(_bits(r["x"]), _bits(ref["x"] * f32(4))) and np.array_equal(r["scale_idx"], ref["scale_idx"])
    fa.check(exp, exp, "self", free)
    stray = [fa.feats.off + 36, fa.feats.off + 40 * HF.REC, fa.found.off, fa.seg_mask.off + 8 * fa.nsegs * 3, fa.seg_off.off + 4 * fa.nsegs * 3,
             fa.cand_xy.off + 4 * 900, fa.cand_flag.off + 4 * 999, fa.cand_n.off + 12, fa.ori_cnt.off, fa.seg_mask.off - 1]
    for where in stray:
        bad = exp.copy()
        bad[where] ^= 0x40
        with pytest.raises(AssertionError):
            fa.check(bad, exp, "tampered", free)
    for where in (fa.seg_mask.off, fa.seg_off.off + 4 * fa.nsegs * 3 - 1, fa.cand_xy.off + 4 * 1000, fa.cand_flag.off + 4 * 899, fa.cand_n.off + 11):
        ok = exp.copy()
        ok[where] ^= 0x40
        fa.check(ok, exp, "scratch", free)
    # the workgroup totals of the batch cases: gx * gy * batch with one strip pair and one group of four bands for a 70 x 24 plane
    assert [((fa.nseg + 1) // 2) * ((-(-24 // 16) + 3) // 4) * b % 8 == 0 for b in (1, 2, 3, 8)] == [False, False, False, True]
