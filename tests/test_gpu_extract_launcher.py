"""vksift_hip_extract_keypoints, vksift_hip_extract_keypoints_multi and vksift_hip_clear_segment_masks, called directly on hand-built Gaussian
stacks across the domain their contract allows (include/vksift_hip.h) — not only on the blurred images, pitches and octave lists a detection
plans. Expected values: orc_extract_keypoints of the CPU oracle in det math mode on a Pyramid.from_planes octave, compared BYTE FOR BYTE over
the whole poisoned arena of a case (tests/hip_features.py): words 0..8 of the first min(found, cap) records and the un-clamped counter must
equal the oracle's, the scratch blocks may change inside their extents only, and every other byte must come back unchanged.

The planes come from tests/extract_planes.py: exact DoG stacks with peaks on chosen columns, rows and scales, TIES placed across every boundary
the streaming scan moves data over, values around the thresholds, noise and the densest stack there is. tests/test_extract_reference.py
asserts on the CPU what each case reaches (and that every plateau tells `>` from `>=`) before a GPU is asked.
Deterministic; one GPU context; default stream, one synchronisation per launch."""
import ctypes as C

import numpy as np
import pytest

import extract_planes as EP
import hip_features as HF

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HF.bind(vk.lib())


def _ok(L, rc, what):
    assert rc == 0, f"{what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"


class tuned:
    """a knob of vksift_hip_tune for the length of a with block"""

    def __init__(self, L, knob, value):
        self.L, self.knob, self.value = L, knob, value

    def __enter__(self):
        self.old = self.L.vksift_hip_tune_get(self.knob)
        assert self.L.vksift_hip_tune(self.knob, self.value) == 0

    def __exit__(self, *exc):
        self.L.vksift_hip_tune(self.knob, self.old)


def even(n):
    return n + (n & 1)


def arena_for(oracle, case, *, room=5, **geom):
    """(arena, pyramids, un-clamped counts): the section holds `room` records more than the fullest image yields"""
    pyr = case.pyramids(oracle)
    counts = [p.extract_keypoints(0, cap=1)[1] for p in pyr]
    fa = HF.FeatureArena(case.planes, None, None, max(counts) + room, fp16=case.fp16, scratch=True, **geom)
    return fa, pyr, counts


def run(L, oracle, case, what, *, octave_idx=0, cap=None, keep=None, scan_reverse=0, **geom):
    """one vksift_hip_extract_keypoints launch on a fresh arena against the oracle; returns (arena, bytes after, counts)"""
    fa, pyr, counts = arena_for(oracle, case, **geom)
    job = fa.job(octave_idx=octave_idx, cap=cap, scan_reverse=scan_reverse, **case.job_kw())
    _ok(L, L.vksift_hip_extract_keypoints(C.byref(job), fa.batch, None, None), what)
    after = fa.read()
    exp, free, found = fa.expected_extraction(pyr, octave_idx=octave_idx, cap=cap, keep=keep)
    fa.check(after, exp, what, free)
    for b in range(fa.batch):
        assert fa.found_after(after, b) == found[b]
    return fa, after, found


# =================================================================================================================== columns, rows, scales
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_columns_and_segments(L, oracle, fp16):
    """S = 1, w in {3, 4, 64, 65, 66, 127, 128, 129, 130, 193, 258}: keypoints of both signs on columns 1, 2, 62 .. 65, 126 .. 129, w - 3, w - 2;
    plateaus of two across one lane's column pair, two lanes, columns 63/64 and 127/128. The pitch is w itself (fp32: odd ones included)"""
    for w in EP.WIDTHS:
        case = EP.columns_case(w, fp16)
        _, _, found = run(L, oracle, case, f"columns w={w}", pitch=even(w) if fp16 else w)
        assert found[0] == len(case.marks["want"])


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_rows_and_bands(L, oracle, fp16):
    """h in {3, 17, 33, 48, 49} with the 16-row band, h in {257, 300} with VKSIFT_TUNE_SCAN_BAND 0, 32 and 48: keypoints on rows 1, 15 .. 17, 31, 32,
    47 .. 49, h - 2; vertical plateaus across rows 15/16, 31/32 and 47/48"""
    for h in (3, 17, 33, 48, 49):
        case = EP.rows_case(h, fp16)
        _, _, found = run(L, oracle, case, f"rows h={h}", pitch=case.w + 2)
        assert found[0] == len(case.marks["want"])
    for h in (257, 300):
        case = EP.rows_case(h, fp16)
        for band in (0, 32, 48):
            with tuned(L, HF.TUNE_SCAN_BAND, band):
                _, _, found = run(L, oracle, case, f"rows h={h} band={band}", pitch=case.w + 28, scan_reverse=band == 32)
            assert found[0] == len(case.marks["want"]) == 10


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("S", range(1, 14))
def test_every_scale_count(L, oracle, S, fp16):
    """all 26 instantiations of the scan: a keypoint on every scale 1 .. S, a plateau across layers, a record that walked to rs = S + 1 (quirk
    Q1); octave_idx -1 .. 6 and three seed sigmas over the S"""
    case = EP.scales_case(S, fp16)
    octave_idx = (S + 5) % 8 - 1
    fa, after, found = run(L, oracle, case, f"S={S}", octave_idx=octave_idx, pitch=case.w + 4, layer_gap=6, image_major=True, base_offset=2)
    recs = fa.records(after, 0, found[0])
    assert (recs["scale_idx"] == S + 1).any() and (recs["octave_idx"] == octave_idx).all()
    assert {(S + 5) % 8 - 1 for S in range(1, 14)} == set(range(-1, 7))


# =================================================================================================================== values
def test_threshold_tiny_edge_and_constant(L, oracle):
    """|c| exactly at 0.8f * dog_threshold and one ulp either side; dog_threshold 0 with fp32 denormals and binary16 subnormal differences;
    edge_limit = inf; constant stacks (found = 0 over the poison), also as the middle image of a batch; planes without an interior"""
    run(L, oracle, EP.threshold_case(), "threshold")
    for fp16 in (False, True):
        fa, after, found = run(L, oracle, EP.tiny_case(fp16), f"tiny fp16={fp16}", pitch=40)
        assert found[0] == 3
    assert run(L, oracle, EP.edge_case(False), "edge 10")[2] == [1]
    assert run(L, oracle, EP.edge_case(True), "edge inf")[2] == [3]
    for fp16 in (False, True):
        assert run(L, oracle, EP.constant_case(1, fp16), "constant")[2] == [0]
        assert run(L, oracle, EP.constant_case(3, fp16), "constant in the middle", found_img_stride=3)[2] == [2, 0, 2]
    for (w, h) in ((1, 1), (2, 5), (5, 2), (3, 3)):
        flat = EP.Case(f"{w}x{h}", [np.zeros((4, h, w), f32)] * 2)
        assert run(L, oracle, flat, f"plane {w}x{h}")[2] == [0, 0]


# =================================================================================================================== compaction, capacity
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_compaction(L, oracle, fp16):
    """noise, 330 x 300, S = 3: two scan chunks, 70+ refinement chunks; the 2x2-periodic stack at 130 x 66: 16 refinement chunks on 9 workgroup
    rows, so both refinement kernels stride"""
    case = EP.noise_case(3, 300, 330, 5, fp16)
    _, _, found = run(L, oracle, case, "noise 330x300", pitch=384 if fp16 else 331)
    assert found[0] > 10000
    per = EP.periodic_case(66, 130, fp16)
    assert run(L, oracle, per, "periodic 130x66")[2] == [4096]


def test_capacities(L, oracle):
    """cap in {0, 1, found - 1, found, found + 1}; cand_cap exactly the candidate count; cand_cap below it: the first cand_cap candidates in
    raster order are refined and the rest is dropped, records and found are those of the kept candidates"""
    case = EP.moves_case()
    tr = case.traces()
    ncand, nkp = len(tr), sum(t["ok"] for *_, t in tr)
    for cap in (0, 1, nkp - 1, nkp, nkp + 1):
        assert run(L, oracle, case, f"cap={cap}", cap=cap)[2] == [nkp]
    run(L, oracle, case, "cand_cap at the candidate count", cand_cap=ncand)
    for cc in (ncand - 1, 100, 1):
        keep = sum(t["ok"] for *_, t in tr[:cc])
        assert keep < nkp or cc == ncand - 1
        assert run(L, oracle, case, f"cand_cap={cc}", cand_cap=cc, keep=[keep])[2] == [keep]


# =================================================================================================================== layout, batch
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("batch", [1, 2, 3, 8])
def test_layouts_and_batches(L, oracle, batch, fp16):
    """batch 1, 2, 3, 8 (the scan's XCD-contiguous order runs with 8, where the workgroup total is a multiple of 8); pitch w, between w and the
    next multiple of 64, and 128; layer gaps, image gaps, both plane orders, base offsets; feat_gap, found_img_stride, sec_index > 0 with
    neighbouring counters, a cand_img_stride above cand_cap, seg blocks longer than needed; scan_reverse 0 and 1"""
    case = EP.noise_case(2, 24, 70, 40, fp16, batch)
    geoms = [dict(pitch=70), dict(pitch=74, img_gap=38, base_offset=2), dict(pitch=128, layer_gap=12, base_offset=4, image_major=True)]
    if not fp16:
        geoms += [dict(pitch=71, img_gap=3, base_offset=1), dict(pitch=73, layer_gap=5, base_offset=3, image_major=True)]   # odd everything
    for i, g in enumerate(geoms):
        for rev in (0, 1):
            run(L, oracle, case, f"batch {batch} layout {i} reverse {rev}", scan_reverse=rev, octave_idx=i - 1, feat_gap=7, found_img_stride=5, sec_index=2,
                nsec=4, front=[[7, 9, 0, 3]] * batch, cand_cap=1500, cand_img_stride=1601, seg_extra=33, **g)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_pointer_refinement(L, oracle, fp16):
    """VKSIFT_TUNE_REFINE_PTR = 1: k_refine_flags / k_cand_emit in the form that octaves beyond 2 GiB take, on a subset of the cases above;
    the edge test on both sides of its limit; the steps of moves_case leave the same arena bytes as the buffer form does"""
    _, buf_bytes, _ = run(L, oracle, EP.moves_case(fp16), "buf moves")
    with tuned(L, HF.TUNE_REFINE_PTR, 1):
        _, ptr_bytes, _ = run(L, oracle, EP.moves_case(fp16), "ptr moves")
        assert np.array_equal(ptr_bytes, buf_bytes)
        if not fp16:
            assert run(L, oracle, EP.edge_case(False), "ptr edge 10")[2] == [1]
            assert run(L, oracle, EP.edge_case(True), "ptr edge inf")[2] == [3]
        for S in (1, 3, 13):
            run(L, oracle, EP.scales_case(S, fp16), f"ptr S={S}", octave_idx=S % 3 - 1, pitch=116, img_gap=10)
        run(L, oracle, EP.columns_case(130, fp16), "ptr columns", pitch=130)
        run(L, oracle, EP.rows_case(49, fp16), "ptr rows")
        run(L, oracle, EP.noise_case(2, 24, 70, 40, fp16, 3), "ptr batch 3", pitch=72, layer_gap=8, image_major=True, base_offset=2)
        run(L, oracle, EP.periodic_case(66, 130, fp16), "ptr periodic")
        run(L, oracle, EP.moves_case(fp16), "ptr cap", cap=7)
        if not fp16:
            run(L, oracle, EP.threshold_case(), "ptr threshold")
        run(L, oracle, EP.tiny_case(fp16), "ptr tiny")


# =================================================================================================================== multi-octave calls
def _multi(L, oracle, cases, what, batch=1, shared_masks=None):
    """the cases as the jobs of ONE vksift_hip_extract_keypoints_multi call, against the oracle and against one single call per job"""
    multi = [arena_for(oracle, c, feat_gap=3, pitch=even(c.w)) for c in cases]
    single = [arena_for(oracle, c, feat_gap=3, pitch=even(c.w)) for c in cases]
    jobs = (HF.OctaveJob * len(cases))(*[fa.job(octave_idx=i % 8 - 1, **c.job_kw()) for i, ((fa, _, _), c) in enumerate(zip(multi, cases))])
    _ok(L, L.vksift_hip_extract_keypoints_multi(jobs, len(cases), batch, None, None), what)
    for i, (((fm, pyr, _), (fs, _, _)), c) in enumerate(zip(zip(multi, single), cases)):
        j = fs.job(octave_idx=i % 8 - 1, **c.job_kw())
        _ok(L, L.vksift_hip_extract_keypoints(C.byref(j), batch, None, None), what)
        am, as_ = fm.read(), fs.read()
        exp, free, _ = fm.expected_extraction(pyr, octave_idx=i % 8 - 1)
        fm.check(am, exp, f"{what}: job {i} ({c.name})", free)
        fs.check(as_, am, f"{what}: single call of job {i} against the multi call", free)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_multi_octave_calls(L, oracle, fp16):
    """jobs of different sizes in one call; 9 jobs (cut 8 + 1); mixed S (cut into runs); VKSIFT_TUNE_MULTI_MAX 1 and 3"""
    nine = [EP.columns_case(w, fp16) for w in (258, 193, 130, 129, 128, 66, 65, 4, 3)]
    _multi(L, oracle, nine[:3] + [EP.rows_case(300, fp16)], "four sizes")
    _multi(L, oracle, nine, "nine jobs")
    mixed = [EP.scales_case(2, fp16), EP.scales_case(2, fp16), EP.columns_case(130, fp16), EP.scales_case(13, fp16), EP.moves_case(fp16), EP.rows_case(33, fp16)]
    assert [c.S for c in mixed] == [2, 2, 1, 13, 2, 1]
    _multi(L, oracle, mixed, "mixed S")
    for mm in (1, 3):
        with tuned(L, HF.TUNE_MULTI_MAX, mm):
            _multi(L, oracle, nine[2:7] + mixed[:2], f"MULTI_MAX={mm}")


@pytest.mark.parametrize("adjacent", [True, False], ids=["adjacent", "apart"])
def test_clear_segment_masks_then_launch(L, oracle, adjacent):
    """vksift_hip_clear_segment_masks + a launch with masks_cleared = 1, for two jobs whose mask regions follow each other in one block (one fill)
    and for two whose regions lie 19 words apart (two fills: the words between them stay poison)"""
    a, b = EP.moves_case(), EP.columns_case(130, False)
    fb, pyr_b, _ = arena_for(oracle, b, pitch=131)
    gap = 0 if adjacent else 19
    fa, pyr_a, _ = arena_for(oracle, a, seg_extra=gap + fb.nsegs)
    ja, jb = fa.job(masks_cleared=1, **a.job_kw()), fb.job(masks_cleared=1, **b.job_kw())
    lo = fa.nsegs + gap                                       # job b's regions inside job a's seg blocks (its own stay untouched poison)
    jb.seg_mask, jb.seg_off = fa.seg_mask.ptr + 8 * lo, fa.seg_off.ptr + 4 * lo
    jobs = (HF.OctaveJob * 2)(ja, jb)
    _ok(L, L.vksift_hip_clear_segment_masks(jobs, 2, 1, None), "clear")
    after = fa.read()
    exp = fa.host.copy()
    for r0, r1 in ((0, fa.nsegs), (lo, lo + fb.nsegs)):
        exp[fa.seg_mask.off + 8 * r0:fa.seg_mask.off + 8 * r1] = 0
    fa.check(after, exp, "after the clear: the two mask regions are zero and nothing else changed")
    fb.check(fb.read(), fb.host, "after the clear: the other arena")
    _ok(L, L.vksift_hip_extract_keypoints_multi(jobs, 2, 1, None, None), "launch")
    exp_a, free_a, _ = fa.expected_extraction(pyr_a, seg_free=[(lo, lo + fb.nsegs)])
    fa.check(fa.read(), exp_a, "job a", free_a)
    exp_b, free_b, _ = fb.expected_extraction(pyr_b)
    free_b[fb.seg_mask.off:fb.seg_mask.off + len(fb.seg_mask.payload)] = False      # its own seg blocks were not named: poison
    free_b[fb.seg_off.off:fb.seg_off.off + len(fb.seg_off.payload)] = False
    fb.check(fb.read(), exp_b, "job b", free_b)


def test_many_scan_chunks(L, oracle):
    """S = 13, 129 x 13600: 130 scan chunks; keypoints in chunk 0, in chunk 66 and in chunk 129 (k_cand_list sums the chunk totals in front of a
    segment 64 at a time)"""
    case = EP.many_chunks_case()
    assert run(L, oracle, case, "many chunks", pitch=129)[2] == [6]


# =================================================================================================================== refusals
def test_refusals_launch_nothing(L, oracle):
    """everything the contract excludes: hipErrorInvalidValue, and not a byte of the poisoned arena changes. Nothing excluded is launched."""
    for fp16 in (False, True):
        case = EP.noise_case(2, 24, 70, 40, fp16, 2)
        fa, _, _ = arena_for(oracle, case, pitch=72, img_gap=4)
        good = fa.job(**case.job_kw())

        def refused(what, n_jobs=1, **fields):
            jobs = (HF.OctaveJob * 2)(fa.job(**case.job_kw()), fa.job(**case.job_kw()))
            for k, v in fields.items():
                setattr(jobs[n_jobs - 1], k, v)
            for name, rc in (("extract", L.vksift_hip_extract_keypoints_multi(jobs, n_jobs, 2, None, None)),
                             ("clear", L.vksift_hip_clear_segment_masks(jobs, n_jobs, 2, None))):
                assert rc == HF.HIP_ERROR_INVALID_VALUE, (what, name, rc)
            fa.check(fa.read(), fa.host, f"{what}: refused, yet the arena changed")

        es = 2 if fp16 else 4
        refused("w 16384", w=16384, pitch=16384)
        refused("h 16384", h=16384)
        refused("w 0", w=0)
        refused("h 0", h=0)
        refused("S 0", S=0)
        refused("S 14", S=14)
        refused("seg_img_stride above", seg_img_stride=good.seg_img_stride + 1)
        refused("seg_img_stride below", seg_img_stride=good.seg_img_stride - 1)
        refused("cand_cap below the chunk count", cand_cap=0)
        refused("cand_img_stride below cand_cap", cand_img_stride=good.cand_cap - 1)
        refused("pitch below w", pitch=68)
        refused("plane_stride below pitch * h", plane_stride=72 * 24 - 2)
        refused("a plane of 2 GiB", pitch=(1 << 31) // es // 24 + 24, plane_stride=1 << 32)
        refused("gauss not 4-byte aligned", gauss=good.gauss + 2)
        refused("the second job of a call", n_jobs=2, S=14)            # the first job is not launched either
        if fp16:
            refused("odd pitch", pitch=73)
            refused("odd plane_stride", plane_stride=good.plane_stride + 1)
            refused("odd img_stride", img_stride=good.img_stride + 1)
        else:
            refused("gauss not 4-byte aligned (1)", gauss=good.gauss + 1)
        _ok(L, L.vksift_hip_extract_keypoints(C.byref(good), 2, None, None), "the unchanged job")   # ... and the job they were derived from is served
        exp, free, _ = fa.expected_extraction(case.pyramids(oracle))
        fa.check(fa.read(), exp, "the unchanged job", free)
