"""The one-launch extraction tail of batches (extract_tail.hip: k_extract_tail, one workgroup per image and octave) against the four launches it
replaces (k_segment_scan, k_cand_list, k_refine_flags, k_cand_emit), which tests/test_gpu_extract_launcher.py holds against the CPU oracle.

Every case calls vksift_hip_extract_keypoints_multi twice on identical poisoned arenas (tests/hip_features.py), with VKSIFT_TUNE_TAIL_FUSED at 1 (the
four launches) and at 2 (the one launch; 3: the same with the 512-thread workgroups of large launches), and requires
  * byte-equal arenas outside seg_off, cand_xy and cand_flag: the record sections (records, and the poison behind the last one), found, cand_n,
    the ballots, every guard zone, the planes
  * that the one launch changed nothing but the record section, the counters, seg_mask and cand_n: seg_off, cand_xy and cand_flag keep their poison
The shapes are the smallest at which the kernel takes each of its paths. Its constants (extract_tail.hip): a workgroup of 1024 threads (512 with
knob value 3) refines one candidate per thread and round, walks the ballots in tiles of 2 segments per thread, and holds 4096 candidates in LDS."""
import numpy as np
import pytest

import extract_planes as EP
import hip_features as HF

pytestmark = pytest.mark.gpu
f32 = np.float32

TUNE_TAIL_FUSED = 13            # VKSIFT_TUNE_TAIL_FUSED of include/vksift_hip.h
ROUND = {2: 1024, 3: 512}       # candidates per refinement round = threads of the workgroup, by knob value
TILE = {2: 2048, 3: 1024}       # segments per tile: TAIL_SPT = 2 per thread
LIST = 4096                     # TAIL_LIST: candidates the LDS list holds


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HF.bind(vk.lib())


def _launch(L, cases, knob, *, cap, cand_cap=None, job_cap=None, ptr=False):
    """the cases as the jobs of one call (same batch) on fresh arenas; returns [(arena, bytes after)]"""
    arenas = [HF.FeatureArena(c.planes, None, None, cap, fp16=c.fp16, scratch=True, cand_cap=cand_cap, feat_gap=3, pitch=c.w + (c.w & 1)) for c in cases]
    jobs = (HF.OctaveJob * len(cases))(*[fa.job(octave_idx=i - 1, cap=job_cap, **c.job_kw()) for i, (fa, c) in enumerate(zip(arenas, cases))])
    try:
        assert L.vksift_hip_tune(TUNE_TAIL_FUSED, knob) == 0
        assert L.vksift_hip_tune(HF.TUNE_REFINE_PTR, 1 if ptr else 0) == 0
        rc = L.vksift_hip_extract_keypoints_multi(jobs, len(cases), cases[0].batch, None, None)
        assert rc == 0, (knob, rc, L.vksift_hip_error_string(rc).decode())
        return [(fa, fa.read()) for fa in arenas]
    finally:
        L.vksift_hip_tune(TUNE_TAIL_FUSED, 0)
        L.vksift_hip_tune(HF.TUNE_REFINE_PTR, 0)


def _payload(fa, blocks):
    m = np.zeros(len(fa.host), bool)
    for blk in blocks:
        m[blk.off:blk.off + len(blk.payload)] = True
    return m


def compare(L, cases, what, *, knob=2, **kw):
    """runs the cases through the four launches and through the one; returns per job (arena, bytes after the one launch)"""
    old = _launch(L, cases, 1, **kw)
    new = _launch(L, cases, knob, **kw)
    for i, ((fo, ao), (fn, an)) in enumerate(zip(old, new)):
        assert np.array_equal(fo.host, fn.host)
        fn.check(an, ao, f"{what}: job {i}, one launch against four", _payload(fn, [fn.seg_off, fn.cand_xy, fn.cand_flag]))
        fn.check(an, fn.host, f"{what}: job {i}, bytes the one launch must leave alone", _payload(fn, [fn.feats, fn.found, fn.seg_mask, fn.cand_n]))
    return new


def counts(fa, after):
    """(found, cand_n) per image"""
    return [fa.found_after(after, b) for b in range(fa.batch)], fa.words(after, fa.cand_n).tolist()


def octaves(fp16, batch=3):
    """S = 3, 160 x 120, 80 x 60 and 40 x 30: widths that are no multiple of 64 (the last segment of a row is partial), largest first"""
    return [EP.noise_case(3, h, w, 11 + w, fp16, batch) for (w, h) in ((160, 120), (80, 60), (40, 30))]


# (a) several octaves, batch 3 · (g) binary16 planes · (h) pointer form
@pytest.mark.parametrize("fp16,ptr", [(False, False), (True, False), (False, True)], ids=["fp32", "fp16", "ptr"])
def test_three_octaves_batch_three(L, fp16, ptr):
    res = compare(L, octaves(fp16), "three octaves", cap=4096, ptr=ptr)
    for fa, after in res:
        found, cand = counts(fa, after)
        assert all(0 < f <= c for f, c in zip(found, cand)) and len(found) == 3
    assert min(counts(*res[0])[1]) > ROUND[2]      # the large octave: more than one round per image


# (b) an image without candidates between two with
def test_constant_image_in_the_batch(L):
    D = EP.noise(3, 60, 80, 5)
    case = EP.Case("noise, constant, noise", [D, np.zeros_like(D), EP.noise(3, 60, 80, 6)])
    (fa, after), = compare(L, [case], "constant image", cap=2048)
    found, cand = counts(fa, after)
    assert found[1] == 0 and cand[1] == 0 and found[0] > 0 and found[2] > 0


# (c) the candidate list overflows: candidates at and beyond cand_cap are dropped
def test_candidate_list_overflow(L):
    case = EP.periodic_case(64, 64)
    ncand = 2 * 31 * 31                              # a maximum and a minimum in every 2 x 2 block of the interior (tests/test_extraction_limits.py)
    (fa, after), = compare(L, [case], "cand_cap 1000", cap=2048, cand_cap=1000)
    found, cand = counts(fa, after)
    assert cand == [ncand] and 0 < found[0] <= 1000   # un-clamped count; only the first cand_cap candidates were refined
    (fa, after), = compare(L, [case], "cand_cap at the count", cap=2048, cand_cap=ncand)
    assert counts(fa, after) == ([ncand], [ncand])


# (d) the record section overflows: found stays un-clamped, cap records are written
def test_record_section_overflow(L):
    case = EP.noise_case(3, 60, 80, 5)
    (fa, after), = compare(L, [case], "cap 5", cap=5)
    assert counts(fa, after)[0][0] > 5
    (fa, after), = compare(L, [case], "cap 5 of 8", cap=8, job_cap=5)
    assert counts(fa, after)[0][0] > 8
    assert (fa.records(after, 0, 8).view(np.uint8).reshape(8, -1)[5:] == HF.POISON_BYTE).all()


# (e) several tiles, several rounds, and a tile with more candidates than the list holds; both workgroup sizes
@pytest.mark.parametrize("knob", [2, 3])
def test_rounds_tiles_and_list_windows(L, knob):
    case = EP.noise_case(3, 192, 256, 3)
    (fa, after), = compare(L, [case], f"256x192 knob {knob}", knob=knob, cap=20000)
    found, cand = counts(fa, after)
    assert fa.nsegs == 3 * 192 * 4 > TILE[knob]
    assert cand[0] > ROUND[knob] and cand[0] > 2 * LIST      # (about one texel in eight: a tile of 1024 segments alone holds more than the list)
    assert 0 < found[0] < 20000
    # the 2x2-periodic stack at 130 x 66: one tile whose 4096 candidates fill the list exactly to its capacity
    per = EP.periodic_case(66, 130)
    (fa, after), = compare(L, [per], f"periodic 130x66 knob {knob}", knob=knob, cap=4200)
    assert counts(fa, after) == ([4096], [4096])


# (f) one scale
def test_one_scale(L):
    case = EP.noise_case(1, 60, 80, 9, False, 2)
    (fa, after), = compare(L, [case], "S = 1", cap=1024)
    assert all(f > 0 for f in counts(fa, after)[0])


# the 512-thread form on the multi-octave call as well
def test_three_octaves_small_workgroups(L):
    compare(L, octaves(False, 2), "three octaves, 512 threads", knob=3, cap=4096)


def test_batch_of_64_takes_the_one_launch_and_detects_the_same(vk):
    """the public API: an instance of batch capacity 64 and 64 frames of 160 x 120 under the built-in rule (the one launch) and with the knob at 1"""
    w, h, n = 160, 120, 64
    cfg = vk.default_config(input_image_max_size=w * h, max_nb_sift_per_buffer=4000)
    cfg.sift_buffer_count = n
    imgs = [vk.gen_synthetic_image(700 + i, w, h) for i in range(n)]
    Lib = vk.lib()
    feats = {}
    try:
        for knob in (1, 0):
            Lib.vksift_hip_tune(TUNE_TAIL_FUSED, knob)
            with vk.Instance(cfg, batch_capacity=n) as inst:
                inst.detectFeaturesBatch(imgs, 0)
                feats[knob] = [inst.downloadFeatures(i) for i in range(n)]
    finally:
        Lib.vksift_hip_tune(TUNE_TAIL_FUSED, 0)
    assert sum(len(f) for f in feats[0]) > n
    for i in range(n):
        assert len(feats[0][i]) == len(feats[1][i]) and feats[0][i].tobytes() == feats[1][i].tobytes(), i
