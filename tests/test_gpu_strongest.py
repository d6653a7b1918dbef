"""The feature budget through the public API (vksift_ext_keepStrongestFeatures) against its specification, tests/np_strongest.py. Detection is
deterministic, so the state before a selection comes from detecting the same images into a second set of buffers; every comparison is byte
equality on the 164-byte records and the 20-byte 2-NN records. No accessor is preceded by an explicit wait: each must return the values
after the selection on its own."""
import os

import numpy as np
import pytest

import np_strongest as NS

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def raw(feats):
    return np.ascontiguousarray(feats).view(np.uint8).reshape(-1, NS.REC)


def selected(feats, n):
    return NS.selected_records(raw(feats), n)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def small(vk):
    return np.load(os.path.join(G, "img_160x120.npy")), np.load(os.path.join(G, "img_192x144.npy"))


@pytest.fixture(scope="module")
def nine(vk, small):
    """nine 160x120 images: the fixture, seven synthetic ones, and a flat one without features"""
    return [small[0]] + [vk.gen_synthetic_image(400 + k, 160, 120) for k in range(7)] + [np.full((120, 160), 90, np.uint8)]


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def test_batch_of_nine_through_the_packed_download(vk, nine):
    cfg = vk.default_config(sift_buffer_count=18, input_image_max_size=160 * 120)
    with vk.Instance(cfg, batch_capacity=9) as inst:
        inst.detectFeaturesBatch(nine, 0)
        inst.detectFeaturesBatch(nine, 9)
        before = [inst.downloadFeatures(9 + i) for i in range(9)]
        counts = sorted(len(f) for f in before)
        budget = counts[4] // 2 + 1
        assert counts[0] == 0 and counts[1] > 8 and counts[-1] > budget
        inst.keepStrongestFeatures(0, 9, budget)
        assert [inst.getFeaturesNumber(i) for i in range(9)] == [min(len(f), budget) for f in before]
        for rounds in range(2):     # the first download of a batch takes the per-section copies, the later ones the packed copy
            for i in range(9):
                assert same(raw(inst.downloadFeatures(i)), selected(before[i], budget)), (rounds, i)
        for i in range(9):          # the other nine are as they were
            assert same(raw(inst.downloadFeatures(9 + i)), raw(before[i]))
        # a second selection with the same budget, and one with a budget nobody exceeds, change nothing
        inst.keepStrongestFeatures(0, 9, budget)
        inst.keepStrongestFeatures(0, 18, counts[-1])
        for i in range(9):
            assert same(raw(inst.downloadFeatures(i)), selected(before[i], budget)) and same(raw(inst.downloadFeatures(9 + i)), raw(before[i]))
        # buffers 9 .. 17 of the untouched detection, a smaller budget, buffers 3 .. 5 only
        inst.keepStrongestFeatures(12, 3, 7)
        for i in range(9):
            want = selected(before[i], 7) if 3 <= i < 6 else raw(before[i])
            assert inst.getFeaturesNumber(9 + i) == len(want) and same(raw(inst.downloadFeatures(9 + i)), want)


def test_single_image_and_the_posted_records(vk, small):
    img = small[1]
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=192 * 144)) as inst:
        inst.detectFeatures(img, 0)
        before = inst.downloadFeatures(0)      # a caller that fetches single detections: the next ones post their records
        budget = len(before) // 3
        assert budget > 8
        for _ in range(2):
            inst.detectFeatures(img, 0)
            inst.keepStrongestFeatures(0, 1, budget)
            assert inst.getFeaturesNumber(0) == budget
            assert same(raw(inst.downloadFeatures(0)), selected(before, budget))
        inst.detectFeatures(img, 0)             # and a detection afterwards is a detection
        assert same(raw(inst.downloadFeatures(0)), raw(before))
        inst.keepStrongestFeatures(0, 1, 1)
        assert same(raw(inst.downloadFeatures(0)), selected(before, 1))


def test_plain_deferred_detections_then_the_selection(vk, nine):
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=160 * 120)
    with vk.Instance(cfg) as ref:
        before = []
        for k in range(4):
            ref.detectFeatures(nine[k], 0)
            before.append(ref.downloadFeatures(0))
    with vk.Instance(cfg) as inst:
        for rounds in range(2):      # the second run of detect calls is staged from its first call on
            for k in range(4):
                inst.detectFeatures(nine[k], 2 + k)
            inst.keepStrongestFeatures(2, 4, 40)
            for k in range(4):
                assert inst.getFeaturesNumber(2 + k) == min(len(before[k]), 40)
                assert same(raw(inst.downloadFeatures(2 + k)), selected(before[k], 40)), (rounds, k)


def _matches_of_uploads(vk, cfg, fa, fb):
    with vk.Instance(cfg) as inst:
        inst.uploadFeatures(fa, 0)
        inst.uploadFeatures(fb, 1)
        inst.matchFeatures(0, 1)
        return inst.downloadMatches()


def test_matching_after_the_selection_equals_matching_the_uploaded_selection(vk, nine):
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=160 * 120)
    img_a, img_b = nine[1], np.roll(nine[1], (2, 3), axis=(0, 1))
    with vk.Instance(cfg) as inst:
        for budget, cached in ((60, False), (35, True), (1, True)):
            # first: the selection in front of the instance's first matching (no cache); then with the cache, whose entries the descriptor
            # launch of the detection and then the selection write
            inst.detectFeatures(img_a, 0)
            inst.detectFeatures(img_b, 1)
            inst.keepStrongestFeatures(0, 2, budget)
            inst.matchFeatures(0, 1)
            m = inst.downloadMatches()
            fa, fb = inst.downloadFeatures(0), inst.downloadFeatures(1)
            assert len(fa) == len(fb) == budget == len(m)
            want = _matches_of_uploads(vk, cfg, fa, fb)
            assert same(np.ascontiguousarray(m).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (budget, cached)
            # the buffers matched once already, then selected from again: their cache entries are rewritten by the selection alone
            if budget > 20:
                inst.keepStrongestFeatures(0, 2, 20)
                inst.matchFeatures(1, 0)
                m = inst.downloadMatches()
                want = _matches_of_uploads(vk, cfg, selected(fb, 20).view(vk.FEATURE_DTYPE).reshape(-1), selected(fa, 20).view(vk.FEATURE_DTYPE).reshape(-1))
                assert same(np.ascontiguousarray(m).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (budget, cached)


def test_uploaded_buffers_and_a_mixed_range(vk, small):
    cfg = vk.default_config(sift_buffer_count=6, input_image_max_size=192 * 144)
    with vk.Instance(cfg) as inst:
        inst.detectFeatures(small[0], 4)
        inst.detectFeatures(small[1], 5)
        fa, fb = inst.downloadFeatures(4), inst.downloadFeatures(5)
        inst.uploadFeatures(fb, 2)
        inst.keepStrongestFeatures(2, 1, 50)
        assert inst.getFeaturesNumber(2) == 50 and same(raw(inst.downloadFeatures(2)), selected(fb, 50))
        # one call over a 160x120 detection, a 192x144 detection, two uploads of different lengths, one of them below the budget
        inst.detectFeatures(small[0], 0)
        inst.detectFeatures(small[1], 1)
        inst.uploadFeatures(fa, 2)
        inst.uploadFeatures(fb[:30], 3)
        inst.keepStrongestFeatures(0, 4, 33)
        for buf, f in ((0, fa), (1, fb), (2, fa), (3, fb[:30])):
            assert inst.getFeaturesNumber(buf) == min(len(f), 33) and same(raw(inst.downloadFeatures(buf)), selected(f, 33)), buf
        inst.matchFeatures(1, 2)    # a detected buffer against an uploaded one, both selected
        m = inst.downloadMatches()
        want = _matches_of_uploads(vk, cfg, inst.downloadFeatures(1), inst.downloadFeatures(2))
        assert same(np.ascontiguousarray(m).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
        assert same(raw(inst.downloadFeatures(4)), raw(fa)) and same(raw(inst.downloadFeatures(5)), raw(fb))


def test_invalid_input_changes_nothing(vk, small):
    cfg = vk.default_config(sift_buffer_count=520, input_image_max_size=160 * 120, max_nb_sift_per_buffer=400)
    bad_input = vk.VKSIFT_INVALID_INPUT_ERROR
    with vk.Instance(cfg) as inst:
        inst.detectFeatures(small[0], 0)
        before = inst.downloadFeatures(0)
        assert len(before) > 20
        for first, count, budget in ((0, 0, 10), (520, 1, 10), (519, 2, 10), (0, 521, 10), (4, 0xFFFFFFFF, 10), (0, 513, 10), (0, 1, 0)):
            assert _errors(vk, lambda: inst.keepStrongestFeatures(first, count, budget)) == bad_input, (first, count, budget)
            assert inst.getFeaturesNumber(0) == len(before) and same(raw(inst.downloadFeatures(0)), raw(before))
        inst.keepStrongestFeatures(0, 512, 10)       # the largest range one call takes
        inst.keepStrongestFeatures(519, 1, 10)
        assert same(raw(inst.downloadFeatures(0)), selected(before, 10)) and inst.getFeaturesNumber(519) == 0


def test_selection_time_needs_profiling(vk, small):
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=160 * 120)) as inst:
        inst.detectFeatures(small[0], 0)
        inst.keepStrongestFeatures(0, 1, 10)
        assert inst.getKeepStrongestTime() == -1.0      # profiling is off
        inst.setProfiling(True)
        assert inst.getKeepStrongestTime() == -1.0      # on, but that run was not timed
        inst.keepStrongestFeatures(0, 1, 5)
        assert 0.0 < inst.getKeepStrongestTime() < 1000.0
        assert inst.getFeaturesNumber(0) == 5
