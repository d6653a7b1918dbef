"""The spatially distributed feature budget through the public API (vksift_ext_keepStrongestFeaturesGrid) against its specification,
tests/np_spread.py. Detection is deterministic, so the state before a selection comes from detecting the same images into a second set of
buffers; every comparison is byte equality on the 164-byte records and the 20-byte 2-NN records. No accessor is preceded by an explicit wait:
each must return the values after the selection on its own."""
import os

import numpy as np
import pytest

import np_spread as NP
import np_strongest as NS

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def raw(feats):
    return np.ascontiguousarray(feats).view(np.uint8).reshape(-1, NS.REC)


def selected(feats, n, w, h, cols, rows):
    return NP.selected_records(raw(feats), n, w, h, cols, rows)


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
    grid = (160, 120, 4, 3)
    with vk.Instance(cfg, batch_capacity=9) as inst:
        inst.detectFeaturesBatch(nine, 0)
        inst.detectFeaturesBatch(nine, 9)
        before = [inst.downloadFeatures(9 + i) for i in range(9)]
        counts = sorted(len(f) for f in before)
        budget = counts[4] // 2 + 1
        assert counts[0] == 0 and counts[1] > 8 and counts[-1] > budget > 12
        inst.keepStrongestFeaturesGrid(0, 9, budget, *grid)
        assert [inst.getFeaturesNumber(i) for i in range(9)] == [min(len(f), budget) for f in before]
        for rounds in range(2):     # the first download of a batch takes the per-section copies, the later ones the packed copy
            for i in range(9):
                assert same(raw(inst.downloadFeatures(i)), selected(before[i], budget, *grid)), (rounds, i)
        for i in range(9):          # the other nine are as they were
            assert same(raw(inst.downloadFeatures(9 + i)), raw(before[i]))
        assert any(not same(selected(f, budget, *grid), NS.selected_records(raw(f), budget)) for f in before)   # (the grid decided something)
        # a second selection with the same arguments, and one with a budget nobody exceeds, change nothing
        inst.keepStrongestFeaturesGrid(0, 9, budget, *grid)
        inst.keepStrongestFeaturesGrid(0, 18, counts[-1], *grid)
        for i in range(9):
            assert same(raw(inst.downloadFeatures(i)), selected(before[i], budget, *grid)) and same(raw(inst.downloadFeatures(9 + i)), raw(before[i]))
        # buffers 9 .. 17 of the untouched detection, a smaller budget and another grid, buffers 3 .. 5 only
        inst.keepStrongestFeaturesGrid(12, 3, 17, 160, 120, 2, 2)
        for i in range(9):
            want = selected(before[i], 17, 160, 120, 2, 2) if 3 <= i < 6 else raw(before[i])
            assert inst.getFeaturesNumber(9 + i) == len(want) and same(raw(inst.downloadFeatures(9 + i)), want)


def test_spread_beats_the_plain_budget_on_coverage(vk, small):
    """4x3 cells, N 60: the result is not the plain budget's, and the weakest cell holds more features than under the plain budget"""
    for img in small:
        h, w = img.shape
        with vk.Instance(vk.default_config(sift_buffer_count=3, input_image_max_size=w * h)) as inst:
            for b in range(3):
                inst.detectFeatures(img, b)
            before = inst.downloadFeatures(2)
            assert len(before) > 60
            inst.keepStrongestFeaturesGrid(0, 1, 60, w, h, 4, 3)
            inst.keepStrongestFeatures(1, 1, 60)
            spread, plain = inst.downloadFeatures(0), inst.downloadFeatures(1)
        assert same(raw(spread), selected(before, 60, w, h, 4, 3)) and same(raw(plain), NS.selected_records(raw(before), 60))
        assert len(spread) == len(plain) == 60
        only_spread = set(map(bytes, raw(spread))) - set(map(bytes, raw(plain)))
        per_cell_spread, per_cell_plain = NP.cell_counts(raw(spread), w, h, 4, 3), NP.cell_counts(raw(plain), w, h, 4, 3)
        print(f"{w}x{h}: {len(before)} features, {len(only_spread)} rows kept by the grid rule only, weakest cell {per_cell_plain.min()} -> {per_cell_spread.min()}")
        assert len(only_spread) > 0
        assert per_cell_spread.min() > per_cell_plain.min()
        q, had = 60 // 12, NP.cell_counts(raw(before), w, h, 4, 3)
        assert (per_cell_spread >= np.minimum(had, q)).all()


def test_single_image_and_the_posted_records(vk, small):
    img = small[1]
    grid = (192, 144, 3, 5)
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=192 * 144)) as inst:
        inst.detectFeatures(img, 0)
        before = inst.downloadFeatures(0)      # a caller that fetches single detections: the next ones post their records
        budget = len(before) // 3
        assert budget > 15
        for _ in range(2):
            inst.detectFeatures(img, 0)
            inst.keepStrongestFeaturesGrid(0, 1, budget, *grid)
            assert inst.getFeaturesNumber(0) == budget
            assert same(raw(inst.downloadFeatures(0)), selected(before, budget, *grid))
        inst.detectFeatures(img, 0)             # and a detection afterwards is a detection
        assert same(raw(inst.downloadFeatures(0)), raw(before))
        inst.keepStrongestFeaturesGrid(0, 1, 1, *grid)
        assert same(raw(inst.downloadFeatures(0)), selected(before, 1, *grid))


def test_plain_deferred_detections_then_the_selection(vk, nine):
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=160 * 120)
    grid = (160, 120, 4, 3)
    with vk.Instance(cfg) as ref:
        before = []
        for k in range(4):
            ref.detectFeatures(nine[k], 0)
            before.append(ref.downloadFeatures(0))
    with vk.Instance(cfg) as inst:
        for rounds in range(2):      # the second run of detect calls is staged from its first call on
            for k in range(4):
                inst.detectFeatures(nine[k], 2 + k)
            inst.keepStrongestFeaturesGrid(2, 4, 40, *grid)
            for k in range(4):
                assert inst.getFeaturesNumber(2 + k) == min(len(before[k]), 40)
                assert same(raw(inst.downloadFeatures(2 + k)), selected(before[k], 40, *grid)), (rounds, k)


def _matches_of_uploads(vk, cfg, fa, fb):
    with vk.Instance(cfg) as inst:
        inst.uploadFeatures(fa, 0)
        inst.uploadFeatures(fb, 1)
        inst.matchFeatures(0, 1)
        return inst.downloadMatches()


def test_matching_after_the_selection_equals_matching_the_uploaded_selection(vk, nine):
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=160 * 120)
    img_a, img_b = nine[1], np.roll(nine[1], (2, 3), axis=(0, 1))
    grid = (160, 120, 4, 3)
    as_feats = lambda r: r.view(vk.FEATURE_DTYPE).reshape(-1)
    with vk.Instance(cfg) as inst:
        for budget, cached in ((60, False), (35, True), (1, True)):
            # first: the selection in front of the instance's first matching (no cache); then with the cache, whose entries the descriptor
            # launch of the detection and then the selection write
            inst.detectFeatures(img_a, 0)
            inst.detectFeatures(img_b, 1)
            inst.keepStrongestFeaturesGrid(0, 2, budget, *grid)
            inst.matchFeatures(0, 1)
            m = inst.downloadMatches()
            fa, fb = inst.downloadFeatures(0), inst.downloadFeatures(1)
            assert len(fa) == len(fb) == budget == len(m)
            want = _matches_of_uploads(vk, cfg, fa, fb)
            assert same(np.ascontiguousarray(m).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (budget, cached)
            # the buffers matched once already, then selected from again: their cache entries are rewritten by the selection alone
            if budget > 24:
                inst.keepStrongestFeaturesGrid(0, 2, 24, *grid)
                inst.matchFeatures(1, 0)
                m = inst.downloadMatches()
                want = _matches_of_uploads(vk, cfg, as_feats(selected(fb, 24, *grid)), as_feats(selected(fa, 24, *grid)))
                assert same(np.ascontiguousarray(m).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (budget, cached)


def test_uploaded_buffers_and_a_mixed_range(vk, small):
    cfg = vk.default_config(sift_buffer_count=6, input_image_max_size=192 * 144)
    grid = (192, 144, 3, 2)     # one frame size for the call, whatever the buffers were detected on
    with vk.Instance(cfg) as inst:
        inst.detectFeatures(small[0], 4)
        inst.detectFeatures(small[1], 5)
        fa, fb = inst.downloadFeatures(4), inst.downloadFeatures(5)
        inst.uploadFeatures(fb, 2)
        inst.keepStrongestFeaturesGrid(2, 1, 50, *grid)
        assert inst.getFeaturesNumber(2) == 50 and same(raw(inst.downloadFeatures(2)), selected(fb, 50, *grid))
        # one call over a 160x120 detection, a 192x144 detection, two uploads of different lengths, one of them below the budget
        inst.detectFeatures(small[0], 0)
        inst.detectFeatures(small[1], 1)
        inst.uploadFeatures(fa, 2)
        inst.uploadFeatures(fb[:30], 3)
        inst.keepStrongestFeaturesGrid(0, 4, 33, *grid)
        for buf, f in ((0, fa), (1, fb), (2, fa), (3, fb[:30])):
            assert inst.getFeaturesNumber(buf) == min(len(f), 33) and same(raw(inst.downloadFeatures(buf)), selected(f, 33, *grid)), buf
        inst.matchFeatures(1, 2)    # a detected buffer against an uploaded one, both selected
        m = inst.downloadMatches()
        want = _matches_of_uploads(vk, cfg, inst.downloadFeatures(1), inst.downloadFeatures(2))
        assert same(np.ascontiguousarray(m).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
        assert same(raw(inst.downloadFeatures(4)), raw(fa)) and same(raw(inst.downloadFeatures(5)), raw(fb))


def test_one_cell_and_fewer_features_than_cells_are_the_plain_budget(vk, small):
    """a twin buffer through vksift_ext_keepStrongestFeatures: the same bytes, records and matcher's view"""
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=192 * 144)
    with vk.Instance(cfg) as inst:
        for budget, cols, rows in ((50, 1, 1), (11, 4, 3), (200, 16, 16), (1, 2, 1)):
            for b in range(4):
                inst.detectFeatures(small[1], b)
            assert inst.getFeaturesNumber(3) > budget
            inst.keepStrongestFeaturesGrid(0, 1, budget, 192, 144, cols, rows)
            inst.keepStrongestFeatures(1, 1, budget)
            assert same(raw(inst.downloadFeatures(0)), raw(inst.downloadFeatures(1))), (budget, cols, rows)
            assert same(raw(inst.downloadFeatures(0)), NS.selected_records(raw(inst.downloadFeatures(3)), budget))
            inst.matchFeatures(0, 2)
            m = inst.downloadMatches()
            inst.matchFeatures(1, 2)
            assert same(np.ascontiguousarray(m).view(np.uint8), np.ascontiguousarray(inst.downloadMatches()).view(np.uint8))


def test_invalid_input_changes_nothing(vk, small):
    cfg = vk.default_config(sift_buffer_count=520, input_image_max_size=160 * 120, max_nb_sift_per_buffer=400)
    bad_input = vk.VKSIFT_INVALID_INPUT_ERROR
    ok = (160, 120, 4, 3)
    with vk.Instance(cfg) as inst:
        inst.detectFeatures(small[0], 0)
        before = inst.downloadFeatures(0)
        assert len(before) > 20
        bad = [(first, count, budget) + ok for first, count, budget in ((0, 0, 10), (520, 1, 10), (519, 2, 10), (0, 521, 10), (4, 0xFFFFFFFF, 10), (0, 513, 10), (0, 1, 0))]
        bad += [(0, 1, 10) + g for g in ((0, 120, 4, 3), (160, 0, 4, 3), (160, 120, 0, 3), (160, 120, 4, 0), (160, 120, 17, 3), (160, 120, 4, 17), (160, 120, 0xFFFFFFFF, 1))]
        for args in bad:
            assert _errors(vk, lambda: inst.keepStrongestFeaturesGrid(*args)) == bad_input, args
            assert inst.getFeaturesNumber(0) == len(before) and same(raw(inst.downloadFeatures(0)), raw(before))
        inst.keepStrongestFeaturesGrid(0, 512, 10, 160, 120, 16, 16)       # the largest range and the largest grid one call takes
        inst.keepStrongestFeaturesGrid(519, 1, 10, 1, 1, 1, 1)
        assert same(raw(inst.downloadFeatures(0)), selected(before, 10, 160, 120, 16, 16)) and inst.getFeaturesNumber(519) == 0


def test_selection_time_needs_profiling(vk, small):
    grid = (160, 120, 4, 3)
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=160 * 120)) as inst:
        inst.detectFeatures(small[0], 0)
        inst.keepStrongestFeaturesGrid(0, 1, 30, *grid)
        assert inst.getKeepStrongestGridTime() == -1.0      # profiling is off
        inst.setProfiling(True)
        assert inst.getKeepStrongestGridTime() == -1.0      # on, but that run was not timed
        inst.keepStrongestFeaturesGrid(0, 1, 20, *grid)
        assert 0.0 < inst.getKeepStrongestGridTime() < 1000.0
        assert inst.getKeepStrongestTime() == -1.0          # the plain budget has not run: its timer is its own
        inst.keepStrongestFeatures(0, 1, 15)
        plain = inst.getKeepStrongestTime()
        assert 0.0 < plain < 1000.0
        inst.keepStrongestFeaturesGrid(0, 1, 13, *grid)
        assert inst.getKeepStrongestTime() == plain and 0.0 < inst.getKeepStrongestGridTime() < 1000.0
        assert inst.getFeaturesNumber(0) == 13
