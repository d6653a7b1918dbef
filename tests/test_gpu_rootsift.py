"""The RootSIFT conversion through the public API (vksift_ext_convertToRootSift) against its specification, tests/np_rootsift.py. Detection is
deterministic, so the state before a conversion comes from detecting the same images into a second set of buffers — the untouched twin; every
comparison is byte equality on the 164-byte records and the 20-byte 2-NN records. No accessor is preceded by an explicit wait: each must return
the values after the conversion on its own."""
import os

import numpy as np
import pytest

import np_match as NM
import np_records as NR
import np_rootsift as RS
import np_strongest as NS

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
u32 = np.uint32


def raw(feats):
    return np.ascontiguousarray(feats).view(np.uint8).reshape(-1, RS.REC)


def root(feats):
    """the records after the conversion"""
    return RS.convert_records(raw(feats))


def rows_of(feats):
    return raw(feats)[:, RS.DESC_AT:]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def words(records):
    return np.ascontiguousarray(records).view(u32).reshape(len(records), -1)


def two_nn(a, b):
    """the 2-NN records of descriptor rows a against b, as the matcher's contract states them (tests/np_match.py)"""
    return NM.match_2nn(a, NM.pad_two(b))


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


def test_batch_of_nine_through_every_download_path(vk, nine):
    cfg = vk.default_config(sift_buffer_count=18, input_image_max_size=160 * 120)
    with vk.Instance(cfg, batch_capacity=9) as inst:
        inst.detectFeaturesBatch(nine, 0)
        inst.detectFeaturesBatch(nine, 9)
        inst.convertToRootSift(0, 9)
        twin = [inst.downloadFeatures(9 + i) for i in range(9)]
        counts = [len(f) for f in twin]
        assert min(counts) == 0 and sorted(counts)[1] > 8        # an empty buffer is fine
        assert [inst.getFeaturesNumber(i) for i in range(9)] == counts
        for rounds in range(2):     # the first download of a batch takes the per-section copies, the later ones the packed copy
            for i in range(9):
                got = raw(inst.downloadFeatures(i))
                assert same(got, root(twin[i])), (rounds, i)
                assert same(got[:, :RS.DESC_AT], raw(twin[i])[:, :RS.DESC_AT])
        assert any((root(f) != raw(f)).any() for f in twin)
        for i in range(9):          # the other nine are as they were
            assert same(raw(inst.downloadFeatures(9 + i)), raw(twin[i]))
        # buffers 9 .. 17 of the untouched detection, buffers 3 .. 5 only; and NOT idempotent: buffers 0 .. 8 a second time
        inst.convertToRootSift(12, 3)
        inst.convertToRootSift(0, 9)
        for i in range(9):
            want = root(twin[i]) if 3 <= i < 6 else raw(twin[i])
            assert inst.getFeaturesNumber(9 + i) == counts[i] and same(raw(inst.downloadFeatures(9 + i)), want), i
            assert same(raw(inst.downloadFeatures(i)), RS.convert_records(root(twin[i]))), i


def test_single_image_and_the_posted_records(vk, small):
    img = small[1]
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=192 * 144)) as inst:
        inst.detectFeatures(img, 0)
        before = inst.downloadFeatures(0)      # a caller that fetches single detections: the next ones post their records
        assert len(before) > 20
        for _ in range(2):
            inst.detectFeatures(img, 0)
            inst.convertToRootSift(0, 1)
            assert inst.getFeaturesNumber(0) == len(before)
            assert same(raw(inst.downloadFeatures(0)), root(before))
        inst.detectFeatures(img, 0)             # and a detection afterwards is a detection
        assert same(raw(inst.downloadFeatures(0)), raw(before))
        inst.convertToRootSift(0, 1)
        assert same(raw(inst.downloadFeatures(0)), root(before))


def test_plain_deferred_detections_then_the_conversion(vk, nine):
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
            inst.convertToRootSift(2, 4)
            for k in range(4):
                assert inst.getFeaturesNumber(2 + k) == len(before[k])
                assert same(raw(inst.downloadFeatures(2 + k)), root(before[k])), (rounds, k)
        assert inst.getDeferredStats()[0] >= 1      # ... and was launched by the conversion, as one batch


def test_matching_after_the_conversion_sees_the_converted_rows(vk, nine):
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=160 * 120)
    img_a, img_b = nine[1], np.roll(nine[1], (2, 3), axis=(0, 1))
    with vk.Instance(cfg) as inst:
        # first the conversion in front of the instance's first matching (no cache: the matching gathers the converted rows itself)
        inst.detectFeatures(img_a, 0)
        inst.detectFeatures(img_b, 1)
        inst.detectFeatures(img_a, 2)
        inst.detectFeatures(img_b, 3)
        inst.convertToRootSift(0, 2)
        inst.matchFeatures(0, 1)
        m = inst.downloadMatches()
        fa, fb = inst.downloadFeatures(2), inst.downloadFeatures(3)
        ra, rb = RS.root_rows(rows_of(fa)), RS.root_rows(rows_of(fb))
        assert len(fa) > 20 and len(fb) > 20 and same(words(m), two_nn(ra, rb))
        assert not same(words(m), two_nn(rows_of(fa), rows_of(fb)))
        # then with the cache: the entries are written by the detection, read by a matching, and rewritten by the conversion alone —
        # a stale entry would give the records of the SIFT rows
        inst.detectFeatures(img_a, 0)
        inst.detectFeatures(img_b, 1)
        inst.matchFeatures(0, 1)
        assert same(words(inst.downloadMatches()), two_nn(rows_of(fa), rows_of(fb)))
        inst.convertToRootSift(0, 2)
        inst.matchFeatures(0, 1)
        assert same(words(inst.downloadMatches()), two_nn(ra, rb))
        inst.matchFeatures(1, 0)
        assert same(words(inst.downloadMatches()), two_nn(rb, ra))
        # the filtered matching: cross-check and ratio over the two directions
        inst.matchFeaturesFiltered([0], [1], ratio=0.8, cross_check=True)
        want = NR.filter_matches(two_nn(ra, rb), two_nn(rb, ra), len(rb), 0.8)
        assert len(want) > 8 and same(words(inst.downloadFilteredMatches(0)), want)
        # a converted buffer against an unconverted one: meaningless, and defined
        inst.matchFeatures(0, 3)
        assert same(words(inst.downloadMatches()), two_nn(ra, rows_of(fb)))


def test_conversion_and_budget_commute(vk, nine):
    cfg = vk.default_config(sift_buffer_count=6, input_image_max_size=160 * 120)
    img_a, img_b = nine[2], np.roll(nine[2], (1, 4), axis=(0, 1))
    with vk.Instance(cfg) as inst:
        for cached in (False, True):     # before the instance's first matching, and with the cache entries following both calls
            for first in (0, 2, 4):
                inst.detectFeatures(img_a, first)
                inst.detectFeatures(img_b, first + 1)
            budget = min(inst.getFeaturesNumber(4), inst.getFeaturesNumber(5)) // 2
            assert budget > 8
            inst.convertToRootSift(0, 2)
            inst.keepStrongestFeatures(0, 2, budget)
            inst.keepStrongestFeatures(2, 2, budget)
            inst.convertToRootSift(2, 2)
            fa, fb = inst.downloadFeatures(4), inst.downloadFeatures(5)
            want_a, want_b = root(NS.selected_records(raw(fa), budget)), root(NS.selected_records(raw(fb), budget))
            for first in (0, 2):
                assert inst.getFeaturesNumber(first) == budget == inst.getFeaturesNumber(first + 1)
                assert same(raw(inst.downloadFeatures(first)), want_a) and same(raw(inst.downloadFeatures(first + 1)), want_b), (cached, first)
            want_m = two_nn(want_a[:, RS.DESC_AT:], want_b[:, RS.DESC_AT:])
            for first in (0, 2):
                inst.matchFeatures(first, first + 1)
                assert same(words(inst.downloadMatches()), want_m), (cached, first)


def test_uploaded_buffers_and_a_mixed_range(vk, small):
    cfg = vk.default_config(sift_buffer_count=6, input_image_max_size=192 * 144)
    with vk.Instance(cfg) as inst:
        inst.detectFeatures(small[0], 4)
        inst.detectFeatures(small[1], 5)
        fa, fb = inst.downloadFeatures(4), inst.downloadFeatures(5)
        inst.uploadFeatures(fb, 2)
        inst.convertToRootSift(2, 1)
        assert inst.getFeaturesNumber(2) == len(fb) and same(raw(inst.downloadFeatures(2)), root(fb))      # still one dense run
        # one call over a 160x120 detection, a 192x144 detection and two uploads of different lengths, one of them empty
        inst.detectFeatures(small[0], 0)
        inst.detectFeatures(small[1], 1)
        inst.uploadFeatures(fa, 2)
        inst.uploadFeatures(fb[:0], 3)
        inst.convertToRootSift(0, 4)
        for buf, f in ((0, fa), (1, fb), (2, fa), (3, fb[:0])):
            assert inst.getFeaturesNumber(buf) == len(f) and same(raw(inst.downloadFeatures(buf)), root(f)), buf
        inst.matchFeatures(1, 2)    # a detected buffer against an uploaded one, both converted
        assert same(words(inst.downloadMatches()), two_nn(RS.root_rows(rows_of(fb)), RS.root_rows(rows_of(fa))))
        assert same(raw(inst.downloadFeatures(4)), raw(fa)) and same(raw(inst.downloadFeatures(5)), raw(fb))
        inst.uploadFeatures(fa, 2)  # an upload afterwards is an upload
        assert same(raw(inst.downloadFeatures(2)), raw(fa))


def test_described_keypoints_keep_their_placed_count(vk, small):
    img = small[1]
    with vk.Instance(vk.default_config(sift_buffer_count=3, input_image_max_size=192 * 144)) as inst:
        inst.detectFeatures(img, 0)
        feats = inst.downloadFeatures(0)
        kps = np.zeros(len(feats), vk.KEYPOINT_DTYPE)
        for name in ("x", "y", "sigma", "orientation"):
            kps[name] = feats[name]
        kps["response"] = feats["intensity"]
        inst.describeKeypoints(img, kps, 1, vk.DESCRIBE_GIVEN)
        inst.describeKeypoints(img, kps, 2, vk.DESCRIBE_GIVEN)
        inst.convertToRootSift(1, 1)
        placed = inst.getPlacedKeypointsNumber(2)
        assert placed > 20 and inst.getPlacedKeypointsNumber(1) == placed      # the count is still true of the converted buffer
        assert same(raw(inst.downloadFeatures(1)), root(inst.downloadFeatures(2)))
        assert inst.getPlacedKeypointsNumber(0) == 0
        inst.convertToRootSift(0, 1)
        assert inst.getPlacedKeypointsNumber(0) == 0                            # ... and a detected buffer has none, before and after
        inst.keepStrongestFeatures(1, 1, placed // 2)
        assert inst.getPlacedKeypointsNumber(1) == 0                            # cut: no longer what the placement left


def test_export_returns_the_converted_rows(vk, small):
    import ctypes as C

    L = vk.lib()     # device memory of the library's own allocator
    L.vksift_hip_malloc.restype = C.c_void_p
    L.vksift_hip_malloc.argtypes = [C.c_size_t]
    L.vksift_hip_free.argtypes = [C.c_void_p]
    L.vksift_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.vksift_hip_stream_sync.argtypes = [C.c_void_p]
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=160 * 120)) as inst:
        inst.detectFeatures(small[0], 0)
        inst.detectFeatures(small[0], 1)
        inst.convertToRootSift(0, 1)
        n = inst.getFeaturesNumber(1)
        assert n > 20
        d = L.vksift_hip_malloc(n * 128)
        assert d
        try:
            assert inst.exportDescriptorsDevice(0, d) == n
            got = np.zeros((n, 128), np.uint8)
            assert L.vksift_hip_memcpy_d2h(got.ctypes.data, d, n * 128, None) == 0 and L.vksift_hip_stream_sync(None) == 0
        finally:
            L.vksift_hip_free(d)
        assert same(got, RS.root_rows(rows_of(inst.downloadFeatures(1))))


def test_invalid_input_changes_nothing(vk, small):
    cfg = vk.default_config(sift_buffer_count=520, input_image_max_size=160 * 120, max_nb_sift_per_buffer=400)
    bad_input = vk.VKSIFT_INVALID_INPUT_ERROR
    with vk.Instance(cfg) as inst:
        inst.detectFeatures(small[0], 0)
        before = inst.downloadFeatures(0)
        assert len(before) > 20
        for first, count in ((0, 0), (520, 1), (519, 2), (0, 521), (4, 0xFFFFFFFF), (0, 513), (0xFFFFFFFF, 1)):
            assert _errors(vk, lambda: inst.convertToRootSift(first, count)) == bad_input, (first, count)
            assert inst.getFeaturesNumber(0) == len(before) and same(raw(inst.downloadFeatures(0)), raw(before))
        inst.convertToRootSift(0, 512)       # the largest range one call takes
        inst.convertToRootSift(519, 1)
        assert same(raw(inst.downloadFeatures(0)), root(before)) and inst.getFeaturesNumber(519) == 0


def test_conversion_time_needs_profiling(vk, small):
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=160 * 120)) as inst:
        inst.detectFeatures(small[0], 0)
        inst.convertToRootSift(0, 1)
        assert inst.getRootSiftTime() == -1.0      # profiling is off
        inst.setProfiling(True)
        assert inst.getRootSiftTime() == -1.0      # on, but that run was not timed
        inst.convertToRootSift(0, 1)
        assert 0.0 < inst.getRootSiftTime() < 1000.0
        assert inst.getKeepStrongestTime() == -1.0  # a timer of its own
