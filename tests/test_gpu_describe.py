"""Caller-supplied keypoints through the public API (vksift_ext_describeKeypoints, vksift_ext_describeKeypointsBatch,
vksift_ext_getPlacedKeypointsNumber) on the two golden images. Every comparison is byte equality on the 164-byte records:

  * round trip: a detection's own features handed back — with their orientations (GIVEN), or as distinct keypoints (ORIENT) — give the
    detection's records for every feature the placement rule takes back (tests/test_np_describe.py: reproducible)
  * restatement: random keypoints over and beyond the scale-space and the borders against tests/np_describe.py (placement, order, counts)
    and tests/np_features.py (orientations, descriptor) on the planes the instance shows, fp32 and binary16
  * a batch equals single calls; the described buffer matches and is budgeted like a detected one; a describe call leaves detections,
    their graphs and the deferral statistics alone; invalid input reports once and changes nothing; an image without an octave."""
import os

import numpy as np
import pytest

import np_describe as ND
import np_features as NF
import np_rootsift as NR
import np_strongest as NS
from test_np_describe import ROUND_TRIP_MIN, SEED_SIGMA, as_keypoints, reproducible

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32, u32 = np.float32, np.uint32
S, MAX_ORI = 3, 4          # the default configuration
BIG = [1 << 30] * 16       # capacities that never bind (max_nb_sift_per_buffer is far above the lists here)


@pytest.fixture(scope="module")
def images(vk):
    return {"192x144": np.load(os.path.join(G, "img_192x144.npy")), "160x120": np.load(os.path.join(G, "img_160x120.npy"))}


def config(vk, img, **kw):
    return vk.default_config(sift_buffer_count=kw.pop("sift_buffer_count", 4), input_image_max_size=img.shape[0] * img.shape[1], **kw)


def octaves(img):
    return ND.octaves_for(img.shape[1], img.shape[0], True)


def stored_order(kps, img, keep, caps=BIG):
    """input indices of the stored keypoints in download order (orientation copies aside), and the placement's counters"""
    octs = octaves(img)
    sections, found, placed, index = ND.place(kps, octs, caps[:len(octs)], ND.sigma_steps(SEED_SIGMA, S), keep)
    return np.concatenate(index) if index else np.zeros(0, np.int64), sections, found, placed


def raw(feats):
    return np.ascontiguousarray(feats).view(np.uint8).reshape(-1, 164)


# ---------------------------------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("name", ["192x144", "160x120"])
def test_given_round_trip(vk, images, name):
    img = images[name]
    with vk.Instance(config(vk, img)) as inst:
        inst.detectFeatures(img, 0)
        feats = inst.downloadFeatures(0)
        kps = as_keypoints(feats)
        inst.describeKeypoints(img, kps, 1, vk.DESCRIBE_GIVEN)
        out = inst.downloadFeatures(1)
        placed = inst.getPlacedKeypointsNumber(1)
    repro, _ = reproducible(feats, img.shape[1], img.shape[0], True, S, True)
    order, _, _, want_placed = stored_order(kps, img, True)
    print(f"{name}: {len(feats)} features, {placed} placed, {int(repro.sum())} reproducible ({100 * repro.mean():.1f} %)")
    assert repro.mean() >= ROUND_TRIP_MIN
    assert placed == want_placed == len(out) == len(order)
    a, b = raw(out), raw(feats)
    bad = [int(i) for k, i in enumerate(order) if repro[i] and a[k].tobytes() != b[i].tobytes()]
    assert not bad, (len(bad), bad[:5])
    # the join key: x, y, sigma and response of every stored record are its keypoint's, bit for bit
    for field, src in (("x", "x"), ("y", "y"), ("sigma", "sigma"), ("intensity", "response")):
        assert np.array_equal(out[field].view(u32), kps[src][order].view(u32))


@pytest.mark.parametrize("name", ["192x144", "160x120"])
def test_orient_round_trip(vk, images, name):
    img = images[name]
    with vk.Instance(config(vk, img)) as inst:
        inst.detectFeatures(img, 0)
        feats = inst.downloadFeatures(0)
        key = lambda f: np.stack([f["x"].view(u32), f["y"].view(u32), f["sigma"].view(u32)], axis=1)
        _, firsts = np.unique(key(feats), axis=0, return_index=True)
        firsts = np.sort(firsts)
        kps = as_keypoints(feats[firsts])
        inst.describeKeypoints(img, kps, 1, vk.DESCRIBE_ORIENT)
        out = inst.downloadFeatures(1)
        placed = inst.getPlacedKeypointsNumber(1)
    repro, _ = reproducible(feats[firsts], img.shape[1], img.shape[0], True, S, False)
    assert repro.mean() >= ROUND_TRIP_MIN and placed == stored_order(kps, img, False)[3]
    groups = lambda f: {k: sorted(r.tobytes() for r in raw(f)[np.all(key(f) == k, axis=1)]) for k in map(tuple, key(f))}
    g_det, g_out = groups(feats), groups(out)
    bad = [i for i in np.flatnonzero(repro) if g_det[tuple(key(feats[firsts])[i])] != g_out.get(tuple(key(feats[firsts])[i]))]
    print(f"{name}: {len(firsts)} distinct keypoints of {len(feats)} features, {int(repro.sum())} reproducible, {len(out)} described features")
    assert not bad, (len(bad), bad[:5])


# ---------------------------------------------------------------------------------------------------------------------- restatement
def random_keypoints(img, n, seed):
    rng = np.random.default_rng(seed)
    h, w = img.shape
    k = np.zeros(n, ND.KEYPOINT_DTYPE)
    k["sigma"] = np.exp(rng.uniform(np.log(0.8), np.log(40.0), n))
    k["x"], k["y"] = rng.uniform(-1.5, w + 1.5, n), rng.uniform(-1.5, h + 1.5, n)
    k["x"][:4], k["y"][:4] = [0.0, w - 0.01, 0.3, w / 2], [0.0, h - 0.01, h - 0.26, 0.1]      # on the borders
    k["orientation"] = rng.uniform(0, float(ND.TWO_PI32), n)
    k["response"] = rng.uniform(-0.2, 0.2, n)
    k["sigma"][5], k["x"][9], k["orientation"][13], k["sigma"][17] = 0.0, np.nan, 6.5, 500.0   # (the orientation only matters when it is kept)
    return k


def restated(inst, kps, img, keep):
    """the records the call must leave, from np_describe and np_features on the planes the instance shows -> (records, placed)"""
    octs = octaves(img)
    _, sections, found, placed = stored_order(kps, img, keep)
    out = []
    for o, words in enumerate(sections):
        planes = {}
        first, extra = [], []
        for wrec in words:
            rec = np.zeros(1, NF.KP_DTYPE)
            rec.view(u32).reshape(-1)[:9] = wrec
            rec = rec[0]
            s = int(rec["scale_idx"])
            if s not in planes:
                planes[s] = inst.downloadScaleSpaceImage(o, s)
            if not keep:
                ang, _ = NF.orientations(planes[s], rec, MAX_ORI)
                rec["orientation"] = ang[0] if len(ang) else f32(0)
                for a in ang[1:]:
                    r2 = rec.copy()
                    r2["orientation"] = a
                    extra.append(r2)
            first.append(rec)
        for rec in first + extra:
            rec["descriptor"], _ = NF.descriptor(planes[int(rec["scale_idx"])], rec, rec["orientation"], False)
            out.append(rec)
    return (np.array(out, NF.KP_DTYPE) if out else np.zeros(0, NF.KP_DTYPE)), placed


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("mode", ["orient", "given"])
@pytest.mark.parametrize("name", ["192x144", "160x120"])
def test_random_keypoints_against_the_restatement(vk, images, name, mode, precision):
    img = images[name]
    keep = mode == "given"
    kps = random_keypoints(img, 60, 7 if name == "192x144" else 8)
    cfg = config(vk, img, pyramid_precision_mode=vk.VKSIFT_PYRAMID_PRECISION_FLOAT16 if precision == "fp16" else vk.VKSIFT_PYRAMID_PRECISION_FLOAT32)
    with vk.Instance(cfg) as inst:
        inst.describeKeypoints(img, kps, 0, vk.DESCRIBE_GIVEN if keep else vk.DESCRIBE_ORIENT)
        n, placed = inst.getFeaturesNumber(0), inst.getPlacedKeypointsNumber(0)
        out = inst.downloadFeatures(0)
        want, want_placed = restated(inst, kps, img, keep)
    differ = -1 if len(out) != len(want) else int(sum(a.tobytes() != b.tobytes() for a, b in zip(raw(out), raw(want))))
    print(f"{name} {mode} {precision}: {len(kps)} keypoints, {placed} placed (restated {want_placed}), {n} features (restated {len(want)}), {differ} records differ")
    assert 20 < want_placed <= len(kps) - 3            # some inadmissible, most not
    assert placed == want_placed and n == len(out) == len(want)
    assert raw(out).tobytes() == raw(want).tobytes()


# ---------------------------------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("mode", ["orient", "given"])
def test_batch_of_three_equals_three_single_calls(vk, images, mode):
    img = images["160x120"]
    imgs = [img, vk.gen_synthetic_image(77, 160, 120), vk.gen_synthetic_image(78, 160, 120)]
    lists = [random_keypoints(img, 60, 20), random_keypoints(img, 20, 21)[:0], random_keypoints(img, 25, 22)]
    m = vk.DESCRIBE_GIVEN if mode == "given" else vk.DESCRIBE_ORIENT
    with vk.Instance(config(vk, img, sift_buffer_count=8), batch_capacity=3) as inst:
        for i in range(3):
            inst.describeKeypoints(imgs[i], lists[i], i, m)
        single = [(inst.downloadFeatures(i), inst.getPlacedKeypointsNumber(i)) for i in range(3)]
        inst.describeKeypointsBatch(imgs, lists, 4, m)
        for i in range(3):
            f, p = inst.downloadFeatures(4 + i), inst.getPlacedKeypointsNumber(4 + i)
            assert p == single[i][1] and f.tobytes() == single[i][0].tobytes(), i
        assert len(single[0][0]) > 20 and len(single[1][0]) == 0 and single[1][1] == 0 and len(single[2][0]) > 5
        # the accessors show image 0 of the batch
        top = inst.downloadScaleSpaceImage(0, 0)
    with vk.Instance(config(vk, img)) as inst:
        inst.detectFeatures(imgs[0], 0)
        inst.getFeaturesNumber(0)
        assert top.tobytes() == inst.downloadScaleSpaceImage(0, 0).tobytes()


# ---------------------------------------------------------------------------------------------------------------------- downstream
def test_described_buffer_matches_and_is_budgeted_like_a_detected_one(vk, images):
    img = images["192x144"]
    with vk.Instance(config(vk, img)) as inst:
        inst.detectFeatures(img, 0)
        feats = inst.downloadFeatures(0)
        kps = as_keypoints(feats)
        kps["response"] = np.random.default_rng(3).permutation(len(kps)).astype(f32) * f32(0.001) - f32(0.1)   # a strength of the caller's own
        for rounds in range(2):           # the second round: the matcher's cache exists, the descriptor launch writes the buffer's entry
            inst.describeKeypoints(img, kps, 1, vk.DESCRIBE_GIVEN)
            inst.matchFeatures(1, 0)
            m = inst.downloadMatches()
            out = inst.downloadFeatures(1)
            order = stored_order(kps, img, True)[0]
            repro, _ = reproducible(feats, img.shape[1], img.shape[0], True, S, True)
            assert len(m) == len(out) == len(order)
            for k, i in enumerate(order):
                if repro[i]:
                    assert m["dist_a_b1"][k] == 0 and np.array_equal(feats["descriptor"][m["idx_b1"][k]], feats["descriptor"][i]), (rounds, k, i)
        budget = len(out) // 3
        inst.keepStrongestFeatures(1, 1, budget)
        kept = inst.downloadFeatures(1)
        assert len(kept) == budget and raw(kept).tobytes() == NS.selected_records(raw(out), budget).tobytes()
        # ... which is the caller's response: the strongest `budget` of the stored keypoints
        want = np.sort(np.abs(kps["response"][order]))[::-1][:budget]
        assert np.array_equal(np.sort(np.abs(kept["intensity"]))[::-1], want)
        assert inst.getPlacedKeypointsNumber(1) == 0       # the buffer is no longer what the placement left


def test_placed_count_ends_with_any_budget_call_and_follows_a_conversion(vk, images):
    """the rule of vksift_ext_getPlacedKeypointsNumber as include/vksift_ext.h states it (the walks of tests/test_gpu_api_model.py met the case the
    header used to describe differently): a budget call that names the buffer ends the count whether or not it cuts — the host does not know, when
    the call is queued, how many features a buffer holds whose counters have not arrived —, and leaves the records of a buffer it does not cut
    alone; a conversion keeps the count"""
    img = images["192x144"]
    with vk.Instance(config(vk, img)) as inst:
        inst.detectFeatures(img, 0)
        kps = as_keypoints(inst.downloadFeatures(0))
        for queued_blind in (True, False):                # the budget behind a describe call nobody has waited for, and behind one whose counts are known
            inst.describeKeypoints(img, kps, 1, vk.DESCRIBE_GIVEN)
            inst.describeKeypoints(img, kps, 2, vk.DESCRIBE_GIVEN)
            if not queued_blind:
                assert inst.getPlacedKeypointsNumber(1) == inst.getPlacedKeypointsNumber(2) > 20
            inst.convertToRootSift(2, 1)
            inst.keepStrongestFeatures(1, 1, len(kps) + 1)                               # does not bind
            assert inst.getPlacedKeypointsNumber(1) == 0, queued_blind
            assert inst.getPlacedKeypointsNumber(2) > 20, queued_blind
            out = inst.downloadFeatures(1)
            inst.keepStrongestFeaturesGrid(2, 1, len(kps) + 1, img.shape[1], img.shape[0], 4, 3)     # nor does this one
            assert inst.getPlacedKeypointsNumber(2) == 0, queued_blind
            assert raw(inst.downloadFeatures(2)).tobytes() == NR.convert_records(raw(out)).tobytes(), queued_blind   # untouched but for the conversion
            inst.describeKeypoints(img, kps, 1, vk.DESCRIBE_GIVEN)
            assert inst.getPlacedKeypointsNumber(1) == len(out) and inst.downloadFeatures(1).tobytes() == out.tobytes(), queued_blind


# ---------------------------------------------------------------------------------------------------------------------- no side effects
def test_detections_around_a_describe_call_are_unaffected(vk, images, monkeypatch):
    img, other = images["160x120"], vk.gen_synthetic_image(5, 160, 120)
    kps = random_keypoints(img, 60, 30)
    for graph in ("0", "1"):
        monkeypatch.setenv("VKSIFT_GRAPH", graph)
        with vk.Instance(config(vk, img)) as inst:
            inst.detectFeatures(img, 0)
            before = inst.downloadFeatures(0)
            inst.detectFeatures(img, 0)            # (VKSIFT_GRAPH=1: the replay of the captured sequence)
            assert inst.downloadFeatures(0).tobytes() == before.tobytes()
            stats = inst.getDeferredStats()
            inst.describeKeypoints(other, kps, 1, vk.DESCRIBE_ORIENT)
            inst.describeKeypoints(other, kps, 0, vk.DESCRIBE_GIVEN)
            assert inst.getPlacedKeypointsNumber(0) > 20
            assert inst.getDeferredStats() == stats
            for _ in range(2):
                inst.detectFeatures(img, 0)
                assert inst.downloadFeatures(0).tobytes() == before.tobytes(), graph
            assert inst.getPlacedKeypointsNumber(0) == 0 and inst.getPlacedKeypointsNumber(1) > 20
    # the staged run of plain detections in front of a describe call is launched first, and counted as before
    monkeypatch.setenv("VKSIFT_GRAPH", "0")
    with vk.Instance(config(vk, img, sift_buffer_count=6)) as inst:
        for rounds in range(2):
            for k in range(3):
                inst.detectFeatures(img, k)
            inst.describeKeypoints(other, kps, 4, vk.DESCRIBE_GIVEN)
            assert all(inst.downloadFeatures(k).tobytes() == before.tobytes() for k in range(3))
        a = inst.getDeferredStats()
    with vk.Instance(config(vk, img, sift_buffer_count=6)) as inst:
        for rounds in range(2):
            for k in range(3):
                inst.detectFeatures(img, k)
            inst.getFeaturesNumber(0)
        assert inst.getDeferredStats() == a


def test_detect_timings_keep_reporting_the_last_detection(vk, images):
    img = images["160x120"]
    with vk.Instance(config(vk, img)) as inst:
        inst.setProfiling(True)
        inst.detectFeatures(img, 0)
        t0, a0 = inst.getDetectTimings(), inst.getAccumulatedDetectTimings()
        inst.describeKeypoints(img, random_keypoints(img, 60, 31), 1, vk.DESCRIBE_ORIENT)
        assert inst.getFeaturesNumber(1) > 20
        assert inst.getDetectTimings() == t0 and inst.getAccumulatedDetectTimings() == a0


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_invalid_input_reports_once_and_changes_nothing(vk, images):
    img = images["160x120"]
    h, w = img.shape
    cfg = config(vk, img, max_nb_sift_per_buffer=300)
    kps = random_keypoints(img, 301, 40)
    lib = vk.lib()
    import ctypes as C
    with vk.Instance(cfg, batch_capacity=2) as inst:
        inst.detectFeatures(img, 0)
        before = inst.downloadFeatures(0)
        assert len(before) > 20
        one = lambda image, ww, hh, k, n, buf, mode: lib.vksift_ext_describeKeypoints(inst._h, image, ww, hh, k, n, buf, mode)
        ptrs = (C.c_void_p * 3)(img.ctypes.data, img.ctypes.data, img.ctypes.data)
        counts = (C.c_uint32 * 3)(10, 301, 0)
        ok_counts = (C.c_uint32 * 3)(10, 10, 10)
        batch = lambda p, count, k, n, buf, mode: lib.vksift_ext_describeKeypointsBatch(inst._h, p, count, w, h, k, n, buf, mode)
        I, K = img.ctypes.data, kps.ctypes.data
        calls = {
            "buffer out of range": lambda: one(I, w, h, K, 10, 4, 0),
            "image too small": lambda: one(I, 12, 12, K, 10, 0, 0),
            "image too large": lambda: one(I, 4 * w, 4 * h, K, 10, 0, 0),
            "NULL keypoints with a count": lambda: one(I, w, h, None, 10, 0, 0),
            "more keypoints than a buffer holds": lambda: one(I, w, h, K, 301, 0, 1),
            "unknown mode": lambda: one(I, w, h, K, 10, 0, 2),
            "NULL image": lambda: one(None, w, h, K, 10, 0, 0),
            "batch above the capacity": lambda: batch(ptrs, 3, K, ok_counts, 0, 0),
            "batch of none": lambda: batch(ptrs, 0, K, ok_counts, 0, 0),
            "batch beyond the last buffer": lambda: batch(ptrs, 2, K, ok_counts, 3, 0),
            "batch, one list too long": lambda: batch(ptrs, 2, K, counts, 0, 1),
            "batch, NULL counts": lambda: batch(ptrs, 2, K, None, 0, 0),
        }
        for what, call in calls.items():
            vk._pending_error.clear()
            call()
            codes = list(vk._pending_error)
            vk._pending_error.clear()
            assert codes == [vk.VKSIFT_INVALID_INPUT_ERROR], (what, codes)
            assert inst.isBufferAvailable(0) and inst.getFeaturesNumber(0) == len(before) and inst.downloadFeatures(0).tobytes() == before.tobytes(), what
        # the limits themselves are fine: a full list, no list at all
        inst.describeKeypoints(img, kps[:300], 0, vk.DESCRIBE_GIVEN)
        assert 100 < inst.getPlacedKeypointsNumber(0) == inst.getFeaturesNumber(0) <= 300
        inst.describeKeypoints(img, None, 0, vk.DESCRIBE_ORIENT)
        assert inst.getFeaturesNumber(0) == 0 and inst.getPlacedKeypointsNumber(0) == 0


def test_an_image_without_an_octave_leaves_the_buffer_empty(vk):
    img = vk.gen_synthetic_image(9, 48, 24)      # shortest side 24: log2(24) - 4 < 1 without up-sampling
    k = np.zeros(3, ND.KEYPOINT_DTYPE)
    k["x"], k["y"], k["sigma"] = [5, 10, 20], [5, 10, 12], [1.6, 2.0, 3.0]
    with vk.Instance(vk.default_config(sift_buffer_count=2, input_image_max_size=160 * 120, use_input_upsampling=False)) as inst:
        inst.detectFeatures(vk.gen_synthetic_image(10, 160, 120), 0)
        assert inst.getFeaturesNumber(0) > 20
        inst.describeKeypoints(img, k, 0, vk.DESCRIBE_GIVEN)
        assert inst.getFeaturesNumber(0) == 0 and inst.getPlacedKeypointsNumber(0) == 0 and len(inst.downloadFeatures(0)) == 0
        assert inst.getScaleSpaceNbOctaves() == 0
