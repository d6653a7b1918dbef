"""GPU-side geometric verification (verify.hip, vksift_ext_verifyHomography) against its restatement tests/np_verify.py: bit equality of the
model, the winner, the count and every mask byte — at the kernel level on synthetic correspondences and through the public API on detected
features —, what the estimate is worth against the ground truth, and the contract of the entry points."""
import numpy as np
import pytest

import np_verify as V
import quality as Q
from pair_checks import corr as _corr, same_homography as _same

pytestmark = pytest.mark.gpu

SLOT_N = [0, 1, 3, 4, 5, 63, 64, 65, 257, 1000, 4097, 100000]   # the last: vksift_getDefaultConfig().max_nb_sift_per_buffer
NB_HYP = [1, 64, 100, 256, 1024, 4096]
SEEDS = [0, 0x5EED0000C0FFEE]
THRESHOLDS = [0.5, 2.5, 10.0]


def _slots():
    """correspondences of every slot: planted homographies with outliers and noise in images up to 16383 px, sizes on the tile and wave
    boundaries of the LDS staging; n = 4, 5 without outliers (so that a model exists), n < 4 arbitrary"""
    out = []
    for i, n in enumerate(SLOT_N):
        w, h = [(640, 480), (16383, 12000), (4000, 3000)][i % 3]
        Ht = Q.homography(w, h, **Q.WARPS[i % 4])
        c, _ = V.synthetic_case(Ht, w, h, n=n, outliers=0.0 if n < 63 else 0.5, noise=0.5, seed=40 + i)
        if n >= 257:
            c[7, 0], c[n - 1, 2] = 16383.0, 16383.0     # the largest coordinate the kernels are specified for
        out.append(c)
    return out


def test_kernel_level_every_size_hypothesis_count_seed_and_threshold_is_bit_equal(vk):
    import torch

    slots = _slots()
    max_n = max(SLOT_N)
    corr = np.full((len(slots), max_n, 4), np.nan, np.float32)     # beyond n: never read (NaN would show in the counts)
    for i, c in enumerate(slots):
        corr[i, :len(c)] = c
    d_corr = torch.from_numpy(corr).cuda()
    d_n = torch.tensor(SLOT_N, dtype=torch.int32).cuda()
    t2s = [V.threshold2(t) for t in THRESHOLDS]
    checked = 0
    for seed in SEEDS:
        # the hypotheses of a smaller nb_hypotheses are a prefix of the largest run's: restated once per (seed, slot)
        hyps = [V.hypotheses(c, max(NB_HYP), seed, i) if len(c) >= 4 else None for i, c in enumerate(slots)]
        counts = [V.inlier_counts(hyps[i][1], c, t2s) if len(c) >= 4 else None for i, c in enumerate(slots)]
        for ti, thr in enumerate(THRESHOLDS):
            for nh in NB_HYP:
                err, res, masks = vk.ransac_homography(d_corr, d_n, nh, thr, seed)
                assert err == 0
                for i, c in enumerate(slots):
                    want = V.ransac(c, nh, thr, seed, slot=i, counts=None if counts[i] is None else counts[i][ti], hyps=hyps[i])
                    ctx = (seed, thr, nh, SLOT_N[i])
                    _same(res[i], want, ctx)
                    assert np.array_equal(masks[i, :len(c)].astype(bool), want["mask"]), ctx
                    assert int(masks[i, :len(c)].sum()) == want["nb_inliers"], ctx      # bytes are 0 / 1
                    checked += 1
    assert checked == len(SEEDS) * len(THRESHOLDS) * len(NB_HYP) * len(SLOT_N)           # no case left out
    # the planted models were found where there was one to find (the comparison above is not one of empty results)
    err, res, masks = vk.ransac_homography(d_corr, d_n, 1024, 2.5, 0)
    for i, n in enumerate(SLOT_N):
        assert int(res[i]["valid"]) == (1 if n >= 4 else 0), n
        if n >= 63:
            assert int(res[i]["nb_inliers"]) > 0.3 * n, (n, res[i])


def test_kernel_level_refusals_launch_nothing(vk):
    import torch

    c, _ = V.synthetic_case(Q.homography(640, 480, **Q.WARPS[0]), 640, 480, n=50, seed=1)
    d_corr = torch.from_numpy(c[None]).cuda()
    d_n = torch.tensor([50], dtype=torch.int32).cuda()
    assert vk.ransac_homography(d_corr, d_n, 0, 2.5, 0)[0] != 0
    assert vk.ransac_homography(d_corr, d_n, 65537, 2.5, 0)[0] != 0
    assert vk.ransac_homography(d_corr, d_n, 64, 0.0, 0)[0] != 0
    assert vk.ransac_homography(d_corr, d_n, 64, -1.0, 0)[0] != 0
    assert vk.ransac_homography(d_corr, d_n, 64, float("nan"), 0)[0] != 0
    assert vk.ransac_homography(d_corr, d_n, 64, float("inf"), 0)[0] != 0
    need = vk.lib().vksift_hip_ransac_scratch_u32(1, 1024)
    assert need > 0 and vk.ransac_homography(d_corr, d_n, 1024, 2.5, 0, scratch_u32=need - 1)[0] != 0
    err, res, _ = vk.ransac_homography(d_corr, d_n, 65536, 2.5, 0)                     # the largest admitted
    assert err == 0 and int(res[0]["valid"]) == 1


# ---- through the public API ------------------------------------------------------------------------------------------------------------
W, H = 640, 480


def _pairs(vk, seed=33):
    base = vk.gen_synthetic_image(seed, W, H)
    Hs = [Q.homography(W, H, **kw) for kw in Q.WARPS]
    return [base] + [Q.warp(base, Ht) for Ht in Hs], Hs


def _verify_all(inst, ids_a, ids_b, nh, thr, seed):
    """(feature sets, filtered matches, homographies, masks) of a verification of the pairs"""
    inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
    inst.verifyHomography(nh, thr, seed)
    hom = [inst.getHomography(k) for k in range(len(ids_a))]
    masks = [inst.downloadInlierMask(k) for k in range(len(ids_a))]
    fms = [inst.downloadFilteredMatches(k) for k in range(len(ids_a))]
    feats = {i: inst.downloadFeatures(i) for i in set(ids_a) | set(ids_b)}
    return feats, fms, hom, masks


def _check_against_restatement(feats, fms, hom, masks, ids_a, ids_b, nh, thr, seed):
    wants = []
    for k in range(len(ids_a)):
        c = _corr(feats[ids_a[k]], feats[ids_b[k]], fms[k])
        want = V.ransac(c, nh, thr, seed, slot=k)
        _same(hom[k], want, k)
        assert np.array_equal(masks[k], want["mask"]), k
        wants.append((c, want))
    return wants


def test_public_api_equals_the_restatement_and_finds_the_warp(vk):
    """the five warps of tests/quality.py in one batched call; the restatement runs on the DOWNLOADED features and filtered matches, so the
    download-order -> record resolution of the gather launch is part of what is compared. Figures (printed; recorded in DESIGN.md):
    share of mask inliers that quality.score's criterion (ground truth, 2.5 px) calls correct, four-corner error of H."""
    imgs, Hs = _pairs(vk)
    ids_a, ids_b = [0] * 5, [1, 2, 3, 4, 5]
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs, 0)
        feats, fms, hom, masks = _verify_all(inst, ids_a, ids_b, 1024, 2.5, 7)
    wants = _check_against_restatement(feats, fms, hom, masks, ids_a, ids_b, 1024, 2.5, 7)
    few = [k for k in range(5) if len(fms[k]) < 8]
    assert set(few) <= {4}, few               # at most the 70 degree warp may leave fewer than 8 filtered matches: valid-or-not only (above)
    for k in range(5):
        if k in few:
            continue
        c, want = wants[k]
        fa, fb, fm = feats[0], feats[ids_b[k]], fms[k]
        px, py = Q.project(Hs[k], c[:, 0].astype(np.float64), c[:, 1].astype(np.float64))
        correct = np.hypot(px - c[:, 2], py - c[:, 3]) < 2.5         # quality.score's criterion, per match
        assert int(correct.sum()) == Q.score(fa, fb, fm["idx_a"], fm["idx_b"], Hs[k], W, H)["correct"]
        # reference: the float64 evaluation of the same hypotheses on the same data (independent of the kernel)
        j64, cnt64, H64, mask64, _ = V.ransac_f64(c, 1024, 2.5, 7, slot=k)
        assert int(hom[k]["valid"]) == 1
        gpu_ok, r_ok, f64_ok = int((masks[k] & correct).sum()), int((want["mask"] & correct).sum()), int((mask64 & correct).sum())
        gpu_bad, f64_bad = int((masks[k] & ~correct).sum()), int((mask64 & ~correct).sum())
        e_gpu, e_64 = V.corner_error(hom[k]["H"], Hs[k], W, H), V.corner_error(H64, Hs[k], W, H)
        print(f"warp {k}: {len(fm)} filtered matches ({int(correct.sum())} correct), GPU mask {int(masks[k].sum())} inliers of which {gpu_ok} correct "
              f"(precision {gpu_ok / max(int(masks[k].sum()), 1):.4f}), float64 {int(mask64.sum())} / {f64_ok} (hypothesis {j64}); "
              f"corner error GPU {e_gpu:.3f} px, float64 {e_64:.3f} px")
        assert gpu_ok == r_ok and e_gpu == V.corner_error(want["H"], Hs[k], W, H)      # the same bits give the same figures
        # fp32 is not below the float64 evaluation by more than one match per pair: correct inliers found, and wrong ones let in
        assert gpu_ok >= f64_ok - 1, (k, gpu_ok, f64_ok)
        assert gpu_bad <= f64_bad + 1, (k, gpu_bad, f64_bad)


def test_clamped_sections_and_an_uploaded_buffer(vk):
    """a small max_nb_sift_per_buffer clamps the sections of every buffer (min(found, capacity) on the device), and one side of a pair is an
    uploaded buffer (one dense section): the rows the gather launch resolves are the rows vksift_downloadFeatures returns"""
    imgs, _ = _pairs(vk, seed=35)
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H, max_nb_sift_per_buffer=600)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs[:3], 0)
        f1 = inst.downloadFeatures(1)
        inst.uploadFeatures(f1[::-1][:500].copy(), 5)              # another order and length than any detected buffer
        ids_a, ids_b = [0, 0, 5, 2], [1, 5, 0, 5]
        feats, fms, hom, masks = _verify_all(inst, ids_a, ids_b, 256, 2.5, 3)
    with vk.Instance(vk.default_config(input_image_max_size=W * H)) as inst:
        inst.detectFeatures(imgs[0], 0)
        assert inst.getFeaturesNumber(0) > len(feats[0])            # sections of the small instance were clamped to their capacity
    assert len(feats[0]) <= 600 and len(feats[5]) == 500
    assert min(len(m) for m in fms) >= 8
    _check_against_restatement(feats, fms, hom, masks, ids_a, ids_b, 256, 2.5, 3)
    assert all(int(h["valid"]) == 1 for h in hom[:3])


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def test_contract_errors_seeds_and_invalidation(vk):
    imgs, _ = _pairs(vk, seed=36)
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=2) as inst:
        inst.detectFeaturesBatch(imgs[:2], 0)
        assert _errors(vk, lambda: inst.verifyHomography(64, 2.5, 0)) == vk.VKSIFT_INVALID_INPUT_ERROR      # nothing matched yet
        inst.matchFeatures(0, 1)
        assert _errors(vk, lambda: inst.verifyHomography(64, 2.5, 0)) == vk.VKSIFT_INVALID_INPUT_ERROR      # a plain matching: nothing filtered
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        assert _errors(vk, lambda: inst.getHomography(0)) == vk.VKSIFT_INVALID_INPUT_ERROR                  # not verified yet
        inst.verifyHomography(512, 2.5, 11)
        first = inst.getHomography(0).tobytes() + inst.downloadInlierMask(0).tobytes()
        for bad in (lambda: inst.verifyHomography(0, 2.5, 0), lambda: inst.verifyHomography(65537, 2.5, 0), lambda: inst.verifyHomography(64, 0.0, 0),
                    lambda: inst.verifyHomography(64, float("nan"), 0), lambda: inst.getHomography(1), lambda: inst.downloadInlierMask(1)):
            assert _errors(vk, bad) == vk.VKSIFT_INVALID_INPUT_ERROR
            assert inst.getHomography(0).tobytes() + inst.downloadInlierMask(0).tobytes() == first           # nothing changed
        inst.verifyHomography(512, 2.5, 11)                                                                # the same seed: the same bytes
        assert inst.getHomography(0).tobytes() + inst.downloadInlierMask(0).tobytes() == first
        inst.verifyHomography(512, 2.5, 12)                                                                # another seed: the restatement's answer for it
        h12, m12 = inst.getHomography(0), inst.downloadInlierMask(0)
        fa, fb, fm = inst.downloadFeatures(0), inst.downloadFeatures(1), inst.downloadFilteredMatches(0)
        want = V.ransac(_corr(fa, fb, fm), 512, 2.5, 12)
        _same(h12, want, "seed 12")
        assert np.array_equal(m12, want["mask"])
        assert int(h12["nb_matches"]) == len(fm) and int(m12.sum()) == int(h12["nb_inliers"])
        inst.setProfiling(True)
        assert inst.getVerifyTime() == -1.0
        inst.verifyHomography(512, 2.5, 12)
        assert 0.0 < inst.getVerifyTime() < 1000.0
        inst.matchFeatures(0, 1)                                                                           # a new matching invalidates the verification
        assert _errors(vk, lambda: inst.getHomography(0)) == vk.VKSIFT_INVALID_INPUT_ERROR
        assert _errors(vk, lambda: inst.downloadInlierMask(0)) == vk.VKSIFT_INVALID_INPUT_ERROR


def test_asynchronous_use_with_a_second_buffer_set(vk):
    """verification queued, the next detection queued into a second buffer set before anything is read: the results are the first set's, and its
    buffers stay busy until the verification has passed"""
    imgs, _ = _pairs(vk, seed=37)
    other = [vk.gen_synthetic_image(900 + i, W, H) for i in range(3)]
    cfg = vk.default_config(sift_buffer_count=6, input_image_max_size=W * H)
    ids_a, ids_b = [0, 0], [1, 2]
    with vk.Instance(cfg, batch_capacity=3) as inst:
        inst.detectFeaturesBatch(imgs[:3], 0)
        inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
        inst.verifyHomography(1024, 2.5, 5)
        inst.detectFeaturesBatch(other, 3)
        busy = [inst.isBufferAvailable(i) for i in range(3)]                # False while the verification runs; True once it has passed
        hom = [inst.getHomography(k) for k in range(2)]
        masks = [inst.downloadInlierMask(k) for k in range(2)]
        assert all(inst.isBufferAvailable(i) for i in range(3))            # the accessors have waited for it
        fms = [inst.downloadFilteredMatches(k) for k in range(2)]
        feats = {i: inst.downloadFeatures(i) for i in range(3)}
        later = inst.downloadFeatures(4)
    assert len(busy) == 3 and len(later) > 100
    _check_against_restatement(feats, fms, hom, masks, ids_a, ids_b, 1024, 2.5, 5)


def test_128_pairs_beyond_one_run_of_slots(vk):
    """128 consecutive pairs: the filtered matching works in runs of 64 slots, the verification serves all of them in one launch sequence;
    pairs of both runs against the restatement"""
    B = 128
    base = [vk.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(4)]
    Ht = Q.homography(W, H, **Q.WARPS[0])
    frames = []
    for i in range(B):                       # chains of slightly warped frames, so that consecutive pairs share geometry
        frames.append(base[i % 4] if i % 32 < 4 else Q.warp(frames[i - 4], Ht))
    a = list(range(B))
    b = [(i + 4) % B for i in a]
    cfg = vk.default_config(sift_buffer_count=B, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=B) as inst:
        inst.detectFeaturesBatch(frames, 0)
        inst.matchFeaturesFiltered(a, b, 0.8, True)
        inst.verifyHomography(256, 2.5, 1)
        ks = (0, 63, 64, 127)
        hom = {k: inst.getHomography(k) for k in ks}
        masks = {k: inst.downloadInlierMask(k) for k in ks}
        fms = {k: inst.downloadFilteredMatches(k) for k in ks}
        feats = {i: inst.downloadFeatures(i) for k in ks for i in (a[k], b[k])}
    for k in ks:
        want = V.ransac(_corr(feats[a[k]], feats[b[k]], fms[k]), 256, 2.5, 1, slot=k)
        _same(hom[k], want, k)
        assert np.array_equal(masks[k], want["mask"]), k
    assert int(hom[0]["valid"]) == 1 and int(hom[0]["nb_inliers"]) > 50
