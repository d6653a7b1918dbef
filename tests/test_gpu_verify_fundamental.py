"""GPU-side verification against a fundamental matrix (verify.hip, vksift_ext_verifyFundamental) against its restatement
tests/np_verify_f.py: bit equality of the model, the winner, its root, the count and every mask byte — at the kernel level on synthetic
two-view correspondences and through the public API on detected features —, that the planted geometry is found, that the homography's
results are untouched by it, and the contract of the entry points."""
import numpy as np
import pytest

import np_verify as V
import np_verify_f as VF
import quality as Q
from pair_checks import corr as _corr, same_fundamental as _same

pytestmark = pytest.mark.gpu

SLOT_N = VF.SLOT_N
assert SLOT_N == [0, 6, 7, 8, 63, 64, 65, 255, 256, 257, 1000]
NB_HYP = [1, 100, 256, 257, 1024]
SEEDS = [0, 0x5EED0000C0FFEE]
THRESHOLDS = [0.5, 2.5]


def test_kernel_level_every_size_hypothesis_count_seed_and_threshold_is_bit_equal(vk):
    import torch

    cases = VF.kernel_test_slots()
    slots = [c for c, _, _ in cases]
    assert float(slots[VF.BIG_SLOT].max()) == 16383.0
    max_n = max(SLOT_N)
    corr = np.full((len(slots), max_n, 4), np.nan, np.float32)     # beyond n: never read (NaN would show in the counts)
    for i, c in enumerate(slots):
        corr[i, :len(c)] = c
    d_corr = torch.from_numpy(corr).cuda()
    d_n = torch.tensor(SLOT_N, dtype=torch.int32).cuda()
    t2s = [VF.threshold2(t) for t in THRESHOLDS]
    checked, planted = 0, 0
    for seed in SEEDS:
        # the models of a smaller nb_hypotheses are a prefix of the largest run's: restated once per (seed, slot)
        hyps = [VF.hypotheses(c, max(NB_HYP), seed, i) if len(c) >= 7 else None for i, c in enumerate(slots)]
        counts = [VF.inlier_counts(hyps[i][1], c, t2s) if len(c) >= 7 else None for i, c in enumerate(slots)]
        for ti, thr in enumerate(THRESHOLDS):
            for nh in NB_HYP:
                err, res, masks = vk.ransac_fundamental(d_corr, d_n, nh, thr, seed)
                assert err == 0
                for i, c in enumerate(slots):
                    want = VF.ransac(c, nh, thr, seed, slot=i, counts=None if counts[i] is None else counts[i][ti], hyps=hyps[i])
                    ctx = (seed, thr, nh, SLOT_N[i])
                    _same(res[i], want, ctx)
                    assert np.array_equal(masks[i, :len(c)].astype(bool), want["mask"]), ctx
                    assert int(masks[i, :len(c)].sum()) == want["nb_inliers"], ctx      # bytes are 0 / 1
                    checked += 1
                if nh == 1024 and thr == 2.5:
                    # the planted geometry is found where there is one to find (the comparison above is not one of empty results)
                    for i, n in enumerate(SLOT_N):
                        true = cases[i][1]
                        assert int(res[i]["valid"]) == (1 if n >= 8 else 0), (seed, n)
                        if n >= 8:
                            got_true = int((masks[i, :n].astype(bool) & true).sum())
                            print(f"seed {seed:#x} n = {n}: {int(res[i]['nb_inliers'])} inliers, {got_true} of the {int(true.sum())} planted")
                            assert 2 * got_true >= int(true.sum()), (seed, n, got_true)
                            if n in (257, 1000):
                                # what fp32 costs: not below the float64 evaluation of the same samples by more than twice the largest shortfall
                                # measured on the CPU (test_np_verify_f.test_what_fp32_costs)
                                _, _, m64 = VF.ransac_f64(slots[i], 1024, 2.5, seed, slot=i)
                                f64_true = int((m64 & true).sum())
                                print(f"    float64 evaluation: {f64_true}")
                                assert got_true >= f64_true - 2 * VF.FP32_MAX_SHORTFALL, (seed, n, got_true, f64_true)
                                planted += 1
    assert checked == len(SEEDS) * len(THRESHOLDS) * len(NB_HYP) * len(SLOT_N)           # no case left out
    assert planted == 2 * len(SEEDS)


def test_kernel_level_refusals_launch_nothing(vk):
    import torch

    c, _, _ = VF.two_view_case(50, 0.5, 0.5, 1, 640, 480)
    d_corr = torch.from_numpy(c[None]).cuda()
    d_n = torch.tensor([50], dtype=torch.int32).cuda()
    assert vk.ransac_fundamental(d_corr, d_n, 0, 2.5, 0)[0] != 0
    assert vk.ransac_fundamental(d_corr, d_n, 65537, 2.5, 0)[0] != 0
    assert vk.ransac_fundamental(d_corr, d_n, 64, 0.0, 0)[0] != 0
    assert vk.ransac_fundamental(d_corr, d_n, 64, -1.0, 0)[0] != 0
    assert vk.ransac_fundamental(d_corr, d_n, 64, float("nan"), 0)[0] != 0
    assert vk.ransac_fundamental(d_corr, d_n, 64, float("inf"), 0)[0] != 0
    need = vk.lib().vksift_hip_ransac_scratch_u32(1, 1024)
    assert need > 0 and vk.ransac_fundamental(d_corr, d_n, 1024, 2.5, 0, scratch_u32=need - 1)[0] != 0
    err, res, _ = vk.ransac_fundamental(d_corr, d_n, 1024, 2.5, 0)                     # admitted: the same inputs with enough scratch
    assert err == 0 and int(res[0]["valid"]) == 1


# ---- through the public API ------------------------------------------------------------------------------------------------------------
W, H = 640, 480


def _pairs(vk, seed=33):
    base = vk.gen_synthetic_image(seed, W, H)
    Hs = [Q.homography(W, H, **kw) for kw in Q.WARPS]
    return [base] + [Q.warp(base, Ht) for Ht in Hs], Hs


def _same_h(got, want, ctx):
    assert (int(got["valid"]), int(got["nb_matches"]), int(got["best_hypothesis"]), int(got["nb_inliers"])) == (
        want["valid"], want["nb_matches"], want["best_hypothesis"], want["nb_inliers"]), ctx
    assert np.asarray(got["H"], np.float32).tobytes() == want["H"].tobytes(), ctx


def _verify_both(inst, ids_a, ids_b, nh, thr, seed):
    """homography, then fundamental matrix; both read AFTER the second verification: (features, filtered matches, F, F masks, H, H masks)"""
    inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
    inst.verifyHomography(nh, thr, seed)
    inst.verifyFundamental(nh, thr, seed)
    r = range(len(ids_a))
    fun = [inst.getFundamental(k) for k in r]
    fmasks = [inst.downloadFundamentalInlierMask(k) for k in r]
    hom = [inst.getHomography(k) for k in r]
    hmasks = [inst.downloadInlierMask(k) for k in r]
    fms = [inst.downloadFilteredMatches(k) for k in r]
    feats = {i: inst.downloadFeatures(i) for i in set(ids_a) | set(ids_b)}
    return feats, fms, fun, fmasks, hom, hmasks


def _check_against_restatements(feats, fms, fun, fmasks, hom, hmasks, ids_a, ids_b, nh, thr, seed):
    wants = []
    for k in range(len(ids_a)):
        c = _corr(feats[ids_a[k]], feats[ids_b[k]], fms[k])
        want = VF.ransac(c, nh, thr, seed, slot=k)
        _same(fun[k], want, k)
        assert np.array_equal(fmasks[k], want["mask"]), k
        if hom is not None:
            want_h = V.ransac(c, nh, thr, seed, slot=k)
            _same_h(hom[k], want_h, k)
            assert np.array_equal(hmasks[k], want_h["mask"]), k
        wants.append((c, want))
    return wants


def test_public_api_both_models_equal_their_restatements(vk):
    """the five warps of tests/quality.py in one batched call, verified with both models; the restatements run on the DOWNLOADED features and
    filtered matches. The frames are related by homographies (a plane), which is the degenerate configuration for F: the estimator still has
    to return what the restatement returns, and a model that explains the matches — every homography-consistent match satisfies the epipolar
    constraint of some F compatible with the plane —, but not a particular F."""
    imgs, Hs = _pairs(vk)
    ids_a, ids_b = [0] * 5, [1, 2, 3, 4, 5]
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs, 0)
        out = _verify_both(inst, ids_a, ids_b, 1024, 2.5, 7)
    feats, fms, fun, fmasks, hom, hmasks = out
    _check_against_restatements(*out, ids_a, ids_b, 1024, 2.5, 7)
    for k in range(5):
        print(f"warp {k}: {len(fms[k])} filtered matches, F {int(fun[k]['nb_inliers'])} inliers (hypothesis {int(fun[k]['best_hypothesis'])} root "
              f"{int(fun[k]['best_root'])}), H {int(hom[k]['nb_inliers'])} inliers")
        if len(fms[k]) >= 16 and int(hom[k]["valid"]):
            assert int(fun[k]["valid"]) == 1
            assert 1.0 <= float(np.abs(fun[k]["F"]).max()) < 2.0
    assert sum(int(f["valid"]) for f in fun) >= 4


def test_clamped_sections_and_an_uploaded_buffer(vk):
    """a small max_nb_sift_per_buffer clamps the sections of every buffer, and one side of a pair is an uploaded buffer (one dense section):
    the rows the gather launch resolves for the second model are the rows vksift_downloadFeatures returns"""
    imgs, _ = _pairs(vk, seed=35)
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H, max_nb_sift_per_buffer=600)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs[:3], 0)
        f1 = inst.downloadFeatures(1)
        inst.uploadFeatures(f1[::-1][:500].copy(), 5)              # another order and length than any detected buffer
        ids_a, ids_b = [0, 0, 5, 2], [1, 5, 0, 5]
        out = _verify_both(inst, ids_a, ids_b, 256, 2.5, 3)
    feats, fms, fun = out[0], out[1], out[2]
    assert len(feats[0]) <= 600 and len(feats[5]) == 500
    assert min(len(m) for m in fms) >= 8
    _check_against_restatements(*out, ids_a, ids_b, 256, 2.5, 3)
    assert all(int(f["valid"]) == 1 for f in fun[:3])


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def test_contract_errors_seeds_and_invalidation(vk):
    imgs, _ = _pairs(vk, seed=36)
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=2) as inst:
        inst.detectFeaturesBatch(imgs[:2], 0)
        assert _errors(vk, lambda: inst.verifyFundamental(64, 2.5, 0)) == vk.VKSIFT_INVALID_INPUT_ERROR     # nothing matched yet
        inst.matchFeatures(0, 1)
        assert _errors(vk, lambda: inst.verifyFundamental(64, 2.5, 0)) == vk.VKSIFT_INVALID_INPUT_ERROR     # a plain matching: nothing filtered
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        assert _errors(vk, lambda: inst.getFundamental(0)) == vk.VKSIFT_INVALID_INPUT_ERROR                 # not verified yet
        inst.verifyHomography(512, 2.5, 11)
        hom_first = inst.getHomography(0).tobytes() + inst.downloadInlierMask(0).tobytes()
        # a verified homography does not make the fundamental matrix's accessors valid
        assert _errors(vk, lambda: inst.getFundamental(0)) == vk.VKSIFT_INVALID_INPUT_ERROR
        assert _errors(vk, lambda: inst.downloadFundamentalInlierMask(0)) == vk.VKSIFT_INVALID_INPUT_ERROR
        inst.verifyFundamental(512, 2.5, 11)
        first = inst.getFundamental(0).tobytes() + inst.downloadFundamentalInlierMask(0).tobytes()
        for bad in (lambda: inst.verifyFundamental(0, 2.5, 0), lambda: inst.verifyFundamental(65537, 2.5, 0), lambda: inst.verifyFundamental(64, 0.0, 0),
                    lambda: inst.verifyFundamental(64, float("nan"), 0), lambda: inst.getFundamental(1), lambda: inst.downloadFundamentalInlierMask(1)):
            assert _errors(vk, bad) == vk.VKSIFT_INVALID_INPUT_ERROR
            assert inst.getFundamental(0).tobytes() + inst.downloadFundamentalInlierMask(0).tobytes() == first   # nothing changed
        assert inst.getHomography(0).tobytes() + inst.downloadInlierMask(0).tobytes() == hom_first               # the other model's results stand
        inst.verifyFundamental(512, 2.5, 11)                                                               # the same seed: the same bytes
        assert inst.getFundamental(0).tobytes() + inst.downloadFundamentalInlierMask(0).tobytes() == first
        inst.verifyFundamental(512, 2.5, 12)                                                               # another seed: the restatement's answer for it
        f12, m12 = inst.getFundamental(0), inst.downloadFundamentalInlierMask(0)
        fa, fb, fm = inst.downloadFeatures(0), inst.downloadFeatures(1), inst.downloadFilteredMatches(0)
        want = VF.ransac(_corr(fa, fb, fm), 512, 2.5, 12)
        _same(f12, want, "seed 12")
        assert np.array_equal(m12, want["mask"])
        assert int(f12["nb_matches"]) == len(fm) and int(m12.sum()) == int(f12["nb_inliers"]) and int(f12["valid"]) == 1
        assert inst.getHomography(0).tobytes() + inst.downloadInlierMask(0).tobytes() == hom_first
        inst.setProfiling(True)
        assert inst.getVerifyTime() == -1.0
        inst.verifyFundamental(512, 2.5, 12)
        assert 0.0 < inst.getVerifyTime() < 1000.0
        inst.matchFeatures(0, 1)                                                                           # a new matching invalidates both models
        for gone in (lambda: inst.getFundamental(0), lambda: inst.downloadFundamentalInlierMask(0), lambda: inst.getHomography(0),
                     lambda: inst.downloadInlierMask(0)):
            assert _errors(vk, gone) == vk.VKSIFT_INVALID_INPUT_ERROR
        inst.matchFeaturesFiltered([0], [1], 0.8, True)                                                    # and a filtered one too, until verified again
        assert _errors(vk, lambda: inst.getFundamental(0)) == vk.VKSIFT_INVALID_INPUT_ERROR
        inst.verifyFundamental(512, 2.5, 11)
        assert inst.getFundamental(0).tobytes() + inst.downloadFundamentalInlierMask(0).tobytes() == first
        assert _errors(vk, lambda: inst.getHomography(0)) == vk.VKSIFT_INVALID_INPUT_ERROR                  # only the model that was run


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
        inst.verifyFundamental(1024, 2.5, 5)
        inst.detectFeaturesBatch(other, 3)
        busy = [inst.isBufferAvailable(i) for i in range(3)]                # False while the verification runs; True once it has passed
        fun = [inst.getFundamental(k) for k in range(2)]
        masks = [inst.downloadFundamentalInlierMask(k) for k in range(2)]
        assert all(inst.isBufferAvailable(i) for i in range(3))            # the accessors have waited for it
        fms = [inst.downloadFilteredMatches(k) for k in range(2)]
        feats = {i: inst.downloadFeatures(i) for i in range(3)}
        later = inst.downloadFeatures(4)
    assert len(busy) == 3 and len(later) > 100
    _check_against_restatements(feats, fms, fun, masks, None, None, ids_a, ids_b, 1024, 2.5, 5)
    assert all(int(f["valid"]) == 1 for f in fun)
