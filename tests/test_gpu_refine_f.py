"""GPU-side refit of the verified fundamental matrices on their inliers (refine_f.hip, vksift_ext_refineFundamental) against its restatement
tests/np_refine_f.py: bit equality of the model, the counts, the round and every mask byte — at the kernel level on synthetic two-view
correspondences and through the public API on detected and on uploaded features —, and the contract of the entry points."""
import numpy as np
import pytest

import np_guided as G
import np_refine_f as RF
import np_verify_f as VF
import quality as Q
from pair_checks import corr as _corr, same_refined_fundamental as _same

pytestmark = pytest.mark.gpu

SLOT_N, SPECIAL, SPECIAL_N, ROUNDS, THRESHOLDS = RF.SLOT_N, RF.SPECIAL, RF.SPECIAL_N, RF.SLOT_ROUNDS, RF.SLOT_THRESHOLDS


def _record_words(rec):
    """a restated RANSAC result as the 14 words of the kernel's start record"""
    w = np.zeros(14, np.uint32)
    w[:9] = np.asarray(rec["F"], np.float32).reshape(9).view(np.uint32)
    w[9], w[10], w[11], w[12], w[13] = rec["nb_matches"], rec["nb_inliers"], rec["best_hypothesis"], rec["best_root"], rec["valid"]
    return w


def test_kernel_level_every_size_round_count_and_threshold_is_bit_equal(vk):
    import torch

    sizes = SLOT_N + [SPECIAL_N] * len(SPECIAL)
    max_n = max(sizes)
    rows = max_n + 192                                                     # a slot stride larger than max_n, in both the correspondences and the masks
    checked = 0
    for thr in THRESHOLDS:
        slots = [t[:3] for t in RF.kernel_test_slots(thr)]
        corr = np.full((len(slots), rows, 4), np.nan, np.float32)          # beyond n: never read (a NaN would show in the sums and the counts)
        masks0 = np.full((len(slots), rows), 1, np.uint8)                  # beyond n: ones that must not count
        recs = np.zeros((len(slots), 14), np.uint32)
        for i, (c, s, m) in enumerate(slots):
            corr[i, :len(c)], masks0[i, :len(c)], recs[i] = c, m, _record_words(s)
        d_corr, d_masks0 = torch.from_numpy(corr).cuda(), torch.from_numpy(masks0).cuda()
        d_recs = torch.from_numpy(recs.view(np.int32)).cuda()
        d_n = torch.tensor(sizes, dtype=torch.int32).cuda()
        for nr in ROUNDS:
            err, res, masks = vk.refit_fundamental(d_corr, d_n, d_recs, d_masks0, nr, thr, overrides={"max_n": max_n})
            assert err == 0
            assert np.array_equal(d_masks0.cpu().numpy(), masks0) and np.array_equal(d_recs.cpu().numpy().view(np.uint32), recs)    # inputs untouched
            for i, (c, s, m) in enumerate(slots):
                want = RF.refit(c, s, m, nr, thr)
                ctx = (thr, nr, i, sizes[i])
                _same(res[i], want, ctx)
                n = len(c)
                assert np.array_equal(masks[i, :n], want["mask"]), ctx
                # bytes are 0 / 1 and sum to nb_inliers; with rounds == 0 the output is the start mask verbatim, whose sum is the start record's count
                # only where that record is consistent with it (the special slots' are not, on purpose)
                assert set(np.unique(masks[i, :n])) <= {0, 1} and int(masks[i, :n].sum()) == (want["nb_inliers"] if want["rounds"] else int((m == 1).sum()) if want["valid"] else 0), ctx
                assert (masks[i, n:] == 0x55).all(), ctx                                # nothing written beyond n
                assert int(res[i]["nb_inliers"]) >= int(s["nb_inliers"]) * int(s["valid"]), ctx
                checked += 1
            if nr == 3 and thr == 2.5:
                # the comparison above is not one of empty results: the rounds were accepted where there was something to fit, and the special
                # slots did what they are there for
                k0 = len(SLOT_N)
                assert [int(res[i]["valid"]) for i in range(len(SLOT_N))] == [1 if n >= 8 else 0 for n in SLOT_N]
                assert all(int(res[i]["rounds"]) >= 1 for i, n in enumerate(SLOT_N) if n >= 8), [int(r["rounds"]) for r in res]
                assert int(res[k0]["valid"]) == 1 and int(res[k0]["rounds"]) == 0 and masks[k0, :SPECIAL_N].all()       # all ones over half outliers: rejected
                assert int(res[k0 + 1]["rounds"]) >= 1 and int(res[k0 + 1]["nb_inliers"]) > 100                        # exactly eight ones: a round runs
                assert int(res[k0 + 2]["rounds"]) == 0 and int(res[k0 + 2]["nb_inliers"]) == 7 and int(masks[k0 + 2, :SPECIAL_N].sum()) == 7
                assert res[k0 + 3].tobytes() == bytes(52) and not masks[k0 + 3, :SPECIAL_N].any()                       # invalid start record
    assert checked == len(THRESHOLDS) * len(ROUNDS) * (len(SLOT_N) + len(SPECIAL))      # no case left out


def test_kernel_level_refusals_launch_nothing(vk):
    import torch

    n = 50
    c, _, _ = VF.two_view_case(n, 0.5, 0.5, 1, 640, 480)
    s = VF.ransac(c, 256, 2.5, 0)
    assert s["valid"] == 1
    d_corr = torch.from_numpy(np.stack([c, c])).cuda()
    d_n = torch.tensor([n, n], dtype=torch.int32).cuda()
    d_recs = torch.from_numpy(np.stack([_record_words(s)] * 2).view(np.int32)).cuda()
    d_masks0 = torch.from_numpy(np.stack([s["mask"].astype(np.uint8)] * 2)).cuda()

    def refused(nr=3, thr=2.5, **over):
        buf = {}
        err = vk.refit_fundamental(d_corr, d_n, d_recs, d_masks0, nr, thr, overrides=over, buffers=buf)[0]
        torch.cuda.synchronize()
        untouched = bool((buf["results"] == -1).all()) and bool((buf["masks"] == 0x55).all())
        return err != 0 and untouched

    assert refused(nslots=0)
    assert refused(nr=0) and refused(nr=9)
    assert refused(thr=0.0) and refused(thr=-1.0) and refused(thr=float("nan")) and refused(thr=float("inf"))
    assert refused(thr=1e-30) and refused(thr=1e30)                                  # the squared threshold is zero / not finite
    assert refused(corr=d_corr.data_ptr() + 4) and refused(corr_stride=n * 16 + 8)
    assert refused(corr_stride=(n - 1) * 16) and refused(mask_stride=n - 1)
    assert refused(masks_out=d_masks0.data_ptr()) and refused(masks_out=d_masks0.data_ptr() + 1) and refused(masks_out=d_masks0.data_ptr() - 1)
    err, res, masks = vk.refit_fundamental(d_corr, d_n, d_recs, d_masks0, 8, 2.5)     # the largest admitted
    assert err == 0 and int(res[0]["valid"]) == 1 and res[0].tobytes() == res[1].tobytes()
    _same(res[0], RF.refit(c, s, s["mask"], 8, 2.5), "admitted")


# ---- through the public API ------------------------------------------------------------------------------------------------------------
W, H = 640, 480
INF = float("inf")


def _pairs(vk, seed=33):
    base = vk.gen_synthetic_image(seed, W, H)
    Hs = [Q.homography(W, H, **kw) for kw in Q.WARPS]
    return [base] + [Q.warp(base, Ht) for Ht in Hs], Hs


def _two_view_features(vk, seed=77):
    """the images the helpers render are related by homographies (a plane: the degenerate configuration for F), so the genuinely two-view pair is
    one of UPLOADED features: np_guided.slot_case's keypoints of random 3-D points seen by two cameras, with descriptors that match across the
    views, distractors and look-alikes. Returns (features of A, features of B, the planted F)"""
    s = G.slot_case(500, 520, seed, W, H, repeat=1, dups=False)
    fa, fb = np.zeros(500, vk.FEATURE_DTYPE), np.zeros(520, vk.FEATURE_DTYPE)
    fa["x"], fa["y"], fa["descriptor"] = s["xa"], s["ya"], s["desc_a"]
    fb["x"], fb["y"], fb["descriptor"] = s["xb"], s["yb"], s["desc_b"]
    return fa, fb, s["F"]


def _existing_bytes(inst, n):
    out = b""
    for k in range(n):
        out += inst.getFundamental(k).tobytes() + inst.downloadFundamentalInlierMask(k).tobytes() + inst.getHomography(k).tobytes() + inst.downloadInlierMask(k).tobytes()
        out += inst.getRefinedHomography(k).tobytes() + inst.downloadRefinedInlierMask(k).tobytes() + inst.downloadFilteredMatches(k).tobytes()
    return out


def _refined_bytes(inst, n):
    return b"".join(inst.getRefinedFundamental(k).tobytes() + inst.downloadRefinedFundamentalInlierMask(k).tobytes() for k in range(n))


def _check_refined(feats, ids_a, ids_b, fms, fun, masks, ref, rmasks, nr, thr, tag):
    """the refined results of every pair against the restatement run on the downloaded features, filtered matches, RANSAC records and masks;
    returns how many pairs had a round accepted"""
    accepted = 0
    for k in range(len(ids_b)):
        c = _corr(feats[ids_a[k]], feats[ids_b[k]], fms[k])
        want = RF.refit(c, fun[k], masks[k], nr, thr)
        _same(ref[k], want, (tag, k))
        assert np.array_equal(rmasks[k], want["mask"].astype(bool)), (tag, k)
        assert int(ref[k]["nb_inliers"]) >= int(fun[k]["nb_inliers"]), (tag, k)            # monotone
        assert int(ref[k]["valid"]) == int(fun[k]["valid"]), (tag, k)
        if not int(fun[k]["valid"]):
            assert ref[k].tobytes() == bytes(52) and not rmasks[k].any(), (tag, k)
            continue
        if int(ref[k]["rounds"]) == 0:                                                     # no round accepted: the verification's model and mask
            assert ref[k]["F"].tobytes() == fun[k]["F"].tobytes() and np.array_equal(rmasks[k], masks[k]), (tag, k)
        else:
            assert int(rmasks[k].sum()) == int(ref[k]["nb_inliers"]) and 1.0 <= float(np.abs(ref[k]["F"]).max()) < 2.0, (tag, k)
            accepted += 1
        print(f"{tag} pair {k}: {len(fms[k])} filtered matches; RANSAC {int(fun[k]['nb_inliers'])} inliers; refined ({int(ref[k]['rounds'])} rounds) {int(ref[k]['nb_inliers'])} inliers")
    return accepted


def test_public_api_equals_the_restatement_leaves_the_rest_alone_and_feeds_guided_matching(vk):
    """the five warps of tests/quality.py and one two-view pair of uploaded features in one batched call; the restatement runs on the DOWNLOADED
    features, filtered matches, RANSAC record and mask, after 1024 hypotheses and after 16 (where the sample is rarely a good one)."""
    imgs, _ = _pairs(vk)
    fa, fb, F_planted = _two_view_features(vk)
    ids_a, ids_b = [0] * 5 + [6], [1, 2, 3, 4, 5, 7]
    P = len(ids_a)
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs, 0)
        inst.uploadFeatures(fa, 6)
        inst.uploadFeatures(fb, 7)
        inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
        inst.verifyHomography(1024, 2.5, 7)
        inst.refineHomography(3, 2.5)
        inst.verifyFundamental(1024, 2.5, 7)
        before = _existing_bytes(inst, P)
        inst.refineFundamental(3, 2.5)
        ref = [inst.getRefinedFundamental(k) for k in range(P)]
        rmasks = [inst.downloadRefinedFundamentalInlierMask(k) for k in range(P)]
        assert _existing_bytes(inst, P) == before                                   # filtered matches, both verified models, their masks, the refined homographies
        fun = [inst.getFundamental(k) for k in range(P)]
        masks = [inst.downloadFundamentalInlierMask(k) for k in range(P)]
        fms = [inst.downloadFilteredMatches(k) for k in range(P)]
        feats = {i: inst.downloadFeatures(i) for i in range(8)}
        # guided matching under the refined models, handed over through `models`
        own = np.stack([np.asarray(r["F"], np.float32).reshape(9) for r in ref])
        inst.matchFeaturesGuided(G.FUNDAMENTAL, own, 2.5, 0.8, INF, True)
        guided = [inst.downloadGuidedMatches(k) for k in range(P)]
        assert _existing_bytes(inst, P) == before
        assert _refined_bytes(inst, P) == b"".join(ref[k].tobytes() + rmasks[k].tobytes() for k in range(P))      # nor the refined ones by the guided matching
        # the same after few hypotheses
        inst.verifyFundamental(16, 2.5, 7)
        inst.refineFundamental(3, 2.5)
        fun16, masks16 = [inst.getFundamental(k) for k in range(P)], [inst.downloadFundamentalInlierMask(k) for k in range(P)]
        ref16, rmasks16 = [inst.getRefinedFundamental(k) for k in range(P)], [inst.downloadRefinedFundamentalInlierMask(k) for k in range(P)]
    accepted = _check_refined(feats, ids_a, ids_b, fms, fun, masks, ref, rmasks, 3, 2.5, "1024 hypotheses,")
    accepted16 = _check_refined(feats, ids_a, ids_b, fms, fun16, masks16, ref16, rmasks16, 3, 2.5, "16 hypotheses,")
    assert sum(int(f["valid"]) for f in fun) >= 5 and accepted >= 1 and accepted16 >= 1
    for k in range(P):
        if not int(fun[k]["valid"]):
            continue
        # the refined mask is the admissibility guided matching applies to the same model
        a, b = feats[ids_a[k]], feats[ids_b[k]]
        adm = G.admissible(G.FUNDAMENTAL, own[k], a["x"], a["y"], b["x"], b["y"], G.threshold2(2.5))
        if int(ref[k]["rounds"]):
            assert np.array_equal(adm[fms[k]["idx_a"], fms[k]["idx_b"]], rmasks[k]), k
        swept = G.sweep(G.FUNDAMENTAL, own[k], a["x"], a["y"], a["descriptor"], b["x"], b["y"], b["descriptor"], 2.5)
        assert guided[k].tobytes() == G.guided(G.FUNDAMENTAL, None, 1, None, None, None, None, None, None, 2.5, 0.8, INF, True, swept=swept).tobytes(), k
    # the two-view pair: its refined model is the planted geometry (the true matches of the uploaded features, 0.3 px noise, lie within a pixel of it)
    k = P - 1
    assert int(ref[k]["valid"]) == 1 and int(ref[k]["rounds"]) >= 1 and int(ref[k]["nb_inliers"]) > 150
    c = _corr(feats[6], feats[7], fms[k])
    e_planted, e_ransac, e_refined = (RF.rms_sampson(M, c[rmasks[k]]) for M in (F_planted, fun[k]["F"], ref[k]["F"]))
    print(f"two-view pair: RMS Sampson distance of the refined inliers under the planted F {e_planted:.3f} px, the RANSAC F {e_ransac:.3f} px, the refined F {e_refined:.3f} px")
    assert e_planted < 1.0 and e_refined <= e_ransac


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def test_contract_errors_invalidation_timing_and_busy_buffers(vk):
    imgs, _ = _pairs(vk, seed=36)
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=W * H)
    bad_input = vk.VKSIFT_INVALID_INPUT_ERROR
    with vk.Instance(cfg, batch_capacity=2) as inst:
        inst.detectFeaturesBatch(imgs[:2], 0)
        assert _errors(vk, lambda: inst.refineFundamental(3, 2.5)) == bad_input                             # nothing matched yet
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        assert _errors(vk, lambda: inst.refineFundamental(3, 2.5)) == bad_input                             # nothing verified yet
        inst.verifyHomography(256, 2.5, 3)
        inst.refineHomography(3, 2.5)
        assert _errors(vk, lambda: inst.refineFundamental(3, 2.5)) == bad_input                             # only the other model has been
        assert _errors(vk, lambda: inst.getRefinedFundamental(0)) == bad_input                              # ... and refined
        inst.verifyFundamental(512, 2.5, 11)
        assert _errors(vk, lambda: inst.getRefinedFundamental(0)) == bad_input                              # not refined yet
        assert _errors(vk, lambda: inst.downloadRefinedFundamentalInlierMask(0)) == bad_input
        inst.refineFundamental(3, 2.5)
        first = _refined_bytes(inst, 1)
        null_out = lambda: (vk.lib().vksift_ext_getRefinedFundamental(inst._h, 0, None), vk._check_pending())
        for bad in (lambda: inst.refineFundamental(0, 2.5), lambda: inst.refineFundamental(9, 2.5), lambda: inst.refineFundamental(3, 0.0),
                    lambda: inst.refineFundamental(3, -2.5), lambda: inst.refineFundamental(3, float("nan")), lambda: inst.refineFundamental(3, INF),
                    lambda: inst.refineFundamental(3, 1e-30), lambda: inst.refineFundamental(3, 1e30),      # the squared threshold is zero / not finite
                    lambda: inst.getRefinedFundamental(1), lambda: inst.downloadRefinedFundamentalInlierMask(1), null_out):
            assert _errors(vk, bad) == bad_input
            assert _refined_bytes(inst, 1) == first                                                        # nothing changed
        inst.refineFundamental(3, 2.5)                                                                     # the same inputs: the same bytes
        assert _refined_bytes(inst, 1) == first
        refined_h = inst.getRefinedHomography(0).tobytes() + inst.downloadRefinedInlierMask(0).tobytes()   # (untouched by the F refinement)
        inst.verifyHomography(256, 2.5, 4)                                                                 # the other model does not invalidate,
        assert _refined_bytes(inst, 1) == first
        assert _errors(vk, lambda: inst.getRefinedHomography(0)) == bad_input                               # (only its own refined results)
        inst.refineHomography(3, 2.5)                                                                      # nor does its refinement
        assert _refined_bytes(inst, 1) == first
        refined_h = inst.getRefinedHomography(0).tobytes() + inst.downloadRefinedInlierMask(0).tobytes()
        inst.setProfiling(True)
        assert inst.getRefineFundamentalTime() == -1.0
        inst.refineFundamental(8, 2.5)
        assert 0.0 < inst.getRefineFundamentalTime() < 1000.0
        assert inst.getRefineTime() == -1.0                                                                # the homography's refinement was not timed
        r8 = inst.getRefinedFundamental(0)
        fun, mask = inst.getFundamental(0), inst.downloadFundamentalInlierMask(0)
        c = _corr(inst.downloadFeatures(0), inst.downloadFeatures(1), inst.downloadFilteredMatches(0))
        _same(r8, RF.refit(c, fun, mask, 8, 2.5), "8 rounds")
        inst.verifyFundamental(512, 2.5, 12)                                                               # a new verification of the fundamental matrix does,
        assert _errors(vk, lambda: inst.getRefinedFundamental(0)) == bad_input
        assert _errors(vk, lambda: inst.downloadRefinedFundamentalInlierMask(0)) == bad_input
        assert inst.getRefinedHomography(0).tobytes() + inst.downloadRefinedInlierMask(0).tobytes() == refined_h       # and leaves the refined homography alone
        inst.refineFundamental(3, 2.5)
        assert int(inst.getRefinedFundamental(0)["valid"]) == 1
        assert inst.getRefinedHomography(0).tobytes() + inst.downloadRefinedInlierMask(0).tobytes() == refined_h       # as does the F refinement
        inst.matchFeaturesFiltered([0], [1], 0.8, True)                                                    # a new matching does
        assert _errors(vk, lambda: inst.getRefinedFundamental(0)) == bad_input
        assert _errors(vk, lambda: inst.downloadRefinedFundamentalInlierMask(0)) == bad_input
        assert _errors(vk, lambda: inst.refineFundamental(3, 2.5)) == bad_input
        inst.verifyFundamental(64, 2.5, 1)
        inst.refineFundamental(1, 2.5)
        assert int(inst.getRefinedFundamental(0)["valid"]) == 1
        inst.matchFeatures(0, 1)                                                                           # a plain one too
        assert _errors(vk, lambda: inst.getRefinedFundamental(0)) == bad_input


def test_queued_refinement_keeps_the_pairs_buffers_busy(vk):
    """a batched detection into other buffers is queued first, so that the verification and the refinement behind it are certainly still queued
    when the host asks: the pairs' buffers are busy until the refinement has passed, and the accessors wait for it"""
    imgs, _ = _pairs(vk, seed=37)
    other = [vk.gen_synthetic_image(900 + i, W, H) for i in range(16)]
    cfg = vk.default_config(sift_buffer_count=18, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=16) as inst:
        inst.detectFeaturesBatch(imgs[:2], 0)
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        assert len(inst.downloadFilteredMatches(0)) > 50                    # (waits: nothing is queued now)
        inst.detectFeaturesBatch(other, 2)
        inst.verifyFundamental(1024, 2.5, 1)
        inst.refineFundamental(8, 2.5)
        busy = [inst.isBufferAvailable(i) for i in range(2)]
        ref, rmask = inst.getRefinedFundamental(0), inst.downloadRefinedFundamentalInlierMask(0)
        assert all(inst.isBufferAvailable(i) for i in range(2))            # the accessors have waited for it
        fun, mask = inst.getFundamental(0), inst.downloadFundamentalInlierMask(0)
        c = _corr(inst.downloadFeatures(0), inst.downloadFeatures(1), inst.downloadFilteredMatches(0))
        assert inst.getFeaturesNumber(17) > 100
    assert busy == [False, False]
    want = RF.refit(c, fun, mask, 8, 2.5)
    _same(ref, want, "queued")
    assert np.array_equal(rmask, want["mask"].astype(bool))
