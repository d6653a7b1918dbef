"""GPU-side refit of the verified homographies on their inliers (refine.hip, vksift_ext_refineHomography) against its restatement
tests/np_refine.py: bit equality of the model, the counts, the round and every mask byte — at the kernel level on synthetic correspondences
and through the public API on detected features —, what the refit is worth against the ground truth, and the contract of the entry points."""
import numpy as np
import pytest

import np_guided as G
import np_refine as R
import np_verify as V
import quality as Q
from pair_checks import corr as _corr, same_refined_homography as _same

pytestmark = pytest.mark.gpu

SLOT_N, SPECIAL, SPECIAL_N, ROUNDS, THRESHOLDS = R.SLOT_N, R.SPECIAL, R.SPECIAL_N, R.SLOT_ROUNDS, R.SLOT_THRESHOLDS


def _record_words(rec):
    """a restated RANSAC result as the 13 words of the kernel's record"""
    w = np.zeros(13, np.uint32)
    w[:9] = np.asarray(rec["H"], np.float32).reshape(9).view(np.uint32)
    w[9], w[10], w[11], w[12] = rec["nb_matches"], rec["nb_inliers"], rec["best_hypothesis"], rec["valid"]
    return w


def test_kernel_level_every_size_round_count_and_threshold_is_bit_equal(vk):
    import torch

    sizes = SLOT_N + [SPECIAL_N] * len(SPECIAL)
    max_n = max(sizes)
    checked = 0
    for thr in THRESHOLDS:
        slots = [t[:3] for t in R.kernel_test_slots(thr)]
        corr = np.full((len(slots), max_n, 4), np.nan, np.float32)     # beyond n: never read (a NaN would show in the sums and the counts)
        masks0 = np.full((len(slots), max_n), 1, np.uint8)             # beyond n: ones that must not count
        recs = np.zeros((len(slots), 13), np.uint32)
        for i, (c, s, m) in enumerate(slots):
            corr[i, :len(c)], masks0[i, :len(c)], recs[i] = c, m, _record_words(s)
        d_corr, d_masks0 = torch.from_numpy(corr).cuda(), torch.from_numpy(masks0).cuda()
        d_recs = torch.from_numpy(recs.view(np.int32)).cuda()
        d_n = torch.tensor(sizes, dtype=torch.int32).cuda()
        for nr in ROUNDS:
            err, res, masks = vk.refit_homography(d_corr, d_n, d_recs, d_masks0, nr, thr)
            assert err == 0
            assert np.array_equal(d_masks0.cpu().numpy(), masks0) and np.array_equal(d_recs.cpu().numpy().view(np.uint32), recs)    # inputs untouched
            for i, (c, s, m) in enumerate(slots):
                want = R.refit(c, s, m, nr, thr)
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
                assert [int(res[i]["valid"]) for i in range(len(SLOT_N))] == [1 if n >= 4 else 0 for n in SLOT_N]
                assert all(int(res[i]["rounds"]) >= 1 for i, n in enumerate(SLOT_N) if n >= 63), [int(r["rounds"]) for r in res]
                assert res[k0].tobytes() == bytes(52) and not masks[k0, :SPECIAL_N].any()
                assert int(res[k0 + 1]["rounds"]) >= 1 and int(res[k0 + 1]["nb_inliers"]) > 100
                assert int(res[k0 + 2]["rounds"]) == 0 and int(res[k0 + 2]["nb_inliers"]) == 4 and int(masks[k0 + 2, :SPECIAL_N].sum()) == 4
                assert int(res[k0 + 3]["valid"]) == 1
    assert checked == len(THRESHOLDS) * len(ROUNDS) * (len(SLOT_N) + len(SPECIAL))      # no case left out


def test_kernel_level_refusals_launch_nothing(vk):
    import torch

    n = 50
    c, _ = V.synthetic_case(Q.homography(640, 480, **Q.WARPS[0]), 640, 480, n=n, seed=1)
    s = V.ransac(c, 64, 2.5, 0)
    d_corr = torch.from_numpy(np.stack([c, c])).cuda()
    d_n = torch.tensor([n, n], dtype=torch.int32).cuda()
    d_recs = torch.from_numpy(np.stack([_record_words(s)] * 2).view(np.int32)).cuda()
    d_masks0 = torch.from_numpy(np.stack([s["mask"].astype(np.uint8)] * 2)).cuda()

    def refused(nr=3, thr=2.5, **over):
        buf = {}
        err = vk.refit_homography(d_corr, d_n, d_recs, d_masks0, nr, thr, overrides=over, buffers=buf)[0]
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
    err, res, masks = vk.refit_homography(d_corr, d_n, d_recs, d_masks0, 8, 2.5)      # the largest admitted
    assert err == 0 and int(res[0]["valid"]) == 1 and res[0].tobytes() == res[1].tobytes()
    _same(res[0], R.refit(c, s, s["mask"], 8, 2.5), "admitted")


# ---- through the public API ------------------------------------------------------------------------------------------------------------
W, H = 640, 480
INF = float("inf")


def _pairs(vk, seed=33):
    base = vk.gen_synthetic_image(seed, W, H)
    Hs = [Q.homography(W, H, **kw) for kw in Q.WARPS]
    return [base] + [Q.warp(base, Ht) for Ht in Hs], Hs


def _existing_bytes(inst, n):
    out = b""
    for k in range(n):
        out += inst.getHomography(k).tobytes() + inst.downloadInlierMask(k).tobytes() + inst.downloadFilteredMatches(k).tobytes()
    return out


def _refined_bytes(inst, n):
    return b"".join(inst.getRefinedHomography(k).tobytes() + inst.downloadRefinedInlierMask(k).tobytes() for k in range(n))


def _check_refined(feats, ids_b, fms, hom, masks, ref, rmasks, Hs, nr, thr, tag):
    """the refined results of every pair against the restatement run on the downloaded features, filtered matches, RANSAC records and masks; prints
    the figures; returns how many pairs had a round accepted"""
    accepted = 0
    for k in range(len(ids_b)):
        c = _corr(feats[0], feats[ids_b[k]], fms[k])
        want = R.refit(c, hom[k], masks[k], nr, thr)
        _same(ref[k], want, (tag, k))
        assert np.array_equal(rmasks[k], want["mask"].astype(bool)), (tag, k)
        assert int(ref[k]["nb_inliers"]) >= int(hom[k]["nb_inliers"]), (tag, k)            # monotone
        assert int(ref[k]["valid"]) == int(hom[k]["valid"]), (tag, k)
        if not int(hom[k]["valid"]):
            assert ref[k].tobytes() == bytes(52) and not rmasks[k].any(), (tag, k)
            continue
        if int(ref[k]["rounds"]) == 0:                                                     # no round accepted: the verification's model and mask
            assert ref[k]["H"].tobytes() == hom[k]["H"].tobytes() and np.array_equal(rmasks[k], masks[k]), (tag, k)
        else:
            assert int(rmasks[k].sum()) == int(ref[k]["nb_inliers"]), (tag, k)
            accepted += 1
        e0, e1 = V.corner_error(hom[k]["H"], Hs[k], W, H), V.corner_error(ref[k]["H"], Hs[k], W, H)
        print(f"{tag} warp {k}: {len(fms[k])} filtered matches; RANSAC {int(hom[k]['nb_inliers'])} inliers, corner error {e0:.3f} px; refined ({int(ref[k]['rounds'])} rounds) "
              f"{int(ref[k]['nb_inliers'])} inliers, corner error {e1:.3f} px")
    return accepted


def test_public_api_equals_the_restatement_leaves_the_rest_alone_and_feeds_guided_matching(vk):
    """the five warps of tests/quality.py in one batched call; the restatement runs on the DOWNLOADED features, filtered matches, RANSAC
    record and mask. Figures (printed; recorded in DESIGN.md section 10.2): inliers and four-corner error of the RANSAC and the refined model,
    after 1024 hypotheses (the setup of tests/test_gpu_verify.py) and after 16 (where the sample is rarely a good one)."""
    imgs, Hs = _pairs(vk)
    ids_a, ids_b = [0] * 5, [1, 2, 3, 4, 5]
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs, 0)
        inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
        inst.verifyHomography(1024, 2.5, 7)
        before = _existing_bytes(inst, 5)
        inst.refineHomography(3, 2.5)
        ref = [inst.getRefinedHomography(k) for k in range(5)]
        rmasks = [inst.downloadRefinedInlierMask(k) for k in range(5)]
        assert _existing_bytes(inst, 5) == before                                   # existing results untouched
        hom = [inst.getHomography(k) for k in range(5)]
        masks = [inst.downloadInlierMask(k) for k in range(5)]
        fms = [inst.downloadFilteredMatches(k) for k in range(5)]
        feats = {i: inst.downloadFeatures(i) for i in range(6)}
        # guided matching under the refined models, handed over through `models`
        own = np.stack([np.asarray(r["H"], np.float32).reshape(9) for r in ref])
        inst.matchFeaturesGuided(G.HOMOGRAPHY, own, 2.5, 0.8, INF, True)
        guided = [inst.downloadGuidedMatches(k) for k in range(5)]
        assert _existing_bytes(inst, 5) == before
        assert _refined_bytes(inst, 5) == b"".join(ref[k].tobytes() + rmasks[k].tobytes() for k in range(5))      # nor the refined ones by the guided matching
        # the same after few hypotheses
        inst.verifyHomography(16, 2.5, 7)
        inst.refineHomography(3, 2.5)
        hom16, masks16 = [inst.getHomography(k) for k in range(5)], [inst.downloadInlierMask(k) for k in range(5)]
        ref16, rmasks16 = [inst.getRefinedHomography(k) for k in range(5)], [inst.downloadRefinedInlierMask(k) for k in range(5)]
    _check_refined(feats, ids_b, fms, hom, masks, ref, rmasks, Hs, 3, 2.5, "1024 hypotheses,")
    accepted16 = _check_refined(feats, ids_b, fms, hom16, masks16, ref16, rmasks16, Hs, 3, 2.5, "16 hypotheses,")
    assert sum(int(h["valid"]) for h in hom) >= 4 and accepted16 >= 1
    for k in range(5):
        if not int(hom[k]["valid"]):
            continue
        # the refined mask is the admissibility guided matching applies to the same model
        fa, fb = feats[0], feats[ids_b[k]]
        if int(ref[k]["rounds"]):
            adm = G.admissible(G.HOMOGRAPHY, own[k], fa["x"], fa["y"], fb["x"], fb["y"], G.threshold2(2.5))
            assert np.array_equal(adm[fms[k]["idx_a"], fms[k]["idx_b"]], rmasks[k]), k
        swept = G.sweep(G.HOMOGRAPHY, own[k], fa["x"], fa["y"], fa["descriptor"], fb["x"], fb["y"], fb["descriptor"], 2.5)
        assert guided[k].tobytes() == G.guided(G.HOMOGRAPHY, None, 1, None, None, None, None, None, None, 2.5, 0.8, INF, True, swept=swept).tobytes(), k
        assert len(guided[k]) > 0.5 * len(fms[k]), k


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
        assert _errors(vk, lambda: inst.refineHomography(3, 2.5)) == bad_input                              # nothing matched yet
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        assert _errors(vk, lambda: inst.refineHomography(3, 2.5)) == bad_input                              # nothing verified yet
        inst.verifyFundamental(256, 2.5, 3)
        assert _errors(vk, lambda: inst.refineHomography(3, 2.5)) == bad_input                              # only the other model has been
        assert _errors(vk, lambda: inst.getRefinedHomography(0)) == bad_input
        inst.verifyHomography(512, 2.5, 11)
        assert _errors(vk, lambda: inst.getRefinedHomography(0)) == bad_input                               # not refined yet
        assert _errors(vk, lambda: inst.downloadRefinedInlierMask(0)) == bad_input
        inst.refineHomography(3, 2.5)
        first = _refined_bytes(inst, 1)
        null_out = lambda: (vk.lib().vksift_ext_getRefinedHomography(inst._h, 0, None), vk._check_pending())
        for bad in (lambda: inst.refineHomography(0, 2.5), lambda: inst.refineHomography(9, 2.5), lambda: inst.refineHomography(3, 0.0),
                    lambda: inst.refineHomography(3, -2.5), lambda: inst.refineHomography(3, float("nan")), lambda: inst.refineHomography(3, INF),
                    lambda: inst.refineHomography(3, 1e-30), lambda: inst.refineHomography(3, 1e30),        # the squared threshold is zero / not finite
                    lambda: inst.getRefinedHomography(1), lambda: inst.downloadRefinedInlierMask(1), null_out):
            assert _errors(vk, bad) == bad_input
            assert _refined_bytes(inst, 1) == first                                                        # nothing changed
        inst.refineHomography(3, 2.5)                                                                      # the same inputs: the same bytes
        assert _refined_bytes(inst, 1) == first
        inst.verifyFundamental(256, 2.5, 4)                                                                # the other model does not invalidate
        assert _refined_bytes(inst, 1) == first
        inst.setProfiling(True)
        assert inst.getRefineTime() == -1.0
        inst.refineHomography(8, 2.5)
        assert 0.0 < inst.getRefineTime() < 1000.0
        r8 = inst.getRefinedHomography(0)
        hom, mask = inst.getHomography(0), inst.downloadInlierMask(0)
        c = _corr(inst.downloadFeatures(0), inst.downloadFeatures(1), inst.downloadFilteredMatches(0))
        _same(r8, R.refit(c, hom, mask, 8, 2.5), "8 rounds")
        inst.verifyHomography(512, 2.5, 12)                                                                # a new verification of the homography does
        assert _errors(vk, lambda: inst.getRefinedHomography(0)) == bad_input
        assert _errors(vk, lambda: inst.downloadRefinedInlierMask(0)) == bad_input
        inst.refineHomography(3, 2.5)
        assert int(inst.getRefinedHomography(0)["valid"]) == 1
        inst.matchFeaturesFiltered([0], [1], 0.8, True)                                                    # a new matching does
        assert _errors(vk, lambda: inst.getRefinedHomography(0)) == bad_input
        assert _errors(vk, lambda: inst.downloadRefinedInlierMask(0)) == bad_input
        assert _errors(vk, lambda: inst.refineHomography(3, 2.5)) == bad_input


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
        inst.verifyHomography(1024, 2.5, 1)
        inst.refineHomography(8, 2.5)
        busy = [inst.isBufferAvailable(i) for i in range(2)]
        ref, rmask = inst.getRefinedHomography(0), inst.downloadRefinedInlierMask(0)
        assert all(inst.isBufferAvailable(i) for i in range(2))            # the accessors have waited for it
        hom, mask = inst.getHomography(0), inst.downloadInlierMask(0)
        c = _corr(inst.downloadFeatures(0), inst.downloadFeatures(1), inst.downloadFilteredMatches(0))
        assert inst.getFeaturesNumber(17) > 100
    assert busy == [False, False]
    want = R.refit(c, hom, mask, 8, 2.5)
    _same(ref, want, "queued")
    assert np.array_equal(rmask, want["mask"].astype(bool))
