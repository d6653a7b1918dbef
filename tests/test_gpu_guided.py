"""GPU-side guided matching (guided.hip, vksift_ext_matchFeaturesGuided) against its restatement tests/np_guided.py: bit equality of every record and
count — at the kernel level on synthetic slots, through the public API on detected features —, that the verification results are untouched by it,
and the contract of the entry points."""
import numpy as np
import pytest

import np_guided as G
import quality as Q

pytestmark = pytest.mark.gpu

INF = float("inf")
THRESHOLDS = [0.5, 2.5, 1e6]
RATIOS = [0.8, 1.01]
MAX_DISTANCES = [INF, 60.0]        # 60: between the planted pairs' distances (descriptor noise of +-3 per byte) and the look-alikes of the widest threshold


def _model(s, kind):
    return s["H"] if kind == G.HOMOGRAPHY else s["F"]


def _upload(slots):
    import torch

    max_n = max(max(len(s["xa"]), len(s["xb"])) for s in slots)
    k = len(slots)
    da, db = np.zeros((k, max_n, 128), np.uint8), np.zeros((k, max_n, 128), np.uint8)
    xa, xb = np.full((k, max_n, 2), np.nan, np.float32), np.full((k, max_n, 2), np.nan, np.float32)
    n = np.zeros((k, 2), np.int32)
    for i, s in enumerate(slots):
        na, nb = len(s["xa"]), len(s["xb"])
        da[i, :na], db[i, :nb] = s["desc_a"], s["desc_b"]
        xa[i, :na, 0], xa[i, :na, 1], xb[i, :nb, 0], xb[i, :nb, 1] = s["xa"], s["ya"], s["xb"], s["yb"]
        n[i] = na, nb
    t = lambda x: torch.from_numpy(x).cuda()
    return t(da), t(xa), t(db), t(xb), t(n)


def test_kernel_level_every_size_model_threshold_and_decision_is_bit_equal(vk):
    import torch

    slots = G.kernel_test_slots()
    assert float(slots[G.BIG_SLOT]["xa"].max()) == 16383.0
    dev = _upload(slots)
    valid = torch.tensor([s["valid"] for s in slots], dtype=torch.int32).cuda()
    d2 = [G.distances2(s["desc_a"], s["desc_b"]) for s in slots]
    args = [[s[k] for k in ("xa", "ya", "desc_a", "xb", "yb", "desc_b")] for s in slots]
    checked, records, seen, tie_decided, cut_some = 0, 0, set(), 0, 0
    for kind in (G.HOMOGRAPHY, G.FUNDAMENTAL):
        models = torch.from_numpy(np.stack([_model(s, kind) for s in slots])).cuda()
        for thr in THRESHOLDS:
            # what does not depend on the decision is restated once per (model, threshold, slot)
            swept = [G.sweep(kind, _model(s, kind), *args[i], thr, d2=d2[i]) for i, s in enumerate(slots)]
            for sw in swept:
                seen |= set(np.minimum(sw[2].sum(axis=1), 3).tolist())
            for cc in (False, True):
                for ratio in RATIOS:
                    for md in MAX_DISTANCES:
                        err, got = vk.guided_match(*dev, models, valid, kind, float(G.threshold2(thr)), ratio, md, cc)
                        assert err == 0
                        for i, s in enumerate(slots):
                            want = G.guided(kind, None, s["valid"], *args[i], thr, ratio, md, cc, swept=swept[i])
                            ctx = (kind, thr, cc, ratio, md, G.SLOT_SIZES[i])
                            assert len(got[i]) == len(want), ctx
                            assert got[i].tobytes() == want.tobytes(), ctx
                            checked += 1
                            records += len(want)
                            tie_decided += int((want["dist_a_b1"] == want["dist_a_b2"]).sum())
                            if md != INF and s["valid"]:
                                free = len(G.guided(kind, None, 1, *args[i], thr, ratio, INF, cc, swept=swept[i]))
                                cut_some += 0 < len(want) < free
    assert checked == 2 * len(THRESHOLDS) * 2 * len(RATIOS) * len(MAX_DISTANCES) * len(slots)     # no case left out
    print(f"{checked} cases, {records} records, {tie_decided} matches decided by the tie rule, max_distance cut some matches of {cut_some} cases")
    assert seen == {0, 1, 2, 3}            # rows with 0, 1, 2 and more than 2 admissible candidates
    assert tie_decided > 0
    assert cut_some > 0                    # the finite max_distance removes some matches but not all
    assert records > 10000


def test_kernel_level_refusals_launch_nothing(vk):
    import torch

    s = G.slot_case(50, 60, 1)
    dev = _upload([s])
    models = torch.from_numpy(s["F"][None]).cuda()
    valid = torch.ones(1, dtype=torch.int32).cuda()
    t2 = float(G.threshold2(2.5))

    def run(kind=G.FUNDAMENTAL, t2=t2, ratio=0.8, md=INF, **kw):
        """the error code of a call that must be refused; everything the launches would write is still as it was handed over"""
        written = {}
        err, got = vk.guided_match(*dev, models, valid, kind, t2, ratio, md, True, buffers=written, **kw)
        assert got is None and sorted(written) == ["out", "out_n", "scratch"]
        for name, t in written.items():
            assert bool((t == -1).all()), name
        return err

    assert run(kind=2) != 0
    for bad in (0.0, -1.0, float("nan"), INF):
        assert run(t2=bad) != 0
    for bad in (0.0, -0.5, float("nan")):
        assert run(ratio=bad) != 0
        assert run(md=bad) != 0
    need = vk.lib().vksift_hip_guided_scratch_u32(1, 60)
    assert need > 0 and run(scratch_u32=need - 1) != 0
    for name, ok in (("desc", 60 * 128), ("norm", 60), ("xy", 60), ("out", 60 * 16)):
        assert run(strides={name: ok - 16}) != 0
    written = {}
    err, got = vk.guided_match(*dev, models, valid, G.FUNDAMENTAL, t2, 0.8, INF, True, buffers=written)            # admitted: the same inputs
    assert err == 0 and len(got[0]) > 10
    assert all(bool((t != -1).any()) for t in written.values())                                    # and then they are written


# ---- through the public API ------------------------------------------------------------------------------------------------------------
W, H = 640, 480
KINDS = [(G.HOMOGRAPHY, "H"), (G.FUNDAMENTAL, "F")]


def _pairs(vk, seed=33):
    base = vk.gen_synthetic_image(seed, W, H)
    Hs = [Q.homography(W, H, **kw) for kw in Q.WARPS]
    return [base] + [Q.warp(base, Ht) for Ht in Hs], Hs


_D2 = {}


def _restate(feats, ids_a, ids_b, k, kind, model, valid, thr, ratio, md, cc):
    fa, fb = feats[ids_a[k]], feats[ids_b[k]]
    key = (fa["descriptor"].tobytes(), fb["descriptor"].tobytes())
    if key not in _D2:                      # the distances of a pair serve every model and decision
        _D2.clear()
        _D2[key] = G.distances2(fa["descriptor"], fb["descriptor"])
    swept = G.sweep(kind, np.asarray(model, np.float32).reshape(9), fa["x"], fa["y"], fa["descriptor"], fb["x"], fb["y"], fb["descriptor"], thr, d2=_D2[key])
    return G.guided(kind, None, valid, None, None, None, None, None, None, thr, ratio, md, cc, swept=swept)


def _verification_bytes(inst, n):
    out = b""
    for k in range(n):
        out += inst.getHomography(k).tobytes() + inst.downloadInlierMask(k).tobytes() + inst.getFundamental(k).tobytes()
        out += inst.downloadFundamentalInlierMask(k).tobytes() + inst.downloadFilteredMatches(k).tobytes()
    return out


def _guided_all(inst, n):
    return [inst.downloadGuidedMatches(k) for k in range(n)]


def _verified_models(inst, n):
    return {G.HOMOGRAPHY: [inst.getHomography(k) for k in range(n)], G.FUNDAMENTAL: [inst.getFundamental(k) for k in range(n)]}


def _check_both_kinds(inst, feats, ids_a, ids_b, thr=2.5, ratio=0.8, md=INF, cc=True):
    n = len(ids_a)
    ver = _verified_models(inst, n)
    out = {}
    for kind, name in KINDS:
        inst.matchFeaturesGuided(kind, None, thr, ratio, md, cc)
        got = _guided_all(inst, n)
        for k in range(n):
            want = _restate(feats, ids_a, ids_b, k, kind, ver[kind][k][name], int(ver[kind][k]["valid"]), thr, ratio, md, cc)
            assert got[k].tobytes() == want.tobytes(), (name, k, len(got[k]), len(want))
        out[kind] = got
    return ver, out


def test_public_api_warps_equal_the_restatement_and_leave_the_verification_alone(vk):
    imgs, Hs = _pairs(vk)
    ids_a, ids_b = [0] * 5, [1, 2, 3, 4, 5]
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs, 0)
        inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
        inst.verifyHomography(1024, 2.5, 7)
        inst.verifyFundamental(1024, 2.5, 7)
        before = _verification_bytes(inst, 5)
        feats = {i: inst.downloadFeatures(i) for i in range(6)}
        fms = [inst.downloadFilteredMatches(k) for k in range(5)]
        ver, got = _check_both_kinds(inst, feats, ids_a, ids_b)
        assert _verification_bytes(inst, 5) == before
        # the caller's own models: the verified ones perturbed
        for kind, name in KINDS:
            own = np.stack([np.asarray(ver[kind][k][name], np.float32).reshape(9) for k in range(5)])
            own = (own * np.float32(1.0 + 1e-4) + np.float32(1e-7)).astype(np.float32)
            own[~np.isfinite(own)] = 0
            inst.matchFeaturesGuided(kind, own, 2.5, 0.8, INF, True)
            for k in range(5):
                want = _restate(feats, ids_a, ids_b, k, kind, own[k], 1, 2.5, 0.8, INF, True)
                assert inst.downloadGuidedMatches(k).tobytes() == want.tobytes(), (name, k)
        assert _verification_bytes(inst, 5) == before

    def close(fa, fb, m, Ht):
        p = Ht @ np.stack([fa["x"][m["idx_a"]], fa["y"][m["idx_a"]], np.ones(len(m))]).astype(np.float64)
        return int((np.hypot(p[0] / p[2] - fb["x"][m["idx_b"]], p[1] / p[2] - fb["y"][m["idx_b"]]) < 3.0).sum())

    for k in range(5):
        g, f = close(feats[0], feats[k + 1], got[G.HOMOGRAPHY][k], Hs[k]), close(feats[0], feats[k + 1], fms[k], Hs[k])
        print(f"warp {k}: within 3 px of the true warp: {g} of {len(got[G.HOMOGRAPHY][k])} guided matches (H), {f} of {len(fms[k])} filtered matches; "
              f"{len(got[G.FUNDAMENTAL][k])} guided matches (F)")
        if int(ver[G.HOMOGRAPHY][k]["valid"]):
            assert g >= f, k
    assert sum(int(v["valid"]) for v in ver[G.HOMOGRAPHY]) >= 4


def test_clamped_sections_and_an_uploaded_buffer(vk):
    """a small max_nb_sift_per_buffer clamps the sections of every buffer, and one side of a pair is an uploaded buffer (one dense section): the rows
    and coordinates the launches resolve are the rows vksift_downloadFeatures returns"""
    imgs, _ = _pairs(vk, seed=35)
    cfg = vk.default_config(sift_buffer_count=8, input_image_max_size=W * H, max_nb_sift_per_buffer=600)
    with vk.Instance(cfg, batch_capacity=6) as inst:
        inst.detectFeaturesBatch(imgs[:3], 0)
        f1 = inst.downloadFeatures(1)
        inst.uploadFeatures(f1[::-1][:500].copy(), 5)              # another order and length than any detected buffer
        ids_a, ids_b = [0, 0, 5, 2], [1, 5, 0, 5]
        inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
        inst.verifyHomography(256, 2.5, 3)
        inst.verifyFundamental(256, 2.5, 3)
        feats = {i: inst.downloadFeatures(i) for i in (0, 1, 2, 5)}
        assert len(feats[0]) <= 600 and len(feats[5]) == 500
        _, got = _check_both_kinds(inst, feats, ids_a, ids_b, ratio=0.9, cc=False)
        assert min(len(g) for g in got[G.HOMOGRAPHY][:3]) >= 8


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def test_contract_errors_invalidation_and_timing(vk):
    imgs, _ = _pairs(vk, seed=36)
    cfg = vk.default_config(sift_buffer_count=4, input_image_max_size=W * H)
    ident = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1]], np.float32)
    bad_input = vk.VKSIFT_INVALID_INPUT_ERROR
    with vk.Instance(cfg, batch_capacity=2) as inst:
        inst.detectFeaturesBatch(imgs[:2], 0)
        assert _errors(vk, lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, ident)) == bad_input             # nothing matched yet
        inst.matchFeatures(0, 1)
        assert _errors(vk, lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, ident)) == bad_input             # a plain matching: nothing filtered
        inst.matchFeaturesFiltered([0], [1], 0.8, True)
        assert _errors(vk, lambda: inst.downloadGuidedMatches(0)) == bad_input                             # no guided matching yet
        assert _errors(vk, lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY)) == bad_input                    # that model has not been verified
        inst.verifyHomography(512, 2.5, 11)
        assert _errors(vk, lambda: inst.matchFeaturesGuided(G.FUNDAMENTAL)) == bad_input                   # only the other one has
        inst.matchFeaturesGuided(G.HOMOGRAPHY)
        assert inst.getGuidedMatchTime() == -1.0                                                           # profiling is off
        inst.setProfiling(True)
        assert inst.getGuidedMatchTime() == -1.0                                                           # on, but that run was not timed
        inst.matchFeaturesGuided(G.HOMOGRAPHY)
        assert 0.0 < inst.getGuidedMatchTime() < 1000.0
        first = inst.downloadGuidedMatches(0).tobytes()
        assert len(first) > 16 * 50
        nan_model, inf_model = ident.copy(), ident.copy()
        nan_model[0, 4], inf_model[0, 8] = np.nan, np.inf
        for bad in (lambda: inst.matchFeaturesGuided(2), lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, 0.0), lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, -2.5),
                    lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, float("nan")), lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, INF),
                    lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, 2.5, 0.0), lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, 2.5, float("nan")),
                    lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, 2.5, 0.8, 0.0), lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, 2.5, 0.8, float("nan")),
                    lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, nan_model), lambda: inst.matchFeaturesGuided(G.FUNDAMENTAL, inf_model),
                    lambda: inst.downloadGuidedMatches(1)):
            assert _errors(vk, bad) == bad_input
            assert inst.downloadGuidedMatches(0).tobytes() == first                                        # nothing changed
        inst.matchFeaturesGuided(G.HOMOGRAPHY)                                                             # the same inputs: the same bytes
        assert inst.downloadGuidedMatches(0).tobytes() == first
        inst.matchFeaturesGuided(G.HOMOGRAPHY, None, 2.5, 0.8, INF, False)                                 # a second run replaces the results
        feats = {i: inst.downloadFeatures(i) for i in (0, 1)}
        hom = inst.getHomography(0)
        want = _restate(feats, [0], [1], 0, G.HOMOGRAPHY, hom["H"], int(hom["valid"]), 2.5, 0.8, INF, False)
        second = inst.downloadGuidedMatches(0).tobytes()
        assert second == want.tobytes() and second != first
        inst.matchFeaturesGuided(G.FUNDAMENTAL, ident, 2.5, 0.8, 200.0, True)                              # a supplied model needs no verification of its kind
        want = _restate(feats, [0], [1], 0, G.FUNDAMENTAL, ident, 1, 2.5, 0.8, 200.0, True)
        assert inst.downloadGuidedMatches(0).tobytes() == want.tobytes()
        inst.matchFeatures(0, 1)                                                                           # a new matching invalidates the results
        assert _errors(vk, lambda: inst.downloadGuidedMatches(0)) == bad_input
        inst.matchFeaturesFiltered([0], [1], 0.8, True)                                                    # and a filtered one too, until run again
        assert _errors(vk, lambda: inst.downloadGuidedMatches(0)) == bad_input
        inst.verifyHomography(512, 2.5, 11)
        inst.matchFeaturesGuided(G.HOMOGRAPHY)
        assert inst.downloadGuidedMatches(0).tobytes() == first


def test_asynchronous_use_with_a_second_buffer_set(vk):
    """guided matching queued, the next detection queued into a second buffer set before anything is read: the results are the first set's, and its
    buffers stay busy until the guided matching has passed"""
    imgs, _ = _pairs(vk, seed=37)
    other = [vk.gen_synthetic_image(900 + i, W, H) for i in range(3)]
    cfg = vk.default_config(sift_buffer_count=6, input_image_max_size=W * H)
    ids_a, ids_b = [0, 0], [1, 2]
    with vk.Instance(cfg, batch_capacity=3) as inst:
        inst.detectFeaturesBatch(imgs[:3], 0)
        inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
        inst.verifyFundamental(1024, 2.5, 5)
        inst.matchFeaturesGuided(G.FUNDAMENTAL)
        inst.detectFeaturesBatch(other, 3)
        busy = [inst.isBufferAvailable(i) for i in range(3)]                # False while the guided matching runs; True once it has passed
        got = _guided_all(inst, 2)
        assert all(inst.isBufferAvailable(i) for i in range(3))            # the accessors have waited for it
        fun = [inst.getFundamental(k) for k in range(2)]
        feats = {i: inst.downloadFeatures(i) for i in range(3)}
        later = inst.downloadFeatures(4)
    assert len(busy) == 3 and len(later) > 100
    for k in range(2):
        want = _restate(feats, ids_a, ids_b, k, G.FUNDAMENTAL, fun[k]["F"], int(fun[k]["valid"]), 2.5, 0.8, INF, True)
        assert got[k].tobytes() == want.tobytes() and len(want) > 50, k
