"""What the stages behind a filtered matching share on the host (csrc/host/vksift_pairs.c), through the public API: every stage timer follows one rule,
and every per-pair result set follows one invalidation table. One 640x480 pair, small arguments: the kernels are tested elsewhere."""
import numpy as np
import pytest

import np_guided as G
import quality as Q

pytestmark = pytest.mark.gpu

W, H = 640, 480
HYPOTHESES, ROUNDS, THRESHOLD = 256, 3, 2.5


@pytest.fixture(scope="module")
def images(vk):
    base = vk.gen_synthetic_image(33, W, H)
    return [base, Q.warp(base, Q.homography(W, H, **Q.WARPS[0]))]


def _instance(vk, images):
    inst = vk.Instance(vk.default_config(sift_buffer_count=4, input_image_max_size=W * H), batch_capacity=2)
    inst.detectFeaturesBatch(images, 0)
    return inst


# the stages in an order in which each finds what it needs: (name, run, its time getter)
def _stages(inst):
    return [("matching", lambda: inst.matchFeaturesFiltered([0], [1], 0.8, True), inst.getMatchTime),
            ("verification H", lambda: inst.verifyHomography(HYPOTHESES, THRESHOLD, 7), inst.getVerifyTime),
            ("verification F", lambda: inst.verifyFundamental(HYPOTHESES, THRESHOLD, 7), inst.getVerifyTime),
            ("refit H", lambda: inst.refineHomography(ROUNDS, THRESHOLD), inst.getRefineTime),
            ("refit F", lambda: inst.refineFundamental(ROUNDS, THRESHOLD), inst.getRefineFundamentalTime),
            ("guided", lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, None, THRESHOLD, 0.8, float("inf"), True), inst.getGuidedMatchTime),
            # a budget no buffer exceeds: the launch runs and the buffers keep what the other stages matched
            ("budget", lambda: inst.keepStrongestFeatures(0, 2, inst.cfg.max_nb_sift_per_buffer), inst.getKeepStrongestTime)]


def test_every_stage_timer_follows_one_rule(vk, images):
    """-1 until the stage has run with profiling on, its interval afterwards, -1 again after every setProfiling(). On the parent of the change that
    introduced the shared timer the step after the second setProfiling(True) fails for the two refits and the feature budget: their flags survived
    the reset, and the getters reported an interval from before it."""
    with _instance(vk, images) as inst:
        stages = _stages(inst)
        getters = {g.__name__: g for _, _, g in stages}
        assert len(getters) == 6
        times = lambda: {n: g() for n, g in getters.items()}
        assert set(times().values()) == {-1.0}                                     # profiling is off
        inst.setProfiling(True)
        assert set(times().values()) == {-1.0}                                     # nothing has run yet
        for name, run, getter in stages:
            run()
            t = getter()
            print(f"{name}: {t:.4f} ms")
            assert 0.0 < t < 1000.0, name                                          # the verification's after each model
        assert all(0.0 < t < 1000.0 for t in times().values()), times()
        # each stage alone after a reset (the matching last: it takes the others' inputs away)
        for name, run, getter in stages[1:] + stages[:1]:
            inst.setProfiling(True)
            assert set(times().values()) == {-1.0}, (name, times())
            run()
            got = times()
            assert 0.0 < got.pop(getter.__name__) < 1000.0, name
            assert set(got.values()) == {-1.0}, (name, got)
        inst.setProfiling(False)
        assert set(times().values()) == {-1.0}


def _accessors(vk, inst):
    """the twelve per-pair accessors of the C API, each as pair -> bytes (into a zeroed buffer as large as any pair's payload can be)"""
    L, nb = vk.lib(), inst.cfg.max_nb_sift_per_buffer

    def count(fn):
        def get(pair):
            n = fn(inst._h, pair)
            vk._check_pending()
            return int(n).to_bytes(4, "little")
        return get

    def into(fn, nbytes):
        def get(pair):
            out = np.zeros(nbytes, np.uint8)
            fn(inst._h, pair, out.ctypes.data)
            vk._check_pending()
            return out.tobytes()
        return get

    return {"filtered n": count(L.vksift_ext_getFilteredMatchesNumber), "filtered": into(L.vksift_ext_downloadFilteredMatches, 16 * nb),
            "H": into(L.vksift_ext_getHomography, 52), "H mask": into(L.vksift_ext_downloadInlierMask, nb),
            "F": into(L.vksift_ext_getFundamental, 56), "F mask": into(L.vksift_ext_downloadFundamentalInlierMask, nb),
            "refined H": into(L.vksift_ext_getRefinedHomography, 52), "refined H mask": into(L.vksift_ext_downloadRefinedInlierMask, nb),
            "refined F": into(L.vksift_ext_getRefinedFundamental, 52), "refined F mask": into(L.vksift_ext_downloadRefinedFundamentalInlierMask, nb),
            "guided n": count(L.vksift_ext_getGuidedMatchesNumber), "guided": into(L.vksift_ext_downloadGuidedMatches, 16 * nb)}


def test_every_pair_result_set_follows_one_invalidation_table(vk, images):
    """A new matching takes every set's results away (a filtered one brings its own back), a new verification of a model takes that model's refit
    away and nothing else; what is still served is served unchanged; no set serves the pair behind its last."""
    with _instance(vk, images) as inst:
        acc = _accessors(vk, inst)
        assert len(acc) == 12
        fill = [run for _, run, _ in _stages(inst)[:6]]
        events = [("a plain matchFeatures", lambda: inst.matchFeatures(0, 1), set(acc)),
                  ("a new matchFeaturesFiltered", fill[0], set(acc) - {"filtered n", "filtered"}),
                  ("verifyHomography again", fill[1], {"refined H", "refined H mask"}),
                  ("verifyFundamental again", fill[2], {"refined F", "refined F mask"})]
        for what, event, refused in events:
            for run in fill:
                run()
            before = {name: get(0) for name, get in acc.items()}
            assert int.from_bytes(before["filtered n"], "little") > 50 and int.from_bytes(before["guided n"], "little") > 50, before      # not a table of empty results
            assert any(before["H mask"]) and any(before["refined F mask"]) and any(before["refined H"]) and any(before["F"])
            for name, get in acc.items():                                           # pair == slots_used
                with pytest.raises(vk.VksiftError) as e:
                    get(1)
                assert e.value.code == vk.VKSIFT_INVALID_INPUT_ERROR, (what, name)
            event()
            for name, get in acc.items():
                if name in refused:
                    with pytest.raises(vk.VksiftError) as e:
                        get(0)
                    assert e.value.code == vk.VKSIFT_INVALID_INPUT_ERROR, (what, name)
                else:
                    assert get(0) == before[name], (what, name)
