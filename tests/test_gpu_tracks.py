"""Feature tracks through the public API (vksift_ext_buildTracks and its accessors) against the restatement tests/np_tracks.py, which is fed from the
downloads of the public pair accessors: byte equality of the statistics, the track records and every buffer's per-feature words for every source; the
invariants that tie the three outputs together; the lifetime of the results; and every refusal, with the earlier tracks compared byte for byte.
Fixture: tests/track_scene.py, six overlapping views in SIFT buffers that are not contiguous, all 15 pairs in one filtered matching."""
import numpy as np
import pytest

import np_tracks as NT
import track_scene as S

pytestmark = pytest.mark.gpu

BUFS = [1, 2, 3, 9, 10, 11]        # view i lives in SIFT buffer BUFS[i]
IDS_A, IDS_B = [BUFS[a] for a in S.IDS_A], [BUFS[b] for b in S.IDS_B]
NP = len(S.PAIRS)


def _instance(vk):
    cfg = vk.default_config(sift_buffer_count=16, input_image_max_size=192 * 144)
    return vk.Instance(cfg, batch_capacity=15)


def _detect_and_match(vk, inst):
    imgs = S.images(vk.gen_synthetic_image_family)
    inst.detectFeaturesBatch(imgs[:3], BUFS[0])
    inst.detectFeaturesBatch(imgs[3:], BUFS[3])
    inst.matchFeaturesFiltered(IDS_A, IDS_B, 0.8, True)


SOURCES = {
    "filtered": lambda vk: vk.TRACKS_FILTERED, "verified_h": lambda vk: vk.TRACKS_VERIFIED_H, "verified_f": lambda vk: vk.TRACKS_VERIFIED_F,
    "refined_h": lambda vk: vk.TRACKS_REFINED_H, "refined_f": lambda vk: vk.TRACKS_REFINED_F, "guided": lambda vk: vk.TRACKS_GUIDED,
}


def _edges(inst, source, k):
    """the edges of pair k as the header defines them, from the public accessors"""
    if source == "guided":
        return NT.pair_edges(inst.downloadGuidedMatches(k))
    fm = inst.downloadFilteredMatches(k)
    if source == "filtered":
        return NT.pair_edges(fm)
    rec, mask = {"verified_h": (inst.getHomography, inst.downloadInlierMask), "verified_f": (inst.getFundamental, inst.downloadFundamentalInlierMask),
                 "refined_h": (inst.getRefinedHomography, inst.downloadRefinedInlierMask),
                 "refined_f": (inst.getRefinedFundamental, inst.downloadRefinedFundamentalInlierMask)}[source]
    return NT.pair_edges(fm, mask(k), bool(int(rec(k)["valid"])))


def _restate(inst, source):
    rows = {b: inst.getFeaturesNumber(b) for b in BUFS}
    return NT.build(rows, [(IDS_A[k], IDS_B[k], _edges(inst, source, k)) for k in range(NP)])


def _read(inst):
    """(stats, records, {buffer: words}) of the tracks the instance holds"""
    return inst.getTrackStats(), inst.downloadTracks(), {b: inst.downloadFeatureTracks(b) for b in BUFS}


def _bytes(got):
    stats, rec, words = got
    return repr(sorted(stats.items())).encode() + rec.tobytes() + b"".join(words[b].tobytes() for b in BUFS)


def _check(vk, inst, source):
    inst.buildTracks(SOURCES[source](vk))
    got = _read(inst)
    stats, rec, words = got
    want_rec, want_words, want_stats = _restate(inst, source)
    print(source, stats, "lengths", np.bincount(rec["length"]).tolist() if len(rec) else [])
    assert stats == want_stats, source
    assert rec.tobytes() == want_rec.tobytes(), source
    for b in BUFS:
        assert words[b].tobytes() == want_words[b].tobytes(), (source, b)
    # the invariants that tie the outputs together, on the library's own outputs
    assert int(rec["length"].sum()) == stats["nb_features"] and len(rec) == stats["nb_tracks"]
    assert int((rec["length"] > rec["nb_buffers"]).sum()) == stats["nb_conflicting"]
    length, bufs_seen, first = np.zeros(len(rec), np.int64), [set() for _ in rec], {}
    for b in BUFS:
        for row in np.flatnonzero(words[b] != vk.NO_TRACK):
            t = int(words[b][row])
            assert t < len(rec)
            length[t] += 1
            bufs_seen[t].add(b)
            first.setdefault(t, (b, int(row)))
    assert length.tolist() == rec["length"].tolist() and [len(s) for s in bufs_seen] == rec["nb_buffers"].tolist()
    assert [first[t] for t in range(len(rec))] == [(int(r["gpu_buffer_id"]), int(r["row"])) for r in rec]
    assert sorted(first.values()) == [first[t] for t in range(len(rec))]       # numbered in the order of the smallest member
    return got


def _pair_bytes(inst, fundamental):
    out = b""
    for k in range(NP):
        out += inst.downloadFilteredMatches(k).tobytes() + inst.getHomography(k).tobytes() + inst.downloadInlierMask(k).tobytes()
        out += inst.getRefinedHomography(k).tobytes() + inst.downloadRefinedInlierMask(k).tobytes() + inst.downloadGuidedMatches(k).tobytes()
        if fundamental:
            out += inst.getFundamental(k).tobytes() + inst.downloadFundamentalInlierMask(k).tobytes()
            out += inst.getRefinedFundamental(k).tobytes() + inst.downloadRefinedFundamentalInlierMask(k).tobytes()
    return out


def test_every_source_equals_the_restatement_and_leaves_the_pair_results_alone(vk):
    with _instance(vk) as inst:
        _detect_and_match(vk, inst)
        inst.verifyHomography(1024, 2.5, 7)
        inst.refineHomography(3, 2.5)
        inst.matchFeaturesGuided(vk.GUIDE_HOMOGRAPHY)
        before = _pair_bytes(inst, False)
        got = {s: _check(vk, inst, s) for s in ("filtered", "verified_h", "refined_h", "guided")}
        assert _pair_bytes(inst, False) == before
        # the fixture's precondition: an empty graph cannot pass
        stats, rec, _ = got["filtered"]
        assert stats["nb_tracks"] > 0 and int(rec["length"].max()) >= 3 and stats["nb_edges"] == sum(len(inst.downloadFilteredMatches(k)) for k in range(NP))
        assert got["verified_h"][0]["nb_edges"] == sum(int(inst.getHomography(k)["nb_inliers"]) for k in range(NP)) > 0
        assert got["guided"][0]["nb_tracks"] > 0
        # the F sources: one run each
        inst.verifyFundamental(1024, 2.5, 7)
        inst.refineFundamental(3, 2.5)
        before = _pair_bytes(inst, True)
        for s in ("verified_f", "refined_f"):
            stats, _, _ = _check(vk, inst, s)
            assert stats["nb_tracks"] > 0
        assert _pair_bytes(inst, True) == before


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def _null(vk, inst, name, *args):
    """the C entry with a NULL output pointer"""
    def call():
        getattr(vk.lib(), name)(inst._h, *args, None)
        vk._check_pending()
    return call


def test_lifetime_and_timing(vk):
    bad = vk.VKSIFT_INVALID_INPUT_ERROR
    with _instance(vk) as inst:
        _detect_and_match(vk, inst)
        inst.verifyHomography(1024, 2.5, 7)
        inst.buildTracks(vk.TRACKS_FILTERED)
        assert inst.getTracksTime() == -1.0                              # profiling is off
        first = _bytes(_read(inst))
        inst.buildTracks(vk.TRACKS_FILTERED)                             # the same inputs: the same bytes
        assert _bytes(_read(inst)) == first
        second = _bytes(_check(vk, inst, "verified_h"))                  # a second build replaces the first
        assert second != first
        inst.verifyHomography(64, 0.5, 99)                               # a re-verification after a build does not touch the tracks built
        inst.refineHomography(2, 0.5)
        assert _bytes(_read(inst)) == second
        inst.setProfiling(True)
        assert inst.getTracksTime() == -1.0                              # on, but that run was not timed
        assert _bytes(_check(vk, inst, "verified_h")) != second          # built again: the new masks
        assert 0.0 < inst.getTracksTime() < 1000.0
        accessors = (inst.getTrackStats, inst.downloadTracks, lambda: inst.downloadFeatureTracks(BUFS[0], 1))
        inst.matchFeatures(BUFS[0], BUFS[1])                             # a new plain matching: every tracks accessor is an error
        for fn in accessors:
            assert _errors(vk, fn) == bad
        inst.matchFeaturesFiltered(IDS_A, IDS_B, 0.8, True)
        inst.buildTracks(vk.TRACKS_FILTERED)
        assert _bytes(_read(inst)) == first                              # the same matching again: the first tracks again
        inst.matchFeaturesFiltered(IDS_A, IDS_B, 0.8, True)              # a new filtered matching invalidates them as well
        for fn in accessors:
            assert _errors(vk, fn) == bad
        assert _bytes(_check(vk, inst, "filtered")) == first


def test_refusals_queue_nothing_and_leave_the_earlier_tracks_alone(vk):
    bad = vk.VKSIFT_INVALID_INPUT_ERROR
    with _instance(vk) as inst:
        imgs = S.images(vk.gen_synthetic_image_family)
        inst.detectFeaturesBatch(imgs[:3], BUFS[0])
        inst.detectFeaturesBatch(imgs[3:], BUFS[3])
        assert _errors(vk, lambda: inst.buildTracks(vk.TRACKS_FILTERED)) == bad                 # nothing matched yet
        assert _errors(vk, inst.getTrackStats) == bad                                           # an accessor before any build
        inst.matchFeatures(BUFS[0], BUFS[1])
        assert _errors(vk, lambda: inst.buildTracks(vk.TRACKS_FILTERED)) == bad                 # a plain matching: nothing filtered
        inst.matchFeaturesFiltered(IDS_A, IDS_B, 0.8, True)
        for fn in (inst.getTrackStats, inst.downloadTracks, lambda: inst.downloadFeatureTracks(BUFS[0], 1)):
            assert _errors(vk, fn) == bad                                                       # still no build
        for src in (vk.TRACKS_VERIFIED_H, vk.TRACKS_VERIFIED_F, vk.TRACKS_REFINED_H, vk.TRACKS_REFINED_F, vk.TRACKS_GUIDED):
            assert _errors(vk, lambda: inst.buildTracks(src)) == bad                            # that stage has not been run
        inst.verifyHomography(512, 2.5, 11)
        inst.buildTracks(vk.TRACKS_VERIFIED_H)
        held = _bytes(_read(inst))
        refused = [lambda: inst.buildTracks(6), lambda: inst.buildTracks(0xFFFFFFFF), lambda: inst.buildTracks(vk.TRACKS_VERIFIED_F),
                   lambda: inst.buildTracks(vk.TRACKS_REFINED_H), lambda: inst.buildTracks(vk.TRACKS_GUIDED),
                   _null(vk, inst, "vksift_ext_getTrackStats"), _null(vk, inst, "vksift_ext_downloadTracks"), _null(vk, inst, "vksift_ext_downloadFeatureTracks", BUFS[0]),
                   lambda: inst.downloadFeatureTracks(0, 1), lambda: inst.downloadFeatureTracks(5, 1), lambda: inst.downloadFeatureTracks(15, 1),
                   lambda: inst.downloadFeatureTracks(16, 1), lambda: inst.downloadFeatureTracks(0xFFFFFFFF, 1)]
        for fn in refused:
            assert _errors(vk, fn) == bad
            assert _bytes(_read(inst)) == held                                                  # earlier tracks untouched
        # a stage run for an earlier matching is not a stage run for the present one
        inst.matchFeaturesFiltered(IDS_A, IDS_B, 0.8, True)
        assert _errors(vk, lambda: inst.buildTracks(vk.TRACKS_VERIFIED_H)) == bad
        assert _errors(vk, inst.getTrackStats) == bad
        inst.buildTracks(vk.TRACKS_FILTERED)
        assert inst.getTrackStats()["nb_tracks"] > 0
