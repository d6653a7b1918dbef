"""Track observations through the public API (vksift_ext_selectTrackObservations and its accessors) against the restatement tests/np_observations.py,
which is fed with downloadTracks, downloadFeatureTracks and downloadFeatures of the same instance: byte equality of the statistics, the offsets, the
track ids and the observations for tracks from each of the six sources; x, y bit-equal to the downloaded features; the tracks, the per-feature words
and the filtered matches byte-identical before and after; the lifetime of the results; and every refusal, with the earlier observations compared byte
for byte. Fixture: the six views of tests/track_scene.py in SIFT buffers that are not contiguous — the sixth uploaded (a dense buffer) — all 15 pairs
and a pair of a buffer with itself in one filtered matching."""
import numpy as np
import pytest

import np_observations as NO
import track_scene as S

pytestmark = pytest.mark.gpu

BUFS = [1, 2, 3, 9, 10, 12]        # view i lives in SIFT buffer BUFS[i]; view 5 is detected into buffer 11, downloaded and uploaded into 12
IDS_A, IDS_B = [BUFS[a] for a in S.IDS_A] + [BUFS[0]], [BUFS[b] for b in S.IDS_B] + [BUFS[0]]
NP = len(IDS_A)


def _instance(vk):
    cfg = vk.default_config(sift_buffer_count=16, input_image_max_size=192 * 144)
    return vk.Instance(cfg, batch_capacity=NP)


def _detect(vk, inst):
    imgs = S.images(vk.gen_synthetic_image_family)
    inst.detectFeaturesBatch(imgs[:3], BUFS[0])
    inst.detectFeaturesBatch(imgs[3:], BUFS[3])          # views 3, 4, 5 into buffers 9, 10, 11
    inst.uploadFeatures(inst.downloadFeatures(11), BUFS[5])


def _match(inst):
    inst.matchFeaturesFiltered(IDS_A, IDS_B, 0.8, True)


SOURCES = ("filtered", "verified_h", "verified_f", "refined_h", "refined_f", "guided")


def _read(inst):
    return inst.getObservationStats(), inst.downloadObservationOffsets(), inst.downloadObservationTrackIds(), inst.downloadObservations()


def _bytes(got):
    stats, offsets, ids, obs = got
    return repr(sorted(stats.items())).encode() + offsets.tobytes() + ids.tobytes() + obs.tobytes()


def _inputs(inst):
    """what the restatement is fed with, and the bytes that must not change"""
    rec, words, feats = inst.downloadTracks(), {b: inst.downloadFeatureTracks(b) for b in BUFS}, {b: inst.downloadFeatures(b) for b in BUFS}
    same = rec.tobytes() + b"".join(words[b].tobytes() for b in BUFS) + repr(sorted(inst.getTrackStats().items())).encode()
    same += b"".join(inst.downloadFilteredMatches(k).tobytes() for k in range(NP))
    return rec, words, feats, same


def _check(inst, params):
    rec, words, feats, before = _inputs(inst)
    inst.selectTrackObservations(*params)
    got = _read(inst)
    stats, offsets, ids, obs = got
    xy = {b: np.stack([feats[b]["x"], feats[b]["y"]], axis=1) for b in BUFS}
    want = NO.select(rec, words, xy, *params)
    print(params, stats)
    assert stats == want[0], params
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), params
    assert _inputs(inst)[3] == before, params
    # the invariants of the header, on the library's own outputs
    assert stats["nb_tracks"] + stats["nb_rejected_length"] + stats["nb_rejected_conflicting"] == len(rec)
    assert offsets[0] == 0 and offsets[-1] == len(obs) == stats["nb_observations"] and len(offsets) == len(ids) + 1
    assert np.all(np.diff(ids.astype(np.int64)) > 0) and np.array_equal(np.diff(offsets), rec["length"][ids])
    for m, t in enumerate(ids):
        o = obs[offsets[m]:offsets[m + 1]]
        key = o["gpu_buffer_id"].astype(np.int64) << 32 | o["row"]
        assert np.all(np.diff(key) > 0) and (int(o[0]["gpu_buffer_id"]), int(o[0]["row"])) == (int(rec[t]["gpu_buffer_id"]), int(rec[t]["row"]))
    for b in BUFS:        # x, y bit for bit
        o = obs[obs["gpu_buffer_id"] == b]
        assert np.array_equal(o["x"].view(np.uint32), feats[b]["x"][o["row"]].view(np.uint32)) and np.array_equal(o["y"].view(np.uint32), feats[b]["y"][o["row"]].view(np.uint32))
    return got


def test_every_source_equals_the_restatement_and_leaves_its_inputs_alone(vk):
    with _instance(vk) as inst:
        _detect(vk, inst)
        _match(inst)
        inst.verifyHomography(1024, 2.5, 7)
        inst.refineHomography(3, 2.5)
        inst.verifyFundamental(1024, 2.5, 7)
        inst.refineFundamental(3, 2.5)
        inst.matchFeaturesGuided(vk.GUIDE_HOMOGRAPHY)
        seen = dict.fromkeys(NO.STATS, 0)
        for source in SOURCES:
            inst.buildTracks(getattr(vk, "TRACKS_" + source.upper()))
            for params in ((2, 0, vk.OBS_KEEP_CONFLICTING), (3, 0, vk.OBS_DROP_CONFLICTING)) + (((2, 2, vk.OBS_DROP_CONFLICTING), (2, 3, vk.OBS_KEEP_CONFLICTING)) if source == "filtered" else ()):
                stats = _check(inst, params)[0]
                for k in NO.STATS:
                    seen[k] += stats[k]
        # the fixture's precondition: an empty table cannot pass (whether the scene has conflicting tracks is the matcher's business: printed)
        print(seen)
        assert seen["nb_tracks"] and seen["nb_observations"] and seen["nb_rejected_length"], seen
        assert inst.getFeaturesNumber(BUFS[5]) == inst.getFeaturesNumber(11) > 0


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def _null(vk, inst, name):
    """the C entry with a NULL output pointer"""
    def call():
        getattr(vk.lib(), name)(inst._h, None)
        vk._check_pending()
    return call


def test_lifetime_refusals_and_timing(vk):
    bad = vk.VKSIFT_INVALID_INPUT_ERROR
    with _instance(vk) as inst:
        _detect(vk, inst)
        accessors = (inst.getObservationStats, inst.downloadObservationOffsets, inst.downloadObservationTrackIds, inst.downloadObservations)
        select = lambda: inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)
        assert _errors(vk, select) == bad                                   # nothing matched yet
        _match(inst)
        assert _errors(vk, select) == bad                                   # no tracks built for the present matching
        for fn in accessors:
            assert _errors(vk, fn) == bad                                   # an accessor before any selection
        inst.buildTracks(vk.TRACKS_FILTERED)
        for fn in accessors:
            assert _errors(vk, fn) == bad                                   # still no selection
        first = _bytes(_check(inst, (2, 0, vk.OBS_KEEP_CONFLICTING)))
        assert inst.getObservationsTime() == -1.0                           # profiling is off
        assert _bytes(_check(inst, (2, 0, vk.OBS_KEEP_CONFLICTING))) == first          # the same inputs: the same bytes
        held = _bytes(_check(inst, (3, 0, vk.OBS_DROP_CONFLICTING)))        # a second selection replaces the first
        assert held != first
        refused = [lambda: inst.selectTrackObservations(1, 0, 0), lambda: inst.selectTrackObservations(0, 0, 0), lambda: inst.selectTrackObservations(3, 2, 0),
                   lambda: inst.selectTrackObservations(2, 0, 2), lambda: inst.selectTrackObservations(2, 0, 0xFFFFFFFF),
                   _null(vk, inst, "vksift_ext_getObservationStats"), _null(vk, inst, "vksift_ext_downloadObservationOffsets"),
                   _null(vk, inst, "vksift_ext_downloadObservationTrackIds"), _null(vk, inst, "vksift_ext_downloadObservations")]
        for fn in refused:
            assert _errors(vk, fn) == bad
            assert _bytes(_read(inst)) == held                              # earlier observations served, untouched
        inst.setProfiling(True)
        assert inst.getObservationsTime() == -1.0                           # on, but that run was not timed
        assert _bytes(_check(inst, (2, 0, vk.OBS_KEEP_CONFLICTING))) == first
        assert 0.0 < inst.getObservationsTime() < 1000.0
        inst.buildTracks(vk.TRACKS_FILTERED)                                # a new build: refused until selected again
        for fn in accessors:
            assert _errors(vk, fn) == bad
        assert _bytes(_check(inst, (2, 0, vk.OBS_KEEP_CONFLICTING))) == first
        inst.matchFeatures(BUFS[0], BUFS[1])                                # a new plain matching: no tracks, no observations
        for fn in accessors + (select,):
            assert _errors(vk, fn) == bad
        _match(inst)                                                        # a new filtered matching as well
        for fn in accessors + (select,):
            assert _errors(vk, fn) == bad
        inst.buildTracks(vk.TRACKS_FILTERED)
        assert _bytes(_check(inst, (2, 0, vk.OBS_KEEP_CONFLICTING))) == first          # the same matching again: the first observations again
