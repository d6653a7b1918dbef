"""Triangulation through the public API (vksift_ext_triangulateTracks and its accessors) against the restatement tests/np_triangulate.py, which is fed
with downloadObservationOffsets and downloadObservations of the same instance: byte equality of the statistics and the points for tracks from two sources
under both conflict policies; the tracks, the observations and the filtered matches byte-identical before and after; the lifetime of the results; and
every refusal, with the earlier points compared byte for byte. Fixture: the six views of tests/track_scene.py, which are exact perspective views of the
plane Z = 256 — view v, the crop at (x0, y0), has the camera P_v = [[256, 0, 0, -256 x0], [0, 256, 0, -256 y0], [0, 0, 1, 0]] — in SIFT buffers that are
not contiguous; the cameras of every other buffer are NaN, which only a camera that is read may not be."""
import numpy as np
import pytest

import np_triangulate as NT
import track_scene as S

pytestmark = pytest.mark.gpu

BUFS = [1, 2, 3, 9, 10, 12]        # view i lives in SIFT buffer BUFS[i]
IDS_A, IDS_B = [BUFS[a] for a in S.IDS_A], [BUFS[b] for b in S.IDS_B]
NP = len(IDS_A)
NB_BUFFERS = 16
THRESHOLD = 1.0
# The views' centres are 4 .. 26 px apart at depth 256: the widest angle of a track has a cosine between 0.9949 and 0.99988. The limit splits them.
COS_LIMIT = 0.9992


def cameras():
    P = np.full((NB_BUFFERS, 3, 4), np.nan, np.float32)
    for b, (_, _, x0, y0) in zip(BUFS, S.VIEWS):
        P[b] = [[256, 0, 0, -256 * x0], [0, 256, 0, -256 * y0], [0, 0, 1, 0]]
    return P


def _instance(vk):
    cfg = vk.default_config(sift_buffer_count=NB_BUFFERS, input_image_max_size=192 * 144)
    return vk.Instance(cfg, batch_capacity=NP)


def _detect(vk, inst):
    imgs = S.images(vk.gen_synthetic_image_family)
    inst.detectFeaturesBatch(imgs[:3], BUFS[0])
    inst.detectFeaturesBatch(imgs[3:5], BUFS[3])
    inst.detectFeaturesBatch(imgs[5:], BUFS[5])


def _match(inst):
    inst.matchFeaturesFiltered(IDS_A, IDS_B, 0.8, True)


def _read(inst):
    return inst.getPointStats(), inst.downloadPoints()


def _bytes(got):
    return repr(sorted(got[0].items())).encode() + got[1].tobytes()


def _inputs(inst):
    """what the restatement is fed with, and the bytes that must not change"""
    offsets, obs = inst.downloadObservationOffsets(), inst.downloadObservations()
    same = offsets.tobytes() + obs.tobytes() + inst.downloadObservationTrackIds().tobytes() + repr(sorted(inst.getObservationStats().items())).encode()
    same += inst.downloadTracks().tobytes() + b"".join(inst.downloadFeatureTracks(b).tobytes() for b in BUFS) + repr(sorted(inst.getTrackStats().items())).encode()
    same += b"".join(inst.downloadFilteredMatches(k).tobytes() for k in range(NP))
    return offsets, obs, same


def _check(inst, threshold=THRESHOLD, cos=1.0):
    offsets, obs, before = _inputs(inst)
    inst.triangulateTracks(cameras(), threshold, cos)
    stats, pts = got = _read(inst)
    # (the restatement indexes cameras by gpu_buffer_id: the NaN cameras are never named)
    want_stats, want = NT.triangulate(offsets, obs, cameras().reshape(NB_BUFFERS, 12), NT.threshold2(threshold), cos)
    print((threshold, cos), stats)
    assert stats == want_stats
    assert pts.dtype == want.dtype and pts.tobytes() == want.tobytes()
    assert _inputs(inst)[2] == before
    # the invariants of the header, on the library's own outputs
    assert stats["nb_accepted"] + stats["nb_failed"] + stats["nb_rejected"] == stats["nb_points"] == inst.getObservationStats()["nb_tracks"] == len(pts)
    assert np.array_equal(pts["nb_observations"], np.diff(offsets)) and pts["steps"].max() <= 2
    return got


def test_two_sources_both_policies_equal_the_restatement_and_leave_their_inputs_alone(vk):
    with _instance(vk) as inst:
        _detect(vk, inst)
        _match(inst)
        inst.verifyHomography(1024, 2.5, 7)
        accepted = angle = 0
        for source in (vk.TRACKS_FILTERED, vk.TRACKS_VERIFIED_H):
            inst.buildTracks(source)
            for params in ((2, 0, vk.OBS_KEEP_CONFLICTING), (3, 0, vk.OBS_DROP_CONFLICTING)):
                inst.selectTrackObservations(*params)
                stats, pts = _check(inst)
                ok = pts[pts["status"] == 0]
                if len(ok):      # (printed, not asserted: points of the plane Z = 256 seen over baselines of a few pixels)
                    print("source", source, params, "median Z of the accepted points: %.2f" % float(np.median(ok["X"][:, 2])), "of", len(ok))
                stats, pts = _check(inst, cos=COS_LIMIT)
                accepted += int((pts["status"] == 0).sum())
                angle += int(((pts["status"] & vk.POINT_ANGLE) != 0).sum())
        assert accepted and angle, (accepted, angle)


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
        accessors = (inst.getPointStats, inst.downloadPoints)
        tri = lambda: inst.triangulateTracks(cameras(), THRESHOLD, 1.0)
        select = lambda: inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)
        assert _errors(vk, tri) == bad                                      # nothing matched yet
        _match(inst)
        assert _errors(vk, tri) == bad                                      # no tracks
        inst.buildTracks(vk.TRACKS_FILTERED)
        assert _errors(vk, tri) == bad                                      # no observations selected for the present tracks
        select()
        for fn in accessors:
            assert _errors(vk, fn) == bad                                   # an accessor before any triangulation
        first = _bytes(_check(inst))
        assert inst.getTriangulateTime() == -1.0                            # profiling is off
        assert _bytes(_check(inst)) == first                                # the same inputs: the same bytes
        held = _bytes(_check(inst, cos=COS_LIMIT))                          # a second triangulation replaces the first
        assert held != first
        broken = cameras()
        broken[BUFS[4], 1, 2] = np.inf
        refused = [lambda: inst.triangulateTracks(None, THRESHOLD, 1.0), lambda: inst.triangulateTracks(broken, THRESHOLD, 1.0)]
        refused += [(lambda t=t: inst.triangulateTracks(cameras(), t, 1.0)) for t in (0.0, -1.0, float("inf"), float("nan"), 1e-30, 1e30)]
        refused += [lambda: inst.triangulateTracks(cameras(), THRESHOLD, float("nan")), _null(vk, inst, "vksift_ext_getPointStats"),
                    _null(vk, inst, "vksift_ext_downloadPoints")]
        for fn in refused:
            assert _errors(vk, fn) == bad
            assert _bytes(_read(inst)) == held                              # earlier points served, untouched
        inst.setProfiling(True)
        assert inst.getTriangulateTime() == -1.0                            # on, but that run was not timed
        assert _bytes(_check(inst)) == first
        assert 0.0 < inst.getTriangulateTime() < 1000.0
        select()                                                            # a new selection: refused until triangulated again
        for fn in accessors:
            assert _errors(vk, fn) == bad
        assert _bytes(_check(inst)) == first
        inst.buildTracks(vk.TRACKS_FILTERED)                                # a new build: no observations, no points
        for fn in accessors + (tri,):
            assert _errors(vk, fn) == bad
        select()
        assert _bytes(_check(inst)) == first
        inst.matchFeatures(BUFS[0], BUFS[1])                                # a new plain matching: nothing left
        for fn in accessors + (tri,):
            assert _errors(vk, fn) == bad
        _match(inst)                                                        # a new filtered matching as well
        for fn in accessors + (tri,):
            assert _errors(vk, fn) == bad
        inst.buildTracks(vk.TRACKS_FILTERED)
        select()
        assert _bytes(_check(inst)) == first                                # the same matching again: the first points again
