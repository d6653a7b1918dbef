"""The per-view index and the camera refinement through the public API (vksift_ext_indexObservationsByView, vksift_ext_refineCameras and their accessors)
against the restatement tests/np_cameras.py, which is fed with the downloaded observation table, points and cameras of the same instance: byte equality of
the index, the statistics and the refined cameras; the index built by the refinement where there is none; two alternations with
vksift_ext_triangulateTracks; the tracks, observations, points and filtered matches byte-identical before and after; the lifetime of both results; every
refusal, with the earlier results compared byte for byte. Fixture: the six views of tests/test_gpu_triangulate.py (exact perspective views of the plane
Z = 256 in SIFT buffers that are not contiguous), their cameras moved by a small rigid motion each."""
import numpy as np
import pytest

import np_cameras as NC
import test_gpu_triangulate as TG

pytestmark = pytest.mark.gpu

BUFS, NB_BUFFERS = TG.BUFS, TG.NB_BUFFERS
THRESHOLD = 2.0


def cameras(angle=0.0005, shift=0.05):
    P = TG.cameras()
    P[BUFS] = NC.perturbed(P[BUFS], angle, shift).reshape(-1, 3, 4)
    return P


def _views(inst):
    return inst.getViewStats(), inst.downloadViewOffsets(), inst.downloadViewObservations()


def _cams(inst):
    return inst.getCameraStats(), inst.downloadRefinedCameras()


def _bytes(got):
    return repr(sorted(got[0].items())).encode() + b"".join(a.tobytes() for a in got[1:])


def _inputs(inst):
    """what the restatement is fed with, and the bytes that must not change"""
    offsets, obs, same = TG._inputs(inst)
    pts = inst.downloadPoints()
    return offsets, obs, pts, same + pts.tobytes() + repr(sorted(inst.getPointStats().items())).encode()


def _check_index(inst, offsets, obs):
    stats, view_offsets, view_obs = _views(inst)
    want_stats, want_offsets, want_obs = NC.index_views(offsets, obs, NB_BUFFERS)
    assert stats == want_stats
    assert view_offsets.tobytes() == want_offsets.tobytes() and view_obs.dtype == want_obs.dtype and view_obs.tobytes() == want_obs.tobytes()
    # the invariants of the header, on the library's own outputs
    assert view_offsets[0] == 0 and view_offsets[-1] == stats["nb_observations"] == len(obs) and stats["nb_views"] == len(BUFS)
    assert set(np.flatnonzero(np.diff(view_offsets))) == set(BUFS)
    return view_offsets, view_obs


def _check_refined(inst, P, nb_steps, offsets, obs, pts):
    """the refinement of the cameras P the last triangulation was given"""
    view_offsets, view_obs = _check_index(inst, offsets, obs)
    stats, rec = got = _cams(inst)
    held = np.zeros((NB_BUFFERS, 12), np.float32)           # what the triangulation copied: the cameras that took part, zeros for every other buffer
    held[BUFS] = P.reshape(NB_BUFFERS, 12)[BUFS]
    want_stats, want = NC.refine_cameras(view_offsets, view_obs, pts, held, BUFS, nb_steps)
    print(nb_steps, stats, rec["steps"][BUFS], rec["cost_start"][BUFS], rec["cost"][BUFS])
    assert stats == want_stats
    assert rec.dtype == want.dtype and rec.tobytes() == want.tobytes()
    assert stats["nb_views"] == len(BUFS) == stats["nb_refined"] + stats["nb_unchanged"] + stats["nb_failed"]
    assert (rec["status"][[b for b in range(NB_BUFFERS) if b not in BUFS]] == NC.ABSENT).all() and rec["steps"].max() <= nb_steps
    return got


def _prepared(vk, inst):
    TG._detect(vk, inst)
    TG._match(inst)
    inst.buildTracks(vk.TRACKS_FILTERED)
    inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)


def test_index_refine_and_two_alternations_equal_the_restatement_and_leave_their_inputs_alone(vk):
    with TG._instance(vk) as inst:
        _prepared(vk, inst)
        P = cameras()
        inst.triangulateTracks(P, THRESHOLD, 1.0)
        offsets, obs, pts, before = _inputs(inst)
        inst.indexObservationsByView()
        _check_index(inst, offsets, obs)
        inst.refineCameras(4)
        stats, rec = _check_refined(inst, P, 4, offsets, obs, pts)
        assert _inputs(inst)[3] == before
        assert stats["nb_refined"] > 0 and (rec["cost"][BUFS] <= rec["cost_start"][BUFS]).all()
        accepted = [inst.getPointStats()["nb_accepted"]]
        for _ in range(2):                                   # the alternation: the refined P goes back as it is
            P = P.copy()
            P[BUFS] = rec["P"][BUFS].reshape(-1, 3, 4)
            inst.triangulateTracks(P, THRESHOLD, 1.0)
            offsets2, obs2, pts, _ = _inputs(inst)
            assert offsets2.tobytes() == offsets.tobytes() and obs2.tobytes() == obs.tobytes()
            accepted.append(inst.getPointStats()["nb_accepted"])
            inst.refineCameras(2)
            stats, rec = _check_refined(inst, P, 2, offsets, obs, pts)
        print("accepted points over the alternations:", accepted)


def test_refinement_builds_the_index_it_lacks(vk):
    with TG._instance(vk) as inst:
        _prepared(vk, inst)
        P = cameras()
        inst.triangulateTracks(P, THRESHOLD, 1.0)
        offsets, obs, pts, before = _inputs(inst)
        with pytest.raises(vk.VksiftError):
            inst.getViewStats()                              # no index yet
        inst.refineCameras(3)
        first = _bytes(_check_refined(inst, P, 3, offsets, obs, pts))
        inst.indexObservationsByView()                       # an explicit index afterwards: the same index, the cameras still served
        inst.refineCameras(3)
        assert _bytes(_check_refined(inst, P, 3, offsets, obs, pts)) == first
        assert _inputs(inst)[3] == before


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def test_lifetime_refusals_and_timing(vk):
    bad = vk.VKSIFT_INVALID_INPUT_ERROR
    with TG._instance(vk) as inst:
        TG._detect(vk, inst)
        P = cameras()
        view_acc = (inst.getViewStats, inst.downloadViewOffsets, inst.downloadViewObservations)
        cam_acc = (inst.getCameraStats, inst.downloadRefinedCameras)
        index, refine = inst.indexObservationsByView, lambda: inst.refineCameras(4)
        tri = lambda: inst.triangulateTracks(P, THRESHOLD, 1.0)
        select = lambda: inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)
        for fn in (index, refine):
            assert _errors(vk, fn) == bad                                   # nothing matched yet
        TG._match(inst)
        inst.buildTracks(vk.TRACKS_FILTERED)
        for fn in (index, refine):
            assert _errors(vk, fn) == bad                                   # no observations selected for the present tracks
        select()
        for fn in view_acc + cam_acc + (refine,):
            assert _errors(vk, fn) == bad                                   # accessors before any index; no triangulation for the present observations
        index()
        views = _bytes(_views(inst))
        assert _errors(vk, refine) == bad and _bytes(_views(inst)) == views # still no triangulation: refused, the index untouched
        tri()
        offsets, obs, pts, before = _inputs(inst)
        for fn in cam_acc:
            assert _errors(vk, fn) == bad                                   # an accessor before any refinement
        refine()
        held = _bytes(_check_refined(inst, P, 4, offsets, obs, pts))
        assert inst.getRefineCamerasTime() == -1.0 and inst.getIndexViewsTime() == -1.0   # profiling is off
        null = lambda name: lambda: (getattr(vk.lib(), name)(inst._h, None), vk._check_pending())
        refused = [lambda: inst.refineCameras(0), lambda: inst.refineCameras(9)]
        refused += [null("vksift_ext_" + n) for n in ("getViewStats", "downloadViewOffsets", "downloadViewObservations", "getCameraStats", "downloadRefinedCameras")]
        for fn in refused:
            assert _errors(vk, fn) == bad
            assert _bytes(_cams(inst)) == held and _bytes(_views(inst)) == views   # earlier results served, untouched
        inst.setProfiling(True)
        refine()
        assert _bytes(_cams(inst)) == held                                  # the same inputs: the same bytes
        assert 0.0 < inst.getRefineCamerasTime() < 1000.0 and inst.getIndexViewsTime() == -1.0
        index()
        assert 0.0 < inst.getIndexViewsTime() < 1000.0 and _bytes(_views(inst)) == views and _bytes(_cams(inst)) == held
        tri()                                                               # a new triangulation: the cameras go, the index stays
        for fn in cam_acc:
            assert _errors(vk, fn) == bad
        assert _bytes(_views(inst)) == views
        refine()
        assert _bytes(_cams(inst)) == held
        assert _inputs(inst)[3] == before
        select()                                                            # a new selection: neither is served
        for fn in view_acc + cam_acc + (refine,):
            assert _errors(vk, fn) == bad
        tri()
        refine()                                                            # (builds the index again)
        assert _bytes(_cams(inst)) == held and _bytes(_views(inst)) == views
        inst.buildTracks(vk.TRACKS_FILTERED)                                # a new build: nothing left
        for fn in view_acc + cam_acc + (index, refine):
            assert _errors(vk, fn) == bad
        select()
        tri()
        refine()
        assert _bytes(_cams(inst)) == held
        inst.matchFeatures(BUFS[0], BUFS[1])                                # a new plain matching: nothing left
        for fn in view_acc + cam_acc + (index, refine):
            assert _errors(vk, fn) == bad
        TG._match(inst)                                                     # a new filtered matching as well
        for fn in view_acc + cam_acc + (index, refine):
            assert _errors(vk, fn) == bad
        inst.buildTracks(vk.TRACKS_FILTERED)
        select()
        tri()
        refine()
        assert _bytes(_cams(inst)) == held and _bytes(_views(inst)) == views    # the same matching again: the first results again
