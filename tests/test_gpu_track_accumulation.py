"""Tracks across matching calls through the public API (vksift_ext_beginTrackAccumulation, vksift_ext_accumulateTrackEdges, vksift_ext_buildTracksAccumulated
and their accessors) on the six views of tests/test_gpu_cameras.py. All fifteen pairs go through an instance whose batch capacity is 4, in four calls; a second
instance whose batch capacity takes the fifteen pairs at once is the reference. Compared byte for byte: the store's edges and statistics with the restatement
(tests/np_track_edges.py) fed the downloaded matches and masks; the accumulated tracks, per-feature words and statistics with vksift_ext_buildTracks of the
second instance; selection, triangulation and camera refinement on the accumulated tracks with the same stages there; one accumulate + build with a plain
build; a rebuild after a new matching with the first build. Lifetime, busy buffers and every refusal."""
import pytest

import np_track_edges as NE
import np_tracks as NT
import test_gpu_cameras as GC
import test_gpu_triangulate as TG

pytestmark = pytest.mark.gpu

BUFS, NB_BUFFERS, NP = TG.BUFS, TG.NB_BUFFERS, TG.NP
CAP = 4
CHUNKS = [(TG.IDS_A[i:i + CAP], TG.IDS_B[i:i + CAP]) for i in range(0, NP, CAP)]
MAX_EDGES = 1 << 16
STEPS = 3


def narrow(vk):
    cfg = vk.default_config(sift_buffer_count=NB_BUFFERS, input_image_max_size=192 * 144)
    return vk.Instance(cfg, batch_capacity=CAP)


def match(inst, chunk):
    inst.matchFeaturesFiltered(chunk[0], chunk[1], 0.8, True)


def track_bytes(inst):
    """the tracks, the per-feature words of every participating buffer and the statistics"""
    return inst.downloadTracks().tobytes() + b"".join(inst.downloadFeatureTracks(b).tobytes() for b in BUFS) + repr(sorted(inst.getTrackStats().items())).encode()


def downstream_bytes(vk, inst):
    """selection, triangulation and camera refinement on the instance's tracks: everything they serve"""
    inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)
    P = GC.cameras()
    inst.triangulateTracks(P, GC.THRESHOLD, 1.0)
    inst.refineCameras(STEPS)
    out = inst.downloadObservationOffsets().tobytes() + inst.downloadObservationTrackIds().tobytes() + inst.downloadObservations().tobytes()
    out += repr(sorted(inst.getObservationStats().items())).encode() + inst.downloadPoints().tobytes() + repr(sorted(inst.getPointStats().items())).encode()
    out += inst.downloadViewOffsets().tobytes() + inst.downloadViewObservations().tobytes() + repr(sorted(inst.getViewStats().items())).encode()
    return out + inst.downloadRefinedCameras().tobytes() + repr(sorted(inst.getCameraStats().items())).encode()


def restate_call(inst, store, chunk, masked):
    """the restatement fed what the instance serves for the present matching"""
    rows = {b: inst.getFeaturesNumber(b) for b in sorted(set(chunk[0]) | set(chunk[1]))}
    pairs = []
    for k, (a, b) in enumerate(zip(*chunk)):
        recs = inst.downloadFilteredMatches(k)
        if masked:
            pairs.append((a, b, NT.pair_edges(recs, inst.downloadInlierMask(k), bool(inst.getHomography(k)["valid"]))))
        else:
            pairs.append((a, b, NT.pair_edges(recs)))
    return NE.accumulate(store, rows, pairs)


def check_store(inst, store):
    assert inst.getTrackEdgeStats() == NE.stats(store)
    got, want = inst.downloadTrackEdges(), NE.edge_records(store)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def check_build(inst, store, max_rows):
    rec, words, stats = NE.build(store, max_rows)
    assert inst.getTrackStats() == stats
    got = inst.downloadTracks()
    assert got.dtype == rec.dtype and got.tobytes() == rec.tobytes()
    for b in BUFS:
        assert inst.downloadFeatureTracks(b).tobytes() == words[b].tobytes(), b


@pytest.fixture(scope="module")
def reference(vk):
    """the instance that takes the fifteen pairs at once: its plain build, and what one accumulate + build gives there"""
    with TG._instance(vk) as inst:
        TG._detect(vk, inst)
        TG._match(inst)
        inst.buildTracks(vk.TRACKS_FILTERED)
        plain = track_bytes(inst)
        stats = inst.getTrackStats()
        down = downstream_bytes(vk, inst)
        inst.beginTrackAccumulation(MAX_EDGES)
        assert track_bytes(inst) == plain                          # 2 batch_capacity >= sift_buffer_count: nothing released, the tracks still served
        inst.accumulateTrackEdges(vk.TRACKS_FILTERED)
        inst.buildTracksAccumulated()
        once = track_bytes(inst)
        edges = inst.getTrackEdgeStats()
    return dict(plain=plain, stats=stats, down=down, once=once, edges=edges)


def test_one_accumulate_and_a_build_equal_the_plain_build(reference):
    assert reference["once"] == reference["plain"]
    assert reference["edges"] == dict(nb_edges=reference["stats"]["nb_edges"], nb_dropped=0, nb_calls=1, nb_changed_buffers=0)
    assert reference["stats"]["nb_tracks"] > 100


def test_four_calls_equal_the_restatement_and_the_instance_that_takes_all_pairs_at_once(vk, reference):
    with narrow(vk) as inst:
        TG._detect(vk, inst)
        match(inst, CHUNKS[0])
        inst.buildTracks(vk.TRACKS_FILTERED)                       # storage for 2 * 4 buffers: the begin below releases it and sizes it for 16
        inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)
        inst.beginTrackAccumulation(MAX_EDGES)
        with pytest.raises(vk.VksiftError):
            inst.getTrackStats()
        store = NE.begin(MAX_EDGES)
        assert inst.getTrackEdgeStats() == NE.stats(store) and len(inst.downloadTrackEdges()) == 0
        for chunk in CHUNKS:
            match(inst, chunk)
            inst.accumulateTrackEdges(vk.TRACKS_FILTERED)
            before = [inst.downloadFilteredMatches(k).tobytes() for k in range(len(chunk[0]))]
            restate_call(inst, store, chunk, False)
            check_store(inst, store)
            assert [inst.downloadFilteredMatches(k).tobytes() for k in range(len(chunk[0]))] == before
        assert NE.stats(store)["nb_calls"] == 4 and NE.stats(store)["nb_changed_buffers"] == 0 and NE.stats(store)["nb_edges"] == reference["stats"]["nb_edges"]
        inst.buildTracksAccumulated()
        check_build(inst, store, vk.default_config().max_nb_sift_per_buffer)
        first = track_bytes(inst)
        assert first == reference["plain"]
        assert downstream_bytes(vk, inst) == reference["down"]
        check_store(inst, store)                                    # the build and the stages behind it leave the store as it was
        # a matching after the build: the tracks go, the store stays, a rebuild gives the same bytes
        match(inst, CHUNKS[3])
        with pytest.raises(vk.VksiftError):
            inst.getTrackStats()
        with pytest.raises(vk.VksiftError):
            inst.downloadObservations()
        check_store(inst, store)
        inst.buildTracksAccumulated()
        assert track_bytes(inst) == first
        # a plain build replaces the accumulated tracks; the store is still there, and builds them again
        inst.buildTracks(vk.TRACKS_FILTERED)
        assert inst.getTrackStats()["nb_edges"] < reference["stats"]["nb_edges"]
        with pytest.raises(vk.VksiftError):
            inst.downloadFeatureTracks(BUFS[0])                     # outside the pair list of the plain build
        inst.buildTracksAccumulated()
        assert track_bytes(inst) == first and downstream_bytes(vk, inst) == reference["down"]


def test_a_masked_source_a_small_capacity_and_a_second_begin(vk):
    with narrow(vk) as inst:
        TG._detect(vk, inst)
        for max_edges in (MAX_EDGES, 1000):                        # the second begin empties the store; its capacity overflows in the second call
            inst.beginTrackAccumulation(max_edges)
            store = NE.begin(max_edges)
            for chunk in CHUNKS:
                match(inst, chunk)
                inst.verifyHomography(1024, 2.5, 7)
                inst.accumulateTrackEdges(vk.TRACKS_VERIFIED_H)
                restate_call(inst, store, chunk, True)
                check_store(inst, store)
            inst.buildTracksAccumulated()
            check_build(inst, store, vk.default_config().max_nb_sift_per_buffer)
            print(max_edges, NE.stats(store), inst.getTrackStats())
        assert NE.stats(store)["nb_edges"] == 1000 and NE.stats(store)["nb_dropped"] > 0


def test_all_participating_buffers_are_busy_while_a_stage_behind_the_build_is_queued(vk):
    outside = [b for b in BUFS if b not in CHUNKS[-1][0] + CHUNKS[-1][1]]
    assert outside == BUFS[:3]
    with narrow(vk) as inst:
        TG._detect(vk, inst)
        inst.beginTrackAccumulation(MAX_EDGES)
        inst.getTrackEdgeStats()
        assert all(inst.isBufferAvailable(b) for b in BUFS)
        for chunk in CHUNKS:                                        # no accessor in between: everything below is queued behind four matchings and RANSACs
            match(inst, chunk)
            inst.verifyHomography(8192, 2.5, 7)
            inst.accumulateTrackEdges(vk.TRACKS_FILTERED)
        inst.buildTracksAccumulated()
        inst.selectTrackObservations(2, 0, vk.OBS_KEEP_CONFLICTING)
        busy = [not inst.isBufferAvailable(b) for b in outside]
        inst.getObservationStats()                                  # the accessor waits
        assert all(inst.isBufferAvailable(b) for b in BUFS)
        assert all(busy), busy


def _errors(vk, fn):
    with pytest.raises(vk.VksiftError) as e:
        fn()
    return e.value.code


def test_refusals_and_timing(vk):
    bad = vk.VKSIFT_INVALID_INPUT_ERROR
    with narrow(vk) as inst:
        TG._detect(vk, inst)
        accumulate, build = lambda: inst.accumulateTrackEdges(vk.TRACKS_FILTERED), inst.buildTracksAccumulated
        for fn in (accumulate, build, inst.getTrackEdgeStats, inst.downloadTrackEdges, lambda: inst.beginTrackAccumulation(0)):
            assert _errors(vk, fn) == bad                           # nothing begun
        inst.beginTrackAccumulation(MAX_EDGES)
        assert _errors(vk, accumulate) == bad                       # no filtered matching
        inst.matchFeatures(BUFS[0], BUFS[1])
        assert _errors(vk, accumulate) == bad                       # a plain matching is none
        match(inst, CHUNKS[0])
        assert _errors(vk, build) == bad                            # nothing accumulated
        assert _errors(vk, lambda: inst.accumulateTrackEdges(6)) == bad
        assert _errors(vk, lambda: inst.accumulateTrackEdges(vk.TRACKS_VERIFIED_H)) == bad      # not verified
        assert _errors(vk, lambda: inst.accumulateTrackEdges(vk.TRACKS_GUIDED)) == bad
        assert _errors(vk, TG._null(vk, inst, "vksift_ext_getTrackEdgeStats")) == bad
        assert _errors(vk, TG._null(vk, inst, "vksift_ext_downloadTrackEdges")) == bad
        assert _errors(vk, lambda: inst.beginTrackAccumulation(0)) == bad
        assert inst.getTrackEdgeStats() == dict(nb_edges=0, nb_dropped=0, nb_calls=0, nb_changed_buffers=0)       # the refusals left the store as begin made it
        assert inst.getAccumulateTime() == -1.0
        inst.setProfiling(True)
        accumulate()
        build()
        stats = inst.getTrackEdgeStats()
        assert stats["nb_calls"] == 1 and stats["nb_edges"] == inst.getTrackStats()["nb_edges"] > 0
        print("accumulate", inst.getAccumulateTime(), "ms, accumulated build", inst.getTracksTime(), "ms")
        assert inst.getAccumulateTime() > 0 and inst.getTracksTime() > 0
        # a buffer that changes between two calls is reported, the table keeps the count of the first call
        n0 = inst.getFeaturesNumber(BUFS[0])
        inst.keepStrongestFeatures(BUFS[0], 1, 40)
        assert inst.getFeaturesNumber(BUFS[0]) == 40 < n0
        match(inst, CHUNKS[0])
        accumulate()
        assert inst.getTrackEdgeStats()["nb_changed_buffers"] == 1 and inst.getTrackEdgeStats()["nb_calls"] == 2
        build()
        words = inst.downloadFeatureTracks(BUFS[0], n0)             # the rows of the table: the count of the first call that named the buffer
        assert (words[40:] != vk.NO_TRACK).any()
