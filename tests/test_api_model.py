"""What tests/test_gpu_api_model.py rests on, pinned on the CPU: (a) the walks of every committed (profile, seed) reach each edge of the host
bookkeeping at least three times, counted in the generator's trace; (b) the executor notices planted bookkeeping faults — a stand-in for the
instance, backed by a second copy of the model and the caches a host keeps beside it, passes with no fault and fails with each one. No GPU: the
records of the describe calls come from tests/golden/api_model_describe.npz (recorded by tests/golden/make_api_model_describe.py; the GPU test holds
the recording to what a quiet instance returns)."""
import collections

import numpy as np
import pytest

import api_model as A
from api_model import SEEDS, STEPS

CASES = [(p, s) for p in A.PROFILES for s in SEEDS[p]]


@pytest.fixture(scope="module")
def walks(oracle):
    """(profile, seed) -> (world, operations, the model they were generated on)"""
    from vulkansift_amd import api as vk

    out = {}
    for p in A.PROFILES:
        w = A.World(p, oracle, vk)
        for s in SEEDS[p]:
            out[p, s] = (w,) + A.generate(s, STEPS, p, w)
    return out


# ====================================================================================================================== (a) reach
# every edge, as the labels of Model.trace: (label, its variants or None for the sum over all of them)
OPS = list(A.INPLACE)
EDGES = [
    ("E1 an in-place operation on a buffer whose detection no accessor has waited for", "E1", OPS),
    ("E2 an in-place operation on an uploaded buffer", "E2", OPS),
    ("E3 one range mixing uploaded and detected buffers and two resolutions (three layout runs and more)", "E3", None),
    ("E4 a matching queued directly behind the in-place operation", "E4", OPS),
    ("E4 ... as the instance's first matching (no cache block yet)", "E4 first matching", None),
    ("E5 a budget that does not bind, then a matching; the cache entry beforehand", "E5", ["valid", "invalid"]),
    ("E6 an in-place operation, a detection or upload into the same buffer, a matching", "E6", None),
    ("E7 describe, then this, then the placed count and a matching", "E7", ["cut", "noncut", "convert"]),
    ("E8 a batched detection of 8, an in-place operation on part of its range, downloads of the whole range (packed copy)", "E8 packed", None),
    ("E9 row of the invalidation table", "E9 row", ["plain matching", "filtered matching", "verify H again", "verify F again"]),
    ("E9 refused call", "E9 refused", ["stage without filtered matching", "guided unverified", "refit unverified", "accessor on a dropped set", "pair == slots_used"]),
    ("E10 two and more plain detections staged (vksift_defer.c's rules, restated) when this entry arrives", "E10", ["budget", "grid", "rootsift", "describe", "match", "export"]),
    ("E10 ... of them on the plain profile alone (batch_capacity 1, VKSIFT_DEFER_MAX 3)", "E10 plain", ["budget", "grid", "rootsift", "describe", "match", "export"]),
    ("E11 exportDescriptorsDevice directly behind the in-place operation", "E11", OPS),
    ("E12 a buffer-changing call queued between a pair stage and the fetch of its results", "E12", None),
]


def test_the_committed_walks_reach_every_edge_three_times(walks):
    count = collections.Counter()
    for (p, s), (_, ops, model) in walks.items():
        assert STEPS <= len(ops) < STEPS + 40
        for t in model.trace:
            count[t[1:]] += 1
            count[t[1:2]] += 1
    missing = []
    for text, label, variants in EDGES:
        for v in variants or [None]:
            n = count[(label,) if v is None else (label, v)]
            print(f"{n:4d}  {text}{'' if v is None else ': ' + v}")
            if n < 3:
                missing.append((label, v, n))
    assert not missing, missing
    assert all(count["E4 first matching", o] >= 1 for o in OPS), "each in-place operation once in front of an instance's first matching"
    # every operation of the two older walks and every new entry occurs
    names = {op[0] for _, ops, _ in walks.values() for op in ops}
    assert names >= {"detect", "batch", "upload", "count", "download", "match", "batchmatch", "filtered", "fetch", "avail", "budget", "grid", "rootsift", "describe",
                     "describe_batch", "export", "placed", "verify", "refine", "guided", "pair", "refuse"}
    guided = [op for _, ops, _ in walks.values() for op in ops if op[0] == "guided"]
    assert any(op[2] is None for op in guided) and any(op[2] is not None for op in guided)       # the verified models and the caller's own
    # grid shapes: 1 x 1, and more cells than the buffer holds features, each on a buffer that the budget cuts
    print(f"{count['grid 1 x 1',]:4d}  a binding 1 x 1 grid\n{count['grid cells > features',]:4d}  a binding grid of more cells than the buffer holds features")
    assert count["grid 1 x 1",] >= 3 and count["grid cells > features",] >= 3


def test_generation_is_deterministic(walks):
    (p, s), (w, ops, _) = next(iter(walks.items()))
    again, _ = A.generate(s, STEPS, p, w)
    assert repr(again) == repr(ops)


# ====================================================================================================================== (b) sensitivity
class FakeError(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


FAULTS = ["cache entry not refreshed after a conversion", "cache entry not refreshed after a cutting budget on a buffer whose counts were unknown",
          "an upload leaves the cache entry valid", "count not updated after a budget", "placed count kept after a cut",
          "refined results kept after a new verification", "filtered set served after a plain matching", "packed copy served after a partial in-place operation"]


class FakeInstance:
    """the methods the executor calls, answered by a second copy of the model and by what a host keeps beside the buffers: the matcher's cache (rows a
    matching reads instead of the buffer while the entry is valid), the packed copy of a batched detection, the counts and the result sets. With
    fault = None every one of them is kept right; with one of FAULTS that rule alone is broken."""
    Error = FakeError

    def __init__(self, world, fault=None):
        assert fault is None or fault in FAULTS
        self.w, self.fault = world, fault
        self.m = A.Model(world)
        self.m.rows = self._rows
        self.cache, self.count, self.placed, self.packed = {}, {}, {}, None

    def _rows(self, b):
        if b not in self.cache:
            self.cache[b] = self.m.bufs[b].recs
        return self.cache[b]

    def _changed(self, ids, keep_cache=(), inplace=False):
        for i in ids:
            if i not in keep_cache:
                self.cache.pop(i, None)
            self.count.pop(i, None)
            self.placed.pop(i, None)
        if self.packed and set(ids) & set(self.packed[0]) and not (inplace and self.fault == FAULTS[7]):
            self.packed = None

    # ---- fills
    def detectFeatures(self, img, b):
        self._changed([b])
        self.m.apply(("detect", self.w.img_index[id(img)], b))

    def detectFeaturesBatch(self, imgs, b):
        ids = list(range(b, b + len(imgs)))
        self._changed(ids)
        self.m.apply(("batch", [self.w.img_index[id(im)] for im in imgs], b))
        self.packed = (ids, None) if len(ids) >= A.PACK_MIN else self.packed

    def uploadFeatures(self, feats, b):
        self._changed([b], keep_cache=[b] if self.fault == FAULTS[2] else ())
        self.m.apply(("upload_raw", feats, b))

    def describeKeypoints(self, img, kps, b, mode):
        self._changed([b])
        self.m.apply(("describe", self.w.describe_entry(img, kps, mode), b))

    def describeKeypointsBatch(self, imgs, lists, b, mode):
        self._changed(list(range(b, b + len(imgs))))
        self.m.apply(("describe_batch", [self.w.describe_entry(im, k, mode) for im, k in zip(imgs, lists)], b))

    # ---- in place
    def _budget(self, op):
        b, cnt, n = op[1:4]
        ids = list(range(b, b + cnt))
        cut = [i for i in ids if len(self.m.bufs[i].recs) > n]
        keep = [i for i in cut if not self.m.bufs[i].known] if self.fault == FAULTS[1] else ()
        old = {i: (len(self.m.bufs[i].recs), self.m.bufs[i].placed) for i in cut}
        self._changed(ids, keep_cache=keep, inplace=True)
        self.m.apply(op)
        for i in cut:
            if self.fault == FAULTS[3]:
                self.count[i] = old[i][0]
            if self.fault == FAULTS[4]:
                self.placed[i] = old[i][1]

    def keepStrongestFeatures(self, b, cnt, n):
        self._budget(("budget", b, cnt, n))

    def keepStrongestFeaturesGrid(self, b, cnt, n, w, h, gc, gr):
        self._budget(("grid", b, cnt, n, w, h, gc, gr))

    def convertToRootSift(self, b, cnt):
        ids = list(range(b, b + cnt))
        self._changed(ids, keep_cache=ids if self.fault == FAULTS[0] else (), inplace=True)
        self.m.apply(("rootsift", b, cnt))

    # ---- matching and the pair stages
    def _plain(self, op):
        kept = self.m.sets["filtered"]
        self.m.apply(op)
        if self.fault == FAULTS[6] and kept is not None:
            self.m.sets["filtered"] = kept

    def matchFeatures(self, a, b):
        self._plain(("match", a, b))

    def matchFeaturesBatch(self, pa, pb):
        self._plain(("batchmatch", list(pa), list(pb)))

    def matchFeaturesFiltered(self, pa, pb, ratio, cross):
        self.m.apply(("filtered", list(pa), list(pb), ratio, cross))

    def _refuse_unless(self, ok):
        self.m.defer_sync()
        if not ok:
            raise FakeError(A.INVALID_INPUT)

    def _filtered(self):
        return self.m.match is not None and self.m.match["kind"] == "filtered"

    def _verify(self, m, nh, thr, seed):
        self._refuse_unless(self._filtered())
        kept = self.m.sets["refined " + m]
        self.m.apply(("verify", m, nh, thr, seed))
        if self.fault == FAULTS[5] and kept is not None:
            self.m.sets["refined " + m] = kept

    def verifyHomography(self, nh, thr, seed):
        self._verify("H", nh, thr, seed)

    def verifyFundamental(self, nh, thr, seed):
        self._verify("F", nh, thr, seed)

    def refineHomography(self, rounds, thr):
        self._refuse_unless(self._filtered() and "H" in self.m.ver)
        self.m.apply(("refine", "H", rounds, thr))

    def refineFundamental(self, rounds, thr):
        self._refuse_unless(self._filtered() and "F" in self.m.ver)
        self.m.apply(("refine", "F", rounds, thr))

    def matchFeaturesGuided(self, kind, models, thr, ratio, max_distance, cross):
        m = "H" if kind == A.G.HOMOGRAPHY else "F"
        self._refuse_unless(self._filtered() and (models is not None or m in self.m.ver))
        self.m.apply(("guided", m, None if models is None else [list(x) for x in np.asarray(models).reshape(-1, 9)], thr, ratio, cross))

    # ---- reads
    def getFeaturesNumber(self, b):
        self.m.defer_sync()
        self.m._waited(b)
        return self.count.get(b, len(self.m.bufs[b].recs))

    def downloadFeatures(self, b):
        self.m.defer_sync()
        self.m._waited(b)
        if self.packed and b in self.packed[0]:
            if self.packed[1] is None:
                self.packed = (self.packed[0], {i: self.m.bufs[i].recs for i in self.packed[0]})
            return self.packed[1][b]
        return self.m.bufs[b].recs

    def getPlacedKeypointsNumber(self, b):
        self.m.defer_sync()
        self.m._waited(b)
        return self.placed.get(b, self.m.bufs[b].placed)

    def export(self, b):
        self.m.defer_sync()
        self.m._waited(b)
        return self.m.bufs[b].recs["descriptor"].tobytes()

    def isBufferAvailable(self, b):
        self.m.defer_sync()
        return True

    def getDeferredStats(self):
        return self.m.defer_batches, self.m.defer_images

    def downloadMatches(self):
        self.m.defer_sync()
        return self.m.match["fwd"][0]

    def downloadMatchesBatch(self, k):
        self.m.defer_sync()
        return self.m.match["fwd"][k]

    def pair_read(self, name, pair):
        self.m.defer_sync()
        try:
            return self.m.observe(("pair", name, pair)) + bytes(8)
        except A.Refused:
            raise FakeError(A.INVALID_INPUT)


def _first_failure(walks, fault):
    """(profile, seed, step) of the first assertion the executor raises over the committed walks, in their order; None if it raises none"""
    for (p, s), (w, ops, _) in walks.items():
        try:
            A.run(FakeInstance(w, fault), ops, A.Model(w), (p, s))
        except AssertionError as e:
            ctx = e.args[0]
            while isinstance(ctx[0], tuple):
                ctx = ctx[0]
            return ctx[:3]
    return None


def test_no_fault_passes_on_every_committed_walk(walks):
    assert _first_failure(walks, None) is None


# the first failing (profile, seed, step or "final ...") of each planted fault, over the committed walks in their order
FIRST_FAILING = {
    "cache entry not refreshed after a conversion": ("plain", 24, 136),
    "cache entry not refreshed after a cutting budget on a buffer whose counts were unknown": ("plain", 24, 18),
    "an upload leaves the cache entry valid": ("batch", 38, 120),
    "count not updated after a budget": ("batch", 23, 24),
    "placed count kept after a cut": ("batch", 23, 16),
    "refined results kept after a new verification": ("plain", 24, 46),
    "filtered set served after a plain matching": ("plain", 24, 16),
    "packed copy served after a partial in-place operation": ("batch", 23, 151),
}


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_is_caught(walks, fault):
    got = _first_failure(walks, fault)
    print(f"{fault}: first caught at {got}")
    assert got is not None, fault
    assert got == FIRST_FAILING[fault], (fault, got)
