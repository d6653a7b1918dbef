"""Model, generator and executor of random walks over every stateful entry of the API (include/vulkansift/vulkansift.h, include/vksift_ext.h).

This module tests STATE, not kernels. Every kernel has its own test against a restatement; what a walk checks is the host bookkeeping that decides
which launch reads which rows, and when: sequence numbers, the matcher's cache entries, posted and packed copies, the placed-keypoint count and the
six per-pair result sets. Every expected value comes from what the project calls its specification — oracle.detect / match_2nn / filter_matches,
np_strongest / np_spread / np_rootsift for the in-place operations, np_verify / np_verify_f / np_refine / np_refine_f / np_guided for the pair
stages — applied to the model's records. The records of a describe call are the exception: they are taken from a table (World.desc) that the GPU
test fills once, before the walk, from describe calls on a fresh quiet instance, and that the CPU test reads from tests/golden/api_model_describe.npz
(tests/test_gpu_describe.py holds the describe kernels to their restatement).

  World      images, their oracle detections, the describe table of one profile
  Model      per buffer: records in download order, kind (detected at a resolution, uploaded, described), the placed-keypoint count the header
             promises; per instance: the last matching, the twelve per-pair accessors (bytes per pair, or refused), stale
  generate   operations from model state alone, deterministic in (seed, steps, profile): single operations and short scenarios that aim at the
             edges E1 .. E12 (tests/test_api_model.py counts them in Model.trace)
  run        executes operations against a duck-typed instance, asserts every observable byte for byte, ends with a full download
  Real       the duck type over vulkansift_amd.api.Instance;  tests/test_api_model.py holds the CPU stand-in with planted faults

Needs no GPU and no built library to import."""
import hashlib
import os

import numpy as np

import np_guided as G
import np_refine as R
import np_refine_f as RF
import np_rootsift as NR
import np_spread as NSP
import np_strongest as NS
import np_verify as V
import np_verify_f as VF
from pair_checks import corr

from vulkansift_amd.api import (DESCRIBE_GIVEN, DESCRIBE_ORIENT, FEATURE_DTYPE, FILTERED_MATCH_DTYPE, FUNDAMENTAL_DTYPE, HOMOGRAPHY_DTYPE, KEYPOINT_DTYPE,
                                REFINED_FUNDAMENTAL_DTYPE, REFINED_HOMOGRAPHY_DTYPE)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_model_describe.npz")
INVALID_INPUT = 1                      # VKSIFT_INVALID_INPUT_ERROR
HYPOTHESES, ROUNDS, THRESHOLD, RATIO = 128, 2, 2.5, 0.8
SIZES = [(256, 192)] * 8 + [(200, 160)] * 2 + [(160, 120)]
PACK_MIN = 8                           # detections of this many images are downloaded through one packed copy (VKSIFT_DL_BATCH_MIN)
INPLACE = ("budget", "grid", "rootsift")
# the twelve per-pair accessors, as tests/test_gpu_pair_stages.py names them, and the result set each belongs to
ACCESSORS = {"filtered n": "filtered", "filtered": "filtered", "H": "H", "H mask": "H", "F": "F", "F mask": "F", "refined H": "refined H",
             "refined H mask": "refined H", "refined F": "refined F", "refined F mask": "refined F", "guided n": "guided", "guided": "guided"}
SETS = ("filtered", "H", "F", "refined H", "refined F", "guided")

PROFILES = {
    # batch_capacity 1: plain detections only, staged and launched as batches (VKSIFT_DEFER), default posting
    "plain": dict(nbuf=6, bc=1, cap=None, env={"VKSIFT_DEFER": "1", "VKSIFT_DEFER_MAX": "3"}),
    # batch capacity 8: every detection with an octave overlaps (a scale-space stream of its own), batched detections of 8 (the packed download).
    # An overlapped detection is never captured: VKSIFT_GRAPH=1 lifts the size limit of the replay, but this profile never captures or replays
    # a graph (tests/test_detect_plan.py: batch_profile holds that on the simulated device; tests/test_gpu_graph_cache.py covers the replay)
    "batch": dict(nbuf=12, bc=8, cap=None, env={"VKSIFT_GRAPH": "1"}),
    # every section of every image clamps; the records are fetched, not posted
    "clamped": dict(nbuf=8, bc=4, cap=120, env={"VKSIFT_POST_FEATURES": "0"}),
}
# the describe table: (image, every `step`-th oracle feature from `first` on as the keypoint list, mode)
DESCRIBE = [(0, 0, 3, DESCRIBE_GIVEN), (1, 1, 4, DESCRIBE_ORIENT), (1, 1, 4, DESCRIBE_GIVEN), (8, 0, 3, DESCRIBE_GIVEN)]
DESCRIBE_BATCH = (0, 2)                # the entries a batched describe call takes: one resolution, one mode
# the committed walks: tests/test_gpu_api_model.py runs them, tests/test_api_model.py pins what they reach
STEPS = 200
SEEDS = {"plain": [24, 29], "batch": [23, 38], "clamped": [23, 30]}

# ---------------------------------------------------------------------------------------------------------------- restatements, cached
_MEMO = {}


def _key(x):
    if isinstance(x, np.ndarray):
        return hashlib.blake2b(np.ascontiguousarray(x).view(np.uint8).reshape(-1), digest_size=16).digest() + str(x.shape[:1]).encode()
    if isinstance(x, (list, tuple)):
        return tuple(_key(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, _key(v)) for k, v in sorted(x.items()))
    return x


def memo(name, fn, *args):
    """fn(*args), once per (name, contents of the arguments): a walk meets the same buffer contents again and again, and the CPU test runs every
    walk several times"""
    k = (name, _key(args))
    if k not in _MEMO:
        _MEMO[k] = fn(*args)
    return _MEMO[k]


def _bytes_view(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 164)


def _as_features(rows):
    return np.ascontiguousarray(rows, np.uint8).reshape(-1).view(FEATURE_DTYPE).copy()


def _record(dtype, want):
    r = np.zeros(1, dtype)
    for name in dtype.names:
        r[name][0] = np.asarray(want[name]).reshape(dtype[name].shape)
    return r.tobytes()


def _mask(want):
    return np.asarray(want["mask"]).astype(np.uint8).tobytes()


# ---------------------------------------------------------------------------------------------------------------- world
class World:
    """what a walk of one profile draws from. oracle: the oracle module; vk: vulkansift_amd.api (the image generator only); describe: None to read the
    recorded table, or a function (image, keypoints, mode) -> (records, placed) that runs a describe call on a quiet instance"""

    def __init__(self, profile, oracle, vk, describe=None):
        self.profile, self.p = profile, PROFILES[profile]
        self.oracle = oracle
        base = [vk.gen_synthetic_image(0xA11CE + i, w, h) for i, (w, h) in enumerate(SIZES)]
        # odd images are shifted copies of their even neighbour, so that filtered matchings and verifications of the two have something to find
        self.imgs = [im if i % 2 == 0 or SIZES[i] != SIZES[i - 1] else np.ascontiguousarray(np.roll(base[i - 1], (3, 5), axis=(0, 1))) for i, im in enumerate(base)]
        kw = {} if self.p["cap"] is None else {"max_nb_sift_per_buffer": self.p["cap"]}
        ocfg = oracle.default_config(math_mode=1, **kw)
        self.clamps = []
        self.ref = []
        for im in self.imgs:
            recs, counts = oracle.detect(ocfg, im)
            self.ref.append(recs)
            self.clamps.append(sum(counts) > len(recs))
        self.kps = []
        for k, first, step, mode in DESCRIBE:
            f = self.ref[k][first::step]
            kp = np.zeros(len(f), KEYPOINT_DTYPE)
            kp["x"], kp["y"], kp["sigma"], kp["orientation"], kp["response"] = f["x"], f["y"], f["sigma"], f["orientation"], f["intensity"]
            self.kps.append(kp)
        if describe is None:
            z = np.load(GOLDEN)
            self.desc = [(_as_features(z[f"{profile}_{d}_records"]), int(z[f"{profile}_{d}_placed"])) for d in range(len(DESCRIBE))]
        else:
            self.desc = [describe(self.imgs[k], self.kps[d], mode) for d, (k, _, _, mode) in enumerate(DESCRIBE)]
        self.img_index = {id(im): i for i, im in enumerate(self.imgs)}
        self.kps_index = {id(kp): d for d, kp in enumerate(self.kps)}

    def describe_entry(self, img, kps, mode):
        d = self.kps_index[id(kps)]
        assert DESCRIBE[d][0] == self.img_index[id(img)] and DESCRIBE[d][3] == mode
        return d


# ---------------------------------------------------------------------------------------------------------------- model
class Buf:
    __slots__ = ("recs", "kind", "res", "placed", "src", "fill", "known", "cache", "hist")

    def __init__(self):
        self.recs, self.kind, self.res, self.placed, self.src = np.zeros(0, FEATURE_DTYPE), "empty", None, 0, None
        self.fill, self.known, self.cache, self.hist = 0, True, False, []


class Refused(Exception):
    """the model's answer to a call the header refuses with VKSIFT_INVALID_INPUT_ERROR"""


class Model:
    """apply(op) moves the state, observe(op) says what a reading operation must return. Besides what the header promises, a model keeps a rough
    shadow of what the host knows (have the counts of a buffer reached it, is its cache entry valid, is there a cache): the expected values never
    depend on it, the edge labels in `trace` do. It says what the call SEQUENCE permits, not what the host knows at run time: counts_valid() turns
    true as soon as a poll finds the detection's event finished, and inplace_begin and the matcher poll, so whether a call labelled E1 runs blind, or
    E5 finds the entry as labelled, depends on timing on hardware. The walks queue without waiting, which is what makes the blind case likely."""

    def __init__(self, world):
        self.w = world
        self.nbuf, self.bc = world.p["nbuf"], world.p["bc"]
        self.bufs = [Buf() for _ in range(self.nbuf)]
        self.match = None            # dict(kind, pa, pb, fwd, filt): the last matching
        self.sets = {s: None for s in SETS}     # per result set: None (refused) or {accessor name: [bytes per pair]}
        self.ver = {}                # "H" / "F": the verified records (restatement dicts) per pair
        self.stale = False
        self.trace, self.step = [], 0
        self.fills, self.cache_exists, self.matchings = 0, False, 0
        # the staged run of plain detections, restated from vksift_defer.c and defer_sync (vksift_internal.h); unlike the shadow above this one is exact:
        # run() holds defer_batches / defer_images to vksift_ext_getDeferredStats at the end of every walk
        env = world.p["env"]
        self.defer_max = min(int(env.get("VKSIFT_DEFER_MAX", 128)), self.nbuf)
        self.defer_on = not env.get("VKSIFT_DEFER", "1").startswith("0") and self.nbuf >= 2 and self.defer_max >= 2
        self.det_cap, self.defer_grow = self.bc, False          # images one launch sequence takes; the last batch filled it: double it
        self.pend_n, self.pend_first, self.pend_res = 0, 0, None
        self.epoch_detects, self.batch_mode = 0, False
        self.defer_batches, self.defer_images = 0, 0
        self.prev = None             # the previous operation
        self.stage_dirty = False     # a buffer-changing call has been queued since the last stage run (E12)
        self.batch_of = {}           # buffer -> the range of the batched detection whose content it and all of that range still hold
        self.e8 = None               # (that range, the in-place operation queued on a part of it, the buffers downloaded since)

    # what a matching reads of a buffer; the CPU stand-in overrides it with its cache
    def rows(self, b):
        return self.bufs[b].recs

    def label(self, *what):
        self.trace.append((self.step,) + what)

    # ---- helpers
    def _fill(self, ids):
        self.fills += 1
        for i in ids:
            self.bufs[i].fill = self.fills

    def _touch_pairs(self, ids):
        if self.match is not None and set(ids) & (set(self.match["pa"]) | set(self.match["pb"])):
            self.stale = True
            self.stage_dirty = True

    def _store(self, b, recs, kind, res, placed, src):
        for i in self.batch_of.pop(b, None) or []:
            self.batch_of.pop(i, None)               # one buffer of the range refilled: the range is no longer one detection's
        if self.e8 is not None and b in self.e8[0]:
            self.e8 = None
        x = self.bufs[b]
        x.recs, x.kind, x.res, x.placed, x.src = recs, kind, res, placed, src
        x.known, x.cache = kind == "up", False
        x.hist = (x.hist + ["describe" if kind == "desc" else "fill"])[-4:]

    def _waited(self, b):
        f = self.bufs[b].fill
        for x in self.bufs:
            if x.fill == f:
                x.known = True

    def layout_runs(self, ids):
        runs, last = 0, None
        for i in ids:
            x = self.bufs[i]
            lay = ("up",) if x.kind in ("up", "empty") else ("det", x.res)
            if lay != last:
                runs, last = runs + 1, lay
        return runs

    def binds(self, b, n):
        return len(self.bufs[b].recs) > n

    # ---- transitions
    def apply(self, op):
        name = op[0]
        self.step += 1
        if name == "detect":
            self._defer_detect(SIZES[op[1]], op[2])
        else:
            # E10: two or more plain detections are STAGED when another entry arrives and launches them (every entry but vksift_detectFeatures
            # starts with defer_sync)
            if self.pend_n >= 2 and name in INPLACE + ("describe", "describe_batch", "match", "batchmatch", "filtered", "export", "batch"):
                ender = {"describe_batch": "describe", "batchmatch": "match", "filtered": "match"}.get(name, name)
                self.label("E10", ender)
                if self.w.profile == "plain":            # the profile configured for deferral: batch_capacity 1, a small VKSIFT_DEFER_MAX
                    self.label("E10 plain", ender)
            self.defer_sync()
        getattr(self, "_op_" + name)(*op[1:])
        self.prev = op

    def _defer_flush(self):
        if self.pend_n:
            self.defer_batches, self.defer_images, self.pend_n = self.defer_batches + 1, self.defer_images + self.pend_n, 0

    def defer_sync(self):
        """what every entry but vksift_detectFeatures starts with: the staged images are launched, the run of detect calls ends"""
        self._defer_flush()
        if self.epoch_detects:
            self.batch_mode, self.epoch_detects = self.epoch_detects >= 2, 0

    def defer_full(self):
        """how many staged images launch the batch at once, for a run that starts now"""
        cap = min(2 * self.det_cap, self.defer_max) if self.pend_n == 0 and self.defer_grow and self.det_cap < self.defer_max else self.det_cap
        return min(max(cap, 2), self.defer_max)

    def _defer_detect(self, res, b):
        """vksift_detectFeatures: staged, or launched at once (the first call after another entry unless the last run held two or more)"""
        run = self.epoch_detects > 0 or self.batch_mode
        self.epoch_detects += 1
        if not (self.defer_on and (run or self.pend_n)):
            return self._defer_flush()
        if self.pend_n:
            if b != self.pend_first + self.pend_n or res != self.pend_res:
                self._defer_flush()
        elif self.defer_grow and self.det_cap < self.defer_max:
            self.det_cap, self.defer_grow = min(2 * self.det_cap, self.defer_max), False
        self.det_cap = max(self.det_cap, 2)
        if self.pend_n == 0:
            self.pend_first, self.pend_res = b, res
        self.pend_n += 1
        if self.pend_n >= min(self.det_cap, self.defer_max):
            self.defer_grow = self.det_cap < self.defer_max
            self._defer_flush()

    def _op_detect(self, k, b):
        self._touch_pairs([b])
        self._store(b, self.w.ref[k], "det", SIZES[k], 0, k)
        self._fill([b])

    def _op_batch(self, ks, b):
        ids = list(range(b, b + len(ks)))
        self._touch_pairs(ids)
        for i, k in zip(ids, ks):
            self._store(i, self.w.ref[k], "det", SIZES[k], 0, k)
        self._fill(ids)
        for i in ids:
            self.batch_of[i] = ids

    def _op_upload(self, k, n, b):
        self._touch_pairs([b])
        self._store(b, self.w.ref[k][:n], "up", None, 0, k)
        self._fill([b])

    def _op_upload_raw(self, recs, b):
        """an upload of records that are not named by (image, length): the CPU stand-in's entry"""
        self._touch_pairs([b])
        self._store(b, np.array(recs, FEATURE_DTYPE), "up", None, 0, None)
        self._fill([b])

    def _op_describe(self, d, b):
        self._touch_pairs([b])
        recs, placed = self.w.desc[d]
        self._store(b, recs, "desc", SIZES[DESCRIBE[d][0]], placed, DESCRIBE[d][0])
        self._fill([b])

    def _op_describe_batch(self, ds, b):
        ids = list(range(b, b + len(ds)))
        self._touch_pairs(ids)
        for i, d in zip(ids, ds):
            recs, placed = self.w.desc[d]
            self._store(i, recs, "desc", SIZES[DESCRIBE[d][0]], placed, DESCRIBE[d][0])
        self._fill(ids)

    def _inplace(self, name, b, cnt, new_recs, max_features=None, cells=None):
        ids = list(range(b, b + cnt))
        self._touch_pairs(ids)
        kinds = {self.bufs[i].kind for i in ids}
        if "up" in kinds and kinds & {"det", "desc"} and len({self.bufs[i].res for i in ids if self.bufs[i].res}) >= 2 and self.layout_runs(ids) >= 3:
            self.label("E3", name)
        whole = self.batch_of.get(b)
        if whole and set(ids) < set(whole):
            self.e8 = (whole, name, set())
        for i in ids:
            x = self.bufs[i]
            if cells is not None and 0 < len(x.recs) < cells and len(x.recs) > max_features:
                self.label("grid cells > features")
            if cells is not None and cells == 1 and len(x.recs) > max_features:
                self.label("grid 1 x 1")
            if x.kind in ("det", "desc") and not x.known:
                self.label("E1", name)
            if x.kind == "up":
                self.label("E2", name)
            cut = max_features is not None and len(x.recs) > max_features
            how = "convert" if max_features is None else "cut" if cut else "noncut"
            x.hist = (x.hist + [f"inplace {name} {how} {'valid' if x.cache else 'invalid'}"])[-4:]
            # the header: a conversion keeps the placed count, a budget call ends it
            if max_features is not None:
                x.placed = 0
            x.recs = new_recs(x.recs)
            # shadow of the host's rules (vksift_strongest.c, vksift_rootsift.c)
            if max_features is None:
                x.cache = self.cache_exists
            elif cut and x.known:
                x.cache = self.cache_exists
            elif not self.cache_exists:
                x.cache = False
            if x.kind != "up":
                x.known = False
        self._fill(ids)

    def _op_budget(self, b, cnt, n):
        self._inplace("budget", b, cnt, lambda r: _as_features(memo("budget", NS.selected_records, _bytes_view(r), n)), n)

    def _op_grid(self, b, cnt, n, w, h, gc, gr):
        self._inplace("grid", b, cnt, lambda r: _as_features(memo("grid", NSP.selected_records, _bytes_view(r), n, w, h, gc, gr)), n, gc * gr)

    def _op_rootsift(self, b, cnt):
        self._inplace("rootsift", b, cnt, lambda r: _as_features(memo("rootsift", NR.convert_records, _bytes_view(r))))

    def _matching(self, kind, pa, pb, ratio=None, cross=None):
        O = self.w.oracle
        first = self.matchings == 0
        for i in dict.fromkeys(list(pa) + list(pb)):
            h = self.bufs[i].hist
            if self.prev and self.prev[0] in INPLACE and self.prev[1] <= i < self.prev[1] + self.prev[2]:
                self.label("E4", self.prev[0])
                if first:
                    self.label("E4 first matching", self.prev[0])
            if h and h[-1].startswith("inplace") and " noncut " in h[-1]:
                self.label("E5", h[-1].split()[-1])
            if len(h) >= 2 and h[-2].startswith("inplace") and h[-1] == "fill":
                self.label("E6")
            if len(h) >= 3 and h[-3] == "describe" and h[-2].startswith("inplace") and h[-1] == "placed":
                self.label("E7", h[-2].split()[2])
        fwd = [memo("match", O.match_2nn, self.rows(a), self.rows(b)) for a, b in zip(pa, pb)]
        filt = None
        if kind == "filtered":
            filt = []
            for k, (a, b) in enumerate(zip(pa, pb)):
                rev = memo("match", O.match_2nn, self.rows(b), self.rows(a)) if cross else None
                ra, rb = memo("filter", O.filter_matches, fwd[k], rev, ratio, cross)
                f = np.zeros(len(ra), FILTERED_MATCH_DTYPE)
                f["idx_a"], f["idx_b"], f["dist_a_b1"], f["dist_a_b2"] = ra, rb, fwd[k]["dist_a_b1"][ra], fwd[k]["dist_a_b2"][ra]
                filt.append(f)
        # the invalidation table (tests/test_gpu_pair_stages.py): a new matching takes every set away, a filtered one brings its own back
        if any(self.sets[s] is not None for s in SETS if s != "filtered"):
            self.label("E9 row", "filtered matching" if kind == "filtered" else "plain matching")
        self.sets = {s: None for s in SETS}
        self.ver = {}
        if filt is not None:
            self.sets["filtered"] = {"filtered n": [len(f).to_bytes(4, "little") for f in filt], "filtered": [f.tobytes() for f in filt]}
        self.match = dict(kind=kind, pa=list(pa), pb=list(pb), fwd=fwd, filt=filt, feats=[(self.rows(a), self.rows(b)) for a, b in zip(pa, pb)])
        self.stale, self.stage_dirty = False, False
        self.matchings += 1
        self.cache_exists = True
        for i in list(pa) + list(pb):
            x = self.bufs[i]
            x.cache = True
            x.hist = (x.hist + ["match"])[-4:]

    def _op_match(self, a, b):
        self._matching("plain", [a], [b])

    def _op_batchmatch(self, pa, pb):
        self._matching("plain", pa, pb)

    def _op_filtered(self, pa, pb, ratio, cross):
        self._matching("filtered", pa, pb, ratio, cross)

    def _corr(self, k):
        fa, fb = self.match["feats"][k]
        return corr(fa, fb, self.match["filt"][k])

    def can_stage(self):
        return self.match is not None and self.match["kind"] == "filtered" and not self.stale

    def _op_verify(self, m, nh, thr, seed):
        assert self.can_stage()
        fn, dtype = (V.ransac, HOMOGRAPHY_DTYPE) if m == "H" else (VF.ransac, FUNDAMENTAL_DTYPE)
        wants = [memo("verify " + m, fn, self._corr(k), nh, thr, seed, k) for k in range(len(self.match["pa"]))]
        if self.sets["refined " + m] is not None:
            self.label("E9 row", "verify " + m + " again")
        self.ver[m] = wants
        self.sets[m] = {m: [_record(dtype, w) for w in wants], m + " mask": [_mask(w) for w in wants]}
        self.sets["refined " + m] = None
        self.stage_dirty = False

    def _op_refine(self, m, rounds, thr):
        assert self.can_stage() and m in self.ver
        fn, dtype = (R.refit, REFINED_HOMOGRAPHY_DTYPE) if m == "H" else (RF.refit, REFINED_FUNDAMENTAL_DTYPE)
        wants = []
        for k, start in enumerate(self.ver[m]):
            s = {"valid": start["valid"], "nb_inliers": start["nb_inliers"], m: start[m]}
            wants.append(memo("refine " + m, lambda c, s, mask, r, t: fn(c, s, mask, r, t), self._corr(k), s, np.asarray(start["mask"]).astype(np.uint8), rounds, thr))
        self.sets["refined " + m] = {"refined " + m: [_record(dtype, w) for w in wants], "refined " + m + " mask": [_mask(w) for w in wants]}
        self.stage_dirty = False

    def _op_guided(self, m, models, thr, ratio, cross):
        assert self.can_stage() and (models is not None or m in self.ver)
        kind = G.HOMOGRAPHY if m == "H" else G.FUNDAMENTAL
        out = []
        for k in range(len(self.match["pa"])):
            fa, fb = self.match["feats"][k]
            M = np.asarray(models[k], np.float32).reshape(9) if models is not None else np.asarray(self.ver[m][k][m], np.float32).reshape(9)
            valid = 1 if models is not None else int(self.ver[m][k]["valid"])

            def go(M, xa, ya, da, xb, yb, db, thr, ratio, cross, valid):
                return G.guided(kind, M, valid, xa, ya, da, xb, yb, db, thr, ratio, float("inf"), cross)
            out.append(memo("guided " + m, go, M, fa["x"].copy(), fa["y"].copy(), fa["descriptor"].copy(), fb["x"].copy(), fb["y"].copy(), fb["descriptor"].copy(),
                            thr, ratio, cross, valid))
        self.sets["guided"] = {"guided n": [len(g).to_bytes(4, "little") for g in out], "guided": [g.tobytes() for g in out]}
        self.stage_dirty = False

    def _op_refuse(self, what, arg):
        # every one of these must be refused with VKSIFT_INVALID_INPUT_ERROR and change nothing
        ok = {"stage without filtered matching": self.match is None or self.match["kind"] != "filtered",
              "guided unverified": self.match is not None and self.match["kind"] == "filtered" and arg not in self.ver,
              "refit unverified": arg not in self.ver,
              "accessor on a dropped set": self.sets[ACCESSORS.get(arg, "filtered")] is None,
              "pair == slots_used": self.sets[ACCESSORS.get(arg, "filtered")] is not None}[what]
        assert ok, (what, arg)
        self.label("E9 refused", what)

    # ---- reads
    def _op_count(self, b):
        self._read(b, "count")

    _op_avail = _op_count

    def _op_download(self, b):
        self._read(b, "download")

    def _op_placed(self, b):
        self._read(b, "placed")

    def _op_export(self, b):
        if self.prev and self.prev[0] in INPLACE and self.prev[1] <= b < self.prev[1] + self.prev[2]:
            self.label("E11", self.prev[0])
        self._read(b, "export")

    def _read(self, b, how):
        self._waited(b)
        x = self.bufs[b]
        x.hist = (x.hist + [how])[-4:]
        if how == "download" and self.e8 is not None and b in self.e8[0]:
            # E8: a batched detection, an in-place operation on part of its range, then downloads of the whole range
            self.e8[2].add(b)
            if self.e8[2] == set(self.e8[0]):
                self.label("E8 packed" if len(self.e8[0]) >= PACK_MIN else "E8", self.e8[1])
                self.e8 = None

    def _op_fetch(self):
        pass

    def _op_pair(self, name, pair):
        if self.stage_dirty and self.sets[ACCESSORS[name]] is not None and ACCESSORS[name] != "filtered":
            self.label("E12", name)

    def observe(self, op):
        """what a reading operation must return; Refused where the call must be refused"""
        name = op[0]
        if name in ("count", "avail"):
            return len(self.bufs[op[1]].recs)
        if name == "download":
            return self.bufs[op[1]].recs.tobytes()
        if name == "placed":
            return self.bufs[op[1]].placed
        if name == "export":
            return self.bufs[op[1]].recs["descriptor"].tobytes()
        if name == "fetch":
            return [m.tobytes() for m in self.match["fwd"]]
        if name == "pair":
            s = self.sets[ACCESSORS[op[1]]]
            if s is None or op[2] >= len(s[op[1]]):
                raise Refused(op)
            return s[op[1]][op[2]]
        raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- generator
def generate(seed, steps, profile, world):
    """the operations of one walk, from model state alone: a prologue (fill, in-place operation, the instance's first matching), then single operations
    and scenarios drawn by probability. Returns (operations, the model they were generated on — its trace holds the edges reached)."""
    rng = np.random.default_rng([seed, sorted(PROFILES).index(profile)])
    m = Model(world)
    ops = []
    nbuf, bc = m.nbuf, m.bc
    same = [k for k in range(len(SIZES)) if SIZES[k] == SIZES[0]]

    def emit(*op):
        m.apply(op)
        ops.append(op)

    def ri(lo, hi):
        return int(rng.integers(lo, hi))

    def pick(seq):
        return seq[ri(0, len(seq))]

    def image():
        return ri(0, len(SIZES))

    def fill(b, how=None):
        how = how or pick(["detect", "detect", "upload", "upload", "describe"])
        if how == "detect":
            emit("detect", image(), b)
        elif how == "upload":
            k = image()
            emit("upload", k, ri(2, len(world.ref[k]) + 1), b)
        else:
            emit("describe", ri(0, len(DESCRIBE)), b)

    def inplace(b, cnt, which=None, bind=None):
        which = which or pick(INPLACE)
        if which == "rootsift":
            return emit("rootsift", b, cnt)
        n0 = len(m.bufs[ri(b, b + cnt)].recs)
        bind = bool(ri(0, 2)) if bind is None else bind
        n = ri(2, max(n0, 3)) if bind else n0 + ri(0, 40) + (0 if n0 else 1)
        if which == "budget":
            return emit("budget", b, cnt, n)
        gc, gr = pick([(1, 1), (2, 2), (4, 3), (16, 16), (3, 1), (16, 9)])
        w, h = m.bufs[b].res or SIZES[0]
        emit("grid", b, cnt, n, w, h, gc, gr)

    def matchable(need_a=1):
        a = [i for i in range(nbuf) if len(m.bufs[i].recs) >= need_a]
        b = [i for i in range(nbuf) if len(m.bufs[i].recs) >= 2]
        return a, b

    def ensure(b, n=2):
        if len(m.bufs[b].recs) < n:
            emit("detect", image(), b)

    def partner(a):
        """a buffer to match a against: with preference one that holds the shifted copy of a's image"""
        _, cand = matchable()
        src = m.bufs[a].src
        twins = [i for i in cand if src is not None and m.bufs[i].src is not None and m.bufs[i].src != src and m.bufs[i].src // 2 == src // 2]
        return pick(twins) if twins and ri(0, 10) < 7 else pick(cand) if cand else None

    def matching(a=None, kind=None):
        if a is None:
            cand, _ = matchable(2)
            if not cand:
                fill(ri(0, nbuf), "detect")
                cand, _ = matchable(2)
            a = pick(cand)
        ensure(a)
        kind = kind or pick(["match", "batchmatch", "filtered"] if bc > 1 else ["match", "filtered"])
        if kind == "match":
            return emit("match", a, partner(a))
        n = ri(1, min(bc, 3) + 1)
        pa = [a] + [pick(matchable(2)[0]) for _ in range(n - 1)]
        pb = [partner(x) for x in pa]
        if kind == "batchmatch":
            return emit("batchmatch", pa, pb)
        emit("filtered", pa, pb, RATIO, bool(ri(0, 4)))

    def pair_read(refused_ok=True):
        name = pick(list(ACCESSORS))
        s = m.sets[ACCESSORS[name]]
        if s is None:
            if m.match is not None and refused_ok and ri(0, 4) == 0:
                emit("refuse", "accessor on a dropped set", name)
            return
        if ri(0, 10) == 0:
            return emit("refuse", "pair == slots_used", name)
        emit("pair", name, ri(0, len(s[name])))

    def stage():
        """one stage run the state allows, or a refused one"""
        if not m.can_stage():
            if m.match is None or m.match["kind"] != "filtered":
                return emit("refuse", "stage without filtered matching", pick(["verify H", "verify F", "refine H", "refine F", "guided H"]))
            return pair_read()                      # stale: no new stage run; what has been computed is still served
        n = len(m.match["pa"])
        kind, r = pick("HF"), ri(0, 100)
        if kind not in m.ver:
            if r < 70:
                return emit("verify", kind, HYPOTHESES, THRESHOLD, ri(0, 1 << 30))
            if r < 80:
                return emit("refuse", "refit unverified", kind)
            if r < 90:
                return emit("refuse", "guided unverified", kind)
        elif r < 20:
            return emit("verify", kind, HYPOTHESES, THRESHOLD, ri(0, 1 << 30))
        elif r < 55:
            return emit("refine", kind, ROUNDS, THRESHOLD)
        elif r < 80:
            return emit("guided", kind, None, THRESHOLD, RATIO, bool(ri(0, 2)))
        if kind == "H":
            models = [[1, 0, float(ri(-6, 7)), 0, 1, float(ri(-6, 7)), 0, 0, 1] for _ in range(n)]
        else:
            models = [[0, 0, 0.001 * ri(1, 9), 0, 0, -1.25, -0.001 * ri(1, 9), 1.25, 0.5 * ri(-4, 5)] for _ in range(n)]
        emit("guided", kind, models, THRESHOLD, RATIO, bool(ri(0, 2)))

    def read(b=None):
        b = ri(0, nbuf) if b is None else b
        emit(pick(["count", "download", "download", "placed", "export", "avail"]), b)

    # ---- scenarios: each aims at edges that single operations reach too rarely
    def sc_inplace_match():                         # E1, E2, E4, E5
        b = ri(0, nbuf)
        if ri(0, 2) or len(m.bufs[b].recs) < 2:
            fill(b)
        ensure(b)
        which = pick(INPLACE)
        inplace(b, 1, which, bind=bool(ri(0, 2)))
        if len(m.bufs[b].recs) >= 2:
            matching(b)

    def sc_sandwich():                              # E5 with a valid entry; the cache against an in-place call or an upload
        b = ri(0, nbuf)
        ensure(b)
        matching(b, "match")
        if ri(0, 4) == 0:
            fill(b, "upload")
        else:
            inplace(b, 1, bind=bool(ri(0, 2)))
        if len(m.bufs[b].recs) >= 2:
            matching(b, pick(["match", "filtered"]))
            emit("fetch")

    def sc_refill():                                # E6
        b = ri(0, nbuf)
        ensure(b)
        inplace(b, 1)
        fill(b, pick(["detect", "upload"]))
        matching(b, "match")
        emit("fetch")

    def sc_describe():                              # E7
        b = ri(0, nbuf)
        if bc > 1 and b + 1 < nbuf and ri(0, 3) == 0:
            emit("describe_batch", list(DESCRIBE_BATCH), b)
        else:
            emit("describe", ri(0, len(DESCRIBE)), b)
        how = pick(["cut", "noncut", "convert"])
        if how == "convert":
            emit("rootsift", b, 1)
        else:
            inplace(b, 1, pick(["budget", "grid"]), bind=how == "cut")
        emit("placed", b)
        if len(m.bufs[b].recs) >= 2:
            matching(b, "match")
            emit("fetch")

    def sc_batch_part():                            # E8
        if bc < 2:
            return sc_inplace_match()
        n = bc if ri(0, 4) else ri(2, bc + 1)
        b = ri(0, nbuf - n + 1)
        first = ri(0, len(same) - n + 1)
        emit("batch", same[first:first + n], b)
        if ri(0, 3) == 0:
            emit("download", b + ri(0, n))            # the packed copy is taken before the in-place call
        lo = ri(0, n)
        inplace(b + lo, ri(1, n - lo + 1))
        for i in rng.permutation(n):
            emit("download", b + int(i))

    def sc_mixed():                                 # E3
        b = ri(0, nbuf - 3)
        order = list(rng.permutation(4))
        for slot, what in zip(range(4), order):
            if what == 0:
                fill(b + slot, "upload")
            elif what == 1:
                emit("detect", pick(same), b + slot)
            elif what == 2:
                emit("detect", pick([8, 9, 10]), b + slot)
            else:
                fill(b + slot)
        inplace(b, 4)
        if ri(0, 2):
            matching(b + ri(0, 4))
        else:
            read(b + ri(0, 4))

    def sc_defer():                                 # E10
        if m.epoch_detects or m.pend_n:
            emit("count", ri(0, nbuf))                # the run starts behind another entry
        if m.defer_full() < 3:
            # two staged images launch at once: a run that fills the capacity makes the next one double it
            b = ri(0, nbuf - 2)
            for i in range(3):
                emit("detect", pick(same), b + i)
            emit("count", b + ri(0, 3))
        staged = ri(2, max(m.defer_full(), 3))         # below what launches the batch by itself
        n = min(staged + (0 if m.batch_mode else 1), nbuf)
        b = ri(0, nbuf - n + 1)
        k = pick(same)
        for i in range(n):
            emit("detect", k if ri(0, 2) else pick(same), b + i)
        end = pick(["budget", "grid", "rootsift", "describe", "match", "export"] + (["batch"] if bc > 1 else []))
        if end in INPLACE:
            inplace(b, ri(1, n + 1), end)
        elif end == "describe":
            emit("describe", ri(0, len(DESCRIBE)), ri(0, nbuf))
        elif end == "match":
            matching(b)
        elif end == "export":
            emit("export", b + ri(0, n))
        else:
            nb = ri(2, bc + 1)
            emit("batch", same[:nb], ri(0, nbuf - nb + 1))

    def sc_export():                                # E11
        b = ri(0, nbuf)
        ensure(b, 1)
        cnt = ri(1, min(3, nbuf - b) + 1)
        inplace(b, cnt)
        emit("export", b + ri(0, cnt))

    def sc_pairs():                                 # E9, E12
        a = None
        twins = [i for i in range(nbuf) if m.bufs[i].src is not None and len(m.bufs[i].recs) >= 2]
        if len(twins) < 2:
            b = ri(0, nbuf - 1)
            emit("detect", 0, b)
            emit("detect", 1, b + 1)
            a = b
        matching(a, "filtered")
        for _ in range(ri(2, 7)):
            stage()
        end = ri(0, 7)
        if end == 0:
            matching(None, "match")                 # row: a plain matching takes everything away, the filtered set too
            emit("refuse", "accessor on a dropped set", pick(["filtered n", "filtered"]))
        elif end == 1:
            matching(None, "filtered")
        elif end in (2, 3) and m.can_stage():      # rows: a new verification of a model takes that model's refit away
            kind = "HF"[end - 2]
            if kind not in m.ver:
                emit("verify", kind, HYPOTHESES, THRESHOLD, ri(0, 1 << 30))
            emit("refine", kind, ROUNDS, THRESHOLD)
            emit("verify", kind, HYPOTHESES, THRESHOLD, ri(0, 1 << 30))
            emit("refuse", "accessor on a dropped set", "refined " + kind + pick(["", " mask"]))
        elif end == 4:                              # E12: a buffer-changing call between the stage and the fetch
            b = pick(m.match["pa"] + m.match["pb"])
            if ri(0, 2):
                inplace(b, 1)
            else:
                fill(b)
        else:
            name = pick([a for a in ACCESSORS if m.sets[ACCESSORS[a]] is not None])
            emit("refuse", "pair == slots_used", name)
        for _ in range(ri(2, 6)):
            pair_read()
        if m.match is not None and ri(0, 2):
            emit("fetch")

    # ---- prologue: the instance's first matching directly behind an in-place operation, no cache block yet (E4)
    b0 = ri(0, nbuf - 1)
    how = pick(["detect", "upload", "batch" if bc > 1 else "detect"])
    if how == "batch":
        emit("batch", same[:2], b0)
    else:
        fill(b0, how)
        fill(b0 + 1, "detect")
    inplace(b0, 2, bind=True)
    ensure(b0)
    ensure(b0 + 1)
    emit(*(("match", b0, b0 + 1) if ri(0, 2) else ("filtered", [b0], [b0 + 1], RATIO, True)))
    emit("fetch")

    scenarios = [sc_inplace_match, sc_sandwich, sc_refill, sc_describe, sc_describe, sc_batch_part, sc_batch_part, sc_batch_part, sc_mixed, sc_defer, sc_defer, sc_defer, sc_export, sc_export,
                 sc_pairs, sc_pairs, sc_pairs]
    while len(ops) < steps:
        r = ri(0, 100)
        if r < 40:
            pick(scenarios)()
        elif r < 46:
            fill(ri(0, nbuf))
        elif r < 50 and bc > 1:
            n = ri(2, bc + 1)
            first = ri(0, len(same) - n + 1)
            emit("batch", same[first:first + n], ri(0, nbuf - n + 1))
        elif r < 55:
            b = ri(0, nbuf)
            inplace(b, ri(1, min(nbuf - b, 4) + 1))
        elif r < 65:
            matching()
        elif r < 72:
            stage()
        elif r < 80:
            pair_read()
        elif r < 85:
            if m.match is not None:
                emit("fetch")
        else:
            read()
    return ops, m


# ---------------------------------------------------------------------------------------------------------------- executor
def run(inst, ops, model, tag=()):
    """every operation against `inst` (Real, or a stand-in with its methods) and against `model`; every observable byte for byte. inst.Error is the
    exception a refused call raises, with the result code in .code."""
    w = model.w
    mode_of = lambda d: DESCRIBE[d][3]
    for step, op in enumerate(ops):
        ctx = tag + (step, op[0], op[1:] if op[0] != "guided" or op[2] is None else (op[1], "own models") + op[3:])
        name = op[0]
        if name == "refuse":
            model.apply(op)
            with_raise(inst, lambda: _refused_call(inst, model, op), ctx)
            continue
        if name == "pair":
            model.apply(op)
            try:
                want = model.observe(op)
            except Refused:
                with_raise(inst, lambda: inst.pair_read(op[1], op[2]), ctx)
                continue
            got = inst.pair_read(op[1], op[2])
            assert got[:len(want)] == want, ctx
            assert not any(got[len(want):]), (ctx, "bytes written behind the payload")
            continue
        if name == "detect":
            inst.detectFeatures(w.imgs[op[1]], op[2])
        elif name == "batch":
            inst.detectFeaturesBatch([w.imgs[k] for k in op[1]], op[2])
        elif name == "upload":
            inst.uploadFeatures(w.ref[op[1]][:op[2]].copy(), op[3])
        elif name == "describe":
            inst.describeKeypoints(w.imgs[DESCRIBE[op[1]][0]], w.kps[op[1]], op[2], mode_of(op[1]))
        elif name == "describe_batch":
            inst.describeKeypointsBatch([w.imgs[DESCRIBE[d][0]] for d in op[1]], [w.kps[d] for d in op[1]], op[2], mode_of(op[1][0]))
        elif name == "budget":
            inst.keepStrongestFeatures(op[1], op[2], op[3])
        elif name == "grid":
            inst.keepStrongestFeaturesGrid(*op[1:])
        elif name == "rootsift":
            inst.convertToRootSift(op[1], op[2])
        elif name == "match":
            inst.matchFeatures(op[1], op[2])
        elif name == "batchmatch":
            inst.matchFeaturesBatch(op[1], op[2])
        elif name == "filtered":
            inst.matchFeaturesFiltered(op[1], op[2], op[3], op[4])
        elif name == "verify":
            (inst.verifyHomography if op[1] == "H" else inst.verifyFundamental)(op[2], op[3], op[4])
        elif name == "refine":
            (inst.refineHomography if op[1] == "H" else inst.refineFundamental)(op[2], op[3])
        elif name == "guided":
            inst.matchFeaturesGuided(G.HOMOGRAPHY if op[1] == "H" else G.FUNDAMENTAL, None if op[2] is None else np.asarray(op[2], np.float32), op[3], op[4],
                                     float("inf"), op[5])
        model.apply(op)
        if name == "count":
            assert inst.getFeaturesNumber(op[1]) == model.observe(op), ctx
        elif name == "avail":
            assert inst.getFeaturesNumber(op[1]) == model.observe(op), ctx          # waits for anything pending on the buffer
            assert inst.isBufferAvailable(op[1]), ctx
        elif name == "download":
            assert inst.downloadFeatures(op[1]).tobytes() == model.observe(op), ctx
        elif name == "placed":
            assert inst.getPlacedKeypointsNumber(op[1]) == model.observe(op), ctx
        elif name == "export":
            assert inst.export(op[1]) == model.observe(op), ctx
        elif name == "fetch":
            want = model.observe(op)
            if model.match["kind"] == "plain" and len(want) == 1:
                assert inst.downloadMatches().tobytes() == want[0], ctx
            else:
                for k, e in enumerate(want):
                    assert inst.downloadMatchesBatch(k).tobytes() == e, ctx + (k,)
                assert inst.downloadMatches().tobytes() == want[0], ctx + ("pair 0",)
    for b in range(model.nbuf):
        assert inst.getFeaturesNumber(b) == len(model.bufs[b].recs), tag + ("final count", b)
        assert inst.downloadFeatures(b).tobytes() == model.bufs[b].recs.tobytes(), tag + ("final", b)
        assert inst.getPlacedKeypointsNumber(b) == model.bufs[b].placed, tag + ("final placed", b)
    # the model's restatement of the deferral is the host's: batches launched from staged detections, and images in them
    assert tuple(inst.getDeferredStats()) == (model.defer_batches, model.defer_images), tag + ("final deferred stats",)


def with_raise(inst, call, ctx):
    try:
        call()
    except inst.Error as e:
        assert e.code == INVALID_INPUT, ctx
        return
    raise AssertionError((ctx, "the call was not refused"))


def _refused_call(inst, model, op):
    what, arg = op[1], op[2]
    if what == "accessor on a dropped set":
        return inst.pair_read(arg, 0)
    if what == "pair == slots_used":
        return inst.pair_read(arg, len(model.sets[ACCESSORS[arg]][arg]))
    if what == "refit unverified":
        return (inst.refineHomography if arg == "H" else inst.refineFundamental)(ROUNDS, THRESHOLD)
    if what == "guided unverified":
        return inst.matchFeaturesGuided(G.HOMOGRAPHY if arg == "H" else G.FUNDAMENTAL, None, THRESHOLD, RATIO, float("inf"), True)
    return {"verify H": lambda: inst.verifyHomography(HYPOTHESES, THRESHOLD, 1), "verify F": lambda: inst.verifyFundamental(HYPOTHESES, THRESHOLD, 1),
            "refine H": lambda: inst.refineHomography(ROUNDS, THRESHOLD), "refine F": lambda: inst.refineFundamental(ROUNDS, THRESHOLD),
            "guided H": lambda: inst.matchFeaturesGuided(G.HOMOGRAPHY, np.eye(3, dtype=np.float32).reshape(1, 9).repeat(max(model.bc, 1), 0), THRESHOLD, RATIO,
                                                         float("inf"), True)}[arg]()


# ---------------------------------------------------------------------------------------------------------------- the real instance
class Real:
    """vulkansift_amd.api.Instance with the two reads the executor needs beside its methods: pair_read (one of the twelve per-pair accessors of the C
    API, into a zeroed buffer as large as any pair's payload can be) and export (vksift_ext_exportDescriptorsDevice into device memory of its own)"""

    def __init__(self, vk, inst, dev=None):
        self.vk, self.inst, self.Error, self._dev = vk, inst, vk.VksiftError, dev
        L, nb = vk.lib(), inst.cfg.max_nb_sift_per_buffer
        self._acc = {"filtered n": (L.vksift_ext_getFilteredMatchesNumber, None), "filtered": (L.vksift_ext_downloadFilteredMatches, 16 * nb),
                     "H": (L.vksift_ext_getHomography, 52), "H mask": (L.vksift_ext_downloadInlierMask, nb),
                     "F": (L.vksift_ext_getFundamental, 56), "F mask": (L.vksift_ext_downloadFundamentalInlierMask, nb),
                     "refined H": (L.vksift_ext_getRefinedHomography, 52), "refined H mask": (L.vksift_ext_downloadRefinedInlierMask, nb),
                     "refined F": (L.vksift_ext_getRefinedFundamental, 52), "refined F mask": (L.vksift_ext_downloadRefinedFundamentalInlierMask, nb),
                     "guided n": (L.vksift_ext_getGuidedMatchesNumber, None), "guided": (L.vksift_ext_downloadGuidedMatches, 16 * nb)}

    def __getattr__(self, name):
        return getattr(self.inst, name)

    def pair_read(self, name, pair):
        fn, nbytes = self._acc[name]
        if nbytes is None:
            n = fn(self.inst._h, pair)
            self.vk._check_pending()
            return int(n).to_bytes(4, "little")
        out = np.zeros(nbytes, np.uint8)
        fn(self.inst._h, pair, out.ctypes.data)
        self.vk._check_pending()
        return out.tobytes()

    def export(self, b):
        import torch

        rows = self.inst.cfg.max_nb_sift_per_buffer
        if self._dev is None or self._dev.numel() < rows * 128:
            self._dev = torch.zeros(rows * 128, dtype=torch.uint8, device="cuda")
        n = self.inst.exportDescriptorsDevice(b, self._dev.data_ptr())
        torch.cuda.synchronize()
        return self._dev[:n * 128].cpu().numpy().tobytes()
