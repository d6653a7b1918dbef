"""Direct access to the two-view launchers of include/vksift_hip.h for tests (plain module, no fixtures): vksift_hip_ransac_homography,
_ransac_fundamental, _refit_homography, _refit_fundamental and _match_guided, with vksift_hip_ransac_scratch_u32 / _guided_scratch_u32.

  * bind(): the ctypes argtypes of the seven entries
  * one class per launch (RansacH, RansacF, RefitH, RefitF, Guided) that turns a case of tests/two_view_cases.py into ONE byte tensor, in the
    manner of tests/hip_records.py (whose Launch they extend; device "cpu" lays out the same bytes without a GPU): every input and output
    block between guard zones of its own; stride padding, rows at and beyond n (where the case has no decoys there), records beyond nslots,
    mask bytes at and beyond n and guided output rows at and beyond out_n poisoned with 0xA5; the counter words between the strided ones hold
    two_view_cases.JUNK_COUNTER
  * launch(L, **changes) / expected() / check(): as in hip_records. expected() calls the restatements on rows [0, min(n_dev, max_n))
  * the scratch is handed over with exactly the words the *_scratch_u32 function asks for (scratch_words() restates the number, the GPU
    test compares it with the library's). Its contents after a launch are unspecified: read() puts the bytes the launch found there back
    into `free` ranges before the comparison — the payload only, the scratch's guard zones and the block behind it stay compared; the key
    scratch of a guided slot whose valid word is 0 is NOT free (guided.hip leaves such slots alone)
"""
import ctypes as C

import numpy as np

import two_view_cases as T
from hip_features import POISON_BYTE
from hip_records import HIP_ERROR_INVALID_VALUE, Launch  # noqa: F401  (re-exported for the tests)

u32, f32 = np.uint32, np.float32


def bind(L):
    vp, w, q, f, z = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t
    ransac = [vp, q, vp, w, w, w, w, f, q, vp, vp, q, vp, z, vp]
    refit = [vp, q, vp, w, w, w, vp, vp, q, w, f, vp, vp, vp]
    sigs = {
        "vksift_hip_ransac_homography": ransac, "vksift_hip_ransac_fundamental": ransac, "vksift_hip_refit_homography": refit, "vksift_hip_refit_fundamental": refit,
        "vksift_hip_match_guided": [vp, q, vp, q, vp, w, vp, q, vp, w, w, vp, w, vp, w, w, f, f, f, w, w, vp, q, vp, vp, z, vp],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    for name in ("vksift_hip_ransac_scratch_u32", "vksift_hip_guided_scratch_u32"):
        getattr(L, name).argtypes = [w, w]
        getattr(L, name).restype = z
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


class TwoView(Launch):
    """what the five launches share: blocks laid out slot by slot, and scratch whose contents are not compared"""

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        self.free = []     # (block, first byte, end byte) of payload the contract leaves unspecified

    def slotted(self, name, stride, parts, *, tail=0, row_bytes=None):
        """a poisoned block of len(parts) slots `stride` bytes apart and `tail` bytes behind them, slot k starting with the bytes parts[k]"""
        flat = np.full(len(parts) * stride + tail, POISON_BYTE, np.uint8)
        for k, p in enumerate(parts):
            p = np.ascontiguousarray(p).view(np.uint8).reshape(-1)
            assert len(p) <= stride
            flat[k * stride:k * stride + len(p)] = p
        return self.block(name, flat, slot_bytes=stride, row_bytes=row_bytes)

    def strided_words(self, name, stride, values, gap):
        """uint32 words: slot k holds values[k] (a sequence) and then `gap` up to `stride` words"""
        words = np.full((len(values), stride), gap, u32)
        for k, v in enumerate(values):
            words[k, :len(v)] = v
        return self.block(name, words, slot_bytes=4 * stride, row_bytes=4)

    def put(self, exp, blk, off, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.view(exp, blk)[off:off + len(data)] = data

    def read(self):
        after = super().read()
        for blk, lo, hi in self.free:
            after[blk.off + lo:blk.off + hi] = self.host[blk.off + lo:blk.off + hi]
        return after

    def scratch_block(self, words):
        self.scratch_u32 = int(words)
        return self.poison("scratch", 4 * max(self.scratch_u32, 1), row_bytes=4)

    def corr_blocks(self, case, slots):
        """the correspondences (every row the slot holds: decoys behind n included) and the strided counters"""
        self.max_n, self.ns = case["max_n"], len(slots)
        self.corr_stride, self.mask_stride = 16 * (case["max_n"] + case["corr_extra"]), case["max_n"] + case["mask_extra"]
        self.pass_strides = case["strides"] if case["strides"] is not None else (self.corr_stride, self.mask_stride)
        assert case["strides"] is None or self.ns == 1
        self.corr = self.slotted("correspondences", self.corr_stride, [s["rows"] for s in slots], row_bytes=16)
        self.n = self.strided_words("counters", case["n_stride"], [[s["n_dev"]] for s in slots], T.JUNK_COUNTER)
        self.slot_n = [min(s["n_dev"], case["max_n"]) for s in slots]


def model_words(r, key, tail):
    return np.concatenate([np.asarray(r[key], f32).reshape(9).view(u32), np.array([int(r[k]) for k in tail], u32)])


def ransac_record(m, r):
    """the 13 / 14 words of a RANSAC record"""
    return model_words(r, T.MODEL_KEY[m], ["nb_matches", "nb_inliers", "best_hypothesis"] + (["best_root"] if m == "f" else []) + ["valid"])


# ---------------------------------------------------------------------------------------------------------------------- RANSAC
class Ransac(TwoView):
    model = None

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        assert case["model"] == self.model
        c = case
        self.words = T.RANSAC_WORDS[self.model]
        self.corr_blocks(c, c["slots"])
        self.results = self.poison("records", (self.ns + 2) * 4 * self.words, row_bytes=4 * self.words)
        self.masks = self.poison("masks", self.ns * self.mask_stride, slot_bytes=self.mask_stride, row_bytes=1)
        self.scratch = self.scratch_block(scratch_words(self.entry, self.ns, c["nb_hyp"]))
        self.behind = self.poison("behind the scratch", 64)
        self.build()
        self.free = [(self.scratch, 0, 4 * self.scratch_u32)]
        self.args = dict(corr=self.corr.ptr, corr_slot_stride=self.pass_strides[0], n_dev=self.n.ptr, n_stride=c["n_stride"], max_n=c["max_n"], nslots=self.ns,
                         nb_hypotheses=c["nb_hyp"], threshold_px=c["thr"], seed=c["seed"], results=self.results.ptr, masks=self.masks.ptr,
                         mask_slot_stride=self.pass_strides[1], scratch=self.scratch.ptr, scratch_u32=self.scratch_u32)

    def expected(self):
        exp = self.host.copy()
        for k, r in enumerate(T.ransac_expected(self.case)):
            assert r["nb_matches"] == self.slot_n[k] == len(r["mask"])
            self.put(exp, self.results, k * 4 * self.words, ransac_record(self.model, r))
            self.put(exp, self.masks, k * self.mask_stride, r["mask"].astype(np.uint8))
        return exp


class RansacH(Ransac):
    entry, model = "ransac_homography", "h"


class RansacF(Ransac):
    entry, model = "ransac_fundamental", "f"


# ---------------------------------------------------------------------------------------------------------------------- refits
class Refit(TwoView):
    model = None

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        assert case["model"] == self.model
        c, base, slots = case, case["base"], T.refit_slots(case)
        self.start_words = T.RANSAC_WORDS[self.model]
        self.corr_blocks(base, slots)
        self.start_results = self.slotted("start records", 4 * self.start_words, [ransac_record(self.model, s["start"]) for s in slots], tail=4 * self.start_words)
        # a start mask is n bytes; where the slot holds decoy rows behind them their bytes are 1 (a kernel that read on would refit on them too)
        marks = [np.concatenate([s["start_mask"][:n], np.ones(min(len(s["rows"]), self.mask_stride) - n, np.uint8)]) for s, n in zip(slots, self.slot_n)]
        self.start_masks = self.slotted("start masks", self.mask_stride, marks, tail=c["start_slack"], row_bytes=1)
        self.results = self.poison("records", (self.ns + 2) * 4 * T.REFIT_WORDS, row_bytes=4 * T.REFIT_WORDS)
        self.masks_out = self.poison("masks_out", self.ns * self.mask_stride + c["out_slack"], slot_bytes=self.mask_stride, row_bytes=1)
        self.build()
        self.args = dict(corr=self.corr.ptr, corr_slot_stride=self.pass_strides[0], n_dev=self.n.ptr, n_stride=base["n_stride"], max_n=base["max_n"], nslots=self.ns,
                         start_results=self.start_results.ptr, start_masks=self.start_masks.ptr, mask_slot_stride=self.pass_strides[1], nb_rounds=c["nb_rounds"],
                         threshold_px=c["thr"], results=self.results.ptr, masks_out=self.masks_out.ptr)

    def launch(self, L, **changes):
        """masks_out may be given relative to start_masks: "start_masks", "start_masks+1", "start_masks-1" (the overlap refusals; +-1: slots apart by
        one byte more / less than nothing, still inside the extent the launch would write)"""
        v = changes.get("masks_out")
        if isinstance(v, str):
            changes["masks_out"] = self.args["start_masks"] + int(v[len("start_masks"):] or 0)
        return super().launch(L, **changes)

    def expected(self):
        exp = self.host.copy()
        key = T.MODEL_KEY[self.model]
        for k, r in enumerate(T.refit_expected(self.case)):
            assert len(r["mask"]) == self.slot_n[k] and r["nb_matches"] == (self.slot_n[k] if r["valid"] else 0)
            self.put(exp, self.results, k * 4 * T.REFIT_WORDS, model_words(r, key, ["nb_matches", "nb_inliers", "rounds", "valid"]))
            self.put(exp, self.masks_out, k * self.mask_stride, r["mask"].astype(np.uint8))
        return exp


class RefitH(Refit):
    entry, model = "refit_homography", "h"


class RefitF(Refit):
    entry, model = "refit_fundamental", "f"


# ---------------------------------------------------------------------------------------------------------------------- guided matching
def shifted_norms(desc):
    d = np.asarray(desc, np.int64) - 128
    return (d * d).sum(axis=1).astype(u32)


class Guided(TwoView):
    entry = "match_guided"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c, slots, mx = case, case["slots"], case["max_n"]
        self.ns = ns = len(slots)
        rows = mx + c["desc_extra"]
        self.desc_stride, self.norm_stride, self.xy_stride, self.out_stride = 128 * rows, rows + c["norm_extra"], mx + c["xy_extra"], 16 * mx + 4 * c["out_extra"]
        held = [e if e is not None else np.zeros((0, 128), np.uint8) for e in c["entries"]]
        self.desc = self.slotted("cache rows", self.desc_stride, held, row_bytes=128)
        self.norms = self.slotted("cache norms", 4 * self.norm_stride, [shifted_norms(e) for e in held], row_bytes=4)
        # the words between the strided ones are decoys: an entry, a count, model entries and a valid word a kernel that ignored the stride would use
        self.tab = self.strided_words("slot table", c["tab_stride"], [s["tab"] for s in slots], 0)
        self.xy = self.slotted("coordinates", 8 * self.xy_stride, [s["xy"][t] for s in slots for t in (0, 1)], row_bytes=8)
        self.n = self.strided_words("counters", c["n_stride"], [s["n_dev"] for s in slots], T.JUNK_COUNTER)
        self.models = self.strided_words("models", c["model_stride"], [s["models"][c["kind"]].view(u32) for s in slots], int(f32(1.0).view(u32)))
        valid = np.array([[s["valid"]] + [0 if s["valid"] else 1] * (c["valid_stride"] - 1) for s in slots], u32)
        self.valid = self.block("valid words", valid, slot_bytes=4 * c["valid_stride"], row_bytes=4)
        self.out = self.poison("records", ns * self.out_stride, slot_bytes=self.out_stride, row_bytes=16)
        self.out_n = self.poison("record counts", (ns + 2) * 4, row_bytes=4)
        self.scratch = self.scratch_block(scratch_words(self.entry, ns, mx))
        self.behind = self.poison("behind the scratch", 64)
        self.build()
        per_slot = 32 * mx    # bytes of key scratch per slot: two directions of max_n pairs of 64-bit keys
        self.free = [(self.scratch, k * per_slot, (k + 1) * per_slot) for k, s in enumerate(slots) if s["valid"]]
        self.args = dict(cache_desc=self.desc.ptr, cache_desc_stride=self.desc_stride, cache_norm=self.norms.ptr, cache_norm_stride=self.norm_stride,
                         slot_tab=self.tab.ptr, slot_tab_stride=c["tab_stride"], xy=self.xy.ptr, xy_side_stride=self.xy_stride, n_dev=self.n.ptr, n_stride=c["n_stride"],
                         max_n=mx, models=self.models.ptr, model_stride=c["model_stride"], valid=self.valid.ptr, valid_stride=c["valid_stride"],
                         model_kind=T.KIND[c["kind"]], t2=float(T.G.threshold2(c["thr"])), ratio=c["ratio"], max_distance=c["max_distance"],
                         cross_check=c["cross_check"], nslots=ns, out=self.out.ptr, out_slot_stride=self.out_stride, out_n=self.out_n.ptr, scratch=self.scratch.ptr,
                         scratch_u32=self.scratch_u32)

    def expected(self):
        exp = self.host.copy()
        for k, recs in enumerate(T.guided_expected(self.case)):
            self.put(exp, self.out, k * self.out_stride, recs)
            self.put(exp, self.out_n, 4 * k, np.array([len(recs)], u32))
        return exp


def scratch_words(entry, nslots, count):
    """what vksift_hip_ransac_scratch_u32(nslots, nb_hypotheses) / vksift_hip_guided_scratch_u32(nslots, max_n) ask for"""
    return nslots * count * 8 if entry == "match_guided" else 2 * nslots * ((count + 255) // 256)


LAUNCHES = {"ransac_homography": RansacH, "ransac_fundamental": RansacF, "refit_homography": RefitH, "refit_fundamental": RefitF, "match_guided": Guided}
