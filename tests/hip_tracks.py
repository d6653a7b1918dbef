"""Direct access to the track launcher of include/vksift_hip.h for tests (plain module, no fixtures): vksift_hip_build_tracks with
vksift_hip_tracks_scratch_u32.

  * bind(): the ctypes argtypes of the two entries
  * Tracks turns a case of tests/track_cases.py into ONE byte tensor, in the manner of tests/hip_two_view.py (whose TwoView it extends; device "cpu" lays
    out the same bytes without a GPU): every input and output block between guard zones of its own; the stride padding of records and masks, the node words
    (all of them: rows that are not stored must stay as they are), the track records and the words behind the four statistics poisoned with 0xA5; the
    counter words between the strided ones — record counts and row counts — hold track_cases.JUNK_COUNTER; the words between the strided valid words and
    slot table entries are decoys
  * launch(L, **changes) / expected() / check(): as in hip_records
  * the scratch is handed over with exactly the words vksift_hip_tracks_scratch_u32 asks for (scratch_words() restates the number). Its contents after a
    launch are unspecified: read() puts the bytes the launch found there back before the comparison — the payload only, the guard zones and the block
    behind it stay compared
"""
import ctypes as C

import numpy as np

import track_cases as TC
from hip_records import HIP_ERROR_INVALID_VALUE  # noqa: F401  (re-exported for the tests)
from hip_two_view import TwoView

u32 = np.uint32


def bind(L):
    vp, w, q, z = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    L.vksift_hip_build_tracks.argtypes = [vp, q, vp, w, w, vp, q, vp, w, vp, w, w, vp, w, vp, w, w, vp, vp, q, vp, vp, z, vp]
    L.vksift_hip_build_tracks.restype = C.c_int
    L.vksift_hip_tracks_scratch_u32.argtypes = [w, w]
    L.vksift_hip_tracks_scratch_u32.restype = z
    return L


def scratch_words(nbufs, node_stride):
    """what vksift_hip_tracks_scratch_u32(nbufs, node_stride) asks for: five words per node, three per block of 256 rows, 64 edge counters, and two"""
    return 5 * nbufs * node_stride + 3 * nbufs * ((node_stride + 255) // 256) + 64 + 2


class Tracks(TwoView):
    entry = "build_tracks"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c, pairs = case, case["pairs"]
        self.ids = [b for b, _ in c["bufs"]]
        assert self.ids == sorted(set(self.ids))
        self.nbufs, self.ns, self.stride = len(self.ids), len(pairs), c["node_stride"]
        rank = {b: r for r, b in enumerate(self.ids)}
        self.rec_stride, self.mask_stride = 16 * (c["max_n"] + c["rec_extra"]), c["max_n"] + c["mask_extra"]
        held = [p["recs"][:c["max_n"] + c["rec_extra"]] for p in pairs]
        full = [np.concatenate([h, np.full((len(h), 2), 0xA5A5A5A5, u32)], axis=1) for h in held]     # 16-byte records: the distances are never read
        self.records = self.slotted("records", self.rec_stride, full, row_bytes=16)
        self.n = self.strided_words("record counts", c["n_stride"], [[p["n_dev"]] for p in pairs], TC.JUNK_COUNTER)
        self.masks = self.valid = None
        if c["masked"]:
            self.masks = self.slotted("masks", self.mask_stride, [p["mask"][:self.mask_stride] for p in pairs], row_bytes=1)
            valid = np.array([[p["valid"]] + [0 if p["valid"] else 1] * (c["valid_stride"] - 1) for p in pairs], u32)
            self.valid = self.block("valid words", valid, slot_bytes=4 * c["valid_stride"], row_bytes=4)
        self.tab = self.strided_words("slot table", c["tab_stride"], [[rank[p["a"]], rank[p["b"]]] for p in pairs], 0)
        # a buffer's row count lives at word 4 r + 1 of the row counters; every other word is junk
        self.count_word = [4 * r + 1 for r in range(self.nbufs)]
        self.buf_tab = self.block("buffer table", np.array([[b, w] for b, w in zip(self.ids, self.count_word)], u32), row_bytes=8)
        rows = np.full(4 * self.nbufs + 2, TC.JUNK_COUNTER, u32)
        rows[self.count_word] = [n for _, n in c["bufs"]]
        self.rows = self.block("row counters", rows, row_bytes=4)
        self.node_words = self.poison("node words", 4 * self.nbufs * self.stride, slot_bytes=4 * self.stride, row_bytes=4)
        self.cap = self.nbufs * c["max_rows"] // 2
        self.tracks = self.poison("track records", 16 * (self.cap + 2), row_bytes=16)
        self.stats = self.poison("statistics", 4 * 6, row_bytes=4)
        self.scratch = self.scratch_block(scratch_words(self.nbufs, self.stride))
        self.behind = self.poison("behind the scratch", 64)
        self.build()
        self.free = [(self.scratch, 0, 4 * self.scratch_u32)]
        self.args = dict(records=self.records.ptr, rec_slot_stride=self.rec_stride, n_dev=self.n.ptr, n_stride=c["n_stride"], max_n=c["max_n"],
                         masks=self.masks.ptr if self.masks else None, mask_slot_stride=self.mask_stride if self.masks else 0,
                         valid=self.valid.ptr if self.valid else None, valid_stride=c["valid_stride"] if self.valid else 0, slot_tab=self.tab.ptr,
                         slot_tab_stride=c["tab_stride"], nslots=self.ns, buf_tab=self.buf_tab.ptr, nbufs=self.nbufs, rows_dev=self.rows.ptr, node_stride=self.stride,
                         max_rows=c["max_rows"], node_words=self.node_words.ptr, tracks=self.tracks.ptr, tracks_cap=self.cap, stats=self.stats.ptr,
                         scratch=self.scratch.ptr, scratch_u32=self.scratch_u32)

    def expected(self):
        exp = self.host.copy()
        rec, words, stats = TC.expected(self.case)
        assert len(rec) <= self.cap
        self.put(exp, self.tracks, 0, rec)
        for r, b in enumerate(self.ids):
            self.put(exp, self.node_words, 4 * r * self.stride, words[b])
        self.put(exp, self.stats, 0, np.array([stats[k] for k in ("nb_tracks", "nb_conflicting", "nb_features", "nb_edges")], u32))
        return exp

    def outputs(self, raw):
        """the bytes of the three output blocks"""
        return [self.view(raw, b).copy() for b in (self.tracks, self.node_words, self.stats)]
