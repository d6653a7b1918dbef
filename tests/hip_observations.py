"""Direct access to the observation launcher of include/vksift_hip.h for tests (plain module, no fixtures): vksift_hip_track_observations with
vksift_hip_observations_scratch_u32, behind a vksift_hip_build_tracks of the same case (tests/hip_tracks.py, whose arena holds this launch's inputs).

  * bind(): the ctypes argtypes of the two entries
  * Observations turns a launched hip_tracks.Tracks plus the selection's parameters into ONE byte tensor of its own, in the manner of tests/hip_two_view.py:
    the SIFT buffers (one per gpu_buffer_id up to the largest, EVERY record of every buffer with a float pattern of its own in its first two words, so a
    read of the wrong record shows), their section counters, the layout tables and the per-rank layout words, then the poisoned outputs — offsets, track
    ids, observations, the words behind the four statistics — and the scratch, each between guard zones
  * the buffer of rank r is laid out by r % 3: dense (VKSIFT_LAYOUT_DENSE | n); three sections with room to spare (cap > found); three sections that
    are clamped (found > cap). Sections start at gaps from each other, so download order is not storage order
  * launch(L, **changes) / expected() / check(): as in hip_records. expected() is tests/np_observations.py on tests/np_tracks.py's outputs
  * the scratch is handed over with exactly the words vksift_hip_observations_scratch_u32 asks for (scratch_words() restates the number), uninitialised
    (poison); read() puts the bytes the launch found there back before the comparison
"""
import ctypes as C

import numpy as np

import np_observations as NO
import track_cases as TC
from hip_records import HIP_ERROR_INVALID_VALUE  # noqa: F401  (re-exported for the tests)
from hip_two_view import TwoView

u32, f32 = np.uint32, np.float32
REC_WORDS, DENSE = 41, 0x80000000
LAYOUT_WORDS, NSEC, FOUND_STRIDE = 33, 3, 5


def bind(L):
    vp, w, q, z = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    L.vksift_hip_track_observations.argtypes = [vp, vp, vp, vp, w, vp, w, w, vp, q, vp, w, vp, vp, w, w, w, vp, vp, q, vp, q, vp, vp, z, vp]
    L.vksift_hip_track_observations.restype = C.c_int
    L.vksift_hip_observations_scratch_u32.argtypes = [w, w, w]
    L.vksift_hip_observations_scratch_u32.restype = z
    return L


def scratch_words(nbufs, node_stride, max_rows):
    """what vksift_hip_observations_scratch_u32 asks for: two words per node, four per element of whole sort blocks of 2048, 256 per sort block, one per
    possible track, four per block of 256 possible tracks, and two"""
    tracks = nbufs * max_rows // 2
    sort_blocks = (nbufs * ((max_rows + 255) // 256) * 256 + 2047) // 2048
    return 2 * nbufs * node_stride + 4 * 2048 * sort_blocks + 256 * sort_blocks + tracks + 4 * max((tracks + 255) // 256, 1) + 2


def buffer_layout(rank, n):
    """-> (layout: None for dense or (off[3], cap[3], found[3]), rows of storage, stored row of every download-order row)"""
    if rank % 3 == 0:
        return None, n + 1, np.arange(n, dtype=np.int64)
    cnt = [n // 2, n // 3, n - n // 2 - n // 3]
    clamp = rank % 3 == 2
    cap = [c if clamp else c + 2 for c in cnt]
    found = [c + 5 + o if clamp else c for o, c in enumerate(cnt)]
    off, at = [], 1
    for c in cap:
        off.append(at)
        at += c + 2
    stored = np.concatenate([off[o] + np.arange(cnt[o], dtype=np.int64) for o in range(NSEC)])
    return (off, cap, found), at, stored


class Observations(TwoView):
    entry = "track_observations"

    def __init__(self, tracks, min_length=2, max_length=0, conflicts=0, device="cuda"):
        c = tracks.case
        super().__init__(dict(c, name=f"{c['name']} / min {min_length} max {max_length} conflicts {conflicts}"), device)
        self.t, self.params = tracks, (min_length, max_length, conflicts)
        self.nbufs, self.stride, self.max_rows = tracks.nbufs, tracks.stride, c["max_rows"]
        rows = {b: min(n, self.max_rows) for b, n in c["bufs"]}
        lay = {b: buffer_layout(r, rows[b]) for r, b in enumerate(tracks.ids)}
        nslots, cap_rows = max(tracks.ids) + 1, max(v[1] for v in lay.values())
        self.buf_stride = 4 * REC_WORDS * cap_rows + 8
        # every record of every buffer: {pattern, pattern + 1} in its first two words (never equal between two records), 0xC3 bytes behind them
        words = np.full((nslots, self.buf_stride // 4), 0xC3C3C3C3, u32)
        phys = np.arange(cap_rows, dtype=np.int64)
        for b in range(nslots):
            words[b, phys * REC_WORDS] = (0x3F000000 + ((b * cap_rows + phys) * 2) % 0x00800000).astype(u32)
            words[b, phys * REC_WORDS + 1] = words[b, phys * REC_WORDS] + 1
        self.feats = self.block("SIFT buffers", words, slot_bytes=self.buf_stride, row_bytes=4 * REC_WORDS)
        found = np.full((nslots, FOUND_STRIDE), TC.JUNK_COUNTER, u32)
        tables, rank_words, self.xy = [np.full(LAYOUT_WORDS, 7, u32)], [], {}      # table 0: a decoy
        for b in tracks.ids:
            sections, _, stored = lay[b]
            if sections is None:
                rank_words.append(DENSE | rows[b])
            else:
                off, cap, fnd = sections
                t = np.zeros(LAYOUT_WORDS, u32)
                t[0], t[1:1 + NSEC], t[17:17 + NSEC] = NSEC, off, cap
                t[1 + NSEC:17], t[17 + NSEC:] = 999999, 999999         # entries at and beyond nsec are not read
                rank_words.append(len(tables))
                tables.append(t)
                found[b, :NSEC] = fnd
            self.xy[b] = words[b].reshape(-1)[:cap_rows * REC_WORDS].reshape(cap_rows, REC_WORDS)[stored, :2].copy().view(f32)
        self.found = self.block("section counters", found, slot_bytes=4 * FOUND_STRIDE, row_bytes=4)
        self.layouts = self.block("layout tables", np.stack(tables), slot_bytes=4 * LAYOUT_WORDS, row_bytes=4)
        self.rank_layouts = self.block("layout words", np.array(rank_words + [0x7FFFFFFF], u32), row_bytes=4)
        self.tracks_cap, self.obs_cap = self.nbufs * self.max_rows // 2, self.nbufs * self.max_rows
        self.offsets = self.poison("offsets", 4 * (self.tracks_cap + 3), row_bytes=4)
        self.track_ids = self.poison("track ids", 4 * (self.tracks_cap + 2), row_bytes=4)
        self.obs = self.poison("observations", 16 * (self.obs_cap + 2), row_bytes=16)
        self.stats = self.poison("statistics", 4 * 6, row_bytes=4)
        self.scratch = self.scratch_block(scratch_words(self.nbufs, self.stride, self.max_rows))
        self.behind = self.poison("behind the scratch", 64)
        self.build()
        self.free = [(self.scratch, 0, 4 * self.scratch_u32)]
        t = tracks
        self.args = dict(node_words=t.node_words.ptr, tracks=t.tracks.ptr, track_stats=t.stats.ptr, buf_tab=t.buf_tab.ptr, nbufs=self.nbufs, rows_dev=t.rows.ptr,
                         node_stride=self.stride, max_rows=self.max_rows, feats_base=self.feats.ptr, buf_stride=self.buf_stride, found_base=self.found.ptr,
                         found_buf_stride=FOUND_STRIDE, rank_layouts=self.rank_layouts.ptr, layouts=self.layouts.ptr, min_length=min_length, max_length=max_length,
                         conflicts=conflicts, offsets=self.offsets.ptr, track_ids=self.track_ids.ptr, tracks_cap=self.tracks_cap, observations=self.obs.ptr,
                         obs_cap=self.obs_cap, stats=self.stats.ptr, scratch=self.scratch.ptr, scratch_u32=self.scratch_u32)

    def restated(self):
        records, words, _ = TC.expected(self.t.case)
        return NO.select(records, words, self.xy, *self.params)

    def expected(self):
        exp = self.host.copy()
        stats, offsets, ids, obs = self.restated()
        assert len(ids) <= self.tracks_cap and len(obs) <= self.obs_cap
        self.put(exp, self.offsets, 0, offsets)
        self.put(exp, self.track_ids, 0, ids)
        self.put(exp, self.obs, 0, obs)
        self.put(exp, self.stats, 0, np.array([stats[k] for k in NO.STATS], u32))
        return exp

    def outputs(self, raw):
        """the bytes of the four output blocks"""
        return [self.view(raw, b).copy() for b in (self.offsets, self.track_ids, self.obs, self.stats)]
