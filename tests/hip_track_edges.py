"""Direct access to the edge store launchers of include/vksift_hip.h for tests (plain module, no fixtures): vksift_hip_append_track_edges with
vksift_hip_track_edges_scratch_u32, and vksift_hip_build_tracks_from_edges.

  * bind(): the ctypes argtypes of the three entries (and those of tests/hip_tracks.py)
  * Store turns a store case — calls: a list of cases of tests/track_cases.py, one per append, plus nb_buffers, max_edges and optionally build =
    dict(node_stride, max_rows) — into ONE byte tensor in the manner of tests/hip_tracks.py: per call the input blocks of a track build and a scratch of
    exactly the words the library asks for; once the store (edge records poisoned, two records of room behind max_edges; the four statistics words zero, two
    poisoned words behind them; the row table 0xFFFFFFFF) and, with `build`, the blocks of a build from the store's own words. append(L, k) / build(L) make
    the calls, expected() is tests/np_track_edges.py on what the contract says the launches read
  * BuildOnly is a build from edges that are written down directly: held records (those at and beyond min(count, max_edges) are decoys), the count word,
    the participating buffers with their row counts, further buffers the row table knows but the rank table does not
"""
import ctypes as C

import numpy as np

import hip_tracks as HT
import np_track_edges as NE
import track_cases as TC
from hip_records import HIP_ERROR_INVALID_VALUE  # noqa: F401  (re-exported for the tests)
from hip_two_view import TwoView

u32 = np.uint32
UNSET = NE.UNSET


def bind(L):
    HT.bind(L)
    vp, w, q, z = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    L.vksift_hip_append_track_edges.argtypes = [vp, q, vp, w, w, vp, q, vp, w, vp, w, w, vp, w, vp, w, vp, w, vp, w, vp, vp, z, vp]
    L.vksift_hip_append_track_edges.restype = C.c_int
    L.vksift_hip_build_tracks_from_edges.argtypes = [vp, vp, w, vp, w, vp, w, vp, w, w, vp, vp, q, vp, vp, z, vp]
    L.vksift_hip_build_tracks_from_edges.restype = C.c_int
    L.vksift_hip_track_edges_scratch_u32.argtypes = [w, w]
    L.vksift_hip_track_edges_scratch_u32.restype = z
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


def append_scratch_words(nslots, max_n):
    """what vksift_hip_track_edges_scratch_u32(nslots, max_n) asks for: a word per slot and block of 256 records"""
    return nslots * ((max_n + 255) // 256)


def call(L, entry, args, **changes):
    args = dict(args)
    for k, v in changes.items():
        if k.startswith("+"):
            args[k[1:]] += v
        else:
            assert k in args, k
            args[k] = v
    return getattr(L, "vksift_hip_" + entry)(*args.values(), None)


class EdgeLaunch(TwoView):
    def build_blocks(self, ids, stride, max_rows):
        """the output blocks of a build over the buffers `ids`, as tests/hip_tracks.py lays them out"""
        self.ids, self.nbufs, self.stride, self.max_rows = ids, len(ids), stride, max_rows
        self.node_words = self.poison("node words", 4 * self.nbufs * stride, slot_bytes=4 * stride, row_bytes=4)
        self.cap = self.nbufs * max_rows // 2
        self.tracks = self.poison("track records", 16 * (self.cap + 2), row_bytes=16)
        self.track_stats = self.poison("track statistics", 4 * 6, row_bytes=4)
        self.build_scratch = self.scratch_block(HT.scratch_words(self.nbufs, stride))
        self.build_scratch_u32 = self.scratch_u32
        self.behind = self.poison("behind the scratch", 64)

    def put_build(self, exp, result):
        rec, words, stats = result
        assert len(rec) <= self.cap
        self.put(exp, self.tracks, 0, rec)
        for r, b in enumerate(self.ids):
            self.put(exp, self.node_words, 4 * r * self.stride, words[b])
        self.put(exp, self.track_stats, 0, np.array([stats[k] for k in ("nb_tracks", "nb_conflicting", "nb_features", "nb_edges")], u32))

    def outputs(self, raw):
        """the bytes of the three output blocks of the build"""
        return [self.view(raw, b).copy() for b in (self.tracks, self.node_words, self.track_stats)]


class Store(EdgeLaunch):
    entry = "append_track_edges"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        self.nb_buffers, self.max_edges = case["nb_buffers"], case["max_edges"]
        self.table = self.block("row table", np.full(self.nb_buffers, UNSET, u32), row_bytes=4)
        self.edges = self.poison("edges", 16 * (self.max_edges + 2), row_bytes=16)
        self.stats = self.block("edge statistics", np.array(list(case.get("preset_stats", (0, 0, 0, 0))) + [0xA5A5A5A5] * 2, u32), row_bytes=4)
        per_call = []
        for k, c in enumerate(case["calls"]):
            pairs, ids = c["pairs"], [b for b, _ in c["bufs"]]
            assert ids == sorted(set(ids))
            rank = {b: r for r, b in enumerate(ids)}
            tag = f" (call {k})"
            rec_stride, mask_stride = 16 * (c["max_n"] + c["rec_extra"]), c["max_n"] + c["mask_extra"]
            held = [p["recs"][:c["max_n"] + c["rec_extra"]] for p in pairs]
            full = [np.concatenate([h, np.full((len(h), 2), 0xA5A5A5A5, u32)], axis=1) for h in held]
            records = self.slotted("records" + tag, rec_stride, full, row_bytes=16)
            n = self.strided_words("record counts" + tag, c["n_stride"], [[p["n_dev"]] for p in pairs], TC.JUNK_COUNTER)
            masks = valid = None
            if c["masked"]:
                masks = self.slotted("masks" + tag, mask_stride, [p["mask"][:mask_stride] for p in pairs], row_bytes=1)
                words = np.array([[p["valid"]] + [0 if p["valid"] else 1] * (c["valid_stride"] - 1) for p in pairs], u32)
                valid = self.block("valid words" + tag, words, slot_bytes=4 * c["valid_stride"], row_bytes=4)
            tab = self.strided_words("slot table" + tag, c["tab_stride"], [[rank[p["a"]], rank[p["b"]]] for p in pairs], 0)
            count_word = [4 * r + 1 for r in range(len(ids))]
            buf_tab = self.block("buffer table" + tag, np.array([[b, w] for b, w in zip(ids, count_word)], u32), row_bytes=8)
            rows = np.full(4 * len(ids) + 2, TC.JUNK_COUNTER, u32)
            rows[count_word] = [r for _, r in c["bufs"]]
            rows = self.block("row counters" + tag, rows, row_bytes=4)
            words = append_scratch_words(len(pairs), c["max_n"])
            scratch = self.poison("append scratch" + tag, 4 * max(words, 1), row_bytes=4)
            per_call.append(dict(c=c, records=records, rec_stride=rec_stride, n=n, masks=masks, mask_stride=mask_stride, valid=valid, tab=tab, ns=len(pairs),
                                 buf_tab=buf_tab, nbufs=len(ids), rows=rows, scratch=scratch, words=words))
        b = case.get("build")
        if b:
            ids = sorted({i for c in case["calls"] for i, _ in c["bufs"] if i < self.nb_buffers})
            rank_tab = np.full(self.nb_buffers, UNSET, u32)
            rank_tab[ids] = np.arange(len(ids))
            self.rank_tab = self.block("rank table", rank_tab, row_bytes=4)
            self.build_tab = self.block("buffer table (build)", np.array([[i, i] for i in ids], u32), row_bytes=8)
            self.build_blocks(ids, b["node_stride"], b["max_rows"])
        self.build()
        self.free = [(k["scratch"], 0, 4 * k["words"]) for k in per_call]
        self.append_args = [self.args_of_call(**k) for k in per_call]
        if b:
            self.free.append((self.build_scratch, 0, 4 * self.build_scratch_u32))
            self.build_args = dict(edges=self.edges.ptr, edge_count=self.stats.ptr, max_edges=self.max_edges, rank_tab=self.rank_tab.ptr, nb_buffers=self.nb_buffers,
                                   buf_tab=self.build_tab.ptr, nbufs=self.nbufs, rows_dev=self.table.ptr, node_stride=self.stride, max_rows=self.max_rows,
                                   node_words=self.node_words.ptr, tracks=self.tracks.ptr, tracks_cap=self.cap, stats=self.track_stats.ptr,
                                   scratch=self.build_scratch.ptr, scratch_u32=self.build_scratch_u32)

    def args_of_call(self, *, c, records, rec_stride, n, masks, mask_stride, valid, tab, ns, buf_tab, nbufs, rows, scratch, words):
        return dict(records=records.ptr, rec_slot_stride=rec_stride, n_dev=n.ptr, n_stride=c["n_stride"], max_n=c["max_n"], masks=masks.ptr if masks else None,
                    mask_slot_stride=mask_stride if masks else 0, valid=valid.ptr if valid else None, valid_stride=c["valid_stride"] if valid else 0, slot_tab=tab.ptr,
                    slot_tab_stride=c["tab_stride"], nslots=ns, buf_tab=buf_tab.ptr, nbufs=nbufs, rows_dev=rows.ptr, max_rows=c["max_rows"], row_table=self.table.ptr,
                    nb_buffers=self.nb_buffers, edges=self.edges.ptr, max_edges=self.max_edges, stats=self.stats.ptr, scratch=scratch.ptr, scratch_u32=words)

    def append(self, L, k, **changes):
        return call(L, "append_track_edges", self.append_args[k], **changes)

    def run_build(self, L, **changes):
        return call(L, "build_tracks_from_edges", self.build_args, **changes)

    def restated(self, calls=None):
        s = NE.begin(self.max_edges)
        for c in self.case["calls"][:calls]:
            _, pairs = TC.read_by_contract(c)
            NE.accumulate(s, dict(c["bufs"]), pairs, max_rows=c["max_rows"], nb_buffers=self.nb_buffers)
        return s

    def expected(self, calls=None, built=True):
        exp = self.host.copy()
        s = self.restated(calls)
        self.put(exp, self.edges, 0, NE.edge_records(s))
        self.put(exp, self.stats, 0, np.array([NE.stats(s)[k] for k in NE.STATS], u32))
        table = np.full(self.nb_buffers, UNSET, u32)
        for b, n in s["table"].items():
            table[b] = n
        self.put(exp, self.table, 0, table)
        if built and self.case.get("build"):
            self.put_build(exp, NE.build(s, self.max_rows))
        return exp


class BuildOnly(EdgeLaunch):
    entry = "build_tracks_from_edges"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c = case
        ids = [b for b, _ in c["bufs"]]
        assert ids == sorted(set(ids)) and all(b < c["nb_buffers"] for b in ids)
        held = np.asarray(c["edges"], u32).reshape(-1, 4)
        assert len(held) >= min(c["count"], c["max_edges"])
        self.edges = self.slotted("edges", 16 * max(len(held), c["max_edges"], 1), [held], row_bytes=16)
        self.count = self.block("edge count", np.array([c["count"]] + [TC.JUNK_COUNTER] * 3, u32), row_bytes=4)
        rank_tab, table = np.full(c["nb_buffers"], UNSET, u32), np.full(c["nb_buffers"], UNSET, u32)
        rank_tab[ids] = np.arange(len(ids))
        for b, n in list(c["bufs"]) + list(c.get("absent", [])):
            table[b] = n
        self.rank_tab = self.block("rank table", rank_tab, row_bytes=4)
        self.build_tab = self.block("buffer table", np.array([[i, i] for i in ids], u32), row_bytes=8)
        self.table = self.block("row table", table, row_bytes=4)
        self.build_blocks(ids, c["node_stride"], c["max_rows"])
        self.build()
        self.free = [(self.build_scratch, 0, 4 * self.build_scratch_u32)]
        self.args = dict(edges=self.edges.ptr, edge_count=self.count.ptr, max_edges=c["max_edges"], rank_tab=self.rank_tab.ptr, nb_buffers=c["nb_buffers"],
                         buf_tab=self.build_tab.ptr, nbufs=self.nbufs, rows_dev=self.table.ptr, node_stride=self.stride, max_rows=self.max_rows,
                         node_words=self.node_words.ptr, tracks=self.tracks.ptr, tracks_cap=self.cap, stats=self.track_stats.ptr, scratch=self.build_scratch.ptr,
                         scratch_u32=self.build_scratch_u32)

    def expected(self):
        c = self.case
        exp = self.host.copy()
        rows = {b: min(n, c["max_rows"]) for b, n in c["bufs"]}
        taken = np.asarray(c["edges"], np.int64).reshape(-1, 4)[:min(c["count"], c["max_edges"])]
        self.put_build(exp, NE.build_from_edges(rows, taken))
        return exp
