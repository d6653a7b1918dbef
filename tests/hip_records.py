"""Direct access to the record-moving launchers of include/vksift_hip.h for tests (plain module, no fixtures): vksift_hip_gather_descriptors,
_shifted_norms, _gather_sections, _pack_features, _filter_matches, _gather_correspondences and _gather_xy.

  * bind(): the ctypes argtypes of the seven entries
  * one class per launch (GatherDesc, Norms, Sections, Pack, Filter, Corr, XY) that turns a case of tests/record_cases.py into ONE byte tensor
    (a hip_planes.Arena; device "cpu" lays out the same bytes without a GPU): every input and output block between guard zones of its own,
    outputs and every byte of slack — the gaps between buffers, the cache entries of buffers the launch does not name, the rows at and beyond
    the written count, the stride padding — poisoned with 0xA5. Counters that must not be read hold a recognisable non-zero value; the two
    records behind a reverse 2-NN table are decoys that only the j < nb guard keeps out (record_cases.filter_slot)
  * launch(L, **changes): the call itself, arguments by name; "+name" adds bytes to a pointer or a stride (the refusal cases)
  * expected(): the whole arena as the contract of the header says it must look after the launch, from tests/np_records.py
  * check(): byte comparison of the whole arena that names the first differing block, slot and row
"""
import ctypes as C

import numpy as np

import hip_planes as HP
import np_records as NR
import record_cases as RC
from hip_features import GUARD, POISON_BYTE, POISON_WORD, Block
from test_section_walk import TABLES, _table, stored_rows

HIP_ERROR_INVALID_VALUE = 1
REC = NR.REC
u32 = np.uint32


def bind(L):
    vp, hp, w, q, f = C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.c_float
    sigs = {
        "vksift_hip_gather_descriptors": [vp, w, vp, vp],
        "vksift_hip_shifted_norms": [vp, w, vp, vp],
        "vksift_hip_gather_sections": [vp, q, hp, w, w, hp, hp, hp, vp, w, w, w, vp, q, vp, q, vp, w, vp],
        "vksift_hip_pack_features": [vp, q, hp, hp, w, w, hp, hp, vp, w, vp, w, vp, vp],
        "vksift_hip_filter_matches": [vp, q, vp, q, vp, w, f, w, vp, q, vp, vp],
        "vksift_hip_gather_correspondences": [vp, q, vp, w, vp, vp, vp, q, vp, w, w, vp, q, vp],
        "vksift_hip_gather_xy": [vp, q, vp, w, vp, vp, w, w, vp, q, vp],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


def host_words(values, room=0):
    """a host array of uint32 the launcher reads (at least `room` entries)"""
    values = [int(v) for v in values]
    return (C.c_uint32 * max(len(values), room, 1))(*values)


class Launch:
    """blocks are declared with block(), build() lays them out; subclasses fill self.args (name -> value, in call order)"""
    entry = None

    def __init__(self, case, device="cuda"):
        self.case, self.arena, self.blocks, self.args = case, HP.Arena(device), [], {}
        self.what = f"{self.entry} [{case['name']}]"

    def block(self, name, payload, *, slot_bytes=None, row_bytes=None, base_off=0):
        """slot_bytes / row_bytes: how check() names a byte of the block; base_off: bytes the block's start lies beyond a 256-byte boundary"""
        blk = Block(name, payload)
        blk.slot_bytes, blk.row_bytes, blk.base_off = slot_bytes, row_bytes, base_off
        self.blocks.append(blk)
        return blk

    def poison(self, name, nbytes, **kw):
        return self.block(name, np.full(nbytes, POISON_BYTE, np.uint8), **kw)

    def build(self):
        for blk in self.blocks:
            body = np.full(len(blk.payload) + 2 * GUARD, POISON_BYTE, np.uint8)
            body[GUARD:GUARD + len(blk.payload)] = blk.payload
            blk.ref = self.arena.plane(blk.name, len(body), 1, kind="u8", data=body.reshape(1, 1, -1), offset=blk.base_off)
        self.arena.build()
        self.host = self.arena.host

    def launch(self, L, **changes):
        args = dict(self.args)
        for k, v in changes.items():
            if k.startswith("+"):
                args[k[1:]] += v
            else:
                args[k] = v
        assert list(args) == list(self.args)
        return getattr(L, "vksift_hip_" + self.entry)(*args.values(), None)

    def view(self, raw, blk, dtype=np.uint8):
        return raw[blk.off:blk.off + len(blk.payload)].view(dtype)

    def read(self):
        return self.arena.read()

    def where(self, byte):
        for blk in self.blocks:
            lo = blk.ref.byte_off
            if lo <= byte < lo + len(blk.payload) + 2 * GUARD:
                o = byte - blk.off
                if o < 0 or o >= len(blk.payload):
                    return f"guard zone of {blk.name!r} ({o} bytes from its start)"
                text = f"{blk.name!r} byte {o}"
                if blk.slot_bytes:
                    text += f": slot / buffer {o // blk.slot_bytes}"
                    o %= blk.slot_bytes
                if blk.row_bytes:
                    text += f", row {o // blk.row_bytes} byte {o % blk.row_bytes}"
                return text
        return self.arena.where(byte)

    def check(self, after, exp=None):
        exp = self.expected() if exp is None else exp
        bad = np.flatnonzero(after != exp)
        if len(bad):
            b = int(bad[0])
            raise AssertionError(f"{self.what}: {len(bad)} bytes differ from the contract, first at arena byte {b}: {self.where(b)}: "
                                 f"expected 0x{int(exp[b]):02x}, got 0x{int(after[b]):02x}")

    def check_untouched(self, after, why):
        self.check(after, self.host)


# ---------------------------------------------------------------------------------------------------------------------- gather_descriptors
class GatherDesc(Launch):
    entry = "gather_descriptors"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        n = case["n"]
        self.recs = RC.buffer_bytes(1, n + 2, 70 + n)[0]
        self.feats = self.block("records", self.recs, row_bytes=REC, base_off=case["base_off"])
        self.desc = self.poison("dense rows", (n + 2) * 128, row_bytes=128)
        self.build()
        self.args = dict(feats=self.feats.ptr, n=n, desc=self.desc.ptr)

    def expected(self):
        exp = self.host.copy()
        n = self.case["n"]
        self.view(exp, self.desc)[:n * 128] = NR.gather_descriptors(self.recs, n).reshape(-1)
        return exp


# ---------------------------------------------------------------------------------------------------------------------- shifted_norms
class Norms(Launch):
    entry = "shifted_norms"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        n = case["n"]
        self.rows = RC.norm_rows(n + 2, case["shift"])
        self.desc = self.block("dense rows", self.rows, row_bytes=128)
        self.norms = self.poison("norms", (n + 2) * 4, row_bytes=4)
        self.build()
        self.args = dict(desc=self.desc.ptr, n=n, norms=self.norms.ptr)

    def expected(self):
        exp = self.host.copy()
        n = self.case["n"]
        self.view(exp, self.norms, u32)[:n] = NR.shifted_norms(self.rows[:n])
        return exp


# ---------------------------------------------------------------------------------------------------------------------- sectioned buffers
def feature_block(launch, bufs, gap_words=3):
    """bufs: (nbuf, extent, 164) record bytes. The SIFT buffers buf_stride = extent * 164 + 4 * gap_words bytes apart, the gaps poisoned
    -> (block, bufs, buf_stride)"""
    nbuf, extent = bufs.shape[:2]
    stride = extent * REC + 4 * gap_words
    flat = np.full(nbuf * stride, POISON_BYTE, np.uint8)
    for b in range(nbuf):
        flat[b * stride:b * stride + extent * REC] = bufs[b].reshape(-1)
    return launch.block("SIFT buffers", flat, slot_bytes=stride, row_bytes=REC), bufs, stride


def counter_block(launch, counts, fbs):
    """the raw counters of every buffer, found_buf_stride words apart; the words behind a buffer's own counters hold JUNK_COUNTER"""
    words = np.full(len(counts) * fbs, RC.JUNK_COUNTER, u32)
    for b, c in enumerate(counts):
        words[b * fbs:b * fbs + len(c)] = c
    return launch.block("section counters", words, slot_bytes=4 * fbs, row_bytes=4)


GATHER_SLOTS = 512


def sectioned_case(name, table, *, nbuf=1, buf_ids=None, counts=None, fixed=False, cache=False, pad=2, fbs=16, seed=1, desc_extra=0, norm_extra=0, n_stride=1,
                   **own):
    """The fields the cases of hip_strongest and hip_rootsift share. table: a name of test_section_walk.TABLES or (nsec, off, cap, found). counts:
    raw counters per buffer (default: the table's own for every buffer). own: the fields of one entry's cases."""
    table = TABLES[table] if isinstance(table, str) else table
    nsec, off, cap, found = table
    counts = [list(c) for c in counts] if counts is not None else [list(found[:nsec])] * nbuf
    assert len(counts) == nbuf and (fbs >= nsec or fixed)
    buf_ids = list(buf_ids if buf_ids is not None else range(nbuf))
    assert len(set(buf_ids)) == len(buf_ids)
    totals = [len(stored_rows(nsec, off, cap, c)) for c in counts]
    return dict(name=name, table=table, nbuf=nbuf, buf_ids=buf_ids, counts=counts, totals=totals, fixed=fixed, cache=cache, pad=pad, fbs=fbs, seed=seed,
                desc_extra=desc_extra, norm_extra=norm_extra, n_stride=n_stride, **own)


def one(total, cap=None):
    return _table(1, [cap if cap is not None else total + 3], [total])


def case_named(cases, name):
    (c,) = [c for c in cases if c["name"] == name]
    return c


class Sectioned(Launch):
    """What the launches over sectioned buffers share (gather_sections, keep_strongest, root_descriptors): the SIFT buffers and their counters,
    the matcher-cache blocks where the case has them, and the argument names. A subclass declares its blocks in arena order — sift_blocks(), any
    of its own, cache_blocks() — and ends with finish(its own arguments), which builds the arena."""

    def sift_blocks(self, bufs):
        c = self.case
        self.nsec, self.off, self.cap, _ = c["table"]
        self.totals = c["totals"] if "totals" in c else RC.sec_totals(c)
        self.named = [self.totals[b] for b in c["buf_ids"]]
        self.feats, self.bufs, self.buf_stride = feature_block(self, bufs)
        self.found = None if c["fixed"] else counter_block(self, c["counts"], c["fbs"])

    def cache_blocks(self, rows, present=True):
        """entries of `rows` rows and two more, plus the slack the case asks for"""
        c = self.case
        self.rows_cap = rows + 2
        self.desc_stride = self.rows_cap * 128 + 16 * c["desc_extra"]
        self.norm_stride = self.rows_cap + c["norm_extra"]
        self.desc = self.norms = self.n = None
        if present:
            self.desc = self.poison("cache rows", c["nbuf"] * self.desc_stride, slot_bytes=self.desc_stride, row_bytes=128)
            self.norms = self.poison("cache norms", c["nbuf"] * self.norm_stride * 4, slot_bytes=self.norm_stride * 4, row_bytes=4)
            self.n = self.poison("cache n", c["nbuf"] * c["n_stride"] * 4, slot_bytes=c["n_stride"] * 4)

    def max_rows(self):
        return max(self.named) if self.case["max_rows"] == "exact" else self.case["max_rows"]

    def finish(self, **own):
        """own: the entry's arguments between found_buf_stride and pad_rows_to (a block stands for its address, None for NULL)"""
        c = self.case
        self.build()
        ptr = lambda blk: blk.ptr if isinstance(blk, Block) else blk
        self.args = dict(feats_base=self.feats.ptr, buf_stride=self.buf_stride, buf_ids=host_words(c["buf_ids"], GATHER_SLOTS + 8), nslots=len(c["buf_ids"]),
                         nsec=self.nsec, sec_off=host_words(self.off, 20), sec_cap=host_words(self.cap, 20),
                         fixed_counts=host_words(c["table"][3], 20) if c["fixed"] else None, found_base=ptr(self.found),
                         found_buf_stride=0 if c["fixed"] else c["fbs"], **{k: ptr(v) for k, v in own.items()}, pad_rows_to=c["pad"], desc=ptr(self.desc),
                         desc_stride=self.desc_stride, norms=ptr(self.norms), norm_stride=self.norm_stride, n_out=ptr(self.n), n_stride=c["n_stride"])

    def expect_entry(self, exp, b, records, counts):
        """the cache entry of buffer b in `exp` as the gather pass writes it for `records` with raw counters `counts`; returns its row count"""
        rows, norms, total = NR.gather_sections(records, self.nsec, self.off, self.cap, counts, self.case["pad"])
        self.view(exp, self.desc)[b * self.desc_stride:][:rows.size] = rows.reshape(-1)
        self.view(exp, self.norms, u32)[b * self.norm_stride:][:len(norms)] = norms
        self.view(exp, self.n, u32)[b * self.case["n_stride"]] = total
        return total


class Sections(Sectioned):
    entry = "gather_sections"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        nsec, off, cap, _ = case["table"]
        self.sift_blocks(RC.buffer_bytes(case["nbuf"], RC.extent_of(off, cap, nsec), case["seed"]))
        self.cache_blocks(max(max(self.named), case["pad"]))
        self.finish(max_rows=self.max_rows())

    def expected(self):
        exp = self.host.copy()
        for b in set(self.case["buf_ids"]):   # the entry of BUFFER b, whichever slot names it
            self.expect_entry(exp, b, self.bufs[b], self.case["counts"][b])
        return exp


class Pack(Launch):
    entry = "pack_features"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c = case
        self.nsec, self.off, self.cap, _ = c["table"]
        self.totals = RC.sec_totals(c)
        self.feats, self.bufs, self.buf_stride = feature_block(self, RC.buffer_bytes(c["nbuf"], RC.extent_of(self.off, self.cap, self.nsec), c["seed"]))
        self.found = counter_block(self, c["counts"], c["fbs"])
        self.out = self.poison("packed records", c["out_records"] * REC, row_bytes=REC)
        self.post = self.poison("found_post", c["nbuf"] * c["fbs"] * 4, slot_bytes=4 * c["fbs"], row_bytes=4) if c["post"] else None
        self.build()
        named = [self.totals[b] for b in c["buf_ids"]]
        max_rows = max(named) if c["max_rows"] == "exact" else c["max_rows"]
        self.args = dict(feats_base=self.feats.ptr, buf_stride=self.buf_stride, buf_ids=host_words(c["buf_ids"], 72), out_rows=host_words(c["out_rows"], 72),
                         nslots=len(c["buf_ids"]), nsec=self.nsec, sec_off=host_words(self.off, 20), sec_cap=host_words(self.cap, 20),
                         found_base=self.found.ptr, found_buf_stride=c["fbs"], out=self.out.ptr, max_rows=max_rows,
                         found_post=self.post.ptr if c["post"] else None)

    def expected(self):
        c = self.case
        exp = self.host.copy()
        for b, row0 in zip(c["buf_ids"], c["out_rows"]):
            recs = NR.pack_features(self.bufs[b], self.nsec, self.off, self.cap, c["counts"][b])
            self.view(exp, self.out)[row0 * REC:][:recs.size] = recs.reshape(-1)
            if c["post"]:   # all found_buf_stride words of the buffer's counters, the words behind its sections included
                self.view(exp, self.post, u32)[b * c["fbs"]:(b + 1) * c["fbs"]] = self.view(self.host, self.found, u32)[b * c["fbs"]:(b + 1) * c["fbs"]]
        return exp


# ---------------------------------------------------------------------------------------------------------------------- filter_matches
class Filter(Launch):
    entry = "filter_matches"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c, slots = case, case["slots"]
        ns = len(slots)
        self.has_rev = slots[0]["rev"] is not None
        assert all((s["rev"] is not None) == self.has_rev for s in slots)
        self.fwd_stride = (max(s["na"] for s in slots) + c["fwd_extra"]) * 20 + 4
        fwd = np.full(ns * self.fwd_stride, POISON_BYTE, np.uint8)
        for k, s in enumerate(slots):
            fwd[k * self.fwd_stride:][:s["fwd"].size * 4] = s["fwd"].view(np.uint8).reshape(-1)
        self.fwd = self.block("forward records", fwd, slot_bytes=self.fwd_stride, row_bytes=20)
        self.rev = None
        self.rev_stride = 0
        if self.has_rev:
            self.rev_stride = (max(len(s["rev"]) for s in slots) + c["fwd_extra"]) * 20 + 8
            rev = np.full(ns * self.rev_stride, POISON_BYTE, np.uint8)
            for k, s in enumerate(slots):
                rev[k * self.rev_stride:][:s["rev"].size * 4] = s["rev"].view(np.uint8).reshape(-1)
            self.rev = self.block("reverse records", rev, slot_bytes=self.rev_stride, row_bytes=20)
        n = np.full(ns * c["n_stride"], POISON_WORD, u32)
        for k, s in enumerate(slots):
            n[k * c["n_stride"]:k * c["n_stride"] + 2] = [s["na"], s["nb"]]
        self.n_fwd = self.block("row counts", n, slot_bytes=4 * c["n_stride"], row_bytes=4)
        # the caller guarantees 16 * N_A bytes per slot (every record may survive); slack behind them on request
        self.out_stride = 16 * max(max(s["na"] for s in slots), 1) + 4 * c["out_extra"]
        self.out = self.poison("filtered records", ns * self.out_stride, slot_bytes=self.out_stride, row_bytes=16)
        self.out_n = self.poison("filtered counts", (ns + 2) * 4, row_bytes=4)
        self.build()
        self.args = dict(fwd=self.fwd.ptr, fwd_slot_stride=self.fwd_stride, rev=self.rev.ptr if self.has_rev else None, rev_slot_stride=self.rev_stride,
                         n_fwd=self.n_fwd.ptr, n_stride=c["n_stride"], ratio=c["ratio"], nslots=ns, out=self.out.ptr, out_slot_stride=self.out_stride,
                         out_n=self.out_n.ptr)

    def kept(self):
        return [NR.filter_matches(s["fwd"], s["rev"], s["nb"], self.case["ratio"]) for s in self.case["slots"]]

    def expected(self):
        exp = self.host.copy()
        for k, recs in enumerate(self.kept()):
            self.view(exp, self.out)[k * self.out_stride:][:recs.size * 4] = recs.view(np.uint8).reshape(-1)
            self.view(exp, self.out_n, u32)[k] = len(recs)
        return exp


# ---------------------------------------------------------------------------------------------------------------------- pair tables
class PairTable(Launch):
    """what vksift_hip_gather_correspondences and vksift_hip_gather_xy share: the buffers, their counters, the layouts and the slot table"""

    def world_blocks(self):
        w = self.case["world"]
        self.feats, self.bufs, self.buf_stride = feature_block(self, RC.buffer_bytes(w["nbuf"], w["extent"], w["seed"]))
        self.found = self.block("section counters", RC.world_found_words(w), slot_bytes=4 * w["fbs"], row_bytes=4)
        self.layouts = self.block("layouts", RC.world_layout_words(w), slot_bytes=4 * NR.LAYOUT_WORDS, row_bytes=4)
        tab = np.array([list(s["buf"]) + list(s["word"]) for s in self.case["slots"]], u32)
        self.slot_tab = self.block("slot table", tab, slot_bytes=16, row_bytes=4)

    def side(self, s, t):
        """(buffer bytes, stored rows) of side t of slot s"""
        return self.bufs[s["buf"][t]], RC.side_rows(self.case["world"], s["buf"][t], s["word"][t])


class Corr(PairTable):
    entry = "gather_correspondences"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c, slots = case, case["slots"]
        self.world_blocks()
        self.f_stride = (c["max_n"] + 3) * 16 + 4
        filt = np.full(len(slots) * self.f_stride, POISON_BYTE, np.uint8)
        for k, s in enumerate(slots):
            filt[k * self.f_stride:][:s["filtered"].size * 4] = s["filtered"].view(np.uint8).reshape(-1)
        self.filtered = self.block("filtered records", filt, slot_bytes=self.f_stride, row_bytes=16)
        self.filtered_n = self.block("filtered counts", np.array([s["filtered_n"] for s in slots], u32), row_bytes=4)
        self.c_stride = 16 * (c["max_n"] + 1 + c["extra"])
        self.corr = self.poison("correspondences", len(slots) * self.c_stride, slot_bytes=self.c_stride, row_bytes=16)
        self.build()
        w = c["world"]
        self.args = dict(feats_base=self.feats.ptr, buf_stride=self.buf_stride, found_base=self.found.ptr, found_buf_stride=w["fbs"], slot_tab=self.slot_tab.ptr,
                         layouts=self.layouts.ptr, filtered=self.filtered.ptr, filtered_slot_stride=self.f_stride, filtered_n=self.filtered_n.ptr,
                         max_n=c["max_n"], nslots=len(slots), corr=self.corr.ptr, corr_slot_stride=self.c_stride)

    def rows(self):
        out = []
        for s in self.case["slots"]:
            (ba, ra), (bb, rb) = self.side(s, 0), self.side(s, 1)
            out.append(NR.gather_correspondences(ba, ra, bb, rb, s["filtered"], min(s["filtered_n"], self.case["max_n"])))
        return out

    def expected(self):
        exp = self.host.copy()
        for k, r in enumerate(self.rows()):
            self.view(exp, self.corr)[k * self.c_stride:][:r.size * 4] = r.view(np.uint8).reshape(-1)
        return exp


class XY(PairTable):
    entry = "gather_xy"

    def __init__(self, case, device="cuda"):
        super().__init__(case, device)
        c, slots = case, case["slots"]
        self.world_blocks()
        self.side_stride = c["max_n"] + c["extra"]
        self.xy = self.poison("coordinates", 2 * len(slots) * self.side_stride * 8, slot_bytes=self.side_stride * 8, row_bytes=8)
        self.build()
        w = c["world"]
        self.args = dict(feats_base=self.feats.ptr, buf_stride=self.buf_stride, found_base=self.found.ptr, found_buf_stride=w["fbs"], slot_tab=self.slot_tab.ptr,
                         layouts=self.layouts.ptr, max_n=c["max_n"], nslots=len(slots), xy=self.xy.ptr, xy_side_stride=self.side_stride)

    def expected(self):
        exp = self.host.copy()
        for k, s in enumerate(self.case["slots"]):
            for t in (0, 1):
                r = NR.gather_xy(*self.side(s, t), self.case["max_n"])
                self.view(exp, self.xy)[(2 * k + t) * self.side_stride * 8:][:r.size * 4] = r.view(np.uint8).reshape(-1)
        return exp


LAUNCHES = {"gather_descriptors": GatherDesc, "shifted_norms": Norms, "gather_sections": Sections, "pack_features": Pack, "filter_matches": Filter,
            "gather_correspondences": Corr, "gather_xy": XY}
