"""Direct access to the matcher launchers of include/vksift_hip.h for tests (plain module, no fixtures): vksift_hip_match_2nn_prenormed,
vksift_hip_match_2nn_desc and vksift_hip_match_2nn_async.

  * bind(): the ctypes argtypes of the three entries (and of vksift_hip_match_scratch_u32, vksift_hip_tune)
  * one class per entry (Prenormed, Desc, Async) that turns a case of tests/match_cases.py into ONE byte tensor (the arena of
    tests/hip_records.py; device "cpu" lays out the same bytes without a GPU): every input, output and scratch block between guard zones
    of its own; records, count words and every byte of slack poisoned with 0xA5, scratch filled with 0xA5 or with zeros (FILLS: each
    shows what the other hides, see MatchLaunch). The scratch of the pointer entries is EXACTLY the documented minimum. The rows of a
    cache entry at and beyond its count are decoys that would win if a kernel read them (match_cases.world); the stride paddings of the
    cache, of the records and of the count words are poison, those of the row flags hold the scratch fill
  * launch(L, **changes): the call itself, arguments by name; "+name" adds to an argument (the refusal cases)
  * expected(): the whole arena as the contract of the header says it must look after the launch, from tests/np_match.py: the N_A records
    of every slot and its two count words, nothing else
  * check(): byte comparison of the whole arena that names the first differing block, slot and row. Scratch — the pointer entries'
    scratch, `redo`, `partial_scratch` — is unspecified inside its documented extent and compared from that extent outward only
  * main(): the cases of one switch group (match_cases.GROUPS) in THIS process — the VKSIFT_MATCH_* switches are read once per process, so
    tests/test_gpu_match_launchers.py starts one child per switch; exits non-zero naming the first differing block
"""
import ctypes as C
import sys

import numpy as np

import hip_records as HR
import match_cases as MC
import np_match as NM
from hip_features import POISON_BYTE, POISON_WORD

HIP_ERROR_INVALID_VALUE = 1
TUNE_SCAN_FORM = 4
CHUNKS = 32
FILLS = (POISON_BYTE, 0)   # what scratch holds before a launch (MatchLaunch)
u32 = np.uint32


def bind(L):
    vp, w, q, z = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    hp = C.POINTER(C.c_uint32)
    sigs = {
        "vksift_hip_match_2nn_prenormed": [vp, vp, w, w, vp, vp, w, vp, z, vp, vp],
        "vksift_hip_match_2nn_desc": [vp, w, w, vp, w, vp, z, vp, vp],
        "vksift_hip_match_2nn_async": [vp, vp, vp, hp, hp, w, w, w, vp, vp, vp, w, q, q, q, q, w, vp, vp],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L.vksift_hip_match_scratch_u32.argtypes = [w, w]
    L.vksift_hip_match_scratch_u32.restype = z
    L.vksift_hip_tune.argtypes = [C.c_int, C.c_int]
    L.vksift_hip_tune.restype = C.c_int
    L.vksift_hip_tune_get.argtypes = [C.c_int]
    L.vksift_hip_tune_get.restype = C.c_int
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


class MatchLaunch(HR.Launch):
    """adds the scratch blocks: free(blk, nbytes, first) leaves nbytes of a block from byte `first` on unspecified. Scratch needs no
    initialisation, so what it holds before the launch is the test's to choose, and both choices see something the other does not: 0xA5 in
    every byte (fill = POISON_BYTE) shows a kernel that counts on zeroed scratch; zeros (fill = 0) show a kernel that leaves a slot or a row
    out — over poisoned row flags the replay kernel would recompute every row the others skipped, and the records would be right all the same"""

    def __init__(self, case, device="cuda", fill=POISON_BYTE):
        super().__init__(case, device)
        self.free_runs, self.fill = [], fill
        self.what += f" (scratch filled with 0x{fill:02x})"

    def scratch_bytes(self, name, nbytes, **kw):
        return self.block(name, np.full(nbytes, self.fill, np.uint8), **kw)

    def free(self, blk, nbytes, first=0):
        assert first + nbytes <= len(blk.payload)
        self.free_runs.append((blk, first, nbytes))

    def check(self, after, exp=None):
        exp = self.expected() if exp is None else exp
        after = after.copy()
        for blk, first, nbytes in self.free_runs:
            after[blk.off + first:blk.off + first + nbytes] = exp[blk.off + first:blk.off + first + nbytes]
        super().check(after, exp)

    def check_untouched(self, after, why):
        """not a byte changed, scratch included"""
        HR.Launch.check(self, after, self.host)

    def written(self):
        """[(block, first byte, bytes)]: what the contract says the launch writes"""
        raise NotImplementedError


# ---------------------------------------------------------------------------------------------------------------------- single pair by pointer
class Pointer(MatchLaunch):
    def pair_blocks(self, joined):
        c = self.case
        self.a, self.b = MC.pair(c)
        na, nb = c["na"], c["nb"]
        if joined:
            self.desc_a = self.block("rows of A, rows of B behind them", np.concatenate([self.a, self.b]), row_bytes=128)
            self.ptr_b = lambda: self.desc_a.ptr + na * 128
        else:
            self.desc_a = self.block("rows of A", self.a, row_bytes=128)
            self.desc_b = self.block("rows of B", self.b, row_bytes=128)
            self.ptr_b = lambda: self.desc_b.ptr
        self.matches = self.poison("records", (na + 2) * 20, row_bytes=20)

    def scratch_block(self, words):
        self.scratch = self.scratch_bytes("scratch", 4 * words, row_bytes=4)
        self.free(self.scratch, 4 * words)

    def written(self):
        return [(self.matches, 0, self.case["na"] * 20)]

    def expected(self):
        exp = self.host.copy()
        self.view(exp, self.matches)[:self.case["na"] * 20] = MC.pair_records(self.case).view(np.uint8).reshape(-1)
        return exp


class Prenormed(Pointer):
    entry = "match_2nn_prenormed"

    def __init__(self, case, device="cuda", fill=POISON_BYTE, scratch_words=None):
        super().__init__(case, device, fill)
        c = case
        self.pair_blocks(joined=False)
        self.norm_a = self.block("norms of A", NM.shifted_norms(self.a), row_bytes=4)
        self.norm_b = self.block("norms of B", NM.shifted_norms(self.b), row_bytes=4)
        words = MC.prenormed_min_words(c["na"]) if scratch_words is None else scratch_words
        self.scratch_block(words)
        self.build()
        self.args = dict(desc_a=self.desc_a.ptr, norm_a=self.norm_a.ptr, na=c["na"], a_index_base=c["base"], desc_b=self.ptr_b(), norm_b=self.norm_b.ptr, nb=c["nb"],
                         scratch=self.scratch.ptr, scratch_u32=words, matches=self.matches.ptr)


class Desc(Pointer):
    entry = "match_2nn_desc"

    def __init__(self, case, device="cuda", fill=POISON_BYTE):
        super().__init__(case, device, fill)
        c = case
        self.pair_blocks(joined=c["joined"])
        words = MC.desc_min_words(c["na"], c["nb"])
        self.scratch_block(words)
        self.build()
        self.args = dict(desc_a=self.desc_a.ptr, na=c["na"], a_index_base=c["base"], desc_b=self.ptr_b(), nb=c["nb"], scratch=self.scratch.ptr, scratch_u32=words,
                         matches=self.matches.ptr)


# ---------------------------------------------------------------------------------------------------------------------- async
class Async(MatchLaunch):
    entry = "match_2nn_async"

    def __init__(self, case, device="cuda", fill=POISON_BYTE):
        super().__init__(case, device, fill)
        c = self.world = MC.world(case)
        counts, cap, x = c["counts"], c["cap"], c["extra"]
        ne, ns = len(counts), len(c["ids_a"])
        self.desc_stride, self.norm_stride = cap * 128 + 16 * x, cap + x
        desc = np.full(ne * self.desc_stride, POISON_BYTE, np.uint8)
        norm = np.full(ne * self.norm_stride, POISON_WORD, u32)
        for e, n in enumerate(counts):
            rows = np.concatenate([c["rows"][e], np.zeros((max(2 - n, 0), 128), np.uint8), c["decoys"][e]])
            assert len(rows) == cap
            desc[e * self.desc_stride:][:cap * 128] = rows.reshape(-1)
            norm[e * self.norm_stride:][:cap] = NM.shifted_norms(rows)
        self.cache_desc = self.block("cache rows", desc, slot_bytes=self.desc_stride, row_bytes=128)
        self.cache_norm = self.block("cache norms", norm, slot_bytes=4 * self.norm_stride, row_bytes=4)
        self.cache_n = self.block("cache n", np.array(counts, u32), row_bytes=4)
        self.max_na, self.ns = c["max_na"], ns
        self.rec_rows = max(max([counts[e] for e in c["ids_a"]]), 1)
        self.match_stride = self.rec_rows * 20 + 4 * x
        self.redo_stride = max(self.max_na, 1) + x
        self.matches = self.poison("records", ns * self.match_stride, slot_bytes=self.match_stride, row_bytes=20)
        self.n_dev = self.poison("count words", ns * c["n_stride"] * 4, slot_bytes=4 * c["n_stride"], row_bytes=4)
        self.redo = self.scratch_bytes("row flags", ns * self.redo_stride * 4, slot_bytes=4 * self.redo_stride, row_bytes=4)
        for k in range(ns):   # max_na words per slot; the padding behind them, up to the next slot's flags, must come back untouched
            self.free(self.redo, 4 * self.max_na, first=4 * k * self.redo_stride)
        self.partial = None
        if c["partial"]:
            self.partial = self.scratch_bytes("partial lists", 5 * self.max_na * CHUNKS * 4, row_bytes=4)
            self.free(self.partial, 5 * self.max_na * CHUNKS * 4)
        self.build()
        self.args = dict(cache_desc=self.cache_desc.ptr, cache_norm=self.cache_norm.ptr, cache_n=self.cache_n.ptr, ids_a=HR.host_words(c["ids_a"], 260),
                         ids_b=HR.host_words(c["ids_b"], 260), max_na=self.max_na, max_nb=c["max_nb"], nb_exact=c["nb_exact"], redo=self.redo.ptr, n_dev=self.n_dev.ptr,
                         matches=self.matches.ptr, nslots=ns, cache_desc_stride=self.desc_stride, cache_norm_stride=self.norm_stride, redo_slot_stride=self.redo_stride,
                         match_slot_stride=self.match_stride, n_slot_stride=c["n_stride"], partial_scratch=self.partial.ptr if self.partial else None)

    def written(self):
        out = []
        for k, (na, _, rec) in enumerate(MC.world_records(self.case)):
            out.append((self.n_dev, k * self.case["n_stride"] * 4, 8))
            if len(rec):
                out.append((self.matches, k * self.match_stride, na * 20))
        return out

    def expected(self):
        exp = self.host.copy()
        for k, (na, nb, rec) in enumerate(MC.world_records(self.case)):
            self.view(exp, self.n_dev, u32)[k * self.case["n_stride"]:][:2] = [na, nb]
            self.view(exp, self.matches)[k * self.match_stride:][:rec.size * 4] = rec.view(np.uint8).reshape(-1)
        return exp


LAUNCHES = {"match_2nn_prenormed": Prenormed, "match_2nn_desc": Desc, "match_2nn_async": Async}


def case_named(entry, name):
    return MC.async_named(name) if entry == "match_2nn_async" else MC.pointer_named(name)


def run(L, entry, case, **kw):
    """one launch, one synchronisation, one comparison of the whole arena"""
    h = LAUNCHES[entry](case, **kw)
    rc = h.launch(L)
    assert rc == 0, f"{h.what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"
    h.check(h.read())
    return h


def main(argv):
    """python tests/hip_match.py SWITCH: the cases of match_cases.GROUPS[SWITCH]; the caller has set the switch in the environment"""
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    switch = argv[1]
    assert os.environ.get(switch) == "0", f"{switch}=0 must be set in the environment of this process"
    from vulkansift_amd import api

    L = bind(api.lib())
    for case in MC.GROUPS[switch]:
        entries = ("match_2nn_async",) if "ids_a" in case else ("match_2nn_prenormed", "match_2nn_desc")
        for entry, fill in [(e, f) for e in entries for f in FILLS]:
            try:
                run(L, entry, case, fill=fill)
            except AssertionError as e:
                print(f"FAILED under {switch}=0: {e}", file=sys.stderr)
                return 1
            print(f"ok under {switch}=0: {entry} [{case['name']}] scratch 0x{fill:02x}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
