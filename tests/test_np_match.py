"""CPU side of tests/test_gpu_match_launchers.py: pins the numpy reference of the matcher (tests/np_match.py) against the loop of
np_restatement.match_2nn, the C oracle and the committed golden records; asserts that the case table (tests/match_cases.py) reaches the
edges it names — rows that need the float replay, quirk Q7 rows, ties across super-chunks, decoys that would win, the regime of every
shape —; models the scratch use of the cell scan from match_stream.h compiled on the host; and lays every arena out on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import hip_match as HM
import match_cases as MC
import np_match as NM
import np_restatement as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
u32 = np.uint32
ids = lambda c: c["name"]


def as_words(struct_records):
    return np.ascontiguousarray(struct_records).view(u32).reshape(-1, 5)


# ---------------------------------------------------------------------------------------------------------------------- the reference
def test_reference_equals_the_loop_restatement():
    """30 tie-heavy shapes, Q7 rows and d2 >= 2^22 among them: the two argmin passes + the Q7 relabel give the loop's records on every row"""
    rng = np.random.default_rng(11)
    q7 = 0
    for k in range(30):
        na, nb = int(rng.integers(1, 70)), int(rng.integers(2, 120))
        gen = (MC.tie_rows, MC.full_rows)[k % 2]
        a, b = gen(2 * k, na, "a").copy(), gen(2 * k + 1, nb, "b").copy()
        if k % 3 == 0:
            b[1] = b[0]
        if nb > 4:
            b[nb - 1] = b[2]
            a[0] = b[2]
        loop = NP.match_2nn(a, b)
        got = NM.match_2nn(a, b, a_index_base=5)
        assert [int(r[0]) for r in got] == [5 + i for i in range(na)]
        for i, (_, bi, si, bd, sd) in enumerate(loop):
            assert (int(got[i, 1]), int(got[i, 2])) == (bi, si), (k, i)
            assert got[i, 3] == np.float32(bd).view(u32) and got[i, 4] == np.float32(sd).view(u32), (k, i)
        d = NM.distances(a, b)
        q7 += int((d[:, 0] == d[:, 1]).sum())
    assert q7 > 100


@pytest.mark.parametrize("family", sorted(MC.FAMILIES))
def test_reference_equals_the_oracle(vk, oracle, family):
    gen = MC.FAMILIES[family]
    a, b = gen(1, 300, "a").copy(), gen(2, 700, "b").copy()
    b[1] = b[0]
    b[650] = b[40]
    a[::9] = b[40]
    assert np.array_equal(NM.match_2nn(a, b), as_words(oracle.match_2nn(a, b)))
    assert np.array_equal(NM.match_2nn(a[:5], NM.pad_two(b[:1])), as_words(oracle.match_2nn(a[:5], np.vstack([b[:1], np.zeros((1, 128), np.uint8)]))))


def test_reference_equals_the_golden_records():
    a, b = np.load(os.path.join(GOLDEN, "desc_a.npy")), np.load(os.path.join(GOLDEN, "desc_b.npy"))
    assert np.array_equal(NM.match_2nn(a, b), as_words(np.load(os.path.join(GOLDEN, "matches_a_b.npy"))))


def test_shifted_norms():
    rows = np.array([[0] * 128, [128] * 128, [255] * 128], np.uint8)
    assert NM.shifted_norms(rows).tolist() == [128 ** 3, 0, 127 * 127 * 128]


def test_index_base_wraps():
    a, b = MC.tie_rows(1, 3), MC.tie_rows(2, 4)
    assert NM.match_2nn(a, b, 0xFFFFFFFE)[:, 0].tolist() == [0xFFFFFFFE, 0xFFFFFFFF, 0]


# ---------------------------------------------------------------------------------------------------------------------- which edge a case reaches
def test_regimes_of_the_pointer_cases(vk):
    """the shapes sit ON the borders of the planner as the code has them (hip/match.hip: vksift_hip_match_2nn_prenormed)"""
    by = {(c["na"], c["nb"]): c["regime"] for c in MC.POINTER}
    assert by[1536, 4096] == "small" and by[1537, 2] == "scan" and by[1, 4097] == "scan" and by[97, 32769] == "scan"
    assert by[1954, 32768] == "packed key <2,64>" and MC.regime(1953, 32768) == "scan" and 1953 * 32768 < MC.PK_WORK <= 1954 * 32768
    assert MC.regime(4097, 15622) == "packed key <4,128>"
    # with the cell scan on (the default) nothing reaches the stream decomposition through the pointer entries
    assert not any(c["regime"] == "stream" for c in MC.POINTER) and [c["regime"] for c in MC.STREAM] == ["stream", "stream", "small"]
    for regime in ("small", "scan"):   # every descriptor family and every index base in both regimes
        assert {c["family"] for c in MC.POINTER if c["regime"] == regime} == set(MC.FAMILIES)
        assert {c["base"] for c in MC.POINTER if c["regime"] == regime} == set(MC.BASES)
        assert {c["joined"] for c in MC.POINTER if c["regime"] == regime} == {False, True}
    assert [c["regime"] for c in MC.SCAN_FORM] == ["small", "scan", "scan"]
    assert by[768, 300] == by[769, 300] == "small" and by[768, 4097] == by[769, 4097] == "scan"
    # the library's own figures
    L = HM.bind(vk.lib())
    for c in MC.POINTER:
        assert MC.desc_min_words(c["na"], c["nb"]) == L.vksift_hip_match_scratch_u32(c["na"], c["nb"])
        assert MC.prenormed_min_words(c["na"]) == L.vksift_hip_match_scratch_u32(c["na"], c["nb"]) - c["na"] - c["nb"]


def test_pointer_cases_reach_their_edges(vk):
    for c in MC.POINTER + MC.STREAM:
        a, b = MC.pair(c)
        rec = MC.pair_records(c)
        d = NM.distances(a[:256], b)
        if c["family"] == "full" and c["nb"] > 8:   # float replay: second distances of d2 >= 2^22
            assert (rec[:, 4].view(np.float32) >= 2048.0).any(), c["name"]
        if c["family"] != "full":                    # Q7: d(b0) == d(b1), best or second among them relabelled
            assert (d[:, 0] == d[:, 1]).all(), c["name"]
        if c["na"] >= 16 and c["nb"] > 16:
            assert (rec[:, 3] == 0).any(), c["name"]   # exact hits
        if c["na"] >= 16 and c["nb"] > 100 and c["family"] != "full":
            assert (rec[:, 3] == rec[:, 4]).any(), c["name"]   # ties between best and second
    big = MC.by_shape(1954, 32768)
    rec = MC.pair_records(big)
    assert rec[:3, 1].tolist() == [4095, 4096, 32767] and (rec[:3, 3] == 0).all()
    assert rec[3, 1:3].tolist() == [5, 8192 + 5] and rec[3, 3] == rec[3, 4] == 0      # a tie across super-chunks: the earlier column first
    tied = rec[rec[:, 3] == rec[:, 4]]
    assert (tied[:, 1] // 4096 != tied[:, 2] // 4096).sum() > 10
    far = MC.pair_records(MC.by_shape(97, 32769))
    assert far[:2, 1].tolist() == [32767, 32768]


def test_async_cases_reach_their_edges(vk):
    names = [c["name"] for c in MC.ASYNC + MC.NO_PK]
    assert len(set(names)) == len(names)
    assert {len(c["ids_a"]) for c in MC.ASYNC} >= {1, 2, 7, 8, 17, 256} and {c["n_stride"] for c in MC.ASYNC} == {2, 4, 5}
    seven = MC.async_named(MC.ASYNC[4]["name"])
    na = [seven["counts"][e] for e in seven["ids_a"]]
    nb = [seven["counts"][e] for e in seven["ids_b"]]
    assert {0, 255, 256, 257} <= set(na) and {0, 1, 2} <= set(nb)
    assert any(a == b for a, b in zip(seven["ids_a"], seven["ids_b"]))                                     # one entry as A and B
    assert seven["ids_a"].count(7) + seven["ids_b"].count(7) >= 3                                          # one entry named by several slots
    assert set(range(len(seven["counts"]))) - set(seven["ids_a"]) - set(seven["ids_b"])                    # entries not named
    assert seven["ids_a"] != sorted(seven["ids_a"])                                                        # in any order
    # which kernels the host queues (restated from the launcher)
    k = {c["name"]: MC.async_kernels(c) for c in MC.ASYNC}
    assert k[MC.ASYNC[0]["name"]] == ["split", "stream"] and MC.ASYNC[0]["max_na"] > MC.SMALL_NA == MC.ASYNC[0]["counts"][0]
    assert k[MC.ASYNC[1]["name"]] == ["split", "stream"] and k[MC.ASYNC[2]["name"]] == ["packed key"]
    assert k[MC.ASYNC[8]["name"]] == []
    assert k[MC.ASYNC[15]["name"]] == ["packed key"] and k[MC.ASYNC[16]["name"]] == ["packed key", "prune<1>"]
    assert k[MC.ASYNC[17]["name"]] == ["packed key", "prune<1> walking the slots"] and MC.ASYNC[17]["ids_b"].index(2) >= 16
    assert [MC.async_kernels(c, pk=False) for c in MC.NO_PK] == [["split", "prune<1>"], ["split", "prune<1>"], ["split", "prune<1>", "prune<2>"]]
    assert [len(c["ids_a"]) for c in MC.NO_PK] == [8, 2, 2]
    # N_B = 4095, 4096, 4097: the best match of rows 0 and 1 in rows 4095 and 4096 where they exist
    recs = MC.world_records(MC.ASYNC[14])
    assert [r[1] for r in recs] == [4095, 4096, 4097]
    assert recs[1][2][0, 1] == 4095 and recs[2][2][0, 1] == 4095 and recs[2][2][1, 1] == 4096 and recs[0][2][0, 3] != 0 and recs[1][2][1, 3] != 0
    assert (recs[2][2][:2, 3] == 0).all()
    # the full-range family: second distances of d2 >= 2^22 in a batch too
    assert any((r[2][:, 4].view(np.float32) >= 2048.0).any() for r in MC.world_records(MC.ASYNC[6]) if len(r[2]))


@pytest.mark.parametrize("case", [c for c in MC.ASYNC if c["family"] == "sift" and c["max_na"]], ids=ids)
def test_decoys_would_win_if_read(vk, case):
    """the rows of a cache entry behind its count: a kernel that read them would report them"""
    w = MC.world(case)
    assert w["covered"]
    recs = MC.world_records(case)
    for k in w["covered"][:4]:
        ea, eb = w["ids_a"][k], w["ids_b"][k]
        seen = np.concatenate([NM.pad_two(w["rows"][eb]), w["decoys"][eb]])
        assert not np.array_equal(NM.match_2nn(w["rows"][ea], seen), recs[k][2]), (case["name"], k)


# ---------------------------------------------------------------------------------------------------------------------- the scratch of the cell scan
def scan_top_word(na, pieces_last):
    """one past the highest word the cell scan writes: [row list: 1 + na][pad to 16 bytes][16 words per (row, piece), 32 pieces per row]"""
    cells = (na + 1 + 3) // 4 * 4
    return cells + ((na - 1) * HM.CHUNKS + pieces_last) * 16


def test_cell_scan_needs_more_than_the_old_minimum(tmp_path):
    """match_stream.h compiled on the host, 256 workgroups (the compute units of an MI355X), 768-row blocks, 256-row tiles: the last row block
    of 200 x 7 680 has 30 pieces, whose lists end behind the 72 + 512 na words the header documented up to ABI version 7 — and inside
    vksift_hip_match_scratch_u32(na, nb) - na - nb, which it documents now. 69 x 7 680 fits either."""
    exe = str(tmp_path / "stream_probe")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vulkansift_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "stream_probe.cpp"), "-o", exe], check=True)
    shapes = [(200, 7680), (1537, 4097), (69, 7680)] + [(c["na"], c["nb"]) for c in MC.POINTER if c["regime"] == "scan"]
    r = subprocess.run([exe], input="".join(f"{na} {nb} 256 768 256\n" for na, nb in shapes), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    last = [int(line.split()[-1]) for line in r.stdout.splitlines() if line.startswith("M")]
    assert len(last) == len(shapes)
    top = {s: scan_top_word(s[0], p) for s, p in zip(shapes, last)}
    assert last[0] == 30 and top[200, 7680] == 102572 > MC.OLD_PRENORMED_MIN(200) == 102472
    assert top[1537, 4097] == 788244 > MC.OLD_PRENORMED_MIN(1537) == 787016
    assert top[69, 7680] <= MC.OLD_PRENORMED_MIN(69)
    for (na, nb), t in top.items():
        assert t <= MC.prenormed_min_words(na), (na, nb)
    # the four-wave form (VKSIFT_TUNE_SCAN_FORM = 1: 512 workgroups, 256-row blocks, 128-row tiles) on the shapes test_prenormed_other_scan_form
    # runs through the scan: 200 x 7 680 has 60 tiles in runs of two, again 30 pieces; 769 x 4 097 has 33 tiles per row block, 17 pieces
    form1 = [(c["na"], c["nb"]) for c in MC.SCAN_FORM if c["regime"] == "scan"]
    assert form1 == [(200, 7680), (769, 4097)]
    r = subprocess.run([exe], input="".join(f"{na} {nb} 512 256 128\n" for na, nb in form1), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pieces = [[int(x) for x in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("M")]
    assert pieces[0] == [30] and len(pieces[1]) == 4 and max(pieces[1]) == 17 and pieces[1][-1] == 17
    for (na, nb), p in zip(form1, pieces):
        assert MC.OLD_PRENORMED_MIN(na) < scan_top_word(na, p[-1]) <= MC.prenormed_min_words(na), (na, nb)
    # whatever the grid: 32 pieces at most, and the row list never needs more than na + 4 words
    for na in (1, 2, 3, 4, 5, 103, 104, 1000003):
        assert scan_top_word(na, HM.CHUNKS) <= MC.prenormed_min_words(na)


# ---------------------------------------------------------------------------------------------------------------------- the arenas
def arena_checks(h):
    exp = h.expected()
    h.check(exp)                                              # the comparison accepts the contract
    diff = exp != h.host
    mask = np.zeros(len(exp), bool)
    for blk, first, nbytes in h.written():
        mask[blk.off + first:blk.off + first + nbytes] = True
    assert not (diff & ~mask).any(), h.what                   # nothing but the records and the count words differs from what went in
    spoiled = exp.copy()
    runs = h.written()
    for blk, first, nbytes in runs[:3] + runs[-3:]:           # one byte behind a written run is noticed
        spoiled[blk.off + first + nbytes] ^= 1
        with pytest.raises(AssertionError):
            h.check(spoiled)
        spoiled[blk.off + first + nbytes] ^= 1
    free = h.free_runs[:3] + h.free_runs[-3:]
    for blk, first, nbytes in free:                           # scratch: free inside its extent — every slot's own run of row flags —,
        if nbytes:                                            # watched from there on: the padding behind an INNER slot's flags too
            spoiled[blk.off + first + nbytes - 1] ^= 1
            h.check(spoiled)
            spoiled[blk.off + first + nbytes - 1] ^= 1
        spoiled[blk.off + first + nbytes] ^= 1
        with pytest.raises(AssertionError):
            h.check(spoiled)
        spoiled[blk.off + first + nbytes] ^= 1


@pytest.mark.parametrize("case", MC.POINTER + MC.STREAM, ids=ids)
def test_pointer_arenas_on_the_cpu(vk, case):
    for entry in ("match_2nn_prenormed", "match_2nn_desc"):
        h = HM.LAUNCHES[entry](case, device="cpu")
        assert h.args["scratch"] % 16 == 0 and h.args["desc_a"] % 16 == 0 and h.args["desc_b"] % 16 == 0
        if entry == "match_2nn_desc":
            assert (h.args["desc_b"] == h.args["desc_a"] + case["na"] * 128) == case["joined"]
        arena_checks(h)


@pytest.mark.parametrize("case", MC.ASYNC + MC.NO_PK, ids=ids)
def test_async_arenas_on_the_cpu(vk, case):
    h = HM.Async(case, device="cpu")
    zeroed = HM.Async(case, device="cpu", fill=0)
    differ = np.flatnonzero(h.host != zeroed.host)
    assert len(differ) and all(h.where(int(b)).startswith(("'row flags'", "'partial lists'")) for b in (differ[0], differ[-1]))   # the fill reaches scratch only
    c = h.world
    assert h.desc_stride > c["cap"] * 128 > max(c["counts"]) * 128 and h.norm_stride > c["cap"] and h.desc_stride % 16 == 0
    assert h.match_stride > 20 * max(c["counts"][e] for e in c["ids_a"]) and h.redo_stride > c["max_na"]
    raw = h.view(h.host, h.cache_desc)
    norms = h.view(h.host, h.cache_norm, u32)
    for e, n in enumerate(c["counts"]):
        if n < 2:   # an entry of fewer than two rows: zero rows with norm 128^3 up to row 2
            assert not raw[e * h.desc_stride + n * 128:e * h.desc_stride + 256].any() and (norms[e * h.norm_stride + n:e * h.norm_stride + 2] == 128 ** 3).all()
    # the row flags are free per slot, max_na words each: the padding of the stride lies between two runs and is compared
    flags = [(first, nbytes) for blk, first, nbytes in h.free_runs if blk is h.redo]
    assert flags == [(4 * k * h.redo_stride, 4 * c["max_na"]) for k in range(len(c["ids_a"]))] and h.redo_stride - max(c["max_na"], 1) == c["extra"] > 0
    arena_checks(h)


def test_refusal_table():
    assert len(MC.REFUSALS) == 12 and len(MC.NOTHING) == 2
    for entry, name, changes in MC.REFUSALS + MC.NOTHING:
        assert HM.case_named(entry, name)["name"] == name
