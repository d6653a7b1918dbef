"""The case table of the matcher launchers (vksift_hip_match_2nn_prenormed, _desc, _async): plain data and seeded rows, imported by
tests/test_np_match.py (CPU: pins the reference and asserts which edge each case reaches) and tests/test_gpu_match_launchers.py (one
launch per case). tests/hip_match.py turns a case into a poisoned arena and the bytes the contract expects.

A case names the REGIME the code dispatches it to (regime() / async_kernels() restate the host planner of hip/match.hip); the shapes are the
smallest that reach each edge. Rows are generated on first use and shared (pair(), world())."""
import functools

import numpy as np

import np_match as NM

SMALL_NA, SMALL_NB, PK_NB, PK_WORK = 1536, 4096, 32768, 64000000
BASES = (0, 1234, 0xFFFF0000)   # a_index_base: none, a shard offset, one that wraps modulo 2^32 inside the rows


# ====================================================================================================================== descriptor families
def sift_rows(seed, n, side="a"):
    """SIFT-like rows (the library's own generator, a host function): d2 far below 2^20"""
    from vulkansift_amd import api

    return api.gen_synthetic_descriptors(seed, n) if n else np.empty((0, 128), np.uint8)


def tie_rows(seed, n, side="a"):
    """bytes from {0, 255}: many exactly equal distances"""
    return (np.random.default_rng(seed).integers(0, 2, (n, 128)) * 255).astype(np.uint8)


def full_rows(seed, n, side="a"):
    """Full-range rows whose two nearest neighbours lie at d2 >= 2^22, where different integers share one float sqrt (quirk Q8) and only the
    float replay orders them. Uniformly random bytes cannot do that — their d2 is about 128 * 65535 / 6 = 1.4 M whatever the other row is —,
    so the two sides differ: query rows are random bytes over the full range, every fourth one from {0, 255} with nine bytes in ten 255;
    reference rows hold bytes below 96, every fourth one from {0, 255} with nine bytes in ten 0. Such a query row is at d2 of about
    128 * 207^2 = 5.5 M and 6.8 M from every reference row (and at 7.5 M from the zero rows of quirk Q6)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256 if side == "a" else 96, (n, 128), dtype=np.uint8)
    rows[::4] = np.where(rng.random(rows[::4].shape) < (0.9 if side == "a" else 0.1), 255, 0)
    return rows


FAMILIES = {"sift": sift_rows, "ties": tie_rows, "full": full_rows}


# ====================================================================================================================== single pair by pointer
def regime(na, nb, pk=True, scan=True):
    """what vksift_hip_match_2nn_prenormed dispatches (na, nb) to, in the order of its tests"""
    if pk and nb <= PK_NB and na * nb >= PK_WORK:
        return "packed key <2,64>" if na <= 4096 else "packed key <4,128>"
    if na <= SMALL_NA and nb <= SMALL_NB:
        return "small"
    return "scan" if scan else "stream"


def pcase(na, nb, family, why, hits=()):
    return dict(na=na, nb=nb, family=family, hits=tuple(hits), regime=regime(na, nb), name=f"{regime(na, nb)}: {na} x {nb} {family}, {why}")


POINTER = [
    pcase(1, 2, "sift", "the smallest problem"),
    pcase(1, 3, "ties", "one row behind b0, b1"),
    pcase(16, 63, "full", "one workgroup, one partial tile"),
    pcase(17, 64, "sift", "two workgroups, one full tile"),
    pcase(17, 65, "ties", "a second tile of one row"),
    pcase(SMALL_NA, SMALL_NB, "sift", "the last shape of the small kernel"),
    pcase(SMALL_NA + 1, 2, "sift", "one partial tile of B"),
    pcase(1, SMALL_NB + 1, "ties", "one query row"),
    pcase(768, 300, "full", "48 workgroups"),
    pcase(769, 300, "ties", "a 49th workgroup of one row"),
    pcase(97, PK_NB + 1, "sift", "beyond the packed-key range", hits=(PK_NB - 1, PK_NB)),
    pcase(200, 7680, "sift", "30 pieces on the last row block, minimum scratch"),
    pcase(1954, PK_NB, "sift", "pieces + merge, several super-chunks", hits=(4095, 4096, PK_NB - 1)),
    # 768 x 300 and 769 x 300 lie below both borders of the small kernel; these two are the row-block border of the cell scan itself
    pcase(768, SMALL_NB + 1, "full", "one full row block, every row replayed"),
    pcase(769, SMALL_NB + 1, "ties", "a second row block of one row"),
]
for _i, _c in enumerate(POINTER):
    _c["base"], _c["joined"] = BASES[_i % 3], _i % 2 == 0   # _desc: B directly behind A in one block (the fused-norms branch) or in a block of its own
SCAN_FORM = [c for c in POINTER if (c["na"], c["nb"]) in ((200, 7680), (769, 300), (769, SMALL_NB + 1))]   # once more under vksift_hip_tune(VKSIFT_TUNE_SCAN_FORM, 1)
# VKSIFT_MATCH_SCAN=0 (a child process): the stream decomposition through the pointer entries
# (33 x 130 stays with the one-launch small kernel, switch or no switch: the small case is tested before the switch is)
STREAM = [dict(pcase(na, nb, fam, why), regime=regime(na, nb, scan=False), name=f"no cell scan, {regime(na, nb, scan=False)}: {na} x {nb} {fam}, {why}", base=BASES[i % 3],
               joined=i % 2 == 1)
          for i, (na, nb, fam, why) in enumerate([(1537, 4096, "sift", "seven row blocks"), (513, 4097, "ties", "a 33rd tile of one row"), (33, 130, "full", "below both borders")])]


def by_shape(na, nb):
    return next(c for c in POINTER if (c["na"], c["nb"]) == (na, nb))


def pointer_named(name):
    return next(c for c in POINTER + STREAM if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _pair(name):
    c = pointer_named(name)
    na, nb, gen = c["na"], c["nb"], FAMILIES[c["family"]]
    rng = np.random.default_rng(na * 7 + nb)
    a, b = gen(na + 17, na, "a").copy(), gen(nb + 1000, nb, "b").copy()
    if c["family"] != "full":
        b[1] = b[0]                                       # quirk Q7 for every row of A
    if nb > 8:
        dup = rng.permutation(np.arange(2, nb))[: nb // 4]
        b[dup] = b[rng.integers(2, nb, len(dup))]         # duplicate rows anywhere in B: across tiles, pieces and super-chunks
    if c["family"] == "ties":
        b[::7] = b[0]
        a[::5] = b[0]
    hit = rng.permutation(na)[: max(na // 10, 1)]
    a[hit] = b[rng.integers(0, nb, len(hit))]             # queries equal to reference rows: zero distances, some to duplicated rows
    for k, col in enumerate(c["hits"]):                   # exact hits at the named columns, from distinct rows
        b[col] = gen(col + 5, 1, "b")[0]
        a[k] = b[col]
    if c["hits"] and nb > 8192 + 5:
        b[8192 + 5] = b[5]                                # a tie of column 5 with a column two super-chunks later
        a[len(c["hits"])] = b[5]
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def pair(case):
    """(a, b) of a pointer case, generated once"""
    return _pair(case["name"])


@functools.lru_cache(maxsize=None)
def _pair_records(name):
    a, b = _pair(name)
    rec = NM.match_2nn(a, b, pointer_named(name)["base"])
    rec.setflags(write=False)
    return rec


def pair_records(case):
    """the records the contract expects of a pointer case, computed once and shared by the tests that need them"""
    return _pair_records(case["name"])


def prenormed_min_words(na):
    """the documented minimum scratch of vksift_hip_match_2nn_prenormed: vksift_hip_match_scratch_u32(na, nb) - na - nb"""
    return 72 + 513 * na


def desc_min_words(na, nb):
    return 2 * na + nb + 72 + 512 * na


OLD_PRENORMED_MIN = lambda na: 72 + 512 * na   # what the header asked for up to ABI version 7: the cell scan writes past it (tests/test_np_match.py)


# ====================================================================================================================== async
def acase(name, counts, slots, *, family="sift", max_na="exact", max_nb="bound", nb_exact=0, n_stride=2, partial=False, shared=(), extra=3, seed=1):
    """counts[e]: rows of cache entry e; slots: (entry of A, entry of B) per slot; max_na: "exact" = the largest N_A of a slot; max_nb: "bound" = a
    capacity above every count, "exact" = the largest N_B of a slot; shared: entries that are prefixes of ONE generated set; extra: rows of
    every entry behind the largest count (decoys), and the unit of the stride paddings"""
    ids_a, ids_b = [s[0] for s in slots], [s[1] for s in slots]
    na_max, nb_max = max([counts[e] for e in ids_a] + [0]), max([counts[e] for e in ids_b] + [0])
    return dict(name=name, counts=list(counts), ids_a=ids_a, ids_b=ids_b, family=family, nb_exact=nb_exact, n_stride=n_stride, partial=partial, shared=tuple(shared),
                extra=extra, seed=seed, max_na=na_max if max_na == "exact" else max_na, max_nb=nb_max if max_nb == "exact" else max(counts) + 1000)


SMALL_COUNTS = [0, 1, 2, 3, 255, 256, 257, 300, 97, 40, 130, 64]
SEVEN = [(4, 0), (5, 1), (6, 2), (0, 7), (7, 7), (7, 4), (3, 5)]   # N_A 255 / 256 / 257 against N_B 0 / 1 / 2, N_A = 0, a self-match, entry 7 four times


def _random_slots(n, seed, entries=len(SMALL_COUNTS) - 2):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, entries)), int(rng.integers(0, entries))) for _ in range(n)]


def _big_slots(n, at):
    """n slots over the entries {0: 97 rows, 1: 300 rows, 2: 32 769 rows}: the large reference set at slot `at` only"""
    small = [(0, 1), (1, 0), (1, 1), (0, 0)]
    return [(0, 2) if k == at else small[k % 4] for k in range(n)]


BIG_COUNTS = [97, 300, PK_NB + 1]
ASYNC = [
    acase("1 slot with partial lists, N_A = 1536: the small kernel", [SMALL_NA, 300], [(0, 1)], partial=True, max_na=1600),
    acase("1 slot with partial lists, N_A = 1537: the stream decomposition", [SMALL_NA + 1, 300], [(0, 1)], partial=True, n_stride=4),
    acase("1 slot without partial lists: the batch kernels", [257, 300], [(0, 1)], n_stride=5),
    acase("2 slots", SMALL_COUNTS, [(7, 8), (4, 7)]),
    acase("7 slots: N_A 0, 255, 256, 257, N_B 0, 1, 2, a self-match, entries not named", SMALL_COUNTS, SEVEN, n_stride=4),
    acase("7 slots, tie-heavy rows", SMALL_COUNTS, SEVEN, family="ties", n_stride=5, seed=2),
    acase("7 slots, full-range rows: every row replayed", SMALL_COUNTS, SEVEN, family="full", seed=3),
    acase("7 slots, max_na a loose capacity of 5000: the same bytes", SMALL_COUNTS, SEVEN, n_stride=4, max_na=5000),
    acase("7 slots, max_na = 0: the count words only", SMALL_COUNTS, SEVEN, n_stride=4, max_na=0),
    acase("7 slots, max_nb exact", SMALL_COUNTS, SEVEN, n_stride=4, max_nb="exact", nb_exact=1),
    acase("8 slots, entries in descending order", SMALL_COUNTS, [(6, 7), (5, 6), (4, 5), (3, 4), (2, 3), (1, 10), (8, 8), (7, 11)], n_stride=5),
    acase("17 slots", SMALL_COUNTS, _random_slots(17, 17)),
    acase("256 slots", SMALL_COUNTS, _random_slots(256, 256), n_stride=4),
    acase("2 slots, N_A = 4097 against N_B = 3: the packed-key grid loops over 17 row blocks", [4097, 3, 40], [(0, 1), (2, 1)]),
    acase("3 slots, N_B = 4095, 4096, 4097 with the best match in rows 4095 and 4096", [40, 4095, 4096, 4097], [(0, 1), (0, 2), (0, 3)], shared=(1, 2, 3), n_stride=5),
    acase("2 slots, N_B = 32769 under a bound: the packed-key kernel", BIG_COUNTS, _big_slots(2, 1)),
    acase("2 slots, N_B = 32769 exact: the pruning kernel takes that slot", BIG_COUNTS, _big_slots(2, 1), max_nb="exact", nb_exact=1),
    acase("17 slots, N_B = 32769 exact at slot 16: the pruning kernel walks the slots", BIG_COUNTS, _big_slots(17, 16), max_nb="exact", nb_exact=1, n_stride=4),
]
# VKSIFT_MATCH_PK=0 (a child process): the B-split and pruning kernels carry the batch, on the borders of their N_A regimes
NO_PK = [
    acase("no packed key, 8 slots, N_A = 1024 and 1025", [1024, 1025, 70], [(0, 2), (1, 2)] * 4, n_stride=4),
    acase("no packed key, 2 slots, N_A = 8192 and 8193", [8192, 8193, 70], [(0, 2), (1, 2)]),
    acase("no packed key, 2 slots, N_A = 32768 and 32769", [PK_NB, PK_NB + 1, 70], [(0, 2), (1, 2)], n_stride=5),
]
GROUPS = {"VKSIFT_MATCH_PK": NO_PK, "VKSIFT_MATCH_SCAN": STREAM}   # switch -> the cases a child process runs with the switch set to 0


def async_named(name):
    return next(c for c in ASYNC + NO_PK if c["name"] == name)


def async_kernels(c, pk=True):
    """the kernels vksift_hip_match_2nn_async queues for a case (besides k_slot_counts and k_match_redo), restated from its host code"""
    n, max_na = len(c["ids_a"]), c["max_na"]
    if max_na == 0:
        return []
    if n == 1 and c["partial"]:
        return ["split"] + (["stream"] if max_na > SMALL_NA else [])
    prune = not pk or (c["max_nb"] > PK_NB and c["nb_exact"] != 0)
    s1 = 0 if pk else (1024 if n >= 8 else 8192)
    out = ["packed key"] if pk else []
    if min(max_na, s1) > 0:
        out.append("split")
    if prune and max_na > s1:
        out.append("prune<1>" + (" walking the slots" if pk and n > 16 else ""))
    if prune and max_na > PK_NB:
        out.append("prune<2>")
    return out


@functools.lru_cache(maxsize=None)
def _world(name):
    c = async_named(name)
    counts, gen = c["counts"], FAMILIES[c["family"]]
    side = lambda e: "b" if e in c["ids_b"] else "a"   # the sides of the full-range family differ (full_rows)
    shared_set = gen(c["seed"] * 1000 + 999, max([counts[e] for e in c["shared"]] + [0]), "b").copy()
    rows = [shared_set[:n].copy() if e in c["shared"] else gen(c["seed"] * 1000 + e, n, side(e)).copy() for e, n in enumerate(counts)]
    if c["shared"]:                                   # the best match of query rows 0 and 1 in rows 4095 and 4096 of the shared set
        a = rows[c["ids_a"][0]]
        a[0], a[1] = shared_set[len(shared_set) - 2], shared_set[len(shared_set) - 1]
    else:
        for k, (ea, eb) in enumerate(zip(c["ids_a"], c["ids_b"])):   # a query equal to a reference row in every slot (the last row of B in every third)
            if ea != eb and counts[ea] and counts[eb]:
                rows[ea][k % counts[ea]] = rows[eb][counts[eb] - 1 if k % 3 == 0 else (7 * k) % counts[eb]]
    # the rows of an entry at and beyond its count: zero rows up to row 2 (vksift_hip_gather_sections), then decoys — copies of the query rows
    # of the slots that match against the entry, which would win if a kernel read them
    cap = max(counts) + c["extra"]
    decoys, covered = [], set()
    for e, n in enumerate(counts):
        users = [k for k, eb in enumerate(c["ids_b"]) if eb == e and counts[c["ids_a"][k]] > 0]
        first = max(n, 2)
        d = np.empty((cap - first, 128), np.uint8)
        for j in range(len(d)):
            if users:
                k = users[j % len(users)]
                qa = rows[c["ids_a"][k]]
                d[j] = qa[(j // len(users)) % len(qa)]
                covered.add(k)
            else:
                d[j] = rows[(e + 1) % len(rows)][j % counts[(e + 1) % len(rows)]] if counts[(e + 1) % len(rows)] else 255
        decoys.append(d)
    for r in rows + decoys:
        r.setflags(write=False)
    return dict(c, rows=rows, decoys=decoys, covered=sorted(covered), cap=cap)


def world(case):
    """the case with its rows: "rows"[e] (counts[e], 128), "decoys"[e]: what the entry holds from row max(count, 2) on, "cap": rows per entry,
    "covered": the slots whose own query rows are among the decoys of their reference entry"""
    return _world(case["name"])


@functools.lru_cache(maxsize=None)
def _world_records(name):
    return NM.expected_async(_world(name))


def world_records(case):
    return _world_records(case["name"])


# ====================================================================================================================== refusals
# (entry, case name, changes): hipErrorInvalidValue and not a byte changed
REFUSALS = [(entry, by_shape(17, 65)["name"], ch) for entry in ("match_2nn_prenormed", "match_2nn_desc")
            for ch in (dict(nb=1), dict(nb=0), dict(scratch=None), {"+scratch_u32": -1})]
REFUSALS += [("match_2nn_prenormed", by_shape(200, 7680)["name"], {"+scratch_u32": -1}), ("match_2nn_desc", by_shape(200, 7680)["name"], {"+scratch_u32": -1})]
REFUSALS += [("match_2nn_async", ASYNC[3]["name"], dict(nslots=0)), ("match_2nn_async", ASYNC[3]["name"], dict(nslots=257))]
NOTHING = [(entry, by_shape(17, 65)["name"], dict(na=0)) for entry in ("match_2nn_prenormed", "match_2nn_desc")]   # returns 0 and changes not a byte
