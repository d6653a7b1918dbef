"""Pins, on the CPU and from the numpy restatements alone, the case tables tests/test_gpu_two_view_launchers.py holds the two-view launchers to:

  * every case of tests/two_view_cases.py laid out by tests/hip_two_view.py for device "cpu": the expected arena differs from the input
    arena exactly in the blocks the header names as written — the nslots records and bytes 0 .. n-1 of every slot's mask; for guided
    matching out_n[i] records per slot and the nslots counts — and in all of them (the GPU comparison is never one of empty results)
  * which edge each case reaches: the clamp, the decoys, the slot word beyond 64, ties at 65 536 hypotheses, a better hypothesis just outside
    nb_hypotheses (j*), which degenerate inputs give valid == 0, which refit rounds are accepted, which guided models yield nothing
  * for the steps whose removal must be noticed, that the EXPECTED BYTES differ from what a kernel without the step would write: the
    min(n, max_n) clamp, the mask bound n (not max_n), the counter stride, the `active` guard of the last workgroup
No GPU."""
import numpy as np
import pytest

import hip_two_view as HT
import np_verify as V
import two_view_cases as T

def laid_out(launch, case):
    h = HT.LAUNCHES[launch](case, "cpu")
    return h, h.expected()


def written(h, exp):
    """per block name the payload offsets where the expected arena differs from the input arena; nothing may differ outside the payloads"""
    diff = exp != h.host
    out, seen = {}, np.zeros(len(exp), bool)
    for blk in h.blocks:
        d = np.flatnonzero(diff[blk.off:blk.off + len(blk.payload)])
        seen[blk.off:blk.off + len(blk.payload)] = True
        if len(d):
            out[blk.name] = d
    assert not diff[~seen].any(), f"{h.what}: the expected arena differs in a guard zone"
    return out


# ====================================================================================================================== layout
@pytest.mark.parametrize("m", "hf")
def test_ransac_layout(m):
    launch = "ransac_" + ("homography" if m == "h" else "fundamental")
    for case in T.RANSAC[m]:
        h, exp = laid_out(launch, case)
        w = written(h, exp)
        assert set(w) <= {"records", "masks"} and "records" in w
        rec = 4 * h.words
        assert w["records"].max() < h.ns * rec and set(w["records"] // rec) == set(range(h.ns))       # every record, none beyond nslots
        want = np.concatenate([k * h.mask_stride + np.arange(n) for k, n in enumerate(h.slot_n)])    # a mask byte is 0 / 1, never the poison
        assert np.array_equal(w.get("masks", np.zeros(0, np.int64)), want)
        # the scratch: exactly what the library's formula asks for, and only its payload is exempt from the comparison
        assert h.free == [(h.scratch, 0, 4 * h.scratch_u32)] and len(h.scratch.payload) == 4 * h.scratch_u32 == 8 * h.ns * -(-case["nb_hyp"] // 256)
        assert case["max_n"] <= 600 and (case["nb_hyp"] <= 512 or case["name"] == "65536 hypotheses")


@pytest.mark.parametrize("m", "hf")
def test_refit_layout(m):
    launch = "refit_" + ("homography" if m == "h" else "fundamental")
    for case in T.REFIT[m]:
        h, exp = laid_out(launch, case)
        w = written(h, exp)
        assert set(w) <= {"records", "masks_out"} and "records" in w
        rec = 4 * T.REFIT_WORDS
        assert w["records"].max() < h.ns * rec and set(w["records"] // rec) == set(range(h.ns))
        want = np.concatenate([k * h.mask_stride + np.arange(n) for k, n in enumerate(h.slot_n)])
        got = w.get("masks_out", np.zeros(0, np.int64))
        # a start mask given back byte for byte (rounds == 0) may hold any byte but is n bytes all the same: no byte at or beyond n
        assert set(got) <= set(want) and len(got) >= len(want) - 2
        assert h.free == [] and len(h.start_masks.payload) != len(h.masks_out.payload) and 1 <= case["nb_rounds"] <= 8


def test_guided_layout():
    for case in T.GUIDED:
        h, exp = laid_out("match_guided", case)
        w = written(h, exp)
        assert set(w) <= {"records", "record counts"}
        recs = T.guided_expected(case)
        assert np.array_equal(w["record counts"], np.arange(4 * h.ns))                      # a count is below 2^24: no byte of it is the poison
        want = np.concatenate([k * h.out_stride + np.arange(16 * len(r)) for k, r in enumerate(recs)])
        got = w.get("records", np.zeros(0, np.int64))
        assert set(got) <= set(want.tolist()) and len(got) > 0.9 * len(want)                # (a distance may hold a 0xa5 byte)
        assert sum(len(r) for r in recs) > 0, case["name"]
        # the key scratch of a slot that is not valid stays compared
        assert [(lo // (32 * case["max_n"])) for _, lo, _ in h.free] == [k for k, s in enumerate(case["slots"]) if s["valid"]]
        assert len(h.scratch.payload) == 32 * h.ns * case["max_n"] and case["max_n"] <= 600


def test_refusals_name_cases():
    for launch, name, changes in T.REFUSALS:
        h = HT.LAUNCHES[launch](T.case_named(T.CASES[launch], name), "cpu")
        assert all(k.lstrip("+") in h.args for k in changes) and h.ns > 1


# ====================================================================================================================== RANSAC edges
def record_bytes(m, r):
    return HT.ransac_record(m, r).tobytes() + r["mask"].tobytes()


@pytest.mark.parametrize("m", "hf")
def test_ransac_cases_reach_their_edges(m):
    K, mod = T.SAMPLE[m], T.NP_RANSAC[m]
    case = T.case_named(T.RANSAC[m], "padded strides")
    assert [s["n_dev"] for s in case["slots"]] == [300, 65, K] and case["n_stride"] == 3 and (case["corr_extra"], case["mask_extra"]) == (5, 13)
    assert [r["valid"] for r in T.ransac_expected(case)][:2] == [1, 1]
    # ignoring n_stride reads the junk words, which the clamp turns into max_n: the expected bytes of slots 1 and 2 differ from that
    for i in (1, 2):
        s = case["slots"][i]
        assert len(s["rows"]) == s["n_dev"] < case["max_n"] < T.JUNK_COUNTER

    # decoys: rows n .. stride of every slot are true inliers; counting them changes the record (and a mask written to max_n would mark them)
    case = T.case_named(T.RANSAC[m], "decoys beyond n")
    for i, (s, r) in enumerate(zip(case["slots"], T.ransac_expected(case))):
        assert len(s["rows"]) == case["max_n"] + case["corr_extra"] > s["n_dev"] and r["valid"] == 1
        more = mod.ransac(s["rows"], case["nb_hyp"], case["thr"], case["seed"], slot=i)
        assert more["nb_inliers"] > r["nb_inliers"] and more["mask"][s["n_dev"]:].all()

    # clamp: all three counters act as 257, and one row more (the first decoy) would change the bytes
    case = T.case_named(T.RANSAC[m], "clamp")
    assert case["max_n"] == 257 and [s["n_dev"] for s in case["slots"]] == [258, 0xFFFFFFFF, 257]
    for i, (s, r) in enumerate(zip(case["slots"], T.ransac_expected(case))):
        assert r["nb_matches"] == 257 and r["valid"] == 1 and len(s["rows"]) == 260
        more = mod.ransac(s["rows"][:258], case["nb_hyp"], case["thr"], case["seed"], slot=i)
        assert record_bytes(m, more)[:len(record_bytes(m, r))] != record_bytes(m, r)

    case = T.case_named(T.RANSAC[m], "one slot, strides 0")
    assert len(case["slots"]) == 1 and case["strides"] == (0, 0) and T.ransac_expected(case)[0]["valid"] == 1

    # many slots: the slot word of the sampler key beyond 64, two workgroups per slot, every n around the sample size, both outcomes
    case = T.case_named(T.RANSAC[m], "many slots")
    assert len(case["slots"]) == 70 and case["max_n"] == 64 and case["nb_hyp"] == 300
    assert [s["n_dev"] for s in case["slots"][:6]] == [0, K - 1, K, K + 1, 63, 64]
    res = T.ransac_expected(case)
    assert all(r["valid"] == (1 if s["n_dev"] >= (K if m == "h" else K + 1) else 0) for s, r in zip(case["slots"], res))
    assert len({record_bytes(m, r) for r in res if r["valid"]}) == sum(r["valid"] for r in res)        # every slot has different data
    assert any(r["valid"] and r["best_hypothesis"] >= 256 for r in res)
    assert mod.sample_k(9, 65, 3, 64, K) != mod.sample_k(9, 1, 3, 64, K) if m == "f" else V.sample(9, 65, 3, 64) != V.sample(9, 1, 3, 64)


@pytest.mark.parametrize("m", "hf")
def test_hypothesis_count_cases(m):
    names = [c["name"] for c in T.RANSAC[m]]
    for nb in T.HYP_COUNTS:
        assert f"{nb} hypotheses" in names
    # 65 536 hypotheses on 40 correspondences: many tie at the best count, over many workgroups; the lowest id wins
    case = T.case_named(T.RANSAC[m], "65536 hypotheses")
    r = T.ransac_expected(case)[1]
    _, per_id = T.hypothesis_counts(m, 65536)
    best = np.flatnonzero(per_id == per_id.max())
    assert len(best) > 1 and len(set(best >> (10 if m == "f" else 8))) > 1                    # ties, and between workgroups
    first = int(best[0])
    assert r["valid"] == 1 and r["nb_inliers"] == per_id.max()
    assert (r["best_hypothesis"], r.get("best_root", 0)) == ((first >> 2, first & 3) if m == "f" else (first, 0))
    # j*: a strictly better hypothesis in the first inactive lane of the last workgroup
    j = T.j_star(m)
    assert j is not None and j == T.J_STAR[m] and j % 256
    case = T.case_named(T.RANSAC[m], f"{j} hypotheses (j*)")
    assert case["nb_hyp"] == j and case["seed"] == T.HYP_SEED[m]
    c = T.hypothesis_counts(m, 1024)[0]
    r = T.ransac_expected(case)[1]
    assert r["valid"] == 1 and r["nb_inliers"] == c[:j].max() < c[j]
    one_more = T.NP_RANSAC[m].ransac(case["slots"][1]["rows"], j + 1, case["thr"], case["seed"], slot=1)
    assert one_more["best_hypothesis"] == j and record_bytes(m, one_more) != record_bytes(m, r)


# valid of every degenerate slot, in the order of two_view_cases.DEGENERATE, as the restatement gives it at both thresholds
DEGENERATE_VALID = {"h": [1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0], "f": [1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0]}


@pytest.mark.parametrize("m", "hf")
def test_degenerate_cases(m):
    for thr in (2.5, 0.5):
        case = T.case_named(T.RANSAC[m], f"degenerate data, threshold {thr}")
        assert case["nb_hyp"] == 256 and case["thr"] == thr and all(s["n_dev"] == 300 == len(s["rows"]) for s in case["slots"])
        res = T.ransac_expected(case)
        assert [r["valid"] for r in res] == DEGENERATE_VALID[m]
        assert 0 < sum(DEGENERATE_VALID[m]) < len(T.DEGENERATE)                             # both outcomes occur
        for r in res:
            assert r["valid"] or (not r["mask"].any() and not np.asarray(r[T.MODEL_KEY[m]]).any() and r["nb_inliers"] == 0 and r["nb_matches"] == 300)
        named = dict(zip(T.DEGENERATE, res))
        assert not named["every third row NaN"]["mask"][::3].any() and named["every third row NaN"]["mask"].any()
        assert named["side B equals side A"]["nb_inliers"] == 300
    rows = dict(zip(T.DEGENERATE, T.degenerate_rows(m)))
    sub = rows["scaled by 1e-41 (subnormal)"]
    assert ((sub.view(np.uint32) & 0x7F800000) == 0).all() and sub.any()                      # every coordinate subnormal, not all zero
    assert np.isfinite(rows["scaled by 1e30"]).all() and np.isinf(rows["+inf and -inf"]).sum() == 2


# ====================================================================================================================== refit edges
REFIT_ROUNDS_8 = {"h": [8, 8, 8, 0, 0, 8, 8, 8], "f": [1, 8, 8, 0, 0, 8, 8, 8]}   # the last accepted round of every special slot with nb_rounds = 8


@pytest.mark.parametrize("m", "hf")
def test_refit_cases_reach_their_edges(m):
    key = T.MODEL_KEY[m]
    for name in ("padded strides", "clamp", "many slots"):
        case = T.case_named(T.REFIT[m], name)
        assert case["base"] is T.case_named(T.RANSAC[m], name) and case["nb_rounds"] == 3
        assert any(r["rounds"] >= 1 for r in T.refit_expected(case))
    case = T.case_named(T.REFIT[m], "clamp")
    assert all(r["nb_matches"] == 257 for r in T.refit_expected(case))
    many = T.refit_expected(T.case_named(T.REFIT[m], "many slots"))
    assert {r["valid"] for r in many} == {0, 1} and len(many) == 70

    one, eight = T.case_named(T.REFIT[m], "special slots, 1 round"), T.case_named(T.REFIT[m], "special slots, 8 rounds")
    trimmed = [dict(s, rows=s["rows"][:T.REFIT_SPECIAL_N]) for s in T.refit_slots(eight)]       # without the decoy rows behind n
    slots, r1, r8 = dict(zip(T.REFIT_SPECIAL, trimmed)), dict(zip(T.REFIT_SPECIAL, T.refit_expected(one))), dict(zip(T.REFIT_SPECIAL, T.refit_expected(eight)))
    assert [r["rounds"] for r in r8.values()] == REFIT_ROUNDS_8[m]
    assert r8["plain"]["rounds"] >= 2 or r8["marked duplicates"]["rounds"] >= 2                 # nb_rounds = 8 on a slot that accepts at least two
    s = slots["mask bytes 2 and 0xff on true inliers"]
    assert sorted(set(s["start_mask"].tolist())) == [0, 1, 2, 0xFF]
    as_ones = T.NP_REFIT[m].refit(s["rows"], s["start"], np.minimum(s["start_mask"], 1), 1, one["thr"])
    got = r1["mask bytes 2 and 0xff on true inliers"]
    assert got["rounds"] == 1 and np.asarray(as_ones[key]).tobytes() != np.asarray(got[key]).tobytes()   # only a byte equal to 1 marks
    assert slots["start valid word 2"]["start"]["valid"] == 2 and r1["start valid word 2"]["valid"] == 1 and r1["start valid word 2"]["rounds"] == 1
    for what in ("NaN on a marked row", "inf on a marked row"):     # the round fails: the start record and the start mask byte for byte
        s, r = slots[what], r8[what]
        assert r["rounds"] == 0 and np.array_equal(r["mask"], s["start_mask"]) and not np.isfinite(s["rows"][s["start_mask"] == 1]).all()
        assert np.asarray(r[key]).tobytes() == np.asarray(s["start"][key]).tobytes()
    for what in ("NaN on an unmarked row", "inf on an unmarked row"):
        s, r = slots[what], r8[what]
        bad = np.flatnonzero(~np.isfinite(s["rows"]).all(axis=1))
        assert r["rounds"] == 8 and len(bad) == 1 and s["start_mask"][bad[0]] == 0 and r["mask"][bad[0]] == 0
    s = slots["marked duplicates"]
    on = s["rows"][s["start_mask"] == 1]
    assert len(np.unique(on, axis=0)) <= len(on) // 2 + 1 and r8["marked duplicates"]["rounds"] >= 1


# ====================================================================================================================== guided edges
def layout_cases(name):
    return [c for c in T.GUIDED if c["layout"] == name]


def same(a, b):
    return a.tobytes() == b.tobytes()


def test_guided_cases_reach_their_edges():
    assert len(T.GUIDED) == len(T.GUIDED_LAYOUTS) * 8 and {(c["kind"], c["cross_check"], c["thr"]) for c in T.GUIDED} == {(k, x, t) for k in "hf" for x in (0, 1) for t in (2.5, 1e6)}
    lay = T.case_named(T.GUIDED_LAYOUTS, "shared entries")
    tabs = [s["tab"] for s in lay["slots"]]
    assert sum(t[0] == 3 for t in tabs) >= 3 and (3, 0) in tabs and (0, 3) in tabs and (3, 3) in tabs and tabs != sorted(tabs) and lay["entries"][1] is None
    lay = T.case_named(T.GUIDED_LAYOUTS, "padded strides")
    assert (lay["tab_stride"], lay["n_stride"], lay["model_stride"], lay["valid_stride"]) == (3, 3, 12, 2) and min(lay["desc_extra"], lay["norm_extra"], lay["xy_extra"], lay["out_extra"]) > 0
    assert sorted(s["n_dev"] for s in lay["slots"]) == sorted(T.GUIDED_SIZES)
    for case in layout_cases("shared entries") + layout_cases("padded strides"):
        recs = T.guided_expected(case)
        assert sum(len(r) > 0 for r in recs) >= 2 and len(recs[-1 if case["layout"] == "shared entries" else 2]) == 0     # (0, 5): nothing
        if case["thr"] == 1e6 and not case["cross_check"]:
            assert any(len(r) == 257 for r in recs)       # every row of A has an admissible candidate: the queues fill and drain many times
    # clamp: three ways of writing (60, 60); the rows beyond are look-alikes that would change the records
    for case in layout_cases("clamp"):
        a, b, c = T.guided_expected(case)
        assert same(a, b) and same(a, c) and len(a) > 0 and case["max_n"] == 60
        s = case["slots"][0]
        wide = T.G.guided(T.KIND[case["kind"]], s["models"][case["kind"]], 1, s["xy"][0][:, 0], s["xy"][0][:, 1], case["entries"][0], s["xy"][1][:, 0], s["xy"][1][:, 1],
                          case["entries"][1], case["thr"], case["ratio"], case["max_distance"], case["cross_check"])
        assert not same(wide[wide["idx_a"] < 60], a)
    # degenerate models: nothing for all four under a homography; under a fundamental matrix nothing for three, and -F is the relation F
    for case in layout_cases("degenerate models"):
        recs = T.guided_expected(case)
        none = T.DEGENERATE_MODEL_SLOTS if case["kind"] == "h" else T.DEGENERATE_MODEL_SLOTS - 1
        assert all(len(r) == 0 for r in recs[:none]) and len(recs[6]) > 0
        assert case["kind"] == "h" or same(recs[3], recs[6])
        assert [s["valid"] for s in case["slots"][4:]] == [2, 0, 1] and same(recs[4], recs[6]) and len(recs[5]) == 0
    for case in layout_cases("NaN coordinates"):
        for s, r in zip(case["slots"], T.guided_expected(case)):
            bad_a, bad_b = np.flatnonzero(np.isnan(s["xy"][0]).any(axis=1)), np.flatnonzero(np.isnan(s["xy"][1]).any(axis=1))
            assert len(bad_a) and len(bad_b) and len(r) and not np.isin(r["idx_a"], bad_a).any() and not np.isin(r["idx_b"], bad_b).any()
