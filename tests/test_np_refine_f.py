"""The restatement of the fundamental-matrix refit (tests/np_refine_f.py) on its own, on the CPU: cases that can be checked by hand, the
reduction order, what fp32 costs against the float64 evaluation of the same estimator, the rank of the result, the monotone rule, and what the
refit is worth against the ground truth."""
import numpy as np
import pytest

import np_guided as G
import np_refine as R
import np_refine_f as RF
import np_verify_f as VF


def _start(F, n, count, valid=1):
    return dict(F=np.asarray(F, np.float32).reshape(3, 3), nb_matches=n, nb_inliers=count, best_hypothesis=0, best_root=0, valid=valid)


def _kept(r, s, m):
    """the chain kept the start record: its model, its count, its mask byte for byte"""
    return (r["valid"], r["rounds"], r["nb_inliers"]) == (1, 0, s["nb_inliers"]) and np.array_equal(r["mask"], m) and \
        np.asarray(r["F"], np.float32).tobytes() == np.asarray(s["F"], np.float32).tobytes()


# ---- (a) hand-checkable ------------------------------------------------------------------------------------------------------------------
# F is defined up to a factor and the published convention fixes only its power of two (largest |entry| in [1, 2)): the refit and the planted
# matrix are compared after the refit is brought to the planted matrix's largest entry (which also fixes the sign). Measured over the twelve
# cases below: the largest |entry difference| 5.06e-8 (entries up to 1.5: the rounding of fp32), the RMS Sampson distance of the exact
# correspondences under the refit at most 0.00936 px (at 16383 px; 0.0018 px at 4000 px, 0.00005 px at 640 px — the B side is the projection
# rounded to fp32, 2^-10 px at 16383 px). Four times those:
EXACT_ENTRY_BOUND = 2.1e-7
EXACT_SAMPSON_BOUND_PX = 0.038


def test_exact_correspondences_give_the_planted_matrix_back():
    worst_e, worst_s = 0.0, 0.0
    for w, h in ((640, 480), (4000, 3000), (16383, 12000)):
        for seed in range(4):
            c, _, Ft = VF.two_view_case(200, 0.0, 0.0, 30 + seed, w, h)
            Fu = np.float64(G.unit_f(Ft))
            off = Fu.copy()
            off[2] += 0.001                                     # the start model is deliberately off; the mask marks every match
            r = RF.refit(c, _start(off, 200, 200), np.ones(200, np.uint8), 3, 2.5)
            assert (r["valid"], r["nb_matches"], r["nb_inliers"], r["rounds"]) == (1, 200, 200, 3) and r["mask"].all()
            F = np.float64(r["F"]).reshape(9)
            assert r["F"].dtype == np.float32 and 1.0 <= np.abs(F).max() < 2.0
            k = int(np.argmax(np.abs(Fu)))
            e = float(np.abs(F * (Fu[k] / F[k]) - Fu).max())
            s = RF.rms_sampson(r["F"], c)
            print(f"{w} px seed {seed}: largest entry difference {e:.2e}, RMS Sampson distance of the exact correspondences {s:.2e} px")
            worst_e, worst_s = max(worst_e, e), max(worst_s, s)
            assert e < EXACT_ENTRY_BOUND and s < EXACT_SAMPSON_BOUND_PX, (w, seed, e, s)
    print(f"largest: entry difference {worst_e:.2e}, RMS Sampson {worst_s:.2e} px")


def _noisy_case(n=60, seed=3):
    c, true, Ft = VF.two_view_case(n, 0.5, 0.5, seed, 640, 480)
    return c, true, _start(G.unit_f(Ft), n, 7)


def test_seven_ones_keep_the_ransac_record():
    c, true, s = _noisy_case()
    m = np.zeros(len(c), np.uint8)
    m[np.flatnonzero(true)[:7]] = 1
    assert RF.fit(c, m == 1, s["F"]) is None
    assert _kept(RF.refit(c, s, m, 8, 2.5), s, m)
    m[np.flatnonzero(true)[7]] = 1                              # the eighth makes a round possible
    assert RF.fit(c, m == 1, s["F"]) is not None


def test_all_marked_matches_in_one_point_keep_the_ransac_record():
    c, true, s = _noisy_case()
    m = np.zeros(len(c), np.uint8)
    m[:10] = 1
    c[:10] = c[0]
    assert RF.fit(c, m == 1, s["F"]) is None                    # no conditioning scale
    assert _kept(RF.refit(c, dict(s, nb_inliers=10), m, 3, 2.5), dict(s, nb_inliers=10), m)
    # one side in one point is enough
    c2, _, _ = _noisy_case()
    c2[:10, 2:] = c2[0, 2:]
    assert RF.fit(c2, m == 1, s["F"]) is None


def test_a_nan_coordinate_on_a_marked_match_keeps_the_ransac_record():
    c, true, s = _noisy_case()
    m = true.astype(np.uint8)
    s = dict(s, nb_inliers=int(m.sum()))
    assert RF.refit(c, s, m, 3, 2.5)["rounds"] >= 1
    for col in range(4):
        bad = c.copy()
        bad[np.flatnonzero(true)[3], col] = np.nan
        assert RF.fit(bad, m == 1, s["F"]) is None, col
        assert _kept(RF.refit(bad, s, m, 3, 2.5), s, m), col
    bad = c.copy()
    bad[np.flatnonzero(~true)[0], 1] = np.nan                   # on a match the mask does not mark: no effect on the fit
    assert RF.fit(bad, m == 1, s["F"]).tobytes() == RF.fit(c, m == 1, s["F"]).tobytes()


def test_an_invalid_start_record_gives_the_zero_record():
    c, true, s = _noisy_case(30)
    for mask in (np.zeros(30, np.uint8), np.ones(30, np.uint8)):                                # whatever its mask holds
        r = RF.refit(c, _start(np.zeros((3, 3)), 30, 0, valid=0), mask, 3, 2.5)
        assert (r["valid"], r["nb_matches"], r["nb_inliers"], r["rounds"]) == (0, 0, 0, 0) and not r["F"].any() and not r["mask"].any() and len(r["mask"]) == 30
    s6 = VF.ransac(c[:6], 16, 2.5, 0)                           # what np_verify_f.ransac leaves for too few matches is such a record
    r = RF.refit(c[:6], s6, s6["mask"], 3, 2.5)
    assert r["valid"] == 0 and len(r["mask"]) == 6


def test_the_documented_reduction_order_is_the_one_implemented():
    """the 44 sums of a linear start against a literal transcription of the order (per-thread strided sums in increasing k, the butterfly, the
    waves in order); and the order matters: the same elements added in another order give other bits on this input"""
    c, true, _, _ = RF.noisy_and_clean(600, 0.5, 0.5, 41, 4000, 3000)
    inl = true
    ca, cb = R.condition(c[:, 0], c[:, 1], inl), R.condition(c[:, 2], c[:, 3], inl)
    x, y, X, Y = (c[:, 0] - ca[0]) * ca[2], (c[:, 1] - ca[1]) * ca[2], (c[:, 2] - cb[0]) * cb[2], (c[:, 3] - cb[1]) * cb[2]
    b = RF.monomials(x, y, X, Y, 8)
    terms = {}
    S = RF.accumulate(b, np.ones_like(x), inl, sum_fn=lambda v: (terms.setdefault("v", v.copy()), R.block_sum(v))[1])
    v = terms["v"]
    assert v.shape == (44, 600) and S.dtype == np.float32
    assert np.array_equal(v[0], np.where(inl, b[0] * b[0], 0)) and np.array_equal(v[8], np.where(inl, b[1] * b[1], 0)) and \
        np.array_equal(v[35], np.where(inl, b[7] * b[7], 0)) and np.array_equal(v[36], np.where(inl, b[0] * b[8], 0))       # i outermost, the right-hand side last
    for q in (0, 7, 20, 43):
        part = [np.float32(0)] * 256
        for k in range(600):
            part[k % 256] = np.float32(part[k % 256] + v[q, k])
        for off in (32, 16, 8, 4, 2, 1):
            part = [np.float32(part[t] + part[(t & ~63) | ((t & 63) ^ off)]) for t in range(256)]
        want = np.float32(np.float32(np.float32(part[0] + part[64]) + part[128]) + part[192])
        assert S[q].tobytes() == want.tobytes(), q
    # perturbed orders: a plain left-to-right sum, and the waves added as w0 + (w1 + (w2 + w3))
    serial = np.zeros(44, np.float32)
    for k in range(600):
        serial = serial + v[:, k]

    def waves_reversed(vals):
        p = np.zeros((vals.shape[0], 256), np.float32)
        for k in range(vals.shape[1]):
            p[:, k % 256] = p[:, k % 256] + vals[:, k]
        p = p.reshape(-1, 4, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            p = p + p[:, :, lane ^ off]
        w = p[:, :, 0]
        return w[:, 0] + (w[:, 1] + (w[:, 2] + w[:, 3]))

    assert serial.tobytes() != S.tobytes() and waves_reversed(v).tobytes() != S.tobytes()
    s = _start(np.eye(3), 600, 0)
    o = RF.fit(c, inl, s["F"])
    assert o is not None and RF.fit(c, inl, s["F"], sum_fn=waves_reversed).tobytes() != o.tobytes()       # and reaches the published model


def test_the_rescoring_is_guided_matchings_admissibility():
    c, true, Ft, _ = RF.noisy_and_clean(300, 0.5, 0.5, 8, 4000, 3000)
    o = G.unit_f(Ft)
    for thr in (0.5, 2.5):
        adm = G.admissible(G.FUNDAMENTAL, o, c[:, 0], c[:, 1], c[:, 2], c[:, 3], G.threshold2(thr))
        assert np.array_equal(RF.score(o, c, thr), np.diagonal(adm)) and 30 < RF.score(o, c, thr).sum() <= 200
    # and for a refined model: the refined mask is that admissibility
    s = VF.ransac(c, 64, 2.5, 3)
    r = RF.refit(c, s, s["mask"], 3, 2.5)
    assert r["rounds"] >= 1
    adm = G.admissible(G.FUNDAMENTAL, r["F"], c[:, 0], c[:, 1], c[:, 2], c[:, 3], G.threshold2(2.5))
    assert np.array_equal(np.diagonal(adm), r["mask"] == 1)


# ---- (b), (c): the cases of the kernel-level GPU test ---------------------------------------------------------------------------------------
def _cases():
    for thr in RF.SLOT_THRESHOLDS:
        for i, (c, s, m, wh, clean) in enumerate(RF.kernel_test_slots(thr)):
            yield thr, i, c, s, m, wh, clean


N_CASES = len(RF.SLOT_THRESHOLDS) * (len(RF.SLOT_N) + len(RF.SPECIAL))


def test_the_slots_are_what_they_are_meant_to_be():
    k0 = len(RF.SLOT_N)
    for thr in RF.SLOT_THRESHOLDS:
        slots = RF.kernel_test_slots(thr)
        assert [len(t[0]) for t in slots] == RF.SLOT_N + [RF.SPECIAL_N] * len(RF.SPECIAL)
        assert [t[1]["valid"] for t in slots[:k0]] == [1 if n >= 8 else 0 for n in RF.SLOT_N]
        assert slots[RF.BIG_SLOT][3][0] == 16383 and (slots[RF.BIG_SLOT][0] == 16383.0).sum() == 2
        assert {t[3][0] for t in slots} == {640, 4000, 16383}
        assert [int(t[2].sum()) for t in slots[k0:k0 + 3]] == [RF.SPECIAL_N, 8, 7] and slots[k0 + 3][1]["valid"] == 0 and slots[k0 + 3][2].any()
        for c, s, m, _, _ in slots[:k0]:
            assert int(m.sum()) == s["nb_inliers"]               # the start records are consistent with their masks


def test_the_monotone_rule_holds_on_every_case():
    checked = 0
    for thr, i, c, s, m, _, _ in _cases():
        prev = None
        for nr in RF.SLOT_ROUNDS:
            r = RF.refit(c, s, m, nr, thr)
            assert r["nb_inliers"] >= s["nb_inliers"] * s["valid"], (thr, i, nr)
            assert r["valid"] == s["valid"] and r["rounds"] <= nr
            assert set(np.unique(r["mask"])) <= {0, 1}
            if r["rounds"]:
                assert int(r["mask"].sum()) == r["nb_inliers"]                                  # after any accepted round
                assert np.array_equal(r["mask"] == 1, RF.score(r["F"], c, thr))
            elif s["valid"]:
                assert _kept(r, s, m), (thr, i, nr)
            if prev is not None:               # more rounds continue the same chain: never fewer inliers
                assert r["nb_inliers"] >= prev["nb_inliers"] and r["rounds"] >= prev["rounds"]
            prev = r
            checked += 1
    assert checked == N_CASES * len(RF.SLOT_ROUNDS)


# |det Fc| / |Fc|_F^3 of the conditioned model after the two projection steps, float64 evaluation of the fp32 entries: the largest value over the
# fits of the cases below (start and final mask of every slot, both thresholds) was 2.8e-10 — the products of the determinant are rounded at 6e-8
# of |F|^3, and the value is that small because the least-squares solution of a two-view scene is close to rank 2 before the projection
# (DESIGN.md section 10.3). Four times that:
DET_BOUND = 1.1e-9
# The largest |RMS Sampson distance under the fp32 fit - under the float64 fit| over the slot's noise-free true correspondences, both fitted from
# the SAME marked matches, over the cases below with nine marked matches or more and a mask from a verification or an accepted round:
# 0.0247 px at 16383 px, 0.0066 px at 4000 px, 0.0010 px at 640 px. Four times that:
FP32_COST_BOUND_PX = 0.099
# Not under that bound, documented and asserted on their own:
#   exactly eight marked matches (slot n = 8, and the start mask of "exactly eight ones"): eight equations in eight unknowns, nothing is averaged,
#   and the normal equations square the condition of an interpolation problem: 0.108 px (0.1082 against 0.0001 px: exact data at 640 px, where
#   the accepted fp32 round is worse than the seven-point model it started from, 0.0003 px, with the same eight inliers) and 2.03 px (12.52
#   against 10.49 px: noisy data at 4000 px, neither model is a usable one). Asserted: these are the only such masks, both arithmetics give a
#   model, and one match more is under the bound again (the slot n = 9: 0.0005 px; the later rounds of "exactly eight ones": 0.0066 px).
#   "all ones over half outliers": the mask marks 150 uniformly random matches, no fundamental matrix explains the marked set, both fits are
#   440 px from the true correspondences and 0.73 px from each other. Asserted: both chains reject the round.


def test_what_fp32_costs_against_float64_and_the_rank_of_the_result():
    worst, det_worst, seen, eights, rejected = {}, 0.0, 0, 0, 0
    marks_outliers, exactly_eight = (len(RF.SLOT_N) + RF.SPECIAL.index(name) for name in ("all ones over half outliers", "exactly eight ones"))
    for thr, i, c, s, m, (w, h), clean in _cases():
        if not s["valid"]:
            continue
        r = RF.refit(c, s, m, 3, thr)
        r64 = RF.refit_f64(c, s, m, 3, thr)
        print(f"thr {thr} slot {i} n {len(c)} ({w} px): inliers RANSAC {s['nb_inliers']}, fp32 chain {r['nb_inliers']} ({r['rounds']} rounds), float64 chain "
              f"{r64['nb_inliers']} ({r64['rounds']} rounds); RMS Sampson of the true correspondences {RF.rms_sampson(s['F'], clean):.4f} -> {RF.rms_sampson(r['F'], clean):.4f} px")
        for which, mask, model in (("start", m, s["F"]), ("final", r["mask"], r["F"])):
            inl = np.asarray(mask) == 1
            if inl.sum() < RF.MIN_MATCHES:
                assert RF.fit(c, inl, model) is None and RF.fit_f64(c, inl, model) is None
                continue
            detail = {}
            o32, o64 = RF.fit(c, inl, model, detail=detail), RF.fit_f64(c, inl, model)
            assert o32 is not None and o64 is not None, (thr, i, which)
            fc = np.float64(detail["fc"]).reshape(3, 3)
            det = abs(np.linalg.det(fc)) / np.linalg.norm(fc) ** 3
            det_worst = max(det_worst, det)
            assert det < DET_BOUND, (thr, i, which, det)
            e32, e64 = RF.rms_sampson(o32, clean), RF.rms_sampson(o64, clean)
            d = abs(e32 - e64)
            if i == marks_outliers:
                print(f"    {which} mask marks outliers: fp32 {e32:.4f} px, float64 {e64:.4f} px")
                assert _kept(r, s, m) and _kept(r64, s, m), (thr, i)
                rejected += 1
            elif inl.sum() == RF.MIN_MATCHES:
                print(f"    {which} mask marks exactly eight: fp32 {e32:.4f} px, float64 {e64:.4f} px")
                assert (i, which) in ((RF.SLOT_N.index(8), "start"), (RF.SLOT_N.index(8), "final"), (exactly_eight, "start")), (thr, i, which)
                eights += 1
            else:
                print(f"    {which} mask ({int(inl.sum())} marked): fp32 {e32:.5f} px, float64 {e64:.5f} px, |difference| {d:.5f} px, |det| / |F|^3 {det:.1e}")
                worst[w] = max(worst.get(w, 0.0), d)
                seen += 1
                assert d < FP32_COST_BOUND_PX, (thr, i, which, d)
    print("largest |fp32 - float64| RMS Sampson distance by image width:", {k: round(v, 5) for k, v in sorted(worst.items())}, "largest |det| / |F|^3", det_worst)
    assert seen >= 40 and set(worst) == {640, 4000, 16383} and eights == 3 * len(RF.SLOT_THRESHOLDS) and rejected >= 2


# ---- (d) what it is worth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(640, 480), (4000, 3000), (16383, 12000)])
def test_the_refit_is_nearer_the_ground_truth_than_the_ransac_model(size):
    """50 % outliers, 0.5 px noise, threshold 2.5 px, 3 rounds, after 16 and after 256 hypotheses (seed 5, RANSAC seed 1234): wherever the
    verification found 100 inliers or more, the RMS Sampson distance of the noise-free true correspondences under the refined model is below
    the one under the RANSAC model (figures in DESIGN.md section 10.3)."""
    w, h = size
    asserted = 0
    for n in (400, 4097):
        c, true, _, clean = RF.noisy_and_clean(n, 0.5, 0.5, 5, w, h)
        hyps = VF.hypotheses(c, 256, 1234, 0)
        for nh in (16, 256):
            s = VF.ransac(c, nh, 2.5, 1234, hyps=hyps)
            r = RF.refit(c, s, s["mask"], 3, 2.5)
            assert r["nb_inliers"] >= s["nb_inliers"]
            if not s["valid"]:
                print(f"{w} px n {n} hypotheses {nh}: no valid model")
                continue
            e0, e1 = RF.rms_sampson(s["F"], clean[true]), RF.rms_sampson(r["F"], clean[true])
            few = s["nb_inliers"] < 100
            sv = np.linalg.svd(np.float64(r["F"]), compute_uv=False)
            print(f"{w} px n {n} hypotheses {nh}: inliers {s['nb_inliers']} -> {r['nb_inliers']} ({r['rounds']} rounds), RMS Sampson {e0:.3f} -> {e1:.4f} px, "
                  f"sigma3 / sigma1 {sv[2] / sv[0]:.1e}" + (" (not asserted)" if few else ""))
            if not few:
                assert e1 < e0, (w, n, nh, e0, e1)
                asserted += 1
    assert asserted == 4
