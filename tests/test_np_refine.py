"""The restatement of the homography refit (tests/np_refine.py) on its own, on the CPU: cases that can be checked by hand, what fp32 costs against
the float64 evaluation of the same algorithm, the monotone rule, and what the refit is worth against the ground truth."""
import numpy as np
import pytest

import np_guided as G
import np_refine as R
import np_verify as V
import quality as Q


def _start(H, n, count, valid=1):
    return dict(H=np.asarray(H, np.float32).reshape(3, 3), nb_matches=n, nb_inliers=count, best_hypothesis=0, valid=valid)


def _exact(Ht, w, h, n, seed):
    c, _ = V.synthetic_case(Ht, w, h, n=n, outliers=0.0, noise=0.0, seed=seed)
    return c


def _transfer(o, c):
    px, py = Q.project(np.asarray(o, np.float64).reshape(3, 3), c[:, 0].astype(np.float64), c[:, 1].astype(np.float64))
    return np.hypot(px - c[:, 2], py - c[:, 3])


# ---- (a) hand-checkable ------------------------------------------------------------------------------------------------------------------
def test_exact_correspondences_give_the_planted_homography_back():
    """The B side is the planted map of the A side rounded to fp32 (2^-15 px at 640 px), so the planted model has residuals of that size; the
    fit starts from a RANSAC record that is deliberately off (a translation of 1 px) and from the mask of all matches. fp32 normal equations of
    condition <= 1e2 lose two of seven digits: 1e-5 of a 640 px image, 0.0064 px; asserted at 0.01 px."""
    w, h = 640, 480
    for i, kw in enumerate(Q.WARPS):
        Ht = Q.homography(w, h, **kw)
        c = _exact(Ht, w, h, 200, 5 + i)
        off = Ht / Ht[2, 2] + np.array([[0, 0, 1.0], [0, 0, -1.0], [0, 0, 0]])
        r = R.refit(c, _start(off, 200, 200), np.ones(200, np.uint8), 3, 2.5)
        assert (r["valid"], r["nb_matches"], r["nb_inliers"], r["rounds"]) == (1, 200, 200, 3) and r["mask"].all()
        assert r["H"].dtype == np.float32 and r["H"][2, 2] == 1.0
        e = V.corner_error(r["H"], Ht, w, h)
        print(f"warp {i}: corner error of the refit on exact data {e:.2e} px")
        assert e < 0.01, (i, e)


def test_four_inliers_are_fitted_exactly():
    w, h = 640, 480
    Ht = Q.homography(w, h, **Q.WARPS[2])
    c = _exact(Ht, w, h, 4, 11)
    r = R.refit(c, _start(Ht / Ht[2, 2], 4, 4), np.ones(4, np.uint8), 1, 0.5)
    assert (r["valid"], r["nb_inliers"], r["rounds"]) == (1, 4, 1)
    assert _transfer(r["H"], c).max() < 0.01          # eight equations, eight unknowns: the residual is rounding (as above)
    # and among other matches: the four marked ones decide the model
    c2, _ = V.synthetic_case(Ht, w, h, n=50, outliers=0.5, noise=0.0, seed=12)
    c2[:4] = c
    m = np.zeros(50, np.uint8)
    m[:4] = 1
    r2 = R.refit(c2, _start(Ht / Ht[2, 2], 50, 4), m, 1, 0.5)
    assert r2["rounds"] == 1 and r2["H"].tobytes() == r["H"].tobytes() and r2["mask"][:4].all() and r2["nb_inliers"] >= 4


def test_four_collinear_inliers_fail_the_round_and_keep_the_ransac_model():
    H0 = np.array([[1.5, 0.25, 3.0], [-0.125, 2.0, 7.0], [0, 0, 1.0]])
    c = np.array([[100.0 + 50.0 * q, 200.0 + 25.0 * q, 0, 0] for q in range(4)] + [[17.0, 400.0, 0, 0], [300.0, 31.0, 0, 0]], np.float32)
    c[:, 2], c[:, 3] = Q.project(H0, c[:, 0].astype(np.float64), c[:, 1].astype(np.float64))
    mask = np.array([1, 1, 1, 1, 0, 0], np.uint8)
    assert R.fit(c, mask == 1) is None                 # the normal equations of collinear points are singular: a zero pivot
    r = R.refit(c, _start(H0, 6, 4), mask, 8, 2.5)
    assert (r["valid"], r["nb_inliers"], r["rounds"]) == (1, 4, 0)
    assert r["H"].tobytes() == H0.astype(np.float32).tobytes() and np.array_equal(r["mask"], mask)
    # all inliers in one point: no conditioning scale
    same = np.repeat(c[:1], 5, axis=0)
    assert R.fit(same, np.ones(5, bool)) is None
    # fewer than four ones
    assert R.fit(c, np.array([1, 1, 1, 0, 0, 0], bool)) is None


def test_an_all_zero_mask_and_an_invalid_start_record_give_the_zero_record():
    w, h = 640, 480
    Ht = Q.homography(w, h, **Q.WARPS[0])
    c, _ = V.synthetic_case(Ht, w, h, n=30, seed=2)
    r = R.refit(c, _start(np.zeros((3, 3)), 30, 0, valid=0), np.zeros(30, np.uint8), 3, 2.5)
    assert (r["valid"], r["nb_matches"], r["nb_inliers"], r["rounds"]) == (0, 0, 0, 0) and not r["H"].any() and not r["mask"].any() and len(r["mask"]) == 30
    r = R.refit(c, _start(np.zeros((3, 3)), 30, 0, valid=0), np.ones(30, np.uint8), 3, 2.5)        # whatever its mask holds
    assert r["valid"] == 0 and not r["mask"].any()
    # what np_verify.ransac leaves for too few matches is such a record
    s = V.ransac(c[:3], 16, 2.5, 0)
    r = R.refit(c[:3], s, s["mask"], 3, 2.5)
    assert r["valid"] == 0 and len(r["mask"]) == 3
    # a valid record with an all-zero mask: no round can start, the record stays
    r = R.refit(c, _start(Ht / Ht[2, 2], 30, 7), np.zeros(30, np.uint8), 3, 2.5)
    assert (r["valid"], r["nb_inliers"], r["rounds"]) == (1, 7, 0)


def test_the_reduction_order_is_the_documented_one():
    """block_sum against a literal transcription of the order: per-thread strided sums, the butterfly, the waves in order"""
    rng = np.random.default_rng(3)
    for n in (0, 1, 255, 256, 257, 1000):
        v = (rng.standard_normal(n) * 1000).astype(np.float32)
        part = [np.float32(0)] * 256
        for k in range(n):
            part[k % 256] = np.float32(part[k % 256] + v[k])
        for off in (32, 16, 8, 4, 2, 1):
            part = [np.float32(part[t] + part[(t & ~63) | ((t & 63) ^ off)]) for t in range(256)]
        want = np.float32(np.float32(np.float32(part[0] + part[64]) + part[128]) + part[192])
        assert R.block_sum(v[None, :])[0].tobytes() == want.tobytes(), n
    assert len(set(np.float32(x).tobytes() for x in part[:64])) == 1          # every lane of a wave holds the same bits


def test_the_rescoring_is_guided_matchings_admissibility():
    w, h = 4000, 3000
    Ht = Q.homography(w, h, **Q.WARPS[1])
    c, _ = V.synthetic_case(Ht, w, h, n=300, seed=8)
    o = (Ht / Ht[2, 2]).astype(np.float32).reshape(9)
    for thr in (0.5, 2.5):
        adm = G.admissible(G.HOMOGRAPHY, o, c[:, 0], c[:, 1], c[:, 2], c[:, 3], G.threshold2(thr))
        assert np.array_equal(R.score(o, c, thr), np.diagonal(adm)) and 30 < R.score(o, c, thr).sum() <= 150


# ---- (b), (c): the cases of the kernel-level GPU test ---------------------------------------------------------------------------------------
def _cases():
    for thr in R.SLOT_THRESHOLDS:
        for i, (c, s, m, wh) in enumerate(R.kernel_test_slots(thr)):
            yield thr, i, c, s, m, wh


def test_the_monotone_rule_holds_on_every_case():
    checked = 0
    for thr, i, c, s, m, _ in _cases():
        prev = None
        for nr in R.SLOT_ROUNDS:
            r = R.refit(c, s, m, nr, thr)
            assert r["nb_inliers"] >= s["nb_inliers"] * s["valid"], (thr, i, nr)
            assert r["valid"] == s["valid"] and r["rounds"] <= nr
            assert set(np.unique(r["mask"])) <= {0, 1}
            if r["rounds"]:
                assert int(r["mask"].sum()) == r["nb_inliers"]
            if prev is not None:               # more rounds continue the same chain: never fewer inliers
                assert r["nb_inliers"] >= prev["nb_inliers"] and r["rounds"] >= prev["rounds"]
            prev = r
            checked += 1
    assert checked == len(R.SLOT_THRESHOLDS) * len(R.SLOT_ROUNDS) * (len(R.SLOT_N) + len(R.SPECIAL))


# The largest four-corner distance between the fp32 and the float64 fit from the same inliers, over the cases below in which the fitted model keeps
# every marked match in front of the plane (d > 0, in both arithmetics), was 0.149 px (148 noise-free inliers of 300 matches in a 16383 x 12000
# image; 0.054 px with noise there, 0.026 px at 4000 px, 0.0003 px at 640 px); recorded in DESIGN.md section 10.2. Four times that:
FP32_COST_BOUND_PX = 0.6
# Not under that bound: the slot "all ones over half outliers". Its mask marks 150 uniformly random matches, so no homography explains the marked
# set, the precondition of the estimator (d > 0 on every marked match, DESIGN.md "h8 != 0") does not hold, and in the fitted model d changes sign
# inside the marked set: 1 / d in the Gauss-Newton rows has a pole there and the two arithmetics part completely (4071.2 px at the corners; the linear
# start alone differs by 6.3 px). What is asserted for it instead: that d does change sign, and that both chains reject the round.


def _in_front(o, c, inl):
    """d > 0 on every marked match under the published model o (float64 evaluation)"""
    o = np.asarray(o, np.float64).reshape(9)
    d = o[6] * c[inl, 0].astype(np.float64) + o[7] * c[inl, 1].astype(np.float64) + o[8]
    return bool((d > 0).all())


def test_what_fp32_costs_against_float64():
    """fp32 and float64 fits from the SAME inliers (the start mask of every case, and the mask the fp32 chain ends with), with 8 or more of them:
    the distance of the images of the four corners, asserted wherever both fitted models keep every marked match in front of the plane. From the
    same mask the two differ by arithmetic only; whole chains may part ways at a match that lies on the threshold, which says nothing about the
    arithmetic (their final counts are printed). Where d changes sign inside the marked set the fit has a pole and no bound holds: that may
    happen only in the slot whose mask marks outliers, and there both chains must reject the round."""
    worst, seen, poles = {}, 0, 0
    marks_outliers = len(R.SLOT_N) + R.SPECIAL.index("all ones over half outliers")
    for thr, i, c, s, m, (w, h) in _cases():
        if not s["valid"]:
            continue
        r = R.refit(c, s, m, 3, thr)
        r64 = R.refit_f64(c, s, m, 3, thr)
        for which, mask in (("start", m), ("final", r["mask"])):
            inl = np.asarray(mask) == 1
            if inl.sum() < 8:
                continue
            o32, o64 = R.fit(c, inl), R.fit_f64(c, inl)
            assert (o32 is None) == (o64 is None), (thr, i)
            if o32 is None:
                continue
            d = V.corner_error(o32.reshape(3, 3), o64.reshape(3, 3), w, h)
            if not (_in_front(o32, c, inl) and _in_front(o64, c, inl)):
                print(f"thr {thr} slot {i} ({which} mask): d changes sign inside the marked set, fp32 - float64 corner distance {d:.1f} px")
                assert i == marks_outliers, (thr, i, which)
                assert not _in_front(o32, c, inl) and not _in_front(o64, c, inl), (thr, i)
                for chain in (r, r64):         # the round is rejected in either arithmetic: the RANSAC model, count and mask stay
                    assert (chain["rounds"], chain["nb_inliers"]) == (0, s["nb_inliers"]) and np.array_equal(chain["mask"], m), (thr, i)
                    assert np.asarray(chain["H"], np.float32).tobytes() == np.asarray(s["H"], np.float32).tobytes()
                poles += 1
                continue
            worst[w] = max(worst.get(w, 0.0), d)
            seen += 1
            assert d < FP32_COST_BOUND_PX, (thr, i, len(c), d)
        print(f"thr {thr} slot {i} n {len(c)} ({w} px): inliers RANSAC {s['nb_inliers']}, fp32 chain {r['nb_inliers']} ({r['rounds']} rounds), float64 chain "
              f"{r64['nb_inliers']} ({r64['rounds']} rounds)")
    print("largest fp32 - float64 corner distance by image width:", {k: round(v, 5) for k, v in sorted(worst.items())})
    assert seen >= 30 and set(worst) == {640, 4000, 16383} and poles >= len(R.SLOT_THRESHOLDS)


# ---- (d) what it is worth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(640, 480), (4000, 3000), (16383, 12000)])
def test_the_refit_is_nearer_the_ground_truth_than_the_ransac_model(size):
    """50 % outliers, 0.5 px noise, threshold 2.5, 3 rounds, after 16 and after 256 hypotheses: wherever the verification found about 100
    inliers or more, the refined model's four-corner error against the planted homography is below the RANSAC model's. With fewer a least-squares
    fit on a dozen noisy points may extrapolate worse than a lucky sample: printed only."""
    w, h = size
    asserted = 0
    for i, kw in enumerate(Q.WARPS):
        Ht = Q.homography(w, h, **kw)
        for n in (400, 4097):
            c, _ = V.synthetic_case(Ht, w, h, n=n, outliers=0.5, noise=0.5, seed=20 + i)
            hyps = V.hypotheses(c, 256, 5, i)
            for nh in (16, 256):
                s = V.ransac(c, nh, 2.5, 5, slot=i, hyps=hyps)
                r = R.refit(c, s, s["mask"], 3, 2.5)
                assert r["nb_inliers"] >= s["nb_inliers"]
                if not s["valid"]:
                    print(f"{w} px warp {i} n {n} hypotheses {nh}: no valid model")
                    continue
                e0, e1 = V.corner_error(s["H"], Ht, w, h), V.corner_error(r["H"], Ht, w, h)
                few = s["nb_inliers"] < 100
                print(f"{w} px warp {i} n {n} hypotheses {nh}: inliers {s['nb_inliers']} -> {r['nb_inliers']} ({r['rounds']} rounds), corner error {e0:.3f} -> {e1:.3f} px"
                      + (" (not asserted)" if few else ""))
                if not few:
                    assert e1 < e0, (w, i, n, nh, e0, e1)
                    asserted += 1
    assert asserted >= 10
