"""The restatement of the RANSAC fundamental-matrix estimator (tests/np_verify_f.py) pinned on the CPU, so that the GPU kernels of verify.hip
are not compared against an unpinned model: the sampler, the seven-point solve, the Sampson test, the cubic root finder against numpy.roots,
and what fp32 costs against a float64 evaluation of the same samples on the inputs of the GPU test."""
import numpy as np
import pytest

import np_verify as V
import np_verify_f as VF


def test_four_draws_reproduce_the_homography_sampler():
    for seed in (0, 1, 0xDEADBEEFCAFE):
        for slot in (0, 5, 511):
            for hyp in list(range(20)) + [255, 256, 65535]:
                for n in (4, 5, 7, 64, 1000, 65535):
                    assert VF.sample_k(seed, slot, hyp, n, 4) == V.sample(seed, slot, hyp, n)


@pytest.mark.parametrize("n", [7, 8, 1000])
def test_seven_distinct_indices(n):
    for seed in (0, 0x5EED0000C0FFEE):
        for slot in (0, 10):
            for hyp in list(range(60)) + [65535]:
                s = VF.sample_k(seed, slot, hyp, n, 7)
                assert len(set(s)) == 7 and min(s) >= 0 and max(s) < n, (seed, slot, hyp, n, s)
                assert s[:4] == V.sample(seed, slot, hyp, n)          # the first four draws are the homography's
    if n == 7:
        assert sorted(VF.sample_k(0, 0, 0, 7, 7)) == list(range(7))


def _scaled_to_pixels(F):
    K = np.diag([1.0 / 8192.0, 1.0 / 8192.0, 1.0])
    return K @ np.asarray(F, np.float64).reshape(3, 3) @ K


@pytest.mark.parametrize("size", [(640, 480), (4000, 3000), (16383, 12000)])
def test_solve_on_noise_free_samples(size):
    """every returned root satisfies the seven epipolar constraints to fp32 accuracy and one of them is the true F up to scale. The bounds:
    the residual of a constraint is a sum of nine products of magnitude <= |F| |xb| |xa| <= 2 * 2^2 (conditioned coordinates lie in
    [-2, 2)), each carrying the relative error of an fp32 Gauss-Jordan elimination of a 7x9 system; 2^-24 times a growth of a few
    thousand, i.e. 1e-3 against an algebraic scale of 1 (measured: below 2e-5). Distance to the true F: entries within 2e-2 after
    normalising both to unit Frobenius norm (the seven-point problem's conditioning amplifies the 2^-24 input rounding; measured: 7e-5)."""
    w, h = size
    c, _, Ft = VF.two_view_case(7 * 40, 0.0, 0.0, 5, w, h)
    c = c.reshape(40, 7, 4)
    models, cnt = VF.solve(c)
    assert models.dtype == np.float32 and ((cnt >= 1) & (cnt <= 3)).all()
    worst_res, worst_dist = 0.0, 0.0
    Ftn = Ft / np.linalg.norm(Ft)
    for k in range(40):
        best = np.inf
        for r in range(3):
            if r >= cnt[k]:
                assert np.isnan(models[k, r]).all()
                continue
            m = models[k, r]
            assert 1.0 <= np.abs(m).max() < 2.0
            F = _scaled_to_pixels(m)
            F /= np.linalg.norm(F)
            # residuals in Hartley-normalised coordinates (so that "small" has a scale): x^b^T F^ x^a with F^ = Tb^-T F Ta^-1
            Ta, Tb = VF._hartley(c[k, :, 0].astype(np.float64), c[k, :, 1].astype(np.float64)), VF._hartley(c[k, :, 2].astype(np.float64), c[k, :, 3].astype(np.float64))
            Fh = np.linalg.inv(Tb).T @ F @ np.linalg.inv(Ta)
            Fh /= np.linalg.norm(Fh)
            pa = Ta @ np.stack([c[k, :, 0], c[k, :, 1], np.ones(7)]).astype(np.float64)
            pb = Tb @ np.stack([c[k, :, 2], c[k, :, 3], np.ones(7)]).astype(np.float64)
            worst_res = max(worst_res, float(np.abs((pb * (Fh @ pa)).sum(axis=0)).max()))
            best = min(best, np.abs(F - Ftn).max(), np.abs(F + Ftn).max())
        worst_dist = max(worst_dist, best)
    print(f"{w}x{h}: largest epipolar residual {worst_res:.3g}, largest distance of the nearest root to the true F {worst_dist:.3g}")
    assert worst_res < 1e-3 and worst_dist < 2e-2


def test_sampson_test_agrees_with_float64_away_from_the_threshold():
    c, true, Ft = VF.two_view_case(1000, 0.5, 0.5, 3, 640, 480)
    idx = VF.samples(1, 0, 64, len(c))
    models, cnt = VF.solve(c[idx])
    checked = 0
    for thr in (0.5, 2.5):
        got = VF.inliers(models.reshape(-1, 9), c, VF.threshold2(thr)).reshape(64, 3, -1)
        for k in range(64):
            for r in range(int(cnt[k])):
                F = _scaled_to_pixels(models[k, r])
                pa = np.stack([c[:, 0], c[:, 1], np.ones(len(c))]).astype(np.float64)
                pb = np.stack([c[:, 2], c[:, 3], np.ones(len(c))]).astype(np.float64)
                l, m = F @ pa, F.T @ pb
                d = np.abs((pb * l).sum(axis=0)) / np.sqrt(l[0] ** 2 + l[1] ** 2 + m[0] ** 2 + m[1] ** 2)
                clear = np.abs(d - thr) > 1e-3 * thr                    # fp32 evaluation of a distance of the order of a pixel: relative 1e-3 is generous
                assert np.array_equal(got[k, r][clear], (d < thr)[clear])
                checked += int(clear.sum())
            assert not got[k, int(cnt[k]):].any()                       # absent roots are all-NaN: no inliers
    assert checked > 2 * 64 * 900


def _roots32(coef):
    r, n = VF.cubic_roots(*(np.array([x], np.float32) for x in coef))
    return [float(x) for x in r[0, :n[0]]], int(n[0])


def test_cubic_root_finder_against_numpy_roots():
    rng = np.random.default_rng(9)
    seen = {1: 0, 3: 0}
    for _ in range(300):
        coef = rng.normal(0, 1, 4) * 10.0 ** rng.integers(-3, 4, 4)   # c0..c3
        coef32 = coef.astype(np.float32)
        want = np.roots(coef32[::-1].astype(np.float64))
        real = sorted(x.real for x in want if abs(x.imag) < 1e-12)
        # only clearly separated, well-conditioned root sets are compared one to one
        others = [x for x in want if abs(x.imag) >= 1e-12]
        if any(abs(x.imag) < 1e-2 * (1 + abs(x)) for x in others) or any(abs(a - b) < 1e-2 * (1 + abs(a)) for a, b in zip(real, real[1:])):
            continue
        got, n = _roots32(coef32)
        assert n == len(real), (coef32, got, real)
        for g, r in zip(got, real):
            assert abs(g - r) <= 1e-4 * (1 + abs(r)) * (1 + 1e-3 * max(abs(x) for x in want)), (coef32, got, real)
        seen[n] += 1
    assert seen[1] > 30 and seen[3] > 30
    # three known roots; one root with a complex pair
    got, n = _roots32([-6.0, 11.0, -6.0, 1.0])
    assert n == 3 and np.allclose(got, [1, 2, 3], atol=1e-5)
    got, n = _roots32([1.0, 1.0, 1.0, 1.0])                             # (a + 1)(a^2 + 1)
    assert n == 1 and abs(got[0] + 1.0) < 1e-6
    # two coincident roots: (a - 1)^2 (a + 2) = a^3 - 3a + 2. The single root is found; the double root touches zero without a reliable change
    # of sign, so it is reported as a pair around 1 or not at all, never as something else
    got, n = _roots32([2.0, -3.0, 0.0, 1.0])
    assert n in (1, 3) and abs(got[0] + 2.0) < 1e-6 and all(abs(g - 1.0) < 1e-3 for g in got[1:])
    # a vanishing leading coefficient: the sample is declared degenerate (no root), as is anything not finite
    for coef in ([1.0, 2.0, 3.0, 0.0], [1.0, 2.0, 3.0, 1e-40], [1.0, 2.0, 3.0, np.inf], [np.nan, 2.0, 3.0, 1.0], [3e38, 2.0, 3.0, 1e-30]):
        got, n = _roots32(coef)
        assert n == 0 and got == []
    # the result is ordered and NaN beyond the count
    r, n = VF.cubic_roots(*(np.array([x], np.float32) for x in [-6.0, 11.0, -6.0, 1.0]))
    assert list(r[0]) == sorted(r[0])
    r, n = VF.cubic_roots(*(np.array([x], np.float32) for x in [1.0, 1.0, 1.0, 1.0]))
    assert n[0] == 1 and np.isnan(r[0, 1:]).all()


def test_degenerate_inputs_give_no_model():
    c, _, _ = VF.two_view_case(7, 0.0, 0.0, 1, 640, 480)
    for bad in (np.zeros((7, 4), np.float32), np.tile(c[:1], (7, 1))):   # seven equal points: no deviation to scale
        models, cnt = VF.solve(bad[None])
        assert cnt[0] == 0 and np.isnan(models).all()
    nan = c.copy()
    nan[3, 2] = np.nan
    models, cnt = VF.solve(nan[None])
    assert cnt[0] == 0 and np.isnan(models).all()
    for n in (0, 6):
        res = VF.ransac(c[:n], 64, 2.5, 0)
        assert res["valid"] == 0 and res["nb_matches"] == n and not res["F"].any() and len(res["mask"]) == n
    res = VF.ransac(c, 64, 2.5, 0)                                        # exactly the sample: 7 inliers at most, 8 are needed
    assert res["valid"] == 0 and res["nb_inliers"] == 0


def test_what_fp32_costs():
    """true inliers inside the fp32 winner's mask against those inside the float64 evaluation's (same samples, SVD null space,
    numpy.roots) on the GPU test's inputs: n = 257 and 1000, 50 % outliers, 1024 hypotheses, 2.5 px, both seeds. Measured 2026-10-17:
        n = 257,  seed 0:                fp32 129 of 129 planted (129 in the mask), float64 129 (129)
        n = 257,  seed 0x5EED0000C0FFEE: fp32 129 (129),                            float64 129 (129)
        n = 1000, seed 0:                fp32 464 of 500 planted (479),             float64 464 (479)
        n = 1000, seed 0x5EED0000C0FFEE: fp32 500 (513),                            float64 500 (513)
    Largest shortfall: 0 (np_verify_f.FP32_MAX_SHORTFALL; the GPU test allows twice that). The fixed free columns with row pivoting lose
    nothing here, so there is no column pivoting. The float64 evaluation also meets the GPU test's condition (at least half of the planted
    inliers) on every listed case."""
    slots = VF.kernel_test_slots()
    worst = -10 ** 9
    for i, n in enumerate(VF.SLOT_N):
        if n not in (257, 1000):
            continue
        c, true, _ = slots[i]
        for seed in (0, 0x5EED0000C0FFEE):
            want = VF.ransac(c, 1024, 2.5, seed, slot=i)
            cnt64, _, m64 = VF.ransac_f64(c, 1024, 2.5, seed, slot=i)
            t32, t64 = int((want["mask"] & true).sum()), int((m64 & true).sum())
            print(f"n = {n}, seed {seed:#x}: fp32 {t32} true inliers of {int(true.sum())} planted ({want['nb_inliers']} in the mask), float64 {t64} ({cnt64})")
            assert want["valid"] == 1
            assert 2 * t64 >= int(true.sum())                              # the condition of the GPU test holds for the float64 evaluation
            worst = max(worst, t64 - t32)
    assert worst <= VF.FP32_MAX_SHORTFALL


def test_the_planted_geometry_is_found_in_every_slot_of_the_gpu_test():
    for i, (c, true, _) in enumerate(VF.kernel_test_slots()):
        n = len(c)
        res = VF.ransac(c, 1024, 2.5, 0, slot=i)
        assert res["valid"] == (1 if n >= 8 else 0), n
        if n >= 8:
            assert 2 * int((res["mask"] & true).sum()) >= int(true.sum()), (n, res["nb_inliers"])
            assert np.abs(res["F"]).max() >= 1.0 and np.abs(res["F"]).max() < 2.0
