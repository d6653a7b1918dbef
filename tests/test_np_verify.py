"""The restatement of the RANSAC homography estimator (tests/np_verify.py) pinned on the CPU, so that the GPU kernels of verify.hip are not
compared against an unpinned model: the sampler, the four-point solve, the estimator on synthetic cases with known truth, degenerate inputs."""
import numpy as np
import pytest

import np_verify as V
import quality as Q

SIZES = ((640, 480), (8000, 6000))


@pytest.mark.parametrize("n", [4, 5, 7, 64, 1000, 65535])
def test_sampler_indices_are_distinct_and_in_range(n):
    for seed in (0, 1, 0xDEADBEEFCAFE):
        for slot in (0, 5, 511):
            for hyp in list(range(40)) + [255, 256, 65535]:
                s = V.sample(seed, slot, hyp, n)
                assert len(set(s)) == 4 and min(s) >= 0 and max(s) < n, (seed, slot, hyp, n, s)
    if n <= 7:  # every index is reachable in every position
        seen = [set() for _ in range(4)]
        for hyp in range(400):
            for k, i in enumerate(V.sample(3, 0, hyp, n)):
                seen[k].add(i)
        assert all(s == set(range(n)) for s in seen)


def test_sampler_fixed_table():
    """(seed, slot, hypothesis, n) -> indices, written down once (splitmix64, integer arithmetic only: the same anywhere)"""
    table = {
        (0, 0, 0, 4): [2, 3, 0, 1],
        (0, 0, 1, 5): [0, 4, 1, 2],
        (1, 0, 0, 7): [2, 6, 0, 5],
        (0, 3, 17, 64): [62, 10, 41, 56],
        (0x5EED, 511, 65535, 1000): [991, 938, 865, 895],
        (2 ** 64 - 1, 7, 1023, 65535): [30276, 35535, 30825, 8818],
        (42, 1, 2, 100000): [5730, 49537, 4655, 80413],
    }
    for k, want in table.items():
        assert V.sample(*k) == want, k
    assert V.seed_key(0) == 0xE220A8397B1DCDAF  # the first splitmix64 output of state 0 (vksift_synth.c's generator)


# Four-corner transfer error (px) of the model solved from four EXACT correspondences (float64 ground truth rounded to fp32) against the
# ground truth: (float64 solve, fp32 solve), measured 2026-10-16 on the CPU, per size and warp of quality.WARPS. The float64 figure is what
# the rounding of the inputs alone costs; the bound asserted below is their sum, doubled. (8000x6000 warp 2 has its horizon inside the
# image: the corners are far beyond the sample, hence the larger figures.)
SOLVE_ERR = {
    (640, 0): (1.7e-5, 2.4e-4), (640, 1): (4.0e-5, 1.8e-4), (640, 2): (2.8e-5, 1.7e-4), (640, 3): (3.9e-5, 1.4e-4), (640, 4): (2.2e-5, 3.0e-4),
    (8000, 0): (5.3e-4, 3.3e-3), (8000, 1): (6.5e-4, 3.8e-3), (8000, 2): (4.2e-2, 3.3e-1), (8000, 3): (2.2e-4, 1.7e-3), (8000, 4): (2.0e-4, 2.6e-3),
}


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("wi", range(5))
def test_solve_reproduces_the_ground_truth_on_exact_correspondences(size, wi):
    w, h = size
    Ht = Q.homography(w, h, **Q.WARPS[wi])
    pts = np.array([[0.1 * w, 0.15 * h], [0.9 * w, 0.2 * h], [0.8 * w, 0.85 * h], [0.2 * w, 0.9 * h]])
    qx, qy = Q.project(Ht, pts[:, 0], pts[:, 1])
    c = np.stack([pts[:, 0], pts[:, 1], qx, qy], 1).astype(np.float32)
    g = V.solve(*(c[i:i + 1] for i in range(4)))[0]
    assert 1.0 <= np.abs(g).max() < 2.0
    P = g.astype(np.float64)
    P[[2, 5]] *= 8192.0
    P[[6, 7]] /= 8192.0
    e32 = V.corner_error(P.reshape(3, 3), Ht, w, h)
    e64 = V.corner_error(V.solve_f64(*(c[i:i + 1] for i in range(4)))[0].reshape(3, 3), Ht, w, h)
    f64_fig, f32_fig = SOLVE_ERR[(w, wi)]
    print(f"{w}x{h} warp {wi}: corner error fp32 {e32:.3g} px, float64 {e64:.3g} px")
    assert e32 <= 2.0 * (f64_fig + f32_fig), (e32, e64)
    # and the four points themselves map onto their images (640x480: the horizon of every warp lies outside the image, so all four are in
    # front of the plane; at 8000x6000 the stronger warps put it inside and the d > 0 rule rightly rejects what lies beyond)
    if w == 640:
        assert V.inliers(g[None, :], c, V.threshold2(0.01)).all()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("wi", range(5))
def test_estimator_on_synthetic_cases(size, wi):
    """400 correspondences, 50 % outliers, 0.5 px noise, 1024 hypotheses, 2.5 px"""
    w, h = size
    Ht = Q.homography(w, h, **Q.WARPS[wi])
    corr, true_in = V.synthetic_case(Ht, w, h, n=400, outliers=0.5, noise=0.5, seed=100 + wi)
    r = V.ransac(corr, 1024, 2.5, 0)
    j64, cnt64, _, _, _ = V.ransac_f64(corr, 1024, 2.5, 0)
    print(f"{w}x{h} warp {wi}: winner {r['best_hypothesis']} with {r['nb_inliers']} inliers ({int((r['mask'] & true_in).sum())} of {int(true_in.sum())} true ones)")
    assert r["valid"] == 1 and r["H"][2, 2] == 1.0
    assert (r["best_hypothesis"], r["nb_inliers"]) == (j64, cnt64)
    assert int(r["mask"].sum()) == r["nb_inliers"]
    assert int((r["mask"] & true_in).sum()) >= 100   # it found the planted model, not an accident among the outliers
    # every correspondence farther than 1e-3 px inside the threshold under the returned H (float64 arithmetic) is in the mask
    H = r["H"].astype(np.float64)
    c = corr.astype(np.float64)
    d = H[2, 0] * c[:, 0] + H[2, 1] * c[:, 1] + H[2, 2]
    err = np.hypot((H[0, 0] * c[:, 0] + H[0, 1] * c[:, 1] + H[0, 2]) / d - c[:, 2], (H[1, 0] * c[:, 0] + H[1, 1] * c[:, 1] + H[1, 2]) / d - c[:, 3])
    inside = (d > 0) & (err < 2.5 - 1e-3)
    assert r["mask"][inside].all()
    assert not r["mask"][(d <= 0) | (err > 2.5 + 1e-3)].any()


def test_hypotheses_do_not_depend_on_their_number():
    corr, _ = V.synthetic_case(Q.homography(640, 480, **Q.WARPS[1]), 640, 480, n=100, seed=5)
    big = V.hypotheses(corr, 300, 9, 2)
    small = V.hypotheses(corr, 70, 9, 2)
    assert np.array_equal(big[0][:70], small[0]) and big[1][:70].tobytes() == small[1].tobytes()
    t2 = V.threshold2(2.5)
    counts = V.inliers(big[1], corr, t2).sum(axis=1)
    a, b = V.ransac(corr, 70, 2.5, 9, 2), V.ransac(corr, 70, 2.5, 9, 2, counts=counts, hyps=big)
    assert a["H"].tobytes() == b["H"].tobytes() and a["best_hypothesis"] == b["best_hypothesis"] and np.array_equal(a["mask"], b["mask"])


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_fewer_than_four_matches_is_invalid(n):
    r = V.ransac(np.arange(4 * n, dtype=np.float32).reshape(n, 4), 64, 2.5, 0)
    assert r["valid"] == 0 and r["nb_matches"] == n and r["nb_inliers"] == 0 and r["best_hypothesis"] == 0
    assert not r["H"].any() and len(r["mask"]) == n and not r["mask"].any()


def test_identical_correspondences_are_invalid():
    corr = np.tile(np.array([[100.0, 50.0, 120.0, 60.0]], np.float32), (50, 1))
    _, H = V.hypotheses(corr, 64, 0, 0)
    assert np.isnan(H).all()             # every cross product is exactly zero: H = 0, the degenerate rule makes it NaN
    r = V.ransac(corr, 64, 2.5, 0)
    assert r["valid"] == 0 and r["nb_inliers"] == 0 and not r["mask"].any() and not r["H"].any()


def test_collinear_samples_never_score_above_the_trivial():
    """All A points on one line (integer coordinates: the cross products are exact), B points generic. With p0, p1, p2 collinear adj(A)
    has rank one, H = b (l . x): points on the line map to d = 0 (no inlier: d > 0 fails), so no hypothesis can count its own sample."""
    rng = np.random.default_rng(3)
    t = rng.permutation(200)[:60].astype(np.float32)
    corr = np.stack([10 + 3 * t, 20 + 2 * t, rng.uniform(0, 639, 60).astype(np.float32), rng.uniform(0, 479, 60).astype(np.float32)], 1).astype(np.float32)
    _, H = V.hypotheses(corr, 256, 0, 0)
    counts = V.inliers(H, corr, V.threshold2(2.5)).sum(axis=1)
    assert counts.max() < 4
    r = V.ransac(corr, 256, 2.5, 0)
    assert r["valid"] == 0 and r["nb_inliers"] == 0 and not r["mask"].any()
    # one collinear triple inside an otherwise good set: a hypothesis that draws it counts fewer than four, and the estimate is unharmed
    good, _ = V.synthetic_case(Q.homography(640, 480, **Q.WARPS[0]), 640, 480, n=40, outliers=0.0, noise=0.1, seed=8)
    good[:3, :2] = np.array([[10, 10], [20, 20], [30, 30]], np.float32)
    idx = np.array([[0, 1, 2, 7]])
    Hc = V.solve(*(good[idx[:, i]] for i in range(4)))
    assert V.inliers(Hc, good, V.threshold2(2.5)).sum() < 4
    assert V.ransac(good, 256, 2.5, 0)["nb_inliers"] >= 30


def test_points_behind_the_plane_and_nan_are_never_inliers():
    H = np.array([[1, 0, 0, 0, 1, 0, 0, 0, -1]], np.float32)   # d = -1 everywhere
    corr = np.array([[10, 20, -10, -20], [np.nan, 0, 0, 0]], np.float32)
    assert not V.inliers(H, corr, V.threshold2(2.5)).any()
    assert V.inliers(-H, corr, V.threshold2(2.5)).tolist() == [[True, False]]
