"""The plane-level entry points of the CPU oracle (orc_blur_plane, orc_blit_input, orc_blit_nearest, orc_store_f16) at shapes
orc_pyramid_build never feeds them. tests/test_gpu_pyramid_launchers.py compares every HIP launcher with these three functions bit
for bit, so they are pinned here first: against the pyramid they were cut out of, against exact index arithmetic, against float64
and against the numpy restatement. CPU only."""
import numpy as np
import pytest

import np_restatement as NP

f32 = np.float32


def test_bindings_shapes(oracle):
    src = np.arange(12, dtype=f32).reshape(3, 4)
    assert np.array_equal(oracle.blur_plane(src, [1.0]), src)  # one tap: a multiplication by k0
    assert oracle.blur_plane(src, [0.5, 0.25]).shape == (3, 4)
    assert oracle.blit_input(np.zeros((3, 5), np.uint8), 10, 6).shape == (6, 10)
    assert oracle.blit_nearest(src, 2, 1).shape == (1, 2)
    v = np.array([1 / 3, 65519.9, 1e-8, -2.5, 0.0], f32)
    assert np.array_equal(oracle.store_f16(v).view(np.uint32), v.astype(np.float16).astype(f32).view(np.uint32))
    assert np.array_equal(v, np.array([1 / 3, 65519.9, 1e-8, -2.5, 0.0], f32))  # a copy: the argument is not modified


@pytest.mark.parametrize("overrides", [
    dict(),
    dict(use_hardware_interpolated_blur=0),
    dict(nb_scales_per_octave=2),
    dict(nb_scales_per_octave=2, use_hardware_interpolated_blur=0, use_input_upsampling=0),
    dict(pyramid_fp16=1),
    dict(pyramid_fp16=1, use_hardware_interpolated_blur=0, nb_scales_per_octave=4),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()) or "default")
def test_same_function_as_the_pyramid(oracle, overrides):
    """Pyramid.gauss(o, s + 1) == orc_blur_plane(Pyramid.gauss(o, s), effective_taps[s + 1]) bit for bit, every octave and scale."""
    cfg = oracle.default_config(**overrides)
    taps, ntaps = oracle.effective_taps(cfg)
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (70, 90), dtype=np.uint8)
    p = oracle.Pyramid(cfg, img)
    try:
        checked = 0
        for o in range(p.nb_octaves):
            for s in range(cfg.nb_scales_per_octave + 2):
                got = oracle.blur_plane(p.gauss(o, s), taps[s + 1, :ntaps[s + 1]], fp16=bool(cfg.pyramid_fp16))
                assert np.array_equal(got.view(np.uint32), p.gauss(o, s + 1).view(np.uint32)), (o, s)
                checked += 1
            if o + 1 < p.nb_octaves:
                w, h = p.resolution(o + 1)
                assert np.array_equal(oracle.blit_nearest(p.gauss(o, cfg.nb_scales_per_octave), w, h), p.gauss(o + 1, 0)), o
        assert checked >= 2 * (cfg.nb_scales_per_octave + 2)
        # ... and the seed: blit (rounded to the pyramid format) + blur
        w0, h0 = p.resolution(0)
        seed = oracle.blit_input(img, w0, h0)
        if cfg.pyramid_fp16:
            seed = oracle.store_f16(seed)
        got = oracle.blur_plane(seed, taps[0, :ntaps[0]], fp16=bool(cfg.pyramid_fp16))
        assert np.array_equal(got.view(np.uint32), p.gauss(0, 0).view(np.uint32))
    finally:
        p.close()


SHORT = (1, 2, 3, 5, 8, 17, 31, 48)


@pytest.mark.parametrize("i", range(1, 20))
def test_one_hot_taps_are_exact_addressing(oracle, i):
    """taps[i] = 1, every other tap 0: the result is exactly t[mirror(x + i)] + t[mirror(x - i)], horizontally then vertically —
    no floating-point argument, only addressing. Sizes 1..48 on either axis, including w < i and h < i (several reflections)."""
    rng = np.random.default_rng(100 + i)
    taps = np.zeros(20, f32)
    taps[i] = 1
    shapes = {(w, h) for w in range(1, 49) for h in SHORT} | {(w, h) for h in range(1, 49) for w in SHORT}
    for w, h in sorted(shapes):
        t = rng.random((h, w), dtype=f32)
        x, y = np.arange(w), np.arange(h)
        hor = t[:, NP.mirror(x + i, w)] + t[:, NP.mirror(x - i, w)]
        ref = hor[NP.mirror(y + i, h), :] + hor[NP.mirror(y - i, h), :]
        for n in (i + 1, 20):  # the one-hot tap last, and followed by zero taps
            got = oracle.blur_plane(t, taps[:n])
            assert np.array_equal(got.view(np.uint32), ref.astype(f32).view(np.uint32)), (w, h, i, n)


def _conv64(src, taps):
    """plain float64 separable convolution with mirrored-repeat borders"""
    k = np.asarray(taps, f32).astype(np.float64)
    a = src.astype(np.float64)
    for axis in (1, 0):
        n = a.shape[axis]
        idx = np.arange(n)
        out = a * k[0]
        for i in range(1, len(k)):
            out = out + (np.take(a, NP.mirror(idx + i, n), axis=axis) + np.take(a, NP.mirror(idx - i, n), axis=axis)) * k[i]
        a = out
    return a


def _gauss_taps(n, sigma):
    k = np.exp(-0.5 * (np.arange(n) / sigma) ** 2)
    return (k / (k[0] + 2 * k[1:].sum())).astype(f32)


def test_float64_bound(oracle):
    """orc_blur_plane against a float64 convolution, inside the textbook rounding bound — derived, not tuned:

    One pass computes acc = fl(c k0), then acc = fl(fma(fl(t(+i) + t(-i)), k_i, acc)) for i = 1..n-1. With u = 2^-24, the term of
    tap i goes through the rounding of its pair sum (none for the centre, whose product is rounded instead) and the roundings of the
    fma steps i..n-1: at most n roundings, so pass(t) = sum_i k_i s_i (1 + theta_i), |theta_i| <= gamma_n = n u / (1 - n u), and
        |pass(t) - exact(t)| <= gamma_n A max|t|,   A = |k0| + 2 sum |k_i|.
    The vertical pass runs on the computed horizontal result h', |h'| <= (1 + gamma_n) A M with M = max|src|; it carries the first
    pass's error through its own (exact) weights, at most A gamma_n A M, and adds gamma_n A max|h'| of its own:
        |result - exact| <= (2 gamma_n + gamma_n^2) A^2 M  <=  2 (n + 2) u A^2 M    for n <= 20
    (2 gamma_n + gamma_n^2 = 2 n u (1 + O(n u)); the two extra units of u cover that factor, the float64 reference's own error
    ~ 2^-53 n A^2 M and the rounding of float64 -> float32 nowhere: the comparison is made in float64). Inputs in [0, 1] keep every
    intermediate far above the subnormal range, where the relative-error model would not hold.

    Largest observed error / bound over the cases below: 0.244 (Gaussian taps), 0.268 (random signed taps)."""
    rng = np.random.default_rng(7)
    u = 2.0 ** -24
    worst = {"gauss": 0.0, "signed": 0.0}
    for n in range(1, 21):
        for w, h in ((1, 1), (3, 50), (50, 3), (7, 9), (64, 48), (131, 77)):
            src = rng.random((h, w), dtype=f32)
            for family, taps in (("gauss", _gauss_taps(n, max(0.3, (n - 1) / 4.0))), ("signed", rng.uniform(-1, 1, n).astype(f32))):
                got = oracle.blur_plane(src, taps).astype(np.float64)
                ref = _conv64(src, taps)
                A = float(np.abs(taps[0].astype(np.float64)) + 2 * np.abs(taps[1:].astype(np.float64)).sum())
                bound = 2 * (n + 2) * u * A * A * float(src.max())
                err = float(np.abs(got - ref).max())
                worst[family] = max(worst[family], err / bound)
                assert err <= bound, (family, n, w, h, err, bound)
    print(f"float64 bound: largest error / bound = {worst['gauss']:.3f} (Gaussian taps), {worst['signed']:.3f} (random signed taps)")
    assert 0 < worst["gauss"] <= 1 and 0 < worst["signed"] <= 1


def test_fp16_mode_rounds_both_passes(oracle):
    """fp16 = 1: the horizontal pass's output and the result are binary16 values; with one tap of 1 it is the identity on binary16 planes"""
    rng = np.random.default_rng(3)
    src = oracle.store_f16(rng.random((9, 12), dtype=f32))
    assert np.array_equal(oracle.blur_plane(src, [1.0], fp16=True), src)
    taps = _gauss_taps(5, 1.2)
    got = oracle.blur_plane(src, taps, fp16=True)
    assert np.array_equal(oracle.store_f16(got), got)
    # binary16 sources whose every partial result is exact in binary16 (small integers): the fp16 mode then equals the fp32 mode
    ints = rng.integers(0, 8, (9, 12)).astype(f32)
    k = np.array([2, 1, 1], f32)
    assert np.array_equal(oracle.blur_plane(ints, k, fp16=True), oracle.blur_plane(ints, k))


def test_blit_input(oracle):
    rng = np.random.default_rng(5)
    for sw, sh in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (16, 9), (33, 31), (64, 65), (129, 2)):
        u8 = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        same = oracle.blit_input(u8, sw, sh)
        assert np.array_equal(same.view(np.uint32), (u8.astype(f32) / f32(255)).view(np.uint32)), (sw, sh)
        up = oracle.blit_input(u8, 2 * sw, 2 * sh)
        ref = NP.upsample2x(u8)
        # the restatement evaluates .25 a + .75 b without the oracle's fused multiply-add: equal to within one rounding of each of its
        # three products and sums per axis (values in [0, 1])
        assert up.shape == ref.shape and np.abs(up.astype(np.float64) - ref).max() <= 6 * 2.0 ** -24, (sw, sh)
        assert up.min() >= 0 and up.max() <= 1
    # all 256 byte values, exactly
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(oracle.blit_input(ramp, 16, 16), ramp.astype(f32) / f32(255))
    # a constant image stays constant under the 2:1 blit up to the rounding of (1 - a) t + a t
    flat = np.full((5, 6), 200, np.uint8)
    assert np.abs(oracle.blit_input(flat, 12, 10) - f32(200) / f32(255)).max() <= 2.0 ** -23


def test_blit_nearest(oracle):
    rng = np.random.default_rng(6)
    for sw, sh, dw, dh in ((2, 2, 1, 1), (8, 6, 4, 3), (9, 7, 4, 3), (7, 9, 3, 4), (51, 33, 25, 16), (1, 1, 1, 1), (5, 5, 5, 5), (3, 3, 7, 5), (64, 48, 32, 24),
                           (101, 1, 50, 1), (1, 101, 1, 50), (13, 11, 5, 9)):
        src = rng.random((sh, sw), dtype=f32)
        got = oracle.blit_nearest(src, dw, dh)
        assert np.array_equal(got, NP.blit_nearest(src, dw, dh)), (sw, sh, dw, dh)
        if sw == 2 * dw and sh == 2 * dh:
            assert np.array_equal(got, NP.downsample_nearest(src, dw, dh))
