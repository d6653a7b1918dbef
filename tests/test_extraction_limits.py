"""How dense can the candidate list of an octave get? (CPU only: the oracle and numpy.)

The extrema scan lists every texel that passes the 26-neighbour test and |D| > 0.8 * intensity_threshold / S (`extract_one` in
oracle/sift_oracle.c) in a per-octave scratch list of fixed capacity; a candidate beyond it would be lost without a word
(k_cand_list, extrema.hip). The capacity therefore has to hold by proof, not by experience with natural images:

  A strict maximum of the 26-neighbourhood is in particular a strict maximum of its own layer's 8-neighbourhood, so no two strict
  maxima of one layer are 8-adjacent: they form an independent set of the king's graph on the (w-2) x (h-2) interior. Cut the interior
  into ceil((w-2)/2) x ceil((h-2)/2) blocks of at most 2x2 texels; the texels of a block are pairwise 8-adjacent, so a block holds at
  most one strict maximum. The same holds for strict minima, and a texel is never both. Per octave of S scales:

      candidates <= S * 2 * ceil((w-2)/2) * ceil((h-2)/2)                       (capacity: that + 64, vksift_instance.c)

The 2x2-periodic texture [[4,2],[3,1]] with tiny sigmas meets the bound exactly: every texel of value 4 is a strict maximum and every
texel of value 1 a strict minimum of its DoG layer. The old capacity S*w*h/4 + 64 (which assumed 1/8 per sign) is half of it; the
fixtures below all exceed it, which is what lets the GPU tests (test_gpu_extraction_limits.py) catch a list that is too short.
"""
import numpy as np
import pytest

# the configuration that makes every texel of the textures a candidate: no up-sampling, no input blur, tiny sigmas, one scale
DENSE_CFG = dict(use_input_upsampling=0, input_image_blur_level=0.0, seed_scale_sigma=0.25, nb_scales_per_octave=1)


def texture(w, h, period4=False):
    """[[4,2],[3,1]] tiled (and, with period4, plus the same pattern at period 4), scaled to 0..255"""
    p = np.array([[4.0, 2.0], [3.0, 1.0]])
    y, x = np.mgrid[0:h, 0:w]
    t = p[y % 2, x % 2]
    if period4:
        t = t + p[(y // 2) % 2, (x // 2) % 2]
    t = (t - t.min()) * (255.0 / (t.max() - t.min()))
    return np.rint(t).astype(np.uint8)


def bound(S, w, h):
    """the proven maximum of strict 26-neighbour extrema in an octave (module docstring)"""
    return S * 2 * ((w - 1) // 2) * ((h - 1) // 2)   # ceil((n-2)/2) == (n-1)//2 for n >= 1


def capacity(S, w, h):
    return bound(S, w, h) + 64


def old_capacity(S, w, h):
    return S * w * h // 4 + 64


def strict_extrema(dog, S, pre):
    """number of texels of scales 1..S of a (S+2, h, w) DoG stack that are strict 26-neighbour maxima or minima with |D| > pre"""
    _, h, w = dog.shape
    n = 0
    for s in range(1, S + 1):
        c = dog[s, 1:h - 1, 1:w - 1]
        is_max = np.ones(c.shape, bool)
        is_min = np.ones(c.shape, bool)
        for ds in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if ds == 0 and dy == 0 and dx == 0:
                        continue
                    v = dog[s + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                    is_max &= c > v
                    is_min &= c < v
        n += int(((is_max | is_min) & (np.abs(c) > pre)).sum())
    return n


def octave_candidates(oracle, cfg, img):
    """[(w, h, candidates, keypoints)] per octave of the oracle's scale-space"""
    S = cfg.nb_scales_per_octave
    pre = np.float32(np.float32(cfg.intensity_threshold) / np.float32(S)) * np.float32(0.8)   # extract_one's float arithmetic
    p = oracle.Pyramid(cfg, img)
    try:
        out = []
        for o in range(p.nb_octaves):
            w, h = p.resolution(o)
            dog = np.stack([p.dog(o, s) for s in range(S + 2)])
            _, nkp = p.extract_keypoints(o, cap=1)
            out.append((w, h, strict_extrema(dog, S, pre), nkp))
        return out
    finally:
        p.close()


# (name, w, h, period4, fp16, octaves that must exceed the old capacity)
FIXTURES = [
    ("p2_256x128", 256, 128, False, False, [0]),
    ("p2_322x242", 322, 242, False, False, [0]),     # odd sizes: the last 64-pixel segment of a row is partly filled
    ("p2_97x61", 97, 61, False, False, [0]),
    ("p2_640x480", 640, 480, False, False, [0]),     # height above 256: 48-row scan bands
    ("p24_320x240", 320, 240, True, False, [0, 1]),  # the period-4 copy fills octave 1 as well
    ("p2_320x240_fp16", 320, 240, False, True, [0]),
]


@pytest.mark.parametrize("name,w,h,period4,fp16,dense", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_dense_textures_exceed_the_old_capacity_and_respect_the_bound(oracle, name, w, h, period4, fp16, dense):
    cfg = oracle.default_config(math_mode=1, input_image_max_size=w * h, pyramid_fp16=int(fp16), **DENSE_CFG)
    S = cfg.nb_scales_per_octave
    octs = octave_candidates(oracle, cfg, texture(w, h, period4))
    assert len(octs) >= max(dense) + 1
    for o, (ow, oh, n, nkp) in enumerate(octs):
        assert n <= bound(S, ow, oh) < capacity(S, ow, oh), (name, o, n)
        # the oracle's own loop visits every candidate once: it cannot yield more keypoints than there are candidates
        assert nkp <= n, (name, o, nkp, n)
        if o in dense:
            # the fixture keeps its purpose: the octave's candidates, and the keypoints they yield, overflow the old list
            assert n > old_capacity(S, ow, oh) and nkp > old_capacity(S, ow, oh), (name, o, n, nkp, old_capacity(S, ow, oh))


def test_the_bound_is_met_exactly(oracle):
    """256x128, the 2x2 pattern: every interior texel of value 4 or 1 is a candidate, 2 * 127 * 63 = 16 002"""
    cfg = oracle.default_config(math_mode=1, input_image_max_size=256 * 128, **DENSE_CFG)
    w, h, n, nkp = octave_candidates(oracle, cfg, texture(256, 128))[0]
    assert (w, h) == (256, 128)
    assert n == bound(1, w, h) == 16002
    assert nkp == n
    assert old_capacity(1, w, h) == 8256


@pytest.mark.parametrize("S,w,h", [(1, 5, 5), (1, 6, 7), (1, 12, 8), (2, 9, 4), (3, 16, 11), (5, 7, 7), (13, 12, 9)])
def test_bound_holds_for_arbitrary_dog_stacks(S, w, h):
    """the proof does not depend on the images SIFT produces: random stacks, stacks with many ties, and stacks whose layers alternate
    between a 2x2-periodic layer (a maximum and a minimum in every 2x2 block) and the same layer at half amplitude"""
    rng = np.random.default_rng(S * 1000 + w * 31 + h)
    y, x = np.mgrid[0:h, 0:w]
    alt = np.where((y % 2 == 1) & (x % 2 == 1), 4.0, np.where((y % 2 == 0) & (x % 2 == 0), -4.0, 0.0)).astype(np.float32)
    stacks = [rng.standard_normal((S + 2, h, w)).astype(np.float32) for _ in range(20)]
    stacks += [rng.integers(-2, 3, (S + 2, h, w)).astype(np.float32) for _ in range(20)]
    stacks.append(np.stack([alt * (1.0 if s % 2 else 0.5) for s in range(S + 2)]))
    best = 0
    for st in stacks:
        n = strict_extrema(st, S, np.float32(0.0))
        assert n <= bound(S, w, h), (S, w, h, n)
        best = max(best, n)
    if S == 1 and w % 2 == 0 and h % 2 == 0:
        assert best == bound(S, w, h)   # the single scale of the alternating stack: every 2x2 block of the interior holds both
