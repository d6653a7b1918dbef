"""orc_pyramid_from_planes / Pyramid.from_planes: an octave rebuilt from the Gaussian planes of a built pyramid is that octave — the same
DoG planes and the same detection, byte for byte, in fp32 and binary16 — and the harness's fixed-point table is orc_descriptor's and
the one the product hands to the descriptor kernel."""
import ctypes as C

import numpy as np
import pytest

import hip_features as HF
from test_np_features import _img


@pytest.mark.parametrize("fp16", [0, 1], ids=["fp32", "fp16"])
@pytest.mark.parametrize("ups", [1, 0], ids=["ups", "noups"])
def test_rebuilt_octave_is_the_octave(oracle, fp16, ups):
    img = _img(7, 96, 72)
    cfg = oracle.default_config(math_mode=1, pyramid_fp16=fp16, use_input_upsampling=ups, nb_octaves=1)
    pyr = oracle.Pyramid(cfg, img)
    assert pyr.nb_octaves == 1
    S = pyr.S
    planes = np.stack([pyr.gauss(0, s) for s in range(S + 3)])
    re = oracle.Pyramid.from_planes(cfg, planes)
    assert re.resolution(0) == pyr.resolution(0)
    for s in range(S + 3):
        assert re.gauss(0, s).tobytes() == planes[s].tobytes()
    for s in range(S + 2):
        assert re.dog(0, s).tobytes() == pyr.dog(0, s).tobytes(), s
    a, ca = pyr.detect()
    b, cb = re.detect()
    assert ca == cb and len(a) > 10 and a.tobytes() == b.tobytes()
    ka, na = pyr.extract_keypoints(0)
    kb, nb = re.extract_keypoints(0)
    assert na == nb and ka.tobytes() == kb.tobytes()
    assert set(ka["octave_idx"].tolist()) == {-1 if ups else 0}


def test_later_octave_rebuilt_alone(oracle):
    """octave 2 of a pyramid without up-sampling, rebuilt alone, is octave 0 of its own pyramid: only octave_idx (and with it x, y, sigma) moves"""
    img = _img(8, 192, 144)
    cfg = oracle.default_config(math_mode=1, use_input_upsampling=0)
    pyr = oracle.Pyramid(cfg, img)
    planes = np.stack([pyr.gauss(2, s) for s in range(pyr.S + 3)])
    re = oracle.Pyramid.from_planes(cfg, planes)
    ka, _ = pyr.extract_keypoints(2)
    kb, _ = re.extract_keypoints(0)
    assert len(ka) == len(kb) >= 3
    for name in ("scale_x", "scale_y", "scale_idx", "intensity"):
        assert ka[name].tobytes() == kb[name].tobytes()
    for k0, k1 in zip(ka[:8], kb[:8]):
        assert np.array_equal(pyr.orientations(2, k0)[1], re.orientations(0, k0)[1])
        assert np.array_equal(pyr.descriptor(2, k0)[1], re.descriptor(0, k0)[1])


def test_fp_table_is_the_oracles(oracle):
    """the table the harness hands to the descriptor kernel against orc_descriptor's own fixed-point scale, through a one-texel probe: the
    plane is zero but for one texel right of the keypoint, the keypoint sits on a texel centre with theta = 0. The only sample whose gradient
    points along +x is the centre one (gradient 0.375, weight e^0, bin 0 exactly, cell weights 0.5 * 0.5), so accumulator (cell (1, 1), bin 0)
    holds uint(0.09375 * fp) = 0.09375 * fp, whatever R."""
    tab = HF.fp_table(oracle, 140)
    assert tab[0] == 65536 and tab[1] == 32768 and np.all(np.diff(tab) <= 0) and tab[-1] == tab[24] == 4096
    cfg = oracle.default_config(math_mode=1, nb_scales_per_octave=1)
    planes = np.zeros((4, 41, 41), np.float32)
    planes[:, 20, 21] = 0.75
    pyr = oracle.Pyramid.from_planes(cfg, planes)
    seen = set()
    for R in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 15, 21, 40, 47, 48, 49, 50, 127, 129, 257, 279):
        kp = HF.make_records([(20, 20, 1, 0, HF.rel_for_R(R), 0.0)])[0]
        assert HF.desc_radius(kp) == R
        _, raw = pyr.descriptor(0, kp)
        assert raw[1 * 32 + 1 * 8 + 0] == 0.09375 * tab[R // 2], (R, raw[40], tab[R // 2])
        seen.add(float(tab[R // 2]))
    assert len(seen) >= 4


def test_fp_table_is_the_products(vk, oracle):
    """the harness's table against vksift_hm_desc_fp_table, which fills the table an instance hands to the descriptor kernel: every entry
    the product computes for a configuration, bit for bit — from the stock one to S = 1 with seed 8 (the public-API case of the launcher
    test, R up to 343) and S = 13; a capacity below the configuration's need cuts the table, entry 0 (R = 1) is 2^16 in both"""
    L = vk.lib()
    L.vksift_hm_desc_fp_table.restype = C.c_uint32
    lengths = set()
    for kw, cap in (({}, 1024), ({"nb_scales_per_octave": 1, "seed_scale_sigma": 8.0}, 1024), ({"nb_scales_per_octave": 1, "seed_scale_sigma": 2.4}, 1024),
                    ({"nb_scales_per_octave": 13}, 1024), ({"nb_scales_per_octave": 2, "seed_scale_sigma": 0.6}, 1024),
                    ({"nb_scales_per_octave": 1, "seed_scale_sigma": 8.0}, 30)):
        vcfg = vk.default_config(**kw)
        tab = np.full(cap + 1, -1.0, np.float32)
        n = L.vksift_hm_desc_fp_table(C.byref(vcfg), tab.ctypes.data_as(C.c_void_p), C.c_uint32(cap))
        assert 2 <= n <= cap and tab[n] == -1.0, kw
        assert tab[:n].tobytes() == HF.fp_table(oracle, n).tobytes(), kw
        assert tab[0] == 65536
        lengths.add(n)
    assert max(lengths) > 160 and 30 in lengths                                       # beyond every R of the launcher test; the cut
