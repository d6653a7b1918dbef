"""Detection at the limits of what config_is_valid accepts, bit for bit against the oracle (det math).

* Dense textures (test_extraction_limits.py): every interior texel of value 4 or 1 of a 2x2-periodic texture is a candidate, twice
  what the per-octave candidate list used to hold (S*w*h/4 + 64). A list that is too short drops the candidates past its end in
  raster order — and with them every keypoint below some row of the octave.
* Config corners: sigmas down to 0 (blur kernels of 1 to 4 taps), no input blur, thresholds of 0 (edge_limit = inf), and the scales
  per octave up to the limit of 13 (every k_extrema_lean instantiation, fp32 and binary16).
* The widest octave: candidate coordinates are packed with 14-bit x and y fields, so octaves with a side of 16384 or more are refused.

Tap counts and the blur forms they take (vksift_hip_blur_form and the launchers of pyramid.hip):
  1 tap      form 0, the generic tile kernel (k_blur_tile); the fused seed launches (vksift_hip_seed_upsampled / _direct, 2..12 taps)
             and vksift_hip_blur_downsample decline it, so the input blit and the down-sampling run as separate launches; the LDS octave
             chain (fp32, small octaves) takes any tap count
  2-4 taps   form 1, the two-texel strip march (k_blur_lean<N>) on widths that are multiples of 4, else form 0; never form 2 (the
             four-texel k_blur_wide exists for 5, 7, 9, 11 and 13 taps); vksift_hip_blur_multi (9, 11, 13, 15 taps) and
             vksift_hip_blur_pair (5 + 7 taps) decline them, so scales S+1 and S+2 go out as one launch per octave
"""
import numpy as np
import pytest

from test_extraction_limits import DENSE_CFG, old_capacity, texture

pytestmark = pytest.mark.gpu

VKSIFT_TUNE_SCAN_BAND = 9


def _cfgs(vk, oracle, **kw):
    okw = {}
    vkw = {}
    for k, v in kw.items():
        if k in ("use_input_upsampling", "use_hardware_interpolated_blur"):
            okw[k] = int(v)
            vkw[k] = bool(v)
        elif k == "descriptor_format":
            okw["use_vlfeat_format"] = int(v)
            vkw[k] = int(v)
        else:
            okw[k] = v
            vkw[k] = v
    return vk.default_config(**vkw), oracle.default_config(math_mode=1, **okw)


def _setup(vk, oracle, w, h, fp16=False, nbuf=2, max_nb=None, **kw):
    """max_nb: by default large enough that no section of the dense fixtures clamps (_ref checks it)"""
    vcfg, ocfg = _cfgs(vk, oracle, input_image_max_size=max(w * h, 1024), max_nb_sift_per_buffer=max_nb or 2 * w * h, **kw)
    vcfg.sift_buffer_count = nbuf
    if fp16:
        vcfg.pyramid_precision_mode = 1
        ocfg.pyramid_fp16 = 1
    return vcfg, ocfg


def _ref(oracle, ocfg, img, clamped=False):
    ref, counts = oracle.detect(ocfg, img)
    assert (len(ref) < sum(counts)) == clamped, (len(ref), counts)
    return ref, counts


def _per_octave(f):
    o, n = np.unique(f["octave_idx"], return_counts=True)
    return dict(zip(o.tolist(), n.tolist()))


def _assert_same(inst, buf, ref, what=""):
    n = inst.getFeaturesNumber(buf)
    got = inst.downloadFeatures(buf)
    assert n == len(ref) and got.tobytes() == ref.tobytes(), (what, "GPU", n, _per_octave(got), "oracle", len(ref), _per_octave(ref))


# (texture, w, h, period4, fp16, hardware-interpolated blur, scan band)
DENSE = [
    ("p2_256x128", 256, 128, False, False, True, 0),
    ("p2_256x128_nohw", 256, 128, False, False, False, 0),
    ("p24_320x240", 320, 240, True, False, True, 0),
    ("p24_320x240_fp16", 320, 240, True, True, True, 0),
    ("p24_320x240_nohw", 320, 240, True, False, False, 0),
    ("p2_320x240_fp16", 320, 240, False, True, True, 0),
    ("p2_322x242", 322, 242, False, False, True, 0),
    ("p2_322x242_fp16_nohw", 322, 242, False, True, False, 0),
    ("p2_97x61", 97, 61, False, False, True, 0),
    ("p2_640x480", 640, 480, False, False, True, 0),
    ("p2_640x480_band48", 640, 480, False, False, True, 48),
]


@pytest.mark.parametrize("name,w,h,period4,fp16,hw,band", DENSE, ids=[d[0] for d in DENSE])
def test_dense_texture_single_image(vk, oracle, name, w, h, period4, fp16, hw, band):
    vcfg, ocfg = _setup(vk, oracle, w, h, fp16=fp16, use_hardware_interpolated_blur=hw, **DENSE_CFG)
    img = texture(w, h, period4)
    ref, counts = _ref(oracle, ocfg, img)
    ow, oh = oracle.scale_space_info(ocfg, w, h)[0]
    assert counts[0] > old_capacity(1, ow, oh)
    L = vk.lib()
    try:
        if band:
            L.vksift_hip_tune(VKSIFT_TUNE_SCAN_BAND, band)   # 48-row bands on octaves taller than 256 rows, whatever the launch size
        with vk.Instance(vcfg) as inst:
            inst.detectFeatures(img, 0)
            _assert_same(inst, 0, ref, name)
    finally:
        L.vksift_hip_tune(VKSIFT_TUNE_SCAN_BAND, 0)


def _mixed_frames(vk, n, w, h, seed):
    """dense textures and natural frames, interleaved: one image's candidates must not spill into another's list"""
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append(texture(w, h, period4=(i % 4 == 0)))
        else:
            out.append(vk.gen_synthetic_image(seed + i, w, h))
    return out


@pytest.mark.parametrize("nb,fp16", [(3, False), (10, False), (10, True)])
def test_dense_textures_in_a_batch(vk, oracle, nb, fp16):
    """3 frames: the single-buffer batch schedule; 10: the batch instance's own launch shapes (multi-octave tail, batch grids)"""
    w, h = 320, 240
    vcfg, ocfg = _setup(vk, oracle, w, h, fp16=fp16, nbuf=nb, **DENSE_CFG)
    imgs = _mixed_frames(vk, nb, w, h, 300)
    refs = [_ref(oracle, ocfg, im)[0] for im in imgs]
    with vk.Instance(vcfg, batch_capacity=nb) as inst:
        inst.detectFeaturesBatch(imgs, 0)
        for i in range(nb):
            _assert_same(inst, i, refs[i], i)


def test_dense_textures_through_deferred_detect_calls(vk, oracle, monkeypatch):
    """plain vksift_detectFeatures calls in a row are staged and launched as batches (deferred submission)"""
    monkeypatch.setenv("VKSIFT_DEFER", "1")
    monkeypatch.delenv("VKSIFT_DEFER_MAX", raising=False)
    w, h, n = 320, 240, 6
    vcfg, ocfg = _setup(vk, oracle, w, h, nbuf=n, **DENSE_CFG)
    imgs = _mixed_frames(vk, n, w, h, 400)
    refs = [_ref(oracle, ocfg, im)[0] for im in imgs]
    with vk.Instance(vcfg) as inst:
        for rep in range(2):
            for i, im in enumerate(imgs):
                inst.detectFeatures(im, i)
            for i in range(n):
                _assert_same(inst, i, refs[i], (rep, i))
        assert inst.getDeferredStats()[1] > 0


def test_dense_sections_clamp_like_the_oracle(vk, oracle):
    """a buffer too small for a dense octave: the stored records, the extra orientations and the counts follow the oracle's clamp rule"""
    w, h = 320, 240
    vcfg, ocfg = _setup(vk, oracle, w, h, max_nb=3000, **DENSE_CFG)
    img = texture(w, h, period4=True)
    ref, counts = _ref(oracle, ocfg, img, clamped=True)
    with vk.Instance(vcfg) as inst:
        inst.detectFeatures(img, 0)
        _assert_same(inst, 0, ref)
    # one octave whose section holds every keypoint exactly, and none of the extra orientations
    w, h = 97, 61
    img = texture(w, h, period4=True)
    p = oracle.Pyramid(_setup(vk, oracle, w, h, **DENSE_CFG)[1], img)
    try:
        assert p.nb_octaves == 1
        nkp = p.extract_keypoints(0, cap=1)[1]
    finally:
        p.close()
    vcfg, ocfg = _setup(vk, oracle, w, h, max_nb=nkp, **DENSE_CFG)
    ref, counts = _ref(oracle, ocfg, img, clamped=True)
    assert len(ref) == nkp and counts[0] > nkp
    with vk.Instance(vcfg) as inst:
        inst.detectFeatures(img, 0)
        _assert_same(inst, 0, ref)


def _assert_matches_equal(m, ref):
    for name in ("idx_a", "idx_b1", "idx_b2"):
        assert np.array_equal(m[name], ref[name]), (name, np.flatnonzero(m[name] != ref[name])[:10])
    for name in ("dist_a_b1", "dist_a_b2"):
        assert np.array_equal(m[name].view(np.uint32), ref[name].view(np.uint32)), name


def test_matching_dense_buffers(vk, oracle):
    """~2.9 k nearly identical descriptors: massive ties, the earlier index wins; against itself and against a natural image"""
    w, h = 96, 64
    vcfg, ocfg = _setup(vk, oracle, w, h, nbuf=3, **DENSE_CFG)
    dense = texture(w, h)
    nat = vk.gen_synthetic_image(96, w, h)
    rd = _ref(oracle, ocfg, dense)[0]
    rn = _ref(oracle, ocfg, nat)[0]
    assert len(rd) > 2500 and len(rn) >= 2
    with vk.Instance(vcfg) as inst:
        inst.detectFeatures(dense, 0)
        inst.detectFeatures(dense, 1)
        inst.detectFeatures(nat, 2)
        _assert_same(inst, 0, rd)
        _assert_same(inst, 2, rn)
        for a, b, ra, rb in [(0, 1, rd, rd), (0, 2, rd, rn), (2, 0, rn, rd)]:
            inst.matchFeatures(a, b)
            assert inst.getMatchesNumber() == len(ra)
            _assert_matches_equal(inst.downloadMatches(), oracle.match_2nn(ra, rb))


# (id, image, config): small sigmas give blur kernels of 1 to 4 taps (see the module docstring for the forms they take)
CORNERS = [
    ("sigma0.2_blur0", "nat", dict(seed_scale_sigma=0.2, input_image_blur_level=0.0, intensity_threshold=0.0005)),
    ("sigma0.2_blur0_dense", "dense", dict(seed_scale_sigma=0.2, input_image_blur_level=0.0, use_input_upsampling=False, nb_scales_per_octave=1)),
    ("sigma0.5_blur0_noups", "nat", dict(seed_scale_sigma=0.5, input_image_blur_level=0.0, use_input_upsampling=False)),
    ("sigma0.5_seed1tap", "nat", dict(seed_scale_sigma=0.5, input_image_blur_level=0.25)),    # blur = seed / 2, up-sampled: 1-tap seed
    ("sigma0.8_blur0_nohw", "nat", dict(seed_scale_sigma=0.8, input_image_blur_level=0.0, use_hardware_interpolated_blur=False)),
    ("sigma0.8_seed1tap_dense", "dense", dict(seed_scale_sigma=0.8, input_image_blur_level=0.4)),
    ("sigma1.0_seed1tap", "nat", dict(seed_scale_sigma=1.0, input_image_blur_level=0.5)),
    ("sigma0.5_blur0_dense_fp16", "dense16", dict(seed_scale_sigma=0.5, input_image_blur_level=0.0, use_input_upsampling=False, nb_scales_per_octave=2)),
    ("sigma0_ups", "nat", dict(seed_scale_sigma=0.0, input_image_blur_level=0.0)),             # every kernel 1 tap
    ("sigma0_noups_dense", "dense", dict(seed_scale_sigma=0.0, input_image_blur_level=0.0, use_input_upsampling=False)),
    ("thr0_edge0", "nat", dict(intensity_threshold=0.0, edge_threshold=0.0)),                   # edge_limit = inf
    ("thr0_edge0_dense", "dense", dict(intensity_threshold=0.0, edge_threshold=0.0, **DENSE_CFG)),
] + [(f"S{S}{'_fp16' if f16 else ''}", "nat16" if f16 else "nat", dict(nb_scales_per_octave=S)) for S in range(9, 14) for f16 in (False, True)]


@pytest.mark.parametrize("name,kind,kw", CORNERS, ids=[c[0] for c in CORNERS])
def test_config_corners(vk, oracle, name, kind, kw):
    w, h = 160, 120
    vcfg, ocfg = _setup(vk, oracle, w, h, fp16=kind.endswith("16"), max_nb=400000, **kw)
    img = texture(w, h, period4=True) if kind.startswith("dense") else vk.gen_synthetic_image(len(name) * 7 + 5, w, h)
    taps = oracle.effective_taps(ocfg)[1]
    if name.startswith("sigma0_"):
        assert (taps == 1).all()
    elif "seed1tap" in name:
        assert taps[0] == 1
    ref, counts = _ref(oracle, ocfg, img)
    if not name.startswith("sigma0_"):
        assert len(ref) > 0
    pyr = oracle.Pyramid(ocfg, img)
    try:
        with vk.Instance(vcfg) as inst:
            inst.detectFeatures(img, 0)
            _assert_same(inst, 0, ref, name)
            # the scale-space itself (with sigma 0 every plane is the input and nothing is detected: the planes are what is checked)
            S = ocfg.nb_scales_per_octave
            assert inst.getScaleSpaceNbOctaves() == pyr.nb_octaves
            for o in range(pyr.nb_octaves):
                for s in range(S + 3):
                    g, r = inst.downloadScaleSpaceImage(o, s), pyr.gauss(o, s)
                    assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), ("gauss", o, s, np.abs(g - r).max())
                for s in range(S + 2):
                    d, r = inst.downloadDoGImage(o, s), pyr.dog(o, s)
                    assert np.array_equal(d.view(np.uint32), r.view(np.uint32)), ("dog", o, s, np.abs(d - r).max())
    finally:
        pyr.close()


def test_widest_octave(vk, oracle):
    """8191x128 up-sampled: octave 0 is 16382 texels wide, the widest the packed candidate coordinates (14-bit x) can address: bit-exact.
    8192x128 up-sampled (a 16384-wide octave 0) is refused through the error callback with VKSIFT_INVALID_INPUT_ERROR, by the plain and
    the batch entry, without touching the buffers; the instance goes on detecting correctly afterwards."""
    vcfg, ocfg = _cfgs(vk, oracle, input_image_max_size=8192 * 128, max_nb_sift_per_buffer=200000)
    vcfg.sift_buffer_count = 3
    ok = vk.gen_synthetic_image(8191, 8191, 128)
    ref = _ref(oracle, ocfg, ok)[0]
    assert oracle.scale_space_info(ocfg, 8191, 128)[0] == (16382, 256) and len(ref) > 1000
    wide = vk.gen_synthetic_image(8192, 8192, 128)
    with vk.Instance(vcfg) as inst:
        inst.detectFeatures(ok, 0)
        _assert_same(inst, 0, ref, "8191x128")
        with pytest.raises(vk.VksiftError) as e:
            inst.detectFeatures(wide, 1)
        assert e.value.code == vk.VKSIFT_INVALID_INPUT_ERROR
        with pytest.raises(vk.VksiftError) as e:
            inst.detectFeaturesBatch([wide], 0)
        assert e.value.code == vk.VKSIFT_INVALID_INPUT_ERROR
        _assert_same(inst, 0, ref, "buffer 0 after the refusals")
        assert inst.getFeaturesNumber(1) == 0
        inst.detectFeatures(ok, 2)
        _assert_same(inst, 2, ref, "8191x128 after the refusals")
