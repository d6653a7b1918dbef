"""Pins the reference of tests/test_gpu_feature_launchers.py on that test's own domain before a GPU is asked: orc_orientations and
orc_descriptor in det math mode on a Pyramid.from_planes octave against the independent numpy restatement (tests/np_features.py), and det
mode against libm mode, on a thinned subset of the launcher test's records — window radii up to r = 130 and R = 257, lambda below 0.08,
border and corner positions, every special orientation, and the S = 13 records on every scale_idx 0 .. 14. The bounds are those of tests/test_np_features.py unless a docstring says otherwise."""
import numpy as np
import pytest

import hip_features as HF
import np_features as NF

f32 = np.float32


def _pyr(oracle, planes, math_mode, fp16=False, vlfeat=0):
    cfg = oracle.default_config(math_mode=math_mode, nb_scales_per_octave=planes.shape[0] - 3, pyramid_fp16=1 if fp16 else 0, use_vlfeat_format=vlfeat)
    return oracle.Pyramid.from_planes(cfg, planes)


@pytest.fixture(scope="module")
def ori_case(oracle):
    S, w, h = 1, 330, 300
    recs, want_r = HF.ori_size_records(w, h, S)
    planes = HF.field("smooth", S, h, w, 11)
    return planes, recs, want_r


def test_orientation_det_against_numpy(oracle, ori_case):
    """Histogram bins within 16 counts and angles within 1e-6, the bounds of tests/test_np_features.py, for every window r = 0 .. 130 and for
    lambda < 0.08. The long windows sum up to 68 000 contributions, each of which may truncate one count differently, but the fixed-point
    scale shrinks with the window, so they need no bound of their own: measured here, the largest bin difference over all records is 1
    count and every angle is identical."""
    planes, recs, want_r = ori_case
    pyr = _pyr(oracle, planes, 1)
    for kp, r in zip(recs, want_r):
        ang_ref, hist_ref = pyr.orientations(0, kp)
        ang, hist = NF.orientations(planes[int(kp["scale_idx"])], kp, max_nb_orientation=0)
        dh = int(np.abs(hist.astype(np.int64) - hist_ref.astype(np.int64)).max())
        assert dh <= 16, (r, float(kp["scale_x"]), dh)
        assert len(ang) == len(ang_ref), (r, ang, ang_ref)
        da = float(np.abs(ang - ang_ref).max(initial=0))
        assert da < 1e-6, (r, da)


def test_orientation_positions_det_against_numpy(oracle):
    S = 3
    for (w, h, r) in ((64, 48, 5), (40, 24, 64), (3, 3, 1), (3, 3, 7)):
        planes = HF.field("smooth", S, h, w, 21)
        pyr = _pyr(oracle, planes, 1)
        rel = HF.rel_for_r(r)
        pos = [(0, 0), (w - 1, h - 1), (0.25, h // 2), (w - 0.5, h // 2), (w - 0.01, h - 0.01), (w // 2, h - 0.5), (0.5, 0.5), (1.5, 2.5),
               (min(1 + r, w - 1) + 0.25, h // 2), (min(r, w - 1) + 0.25, h // 2)]
        for i, (x, y) in enumerate(pos):
            kp = HF.make_records([(x, y, i % (S + 2), 0, rel, 0.0)])[0]
            ang_ref, hist_ref = pyr.orientations(0, kp)
            ang, hist = NF.orientations(planes[int(kp["scale_idx"])], kp, max_nb_orientation=0)
            assert np.abs(hist.astype(np.int64) - hist_ref.astype(np.int64)).max() <= 16, (w, h, r, x, y)
            assert len(ang) == len(ang_ref) and np.abs(ang - ang_ref).max(initial=0) < 1e-6


def _desc_records(w, h, S):
    rows = []
    th = HF.thetas()
    for i, R in enumerate(HF.DESC_R):
        for j, t in enumerate((0.0, th[1], th[2], th[3], th[4], th[10 + 7 * i], th[-1 - i])):
            x, y = ((w / 2 - 0.3, h / 2 + 0.2), (5.5, h - 1.5), (w - 0.4, 3.5))[j % 3]
            rows.append((x, y, (i + j) % (S + 2), (i % 8) - 1, HF.rel_for_R(R), t))
    return HF.make_records(rows)


@pytest.mark.parametrize("vlfeat", [0, 1], ids=["ubc", "vlfeat"])
def test_descriptor_det_against_numpy(oracle, vlfeat):
    """Raw accumulators within 4 counts and bytes within 1 for R = 1 .. 257 on a 36 x 515 plane (windows of one, two and three passes), at
    theta = 0, the fp32 neighbours of pi/2 .. 2 pi, peak values and random ones. The numpy side clips the window to the interior as the
    shader does; a long window does not add contributions to a bin beyond those of the 5 x 5-cell footprint, so the bound of
    tests/test_np_features.py holds unchanged (measured: raw accumulators differ by at most 1 count, no byte differs)."""
    S, w, h = 1, 36, 515
    planes = HF.field("smooth", S, h, w, 80 + h)
    pyr = _pyr(oracle, planes, 1, vlfeat=vlfeat)
    for kp in _desc_records(w, h, S):
        desc_ref, raw_ref = pyr.descriptor(0, kp)
        desc, raw = NF.descriptor(planes[int(kp["scale_idx"])], kp, kp["orientation"], vlfeat=bool(vlfeat))
        dr = int(np.abs(raw.astype(np.int64) - raw_ref.astype(np.int64)).max())
        db = int(np.abs(desc.astype(np.int32) - desc_ref.astype(np.int32)).max())
        assert dr <= 4 and db <= 1, (HF.desc_radius(kp), float(kp["orientation"]), dr, db)


def test_descriptor_positions_det_against_numpy(oracle):
    S = 3
    for (w, h, R) in ((40, 24, 129), (3, 3, 1), (3, 3, 9), (64, 48, 21)):
        planes = HF.field("smooth", S, h, w, 95)
        pyr = _pyr(oracle, planes, 1)
        pos = [(0, 0), (w - 1, h - 1), (0.25, h // 2), (w - 0.5, h // 2), (w - 0.01, h - 0.01), (w // 2, h - 0.5), (0.5, 0.5), (1.5, 2.5), (1, h // 2)]
        for i, (x, y) in enumerate(pos):
            kp = HF.make_records([(x, y, i % (S + 2), 0, HF.rel_for_R(R), (0.0, 0.7, float(f32(np.pi)), 5.9)[i % 4])])[0]
            desc_ref, raw_ref = pyr.descriptor(0, kp)
            desc, raw = NF.descriptor(planes[int(kp["scale_idx"])], kp, kp["orientation"])
            assert np.abs(raw.astype(np.int64) - raw_ref.astype(np.int64)).max() <= 4, (w, h, R, x, y)
            assert np.abs(desc.astype(np.int32) - desc_ref.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_thirteen_scales_det_against_numpy_and_libm(oracle, fp16):
    """S = 13: the launcher test's records on every scale_idx 0 .. 14 of a 16-layer octave, both stages; the numpy side is handed the layer
    the record names, so an oracle that read a neighbouring layer would show. Bounds as above."""
    S, w, h = HF.S_MAX, 40, 24
    for family, ori_seed, desc_seed, plane_seed in (("smooth", 170, 180, 172), ("periodic", 171, 181, 173)):
        for stage, seed, ps in (("orientation", ori_seed, plane_seed), ("descriptor", desc_seed, plane_seed + 10)):
            planes = HF.field(family, S, h, w, ps, fp16)
            det, libm = _pyr(oracle, planes, 1, fp16), _pyr(oracle, planes, 0, fp16)
            recs = HF.thirteen_scale_records(w, h, seed)
            assert {int(k["scale_idx"]) for k in recs} == set(range(S + 2))
            for kp in recs:
                layer = planes[int(kp["scale_idx"])]
                if stage == "orientation":
                    ang_ref, hist_ref = det.orientations(0, kp)
                    ang, hist = NF.orientations(layer, kp, max_nb_orientation=0)
                    assert np.abs(hist.astype(np.int64) - hist_ref.astype(np.int64)).max() <= 16, (family, int(kp["scale_idx"]))
                    assert len(ang) == len(ang_ref) and np.abs(ang - ang_ref).max(initial=0) < 1e-6
                    b, _ = libm.orientations(0, kp)
                    assert len(ang_ref) == len(b) and np.abs(ang_ref - b).max(initial=0) < 1e-4
                else:
                    desc_ref, raw_ref = det.descriptor(0, kp)
                    desc, raw = NF.descriptor(layer, kp, kp["orientation"])
                    assert np.abs(raw.astype(np.int64) - raw_ref.astype(np.int64)).max() <= 4, (family, int(kp["scale_idx"]))
                    assert np.abs(desc.astype(np.int32) - desc_ref.astype(np.int32)).max() <= 1
                    d = desc_ref.astype(np.int32) - libm.descriptor(0, kp)[0].astype(np.int32)
                    assert np.abs(d).max() <= 1 and np.sqrt((d.astype(np.float64) ** 2).sum()) / 512.0 < 6e-4


def test_det_against_libm(oracle, ori_case):
    """DESIGN.md §2's tolerance line on the same records: the same number of orientations, |dtheta| < 1e-4 rad; descriptors with no byte off by
    more than 1 and RMS / 512 < 6e-4"""
    planes, recs, want_r = ori_case
    det, libm = _pyr(oracle, planes, 1), _pyr(oracle, planes, 0)
    for kp in recs:
        a, _ = det.orientations(0, kp)
        b, _ = libm.orientations(0, kp)
        assert len(a) == len(b) and np.abs(a - b).max(initial=0) < 1e-4, (HF.ori_radius(kp), a, b)
    S, w, h = 1, 36, 515
    planes = HF.field("smooth", S, h, w, 80 + h)
    det, libm = _pyr(oracle, planes, 1), _pyr(oracle, planes, 0)
    for kp in _desc_records(w, h, S):
        da, _ = det.descriptor(0, kp)
        db, _ = libm.descriptor(0, kp)
        d = da.astype(np.int32) - db.astype(np.int32)
        assert np.abs(d).max() <= 1 and np.sqrt((d.astype(np.float64) ** 2).sum()) / 512.0 < 6e-4, (HF.desc_radius(kp), float(kp["orientation"]))
