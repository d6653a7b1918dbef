"""vksift_hip_orientations(_multi) and vksift_hip_descriptors(_multi)(_dense), called directly on hand-built keypoint records across the
domain their contract allows (include/vksift_hip.h) — not only on the keypoints that images happen to yield. Expected values:
orc_orientations / orc_descriptor of the CPU oracle in det math mode on a Pyramid.from_planes octave (pinned on the CPU by
tests/test_feature_reference.py), compared BYTE FOR BYTE over the whole poisoned arena of a case (tests/hip_features.py): every record, the
counter, the dense rows and the posting must equal the oracle's, and every byte the contract does not name must come back unchanged.

Every case asserts on the CPU that its records reach what the case is named for (window radius, number of passes, fast path or not,
found against cap) before the GPU is asked. Deterministic; one GPU context; default stream, one synchronisation per launch."""
import ctypes as C

import numpy as np
import pytest

import hip_features as HF

pytestmark = pytest.mark.gpu
f32 = np.float32
PI = np.pi
DESC_MAX_ROWS = 256  # features.hip: window rows per pass of k_descriptor


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HF.bind(vk.lib())


@pytest.fixture(scope="module")
def TAB(oracle):
    return HF.fp_table(oracle, 160)  # R up to 319


def _cfg(oracle, S, fp16=False, vlfeat=0):
    return oracle.default_config(math_mode=1, nb_scales_per_octave=S, pyramid_fp16=1 if fp16 else 0, use_vlfeat_format=vlfeat)


def _pyramids(oracle, planes, fp16, vlfeat=0):
    cfg = _cfg(oracle, planes.shape[1] - 3, fp16, vlfeat)
    return [oracle.Pyramid.from_planes(cfg, p) for p in planes]


def _ok(L, rc, what):
    assert rc == 0, f"{what}: returned {rc} ({L.vksift_hip_error_string(rc).decode()})"


def run_orientation(L, oracle, planes, recs, found, cap, what, *, fp16=False, max_ori=4, **geom):
    """one vksift_hip_orientations launch on a fresh arena against the oracle; returns (arena, bytes after, kept angles per image)"""
    fa = HF.FeatureArena(planes, recs, found, cap, fp16=fp16, **geom)
    job = fa.job(max_ori=max_ori)
    _ok(L, L.vksift_hip_orientations(C.byref(job), fa.batch, None), what)
    after = fa.read()
    exp, free, angles = fa.expected_orientation(_pyramids(oracle, planes, fp16), max_ori)
    fa.check(after, exp, what, free)
    return fa, after, angles


def run_descriptor(L, oracle, planes, recs, found, cap, what, *, fp16=False, vlfeat=0, dense=None, post=False, **geom):
    fa = HF.FeatureArena(planes, recs, found, cap, fp16=fp16, dense=dense, post=post, **geom)
    job = fa.job(use_vlfeat=vlfeat)
    if dense is not None or post:
        d = fa.dense_rows()
        _ok(L, L.vksift_hip_descriptors_multi_dense(C.byref(job), 1, fa.batch, C.byref(d), None), what)
    else:
        _ok(L, L.vksift_hip_descriptors(C.byref(job), fa.batch, None), what)
    after = fa.read()
    exp = fa.expected_descriptor(_pyramids(oracle, planes, fp16, vlfeat), dense=dense is not None, post=post)
    fa.check(after, exp, what)
    return fa, after


def _stack(*fields):
    return np.stack(fields)


def _theta_near(v):
    return float(f32(v))


# =================================================================================================================== orientation
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_orientation_window_sizes(L, oracle, fp16):
    """r over one, two and three passes of the fixed-point-scale loop (64 lanes per pass), the may_clamp branch, on smooth, half-black and
    (fp32) planes whose left half is scaled by 2^-60; interior and border windows; every scale_idx and octave_idx"""
    S, w, h = 1, 330, 300
    recs, want_r = HF.ori_size_records(w, h, S)
    assert [HF.ori_radius(k)[0] for k in recs] == want_r
    assert sorted({r // 64 + 1 for r in want_r}) == [1, 2, 3]                      # passes of the loop `for (cb = 0; cb <= r; cb += 64)`
    assert sum(HF.ori_radius(k)[1] < 0.08 for k in recs) == 6                      # may_clamp
    assert {int(k["scale_idx"]) for k in recs} == set(range(S + 2)) and {int(k["octave_idx"]) for k in recs} == set(range(-1, 7))
    fast = [HF.ori_fast_path(k, w, h) for k in recs]
    assert any(f and r >= 128 for f, r in zip(fast, want_r)) and any(not f and r >= 128 for f, r in zip(fast, want_r))
    fams = ("smooth", "blackhalf", "const") if fp16 else ("smooth", "blackhalf", "tiny")
    planes = _stack(*[HF.field(f, S, h, w, 11 + i, fp16) for i, f in enumerate(fams)])
    n = len(recs)
    _, after, angles = run_orientation(L, oracle, planes, [recs] * 3, [n] * 3, n + 40, "orientation window sizes", fp16=fp16, max_ori=0, pitch=w + 6)
    assert sum(len(a) > 0 for a in angles[0]) > n // 2                              # the smooth image has peaks to compare
    if fp16:
        assert all(len(a) == 0 for a, f in zip(angles[2], fast) if f)               # constant inside the image: no peak, theta stays what it was


def test_orientation_positions(L, oracle):
    """the switch of the interior fast path on each of the four sides (the last keypoint that takes it, the first that does not), the corners,
    centres that round to 0 and to w (h), fractions of exactly .5, a window larger than the plane, 3 x 3 planes"""
    S = 3
    took_fast = 0
    for (w, h, r) in ((64, 48, 5), (40, 24, 64), (40, 24, 3), (3, 3, 1), (3, 3, 0), (3, 3, 7), (17, 3, 2), (3, 19, 2)):
        rel = HF.rel_for_r(r) if r else 0.1
        pos, names = [], []
        cxm, cym = w // 2, h // 2
        # on each side: cx - r == 1 (fast, if the other sides allow) and cx - r == 0 (not fast); cx + r == w - 2 and w - 1; the same in y
        for tag, (x, y) in {"left in": (1 + r, cym), "left out": (r, cym), "right in": (w - 2 - r, cym), "right out": (w - 1 - r, cym),
                            "top in": (cxm, 1 + r), "top out": (cxm, r), "bottom in": (cxm, h - 2 - r), "bottom out": (cxm, h - 1 - r)}.items():
            if 0 <= x + 0.25 < w and 0 <= y - 0.25 < h:
                pos.append((x + 0.25, y - 0.25)), names.append(tag)
        pos += [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]                                        # corners
        pos += [(0.25, cym), (0.49, 0.49), (w - 0.5, cym), (w - 0.01, h - 0.01), (cxm, h - 0.5), (cxm, 0.3)]  # centre rounds to 0 / w / h
        pos += [(min(cxm + 0.5, w - 0.5), min(cym + 0.5, h - 0.5)), (0.5, 0.5), (1.5, 2.5)]              # roundf rounds half away
        pos = [(x, y) for (x, y) in pos if 0 <= f32(x) < w and 0 <= f32(y) < h]
        names += [""] * (len(pos) - len(names))
        recs = HF.make_records([(x, y, i % (S + 2), 0, rel, 0.0) for i, (x, y) in enumerate(pos)])
        assert all(HF.ori_radius(k)[0] == r for k in recs)
        # a keypoint on the switch takes the fast path when the window has room in the other direction too; one texel beyond it never does
        room_x, room_y = 1 + 2 * r <= w - 2, 1 + 2 * r <= h - 2
        mid_x, mid_y = cxm - r >= 1 and cxm + r <= w - 2, cym - r >= 1 and cym + r <= h - 2
        fast = [HF.ori_fast_path(k, w, h) for k in recs]
        for f, tag in zip(fast, names):
            if tag:
                along_x = tag.startswith(("left", "right"))
                assert f == (tag.endswith(" in") and (room_x and mid_y if along_x else room_y and mid_x)), (w, h, r, tag)
        took_fast += sum(f for f, tag in zip(fast, names) if tag)
        if not (room_x and room_y):
            assert not any(fast)
        if (w, h, r) == (64, 48, 5):
            assert sum(f for f, tag in zip(fast, names) if tag) == 4                  # the last fast keypoint on each of the four sides
            assert HF.round_half_away(recs[len(names) - 3]["scale_x"]) == cxm + 1
        if r == 64:
            assert 2 * r + 1 > max(w, h)
        assert {HF.round_half_away(k["scale_x"]) for k in recs} >= {0, w} and {HF.round_half_away(k["scale_y"]) for k in recs} >= {0, h}
        planes = _stack(HF.field("smooth", S, h, w, 21))
        run_orientation(L, oracle, planes, [recs], [len(recs)], len(recs) + 30, f"orientation positions {w}x{h} r={r}", max_ori=0, pitch=w + 3)
    assert took_fast == 12          # four sides each of 64 x 48 (r = 5), 40 x 24 (r = 3) and 3 x 3 (r = 0: its centre texel, the only interior one)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_orientation_thirteen_scales(L, oracle, fp16):
    """S = 13, the most a configuration may ask for: 16 layers, records on every scale_idx 0 .. 14 (the layer offset scale_idx * plane_stride
    up to its largest value), two images, both plane layouts with gaps between layers and images"""
    S, w, h = HF.S_MAX, 40, 24
    recs = [HF.thirteen_scale_records(w, h, 170 + b) for b in range(2)]
    for r in recs:
        assert {int(k["scale_idx"]) for k in r} == set(range(S + 2)) and max(HF.ori_radius(k)[0] for k in r) == 64
    planes = _stack(*[HF.field(("smooth", "periodic")[b], S, h, w, 172 + b, fp16) for b in range(2)])
    assert planes.shape[1] == 16 and len({p.tobytes() for p in planes[0]}) == 16      # every layer differs: a wrong one shows
    n = len(recs[0])
    for image_major in (False, True):
        geom = dict(pitch=w + 7, layer_gap=13, base_offset=3, image_major=True) if image_major else dict(pitch=w + 2, img_gap=37, base_offset=1)
        run_orientation(L, oracle, planes, recs, [n, n], n + 50, f"orientation S=13 image_major={image_major}", fp16=fp16, max_ori=4, **geom)


def _many(w, h, n, S, rel, seed, octave_idx=0):
    rng = np.random.default_rng(seed)
    return HF.make_records([(rng.uniform(0, w - 0.001), rng.uniform(0, h - 0.001), int(rng.integers(0, S + 2)), octave_idx, rel, 0.0) for _ in range(n)])


def test_orientation_counters_and_max_ori(L, oracle):
    """found 0, 1, cap - 1, cap, cap + 7 on entry; max_ori 0, 1, 2, 4, 18, 40 on a pattern with up to five peaks per keypoint; extras that cross cap;
    cap 1 .. 5 (grid sizing (cap + 3) / 4). One launch per max_ori holds the five counter cases as a batch of five (image-fastest grid);
    the single-image launches take the other grid order."""
    S, w, h, cap = 3, 48, 48, 12
    img = HF.field("periodic", S, h, w, 31)
    pool = HF.star_points(w, h, cap, S, 1.3, 32)
    peaks = max(len(_pyramids(oracle, img[None], False)[0].orientations(0, k)[0]) for k in pool)
    assert peaks >= 5
    founds = [0, 1, cap - 1, cap, cap + 7]
    recs = [pool[:min(f, cap)] for f in founds]
    planes = _stack(*[img] * 5)
    for max_ori in (0, 1, 2, 4, 18, 40):
        fa, after, angles = run_orientation(L, oracle, planes, recs, founds, cap, f"orientation counters max_ori={max_ori}", max_ori=max_ori,
                                            found_img_stride=3, ori_img_stride=cap + 2, feat_gap=5)
        keep = 18 if max_ori == 0 else min(max_ori, 18)
        extras = [sum(max(len(a) - 1, 0) for a in per) for per in angles]
        assert max(len(a) for per in angles for a in per) == min(peaks, keep)        # the cut is what is kept
        for b, f in enumerate(founds):
            assert fa.found_after(after, b) == f + extras[b]                         # un-clamped
        if keep > 1:
            assert founds[2] + extras[2] > cap and extras[1] > 0 and founds[1] + extras[1] <= cap  # extras cross cap / stay below it
    for f in founds:  # single image (keypoint-fastest grid)
        run_orientation(L, oracle, planes[:1], [pool[:min(f, cap)]], [f], cap, f"orientation counters found={f}", max_ori=4)
    for c in (1, 2, 3, 4, 5):
        for f in (c, c + 7):
            run_orientation(L, oracle, planes[:1], [pool[:c]], [f], c, f"orientation cap={c} found={f}", max_ori=4)


@pytest.mark.parametrize("batch", [1, 2])
def test_orientation_finalize_carry(L, oracle, batch):
    """2 500 small-window keypoints with extras: k_orientation_finalize's prefix carry over three 1024-keypoint blocks, with the appended
    copies clipped at cap in the middle of the third block's output, and without clipping"""
    S, w, h, n = 1, 64, 48, 2500
    img = HF.field("periodic", S, h, w, 41)
    planes = _stack(*[img] * batch)
    pool = HF.star_points(w, h, n, S, 0.5, 42)
    assert all(HF.ori_radius(k)[0] == 2 for k in pool[:50])
    for cap in (n + 3000, 4 * n):
        founds = [n, 1500][:batch]
        fa, after, angles = run_orientation(L, oracle, planes, [pool[:f] for f in founds], founds, cap, f"finalize carry cap={cap}", max_ori=4)
        for b in range(batch):
            ex = [max(len(a) - 1, 0) for a in angles[b]]
            assert founds[0] > 2048 and sum(ex[:1024]) > 0 and sum(ex[1024:2048]) > 0     # a carry into the second and the third block
            assert (founds[b] + sum(ex) > cap) == (cap == n + 3000 and b == 0)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("batch", [1, 3, 8, 9])
def test_orientation_batches_and_strides(L, oracle, batch, fp16):
    """batch 1 (keypoint-fastest grid), 3, 8 and 9 (image-fastest; from 8 up the grid is sized by w * h / 512 and every workgroup strides over
    several keypoints), every stride of the job non-trivial, both plane layouts"""
    S, w, h, n = 3, 40, 24, 75
    planes = _stack(*[HF.field(("smooth", "blackhalf", "periodic")[b % 3], S, h, w, 50 + b, fp16) for b in range(batch)])
    founds = [max(n - 9 * b, 0) for b in range(batch)]
    recs = [_many(w, h, f, S, (0.8, 1.7)[b % 2], 60 + b, octave_idx=b % 3) for b, f in enumerate(founds)]
    if batch >= 8:
        assert w * h // 512 < 32 and n > 2 * 32                                          # 8 workgroups of 4 keypoints per image: three sweeps
    for image_major in (False, True):
        geom = dict(pitch=w + 7, layer_gap=13, base_offset=3, image_major=True) if image_major else dict(pitch=w + 2, img_gap=37, base_offset=1)
        run_orientation(L, oracle, planes, recs, founds, n + 60, f"orientation batch {batch} image_major={image_major}", fp16=fp16, max_ori=3,
                        feat_gap=11, found_img_stride=5, ori_img_stride=n + 67, sec_index=2, nsec=4,
                        front=[[7, 9, 0, 3]] * batch, **geom)


def _three_jobs(oracle, fp16, seed):
    S = 3
    out = []
    for i, (w, h, n, cap) in enumerate(((40, 24, 30, 90), (97, 61, 55, 70), (17, 33, 9, 9))):
        planes = _stack(*[HF.field(("smooth", "periodic")[(i + b) % 2], S, h, w, seed + 10 * i + b, fp16) for b in range(3)])
        recs = [_many(w, h, n, S, 0.9 + 0.6 * i, seed + 100 + 10 * i + b, octave_idx=i) for b in range(3)]
        for r in recs:
            r["orientation"] = np.random.default_rng(seed + i).uniform(0, 2 * PI, len(r)).astype(f32)
        out.append((planes, recs, [n] * 3, cap))
    return out


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_multi_against_three_single_calls(L, oracle, TAB, fp16):
    """_multi with three jobs of different sizes in one call: the same bytes as three single calls, and both are the oracle's"""
    specs = _three_jobs(oracle, fp16, 70)
    for stage in ("orientation", "descriptor"):
        multi = [HF.FeatureArena(p, r, f, c, fp16=fp16, pitch=p.shape[3] + 1, tab=TAB) for (p, r, f, c) in specs]
        single = [HF.FeatureArena(p, r, f, c, fp16=fp16, pitch=p.shape[3] + 1, tab=TAB) for (p, r, f, c) in specs]
        jobs = (HF.OctaveJob * 3)(*[fa.job(max_ori=4) for fa in multi])
        if stage == "orientation":
            _ok(L, L.vksift_hip_orientations_multi(jobs, 3, 3, None), "orientations_multi")
            for fa in single:
                j = fa.job(max_ori=4)
                _ok(L, L.vksift_hip_orientations(C.byref(j), 3, None), "orientations")
        else:
            _ok(L, L.vksift_hip_descriptors_multi(jobs, 3, 3, None), "descriptors_multi")
            for fa in single:
                j = fa.job(max_ori=4)
                _ok(L, L.vksift_hip_descriptors(C.byref(j), 3, None), "descriptors")
        for i, (fm, fs) in enumerate(zip(multi, single)):
            am, as_ = fm.read(), fs.read()
            pyr = _pyramids(oracle, specs[i][0], fp16)
            if stage == "orientation":
                exp, free, _ = fm.expected_orientation(pyr, 4)
                fm.check(am, exp, f"orientations_multi job {i}", free)
            else:
                free = None
                fm.check(am, fm.expected_descriptor(pyr), f"descriptors_multi job {i}")
            fs.check(as_, am, f"{stage}: single call of job {i} against the multi call", free)


# =================================================================================================================== descriptor
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_descriptor_window_sizes_and_passes(L, oracle, TAB, fp16):
    """R from 1 (table index 0) to 257; plane heights that give clipped window heights of 0, 1, 255, 256, 257, 511, 512 and 513 rows: no pass,
    one, two and three passes of k_descriptor's row-span loop, incl. a pass of exactly DESC_MAX_ROWS rows and a pass of a single row"""
    S, w = 1, 36
    seen_bh, seen_R = set(), set()
    for h in (3, 257, 258, 259, 513, 514, 515):
        rows = []
        for i, R in enumerate(HF.DESC_R):
            th = (0.0, 1.1, _theta_near(PI / 2), 4.0)[i % 4]
            rows.append((w / 2 - 0.3, h / 2 + 0.2, i % (S + 2), (i % 8) - 1, HF.rel_for_R(R), th))   # centred: the whole height when R allows
            rows.append((5.5, h - 1.5, (i + 1) % (S + 2), 0, HF.rel_for_R(R), th + 0.5))                 # at the bottom border
        rows.append((w / 2, h - 0.2, 0, 0, HF.rel_for_R(1), 0.3))                                        # centre rounds to h, R = 1: no row at all
        recs = HF.make_records(rows)
        assert [HF.desc_radius(k) for k in recs[:-1:2]] == HF.DESC_R and HF.desc_radius(recs[-1]) == 1
        assert HF.desc_rows(recs[-1], w, h)[1] <= 0
        seen_bh |= {HF.desc_rows(k, w, h)[1] for k in recs}
        seen_R |= {HF.desc_radius(k) for k in recs}
        planes = _stack(HF.field("smooth", S, h, w, 80 + h, fp16))
        run_descriptor(L, oracle, planes, [recs], [len(recs)], len(recs) + 2, f"descriptor windows h={h}", fp16=fp16, tab=TAB, pitch=w + 4)
    assert seen_bh >= {0, 1, 255, 256, 257, 511, 512, 513} and seen_R == set(HF.DESC_R)
    passes = {-(-bh // DESC_MAX_ROWS) for bh in seen_bh if bh > 0}
    assert passes == {1, 2, 3}
    assert HF.desc_radius(recs[0]) // 2 == 0 and TAB[0] == 65536                    # R = 1: table index 0


@pytest.mark.parametrize("vlfeat", [0, 1], ids=["ubc", "vlfeat"])
def test_descriptor_orientations_and_families(L, oracle, TAB, vlfeat):
    """theta = 0 (ksin == 0 exactly: the row spans' else-branch), the fp32 neighbours of pi/2, pi, 3pi/2, 2pi, all 72 values a peak can take,
    random ones; on smooth, half-black, left half scaled by 2^-60 (general-form fallback) and constant planes (norm 0: all-zero bytes); UBC and VLFeat"""
    S, w, h = 3, 72, 56
    th = HF.thetas()
    assert th[0] == 0.0 and oracle.lib().orc_dm_sinf(0.0) == 0.0 and len(th) == 1 + 9 + 72 + 24 and max(th) <= float(f32(2 * PI))
    rng = np.random.default_rng(91)
    rows = [(rng.uniform(8, w - 8), rng.uniform(8, h - 8), i % (S + 2), 1, (0.6, 1.0, 2.0)[i % 3], t) for i, t in enumerate(th)]
    recs = HF.make_records(rows)
    fams = ("smooth", "blackhalf", "tiny", "const")
    planes = _stack(*[HF.field(f, S, h, w, 92 + i) for i, f in enumerate(fams)])
    n = len(recs)
    fa, after = run_descriptor(L, oracle, planes, [recs] * 4, [n] * 4, n, f"descriptor orientations vlfeat={vlfeat}", vlfeat=vlfeat, tab=TAB, pitch=w + 1)
    assert not fa.records(after, 3, n)["descriptor"].any()                          # constant plane
    assert fa.records(after, 2, n)["descriptor"].any(axis=1).sum() > n // 3         # windows that reach the unscaled half describe it
    assert 0 < np.abs(planes[2][:, :, :w // 2]).max() < 2.0 ** -59                   # gradients below 2^-48: the short forms' guard trips


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_descriptor_positions(L, oracle, TAB, fp16):
    """corners, borders, centres that round to 0 and to w (h), fractions of .5, windows larger than the plane, 3 x 3 planes; empty windows
    (dx1 < dx0 or bh <= 0) leave all-zero descriptors"""
    S = 3
    empty = 0
    for (w, h, R) in ((40, 24, 129), (40, 24, 6), (3, 3, 1), (3, 3, 2), (3, 3, 9), (17, 3, 4), (3, 19, 4), (64, 48, 21)):
        cxm, cym = w // 2, h // 2
        pos = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (0.25, cym), (0.49, 0.49), (w - 0.5, cym), (w - 0.01, h - 0.01), (cxm, h - 0.5),
               (cxm, 0.3), (min(cxm + 0.5, w - 0.5), min(cym + 0.5, h - 0.5)), (0.5, 0.5), (1.5, 2.5), (1, cym), (w - 2, cym), (cxm, 1), (cxm, h - 2)]
        pos = [(x, y) for (x, y) in pos if 0 <= f32(x) < w and 0 <= f32(y) < h]
        ths = [0.0, 0.7, _theta_near(PI), 5.9]
        recs = HF.make_records([(x, y, i % (S + 2), 0, HF.rel_for_R(R), ths[i % 4]) for i, (x, y) in enumerate(pos)])
        assert all(HF.desc_radius(k) == R for k in recs)
        empty += sum(min(HF.desc_rows(k, w, h)) <= 0 for k in recs)
        planes = _stack(HF.field("smooth", S, h, w, 95, fp16))
        run_descriptor(L, oracle, planes, [recs], [len(recs)], len(recs) + 1, f"descriptor positions {w}x{h} R={R}", fp16=fp16, tab=TAB, pitch=w + 5)
    assert empty >= 4


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("batch", [1, 3, 8, 9])
def test_descriptor_batches_and_strides(L, oracle, TAB, batch, fp16):
    """batch 1 and 3 (four waves per keypoint), 8 and 9 (two waves, grid sized by w * h / 512: workgroups stride over keypoints); found below,
    at and above cap per image; every stride non-trivial; both plane layouts"""
    S, w, h, cap = 3, 40, 24, 70
    planes = _stack(*[HF.field(("smooth", "blackhalf", "periodic")[b % 3], S, h, w, 100 + b, fp16) for b in range(batch)])
    founds = [(cap + 7, cap, cap - 1, 1, 0, 40, 69, 77, 33)[b] for b in range(batch)]
    recs = []
    for b, f in enumerate(founds):
        r = _many(w, h, min(f, cap), S, (0.8, 1.7)[b % 2], 110 + b, octave_idx=b % 3)
        r["orientation"] = np.random.default_rng(120 + b).uniform(0, 2 * PI, len(r)).astype(f32)
        recs.append(r)
    if batch >= 8:
        assert w * h // 512 < 32 < cap
    for image_major in (False, True):
        geom = dict(pitch=w + 7, layer_gap=13, base_offset=3, image_major=True) if image_major else dict(pitch=w + 2, img_gap=37, base_offset=1)
        run_descriptor(L, oracle, planes, recs, founds, cap, f"descriptor batch {batch} image_major={image_major}", fp16=fp16, tab=TAB, vlfeat=batch % 2,
                       feat_gap=11, found_img_stride=5, sec_index=1, nsec=3, front=[[4, 0, 9]] * batch, **geom)
    for c in (1, 2, 3, 4, 5):
        for f in (0, 1, c - 1, c, c + 7):
            run_descriptor(L, oracle, planes[:1], [recs[0][:min(f, c)]], [f], c, f"descriptor cap={c} found={f}", fp16=fp16, tab=TAB)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_descriptor_thirteen_scales(L, oracle, TAB, fp16):
    """S = 13: 16 layers, records on every scale_idx 0 .. 14, two images, both plane layouts with gaps between layers and images"""
    S, w, h = HF.S_MAX, 40, 24
    recs = [HF.thirteen_scale_records(w, h, 180 + b) for b in range(2)]
    for r in recs:
        assert {int(k["scale_idx"]) for k in r} == set(range(S + 2)) and max(HF.desc_radius(k) for k in r) > max(w, h)
    planes = _stack(*[HF.field(("smooth", "periodic")[b], S, h, w, 182 + b, fp16) for b in range(2)])
    assert planes.shape[1] == 16 and len({p.tobytes() for p in planes[0]}) == 16
    n = len(recs[0])
    for image_major in (False, True):
        geom = dict(pitch=w + 7, layer_gap=13, base_offset=3, image_major=True) if image_major else dict(pitch=w + 2, img_gap=37, base_offset=1)
        run_descriptor(L, oracle, planes, recs, [n, n], n, f"descriptor S=13 image_major={image_major}", fp16=fp16, tab=TAB, vlfeat=int(image_major), **geom)


# =================================================================================================================== dense rows, posting
def _dense_case(batch, fp16, seed, n=23):
    S, w, h = 3, 40, 24
    planes = _stack(*[HF.field("smooth", S, h, w, seed + b, fp16) for b in range(batch)])
    recs = []
    for b in range(batch):
        r = _many(w, h, n, S, 1.1, seed + 20 + b)
        r["orientation"] = np.random.default_rng(seed + 40 + b).uniform(0, 2 * PI, n).astype(f32)
        recs.append(r)
    return planes, recs


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_dense_rows(L, oracle, TAB, batch):
    """the matcher's dense rows: row offset behind the sections in front (their counters below and above their capacities), rows, norms
    (= sum (byte - 128)^2), n; sec_index 0 and 2; non-trivial strides; four-wave (batch 1, 3) and two-wave (8) kernels"""
    n = 23
    planes, recs = _dense_case(batch, False, 130, n)
    for sec_index, caps, counters in ((0, [30, 10, 10], [n, 5, 17]), (2, [10, 12, 30], [4, 50, n]), (2, [10, 12, 20], [13, 3, n + 6])):
        stored = [min(c, k) for c, k in zip(counters, caps)]
        assert sum(stored[:sec_index]) > 0 or sec_index == 0
        assert any(c > k for c, k in zip(counters, caps)) and any(c < k for c, k in zip(counters, caps))
        cap = caps[sec_index]
        found = counters[sec_index]
        rr = [r[:min(found, cap)] for r in recs]
        fa, after = run_descriptor(L, oracle, planes, rr, [found] * batch, cap, f"dense rows batch {batch} sec {sec_index}", tab=TAB, dense=caps,
                                   sec_index=sec_index, nsec=3, front=[counters] * batch, found_img_stride=4, dense_strides=(3, 5, 2, 0))
        if sec_index == 0:
            assert fa.words(after, fa.d_n)[0] == sum(stored)


@pytest.mark.parametrize("total", [0, 1])
def test_dense_rows_q6_zero_fill(L, oracle, TAB, total):
    """a buffer with fewer than two features: the rows below 2 are zero-filled and their norms are 128^3 (quirk Q6)"""
    planes, recs = _dense_case(2, False, 140, 1)
    fa, after = run_descriptor(L, oracle, planes, [r[:total] for r in recs], [total] * 2, 5, f"Q6 total {total}", tab=TAB, dense=[5, 4],
                               sec_index=0, nsec=2, front=[[total, 0]] * 2, found_img_stride=2, dense_strides=(1, 1, 1, 0))
    norms = fa.words(after, fa.d_norm)
    assert norms[1] == 128 ** 3 and (norms[0] == 128 ** 3) == (total == 0)
    assert not after[fa.d_desc.off + 128 * total:fa.d_desc.off + 256].any()


@pytest.mark.parametrize("rows", [False, True], ids=["post", "post+rows"])
def test_posting(L, oracle, TAB, rows):
    """feature posting of a single image: 41 words per record at the section's row offset, and the section counters beside them"""
    n = 23
    planes, recs = _dense_case(1, False, 150, n)
    for sec_index, caps, counters in ((0, [30, 10], [n, 5]), (1, [10, 30], [14, n])):
        fa, after = run_descriptor(L, oracle, planes, recs, [n], caps[sec_index], f"posting sec {sec_index} rows={rows}", tab=TAB,
                                   dense=caps if rows else None, post=True, sec_index=sec_index, nsec=2, front=[counters], dense_strides=(0, 0, 0, 7))
        if sec_index == 0:
            assert fa.words(after, fa.d_found_post).tolist() == counters


def test_refusals_launch_nothing(L, oracle, TAB):
    """posting with batch >= 8, nsec 0 or 17, sec_index >= nsec: hipErrorInvalidValue and not a byte of the arena changes"""
    planes, recs = _dense_case(8, False, 160, 5)
    fa = HF.FeatureArena(planes, recs, [5] * 8, 6, tab=TAB, dense=[6, 6], post=True, sec_index=1, nsec=2, front=[[3, 5]] * 8, found_img_stride=2)
    job = fa.job()

    def refused(d, batch, what):
        rc = L.vksift_hip_descriptors_multi_dense(C.byref(job), 1, batch, C.byref(d), None)
        assert rc == HF.HIP_ERROR_INVALID_VALUE, (what, rc)
        after = fa.read()
        fa.check(after, fa.host, what + ": refused, yet the arena changed")

    refused(fa.dense_rows(), 8, "posting with batch 8")
    refused(fa.dense_rows(), 9, "posting with batch 9")
    refused(fa.dense_rows(nsec=0), 1, "nsec 0")
    refused(fa.dense_rows(nsec=17), 1, "nsec 17")
    refused(fa.dense_rows(nsec=1), 1, "sec_index >= nsec")
    d = fa.dense_rows()
    d.post = None  # rows only: batch 8 is served
    _ok(L, L.vksift_hip_descriptors_multi_dense(C.byref(job), 1, 8, C.byref(d), None), "rows with batch 8")
    fa.post = False
    fa.check(fa.read(), fa.expected_descriptor(_pyramids(oracle, planes, False), dense=True), "rows with batch 8")


# =================================================================================================================== the public API
def long_window_image(w=448, h=416):
    """four broad blobs of either sign on a bright ground, plus a faint texture that gives the long windows gradients everywhere"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 200 + 6 * np.cos(xx / 5.0) * np.cos(yy / 7.0)
    for (cx, cy, bs, a) in ((0.52 * w, 0.48 * h, 10, -150), (0.2 * w, 0.25 * h, 9, 50), (0.8 * w, 0.8 * h, 11, -120), (0.15 * w, 0.8 * h, 12, 45)):
        img = img + a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * bs ** 2))
    return np.clip(img, 0, 255).astype(np.uint8)


LONG_CFG = dict(nb_scales_per_octave=1, seed_scale_sigma=8.0, use_input_upsampling=0, nb_octaves=1, intensity_threshold=0.005)


def long_window_reference(oracle, fp16=False):
    cfg = oracle.default_config(math_mode=1, pyramid_fp16=1 if fp16 else 0, **LONG_CFG)
    img = long_window_image()
    ref, counts = oracle.detect(cfg, img)
    return cfg, img, ref, counts


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_long_windows_through_the_public_api(vk, oracle, fp16):
    """S = 1 with seed_scale_sigma = 8: a keypoint's sigma relative to its octave reaches 21 (the stock configurations stay below 10), its
    orientation window r = 96 and its descriptor window R = 226, clipped to 414 rows: two passes of both loops, as a user reaches them.
    vksift_detectFeatures byte for byte against the oracle, as test_gpu_extraction_limits._assert_same does"""
    from test_gpu_extraction_limits import _assert_same

    cfg, img, ref, counts = long_window_reference(oracle, fp16)
    h, w = img.shape
    assert len(ref) == sum(counts) >= 1
    assert max(HF.ori_radius(k)[0] for k in ref) >= 64
    assert any(HF.desc_radius(k) >= 128 and HF.desc_rows(k, w, h)[1] > DESC_MAX_ROWS for k in ref)
    vcfg = vk.default_config(input_image_max_size=w * h, pyramid_precision_mode=1 if fp16 else 0, use_input_upsampling=False,
                             **{k: v for k, v in LONG_CFG.items() if k != "use_input_upsampling"})
    with vk.Instance(vcfg) as inst:
        inst.detectFeatures(img, 0)
        _assert_same(inst, 0, ref, "long windows")
