"""Pair mode of the two-wave descriptor launch (features.hip k_descriptor<2, ...>, batches of 8 and more): a workgroup owns keypoints 2 kb and
2 kb + 1 of a sweep; where both windows have R <= VKSIFT_TUNE_DESC_SOLO_R each wave describes one of them alone (solo), otherwise both waves
describe the two one after the other (team). The histogram sums are integer adds, so the bytes may not depend on the mode.

vksift_hip_descriptors(_multi_dense) on hand-built keypoint lists in batches of 8, on the arena of tests/hip_features.py: every case is compared
BYTE FOR BYTE over its whole poisoned arena with orc_descriptor of the CPU oracle (det math mode), at knob values 0 (no solo keypoint: the
launch of the four-wave form's mapping), the built-in value and 63 (every keypoint up to the largest R a half of the row arrays can hold),
with the matcher's dense rows on and off. The expected arena of a case is computed once and shared by its six launches.

Every case asserts on the CPU, from the records alone, which mode each of its pairs takes at each knob value, so the cases keep reaching the
boundary they are named for whatever the built-in value becomes."""
import ctypes as C

import numpy as np
import pytest

import hip_features as HF

pytestmark = pytest.mark.gpu
f32 = np.float32
PI = np.pi
TUNE_DESC_SOLO_R = 14      # VKSIFT_TUNE_DESC_SOLO_R of include/vksift_hip.h
SOLO_MAX_R = 63            # features.hip DESC_SOLO_MAX_R: 2 R + 1 rows fit half of the row arrays
HALF_ROWS = 128            # DESC_MAX_ROWS / 2
BATCH = 8                  # the smallest batch that takes the two-wave form
S = 1


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HF.bind(vk.lib())


@pytest.fixture(scope="module")
def TAB(oracle):
    return HF.fp_table(oracle, 40)  # R up to 79


@pytest.fixture(scope="module")
def BUILT_IN(L):
    v = L.vksift_hip_tune_get(TUNE_DESC_SOLO_R)
    assert 0 <= v <= SOLO_MAX_R
    return v


def knob_values(built_in):
    return sorted({0, built_in, SOLO_MAX_R})


def boundaries(built_in):
    """the radii at which some knob value under test switches the mode"""
    return sorted({built_in, SOLO_MAX_R} - {0})


def stride(w, h, cap, solo_r):
    """keypoints per sweep of an image's share of the grid (features.hip octave_blocks, batch >= 8)"""
    dense = max(w * h // 512, 32)
    per = 2 if solo_r else 1
    return per * max((min(cap, dense) + per - 1) // per, 1)


def modes(recs, solo_r):
    """the mode of every pair (k0, k0 + 1) of the first len(recs) records of an image: 'solo' / 'team'; an odd last keypoint: 'team'"""
    if solo_r == 0:
        return ["team"] * len(recs)
    out = []
    for k0 in range(0, len(recs), 2):
        pair = recs[k0:k0 + 2]
        out.append("solo" if len(pair) == 2 and all(HF.desc_radius(k) <= min(solo_r, SOLO_MAX_R) for k in pair) else "team")
    return out


def planes_of(w, h, seed):
    fams = ("smooth", "blackhalf", "periodic")
    return np.stack([HF.field(fams[b % 3], S, h, w, seed + b) for b in range(BATCH)])


def records(rows):
    """rows of (x, y, R, theta)"""
    recs = HF.make_records([(x, y, i % (S + 2), i % 3, HF.rel_for_R(R), th) for i, (x, y, R, th) in enumerate(rows)])
    assert [HF.desc_radius(k) for k in recs] == [r[2] for r in rows]
    return recs


def run_case(L, oracle, TAB, built_in, planes, recs, founds, cap, what, **geom):
    """the case at every knob value, dense rows off and on; the knob goes back to what it was"""
    cfg = oracle.default_config(math_mode=1, nb_scales_per_octave=S)
    pyr = [oracle.Pyramid.from_planes(cfg, p) for p in planes]
    before = L.vksift_hip_tune_get(TUNE_DESC_SOLO_R)
    try:
        for dense in (None, [cap + 3, cap]):
            kw = dict(geom)
            if dense is not None:
                kw.update(dense=dense, sec_index=1, nsec=2, front=[[5 + b, 0] for b in range(BATCH)], found_img_stride=3, dense_strides=(1, 2, 1, 0))
            exp = None
            for knob in knob_values(built_in):
                fa = HF.FeatureArena(planes, recs, founds, cap, tab=TAB, **kw)
                if exp is None:
                    exp = fa.expected_descriptor(pyr, dense=dense is not None)
                job = fa.job()
                assert L.vksift_hip_tune(TUNE_DESC_SOLO_R, knob) == 0
                if dense is not None:
                    d = fa.dense_rows()
                    rc = L.vksift_hip_descriptors_multi_dense(C.byref(job), 1, BATCH, C.byref(d), None)
                else:
                    rc = L.vksift_hip_descriptors(C.byref(job), BATCH, None)
                assert rc == 0, (what, knob, rc)
                fa.check(fa.read(), exp, f"{what}, knob {knob}, dense rows {'on' if dense else 'off'}")
    finally:
        L.vksift_hip_tune(TUNE_DESC_SOLO_R, before)


def _interior(rng, w, h, n, margin=3.0):
    return [(rng.uniform(margin, w - margin), rng.uniform(margin, h - margin)) for _ in range(n)]


def test_counts_per_image(L, oracle, TAB, BUILT_IN):
    """64 x 64: images with 0, 1, 2, 3 keypoints, an odd count above the stride of either mapping, an even one, exactly one sweep, and a count
    above the section capacity; small and large windows mixed, so that the workgroups of one launch take different modes"""
    w, h, cap = 64, 64, 70
    assert stride(w, h, cap, 0) == 32 and stride(w, h, cap, SOLO_MAX_R) == 32
    founds = [0, 1, 2, 3, 35, 66, 32, cap + 9]
    assert founds[4] % 2 == 1 and founds[4] > 32 and founds[7] > cap
    rng = np.random.default_rng(300)
    radii = [3, 7] + [r for b in boundaries(BUILT_IN) for r in (b, b + 1)]
    recs = []
    for b, f in enumerate(founds):
        n = min(f, cap)
        rows = [(x, y, radii[int(rng.integers(0, len(radii)))], rng.uniform(0, 2 * PI)) for (x, y) in _interior(rng, w, h, n)]
        recs.append(records(rows))
    for knob in knob_values(BUILT_IN):
        seen = {m for r in recs for m in modes(r, knob)}
        assert seen == ({"team"} if knob == 0 else {"solo", "team"}), (knob, seen)
    assert modes(recs[4], SOLO_MAX_R)[-1] == "team" and len(modes(recs[4], SOLO_MAX_R)) == 18      # the odd last keypoint
    run_case(L, oracle, TAB, BUILT_IN, planes_of(w, h, 310), recs, founds, cap, "counts per image", pitch=w + 3, feat_gap=7)


def test_pairs_around_the_threshold(L, oracle, TAB, BUILT_IN):
    """200 x 120: for every radius b at which a knob value under test switches the mode, the pairs (b, b), (b + 1, b), (b, b + 1) and
    (b + 1, b + 1), in that order in image 0, shifted by one keypoint in image 1 (the same keypoints meet other partners), reversed in image 2;
    mode changes between consecutive sweeps of a workgroup in both directions (images 3 and 4: the pairs alternate with the stride)"""
    w, h, cap = 200, 120, 120
    st = stride(w, h, cap, SOLO_MAX_R)
    assert st == 46 and stride(w, h, cap, 0) == 46
    rng = np.random.default_rng(320)
    quad = []
    for b in boundaries(BUILT_IN):
        quad += [b, b, b + 1, b, b, b + 1, b + 1, b + 1]

    def rows_of(radii, centred=False):
        pos = [(w / 2 + rng.uniform(-20, 20), h / 2 + rng.uniform(-8, 8)) for _ in radii] if centred else _interior(rng, w, h, len(radii))
        return [(x, y, R, rng.uniform(0, 2 * PI)) for (x, y), R in zip(pos, radii)]

    small, large = 4, SOLO_MAX_R + 1
    alt_a = [small if (k // st) % 2 == 0 else large for k in range(2 * st + 6)]       # solo in sweep 0, team in sweep 1, solo in sweep 2
    alt_b = [large if (k // st) % 2 == 0 else small for k in range(2 * st + 5)]       # team, solo, team; odd count
    lists = [quad, [small] + quad, quad[::-1], alt_a, alt_b, quad + [small], [large, small] * 9, [small] * 11]
    recs = [records(rows_of(r, centred=i < 3)) for i, r in enumerate(lists)]
    founds = [len(r) for r in recs]
    for i, b in zip(range(0, len(quad), 8), boundaries(BUILT_IN)):
        assert modes(recs[0][i:i + 8], b) == ["solo", "team", "team", "team"]           # both just under / one over, either order / both over
        assert modes(recs[0][i:i + 8], b + 1 if b < SOLO_MAX_R else b) == (["solo"] * 4 if b < SOLO_MAX_R else ["solo", "team", "team", "team"])
    m = modes(recs[3], SOLO_MAX_R)
    assert m[0] == "solo" and m[st // 2] == "team" and m[st] == "solo"                   # one workgroup: solo -> team -> solo
    m = modes(recs[4], SOLO_MAX_R)
    assert m[0] == "team" and m[st // 2] == "solo" and m[st] == "team" and founds[4] % 2 == 1
    run_case(L, oracle, TAB, BUILT_IN, planes_of(w, h, 330), recs, founds, cap, "pairs around the threshold", pitch=w + 1, img_gap=29, base_offset=1)


@pytest.mark.parametrize("size", [(64, 64), (200, 120)], ids=["64x64", "200x120"])
def test_solo_windows_clipped_by_the_border(L, oracle, TAB, BUILT_IN, size):
    """solo keypoints whose window is cut by the left, right, top and bottom border, by two of them at each corner, and (64 x 64, R = 63) by
    all four; every pair is solo at the knob values that allow its radius"""
    w, h = size
    R = 12
    pos = [(2.3, h / 2), (w - 3.4, h / 2), (w / 2, 1.6), (w / 2, h - 2.7), (1.2, 1.4), (w - 2.2, 2.0), (3.0, h - 1.6), (w - 1.7, h - 2.2),
           (0.2, h / 2), (w - 0.6, h / 2 + 0.5), (w / 2 + 0.5, 0.3), (w / 2, h - 0.51)]
    rows = [(x, y, R, 0.4 * i) for i, (x, y) in enumerate(pos)]
    rows += [(w / 2 - 0.3, h / 2 + 0.2, SOLO_MAX_R, 1.0), (w / 2 + 4.1, h / 2 - 3.0, SOLO_MAX_R, 2.5)]
    recs0 = records(rows)
    for k in recs0[:8]:
        bw, bh = HF.desc_rows(k, w, h)
        assert 0 < min(bw, bh) and (bw < 2 * R + 1 or bh < 2 * R + 1)                    # clipped, not empty
    sides = [(HF.round_half_away(k["scale_x"]), HF.round_half_away(k["scale_y"])) for k in recs0[:4]]
    assert sides[0][0] - R < 1 and sides[1][0] + R > w - 2 and sides[2][1] - R < 1 and sides[3][1] + R > h - 2
    if size == (64, 64):
        assert HF.desc_rows(recs0[-1], w, h) == (w - 2, h - 2)                            # all four sides
    assert modes(recs0, SOLO_MAX_R) == ["solo"] * 7
    recs = [recs0[:len(recs0) - b] for b in range(BATCH)]
    run_case(L, oracle, TAB, BUILT_IN, planes_of(w, h, 340 + w), recs, [len(r) for r in recs], len(recs0) + 2, f"clipped solo windows {w}x{h}", pitch=w + 5)


def test_solo_window_of_the_most_rows(L, oracle, TAB, BUILT_IN):
    """R = 63, the largest solo radius, unclipped in y on a 72 x 131 plane: 2 R + 1 = 127 rows, the most a solo wave's half of the row arrays is
    asked to hold (128 entries; its prefix array takes one more), beside windows of 126 rows, and R = 64 in team mode"""
    w, h = 72, 131
    rows = [(w / 2 - 0.2, 65.1, SOLO_MAX_R, 0.3), (w / 2 + 3.3, 64.8, SOLO_MAX_R, 4.0), (20.5, 64.0, SOLO_MAX_R, 1.2), (50.0, 67.0, SOLO_MAX_R, 5.5),
            (w / 2, 65.0, SOLO_MAX_R + 1, 2.2), (w / 2 + 1, 65.0, SOLO_MAX_R, 0.0)]
    recs0 = records(rows)
    bh = [HF.desc_rows(k, w, h)[1] for k in recs0]
    assert bh[:3] == [2 * SOLO_MAX_R + 1] * 3 == [HALF_ROWS - 1] * 3 and bh[3] == 126 and bh[4] == h - 2 > HALF_ROWS
    assert modes(recs0, SOLO_MAX_R) == ["solo", "solo", "team"] and modes(recs0, SOLO_MAX_R - 1) == ["team"] * 3
    recs = [recs0[:(6, 2, 4, 5, 1, 6, 3, 0)[b]] for b in range(BATCH)]
    run_case(L, oracle, TAB, BUILT_IN, planes_of(w, h, 360), recs, [len(r) for r in recs], 6, "127-row solo windows", pitch=w + 2)


def test_section_capacity_clamp(L, oracle, TAB, BUILT_IN):
    """found above cap, with cap odd and below one sweep, at it, and above it: the keypoints at and beyond cap do not exist; the last one
    below an odd cap has no partner (team) although the record behind it is poison"""
    w, h = 64, 64
    rng = np.random.default_rng(380)
    for cap in (5, 31, 32, 45):
        founds = [cap + 7, cap, cap + 1, cap - 1, 2 * cap, 0, 1, cap + 100]
        recs = [records([(x, y, (4, 9)[i % 2], rng.uniform(0, 2 * PI)) for i, (x, y) in enumerate(_interior(rng, w, h, min(f, cap)))]) for f in founds]
        if cap % 2:
            assert modes(recs[0], SOLO_MAX_R)[-1] == "team" and modes(recs[0], SOLO_MAX_R)[0] == "solo"
        run_case(L, oracle, TAB, BUILT_IN, planes_of(w, h, 390), recs, founds, cap, f"section capacity {cap}", pitch=w)
