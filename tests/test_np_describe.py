"""The placement rule of caller-supplied keypoints (tests/np_describe.py; vksift_hip_place_keypoints restates it on the GPU) on the CPU:
the round trip on the golden feature sets — placing a detected feature's (x, y, sigma) gives back the octave, scale and position it was
detected at — the admissibility edges, the clamps at both ends of the octave list, input order, capacity and counters, and the size of the
public keypoint struct."""
import os
import subprocess

import numpy as np
import pytest

import hip_place as HPL
import np_describe as ND

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
f32, u32 = np.float32, np.uint32

# name -> (image w, h, up-sampling, S)
SETS = {
    "feats_192x144_default_np": (192, 144, True, 3),
    "feats_160x120_default_det": (160, 120, True, 3),
    "feats_192x144_s2_np": (192, 144, True, 2),
    "feats_192x144_noups_vlfeat_np": (192, 144, False, 3),
}
SEED_SIGMA = 1.6
ROUND_TRIP_MIN = 0.90   # the share that must come back; the rest moved more than half a scale in the refinement


def as_keypoints(feats):
    kps = np.zeros(len(feats), ND.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["sigma"], kps["orientation"], kps["response"] = feats["x"], feats["y"], feats["sigma"], feats["orientation"], feats["intensity"]
    return kps


def reproducible(feats, w, h, ups, S, keep_orientation=True):
    """bool per feature: (the placement of its (x, y, sigma) is admissible and gives its octave_idx and scale_idx back, it gives scale_x and
    scale_y back in every bit). keep_orientation: admissible for VKSIFT_EXT_DESCRIBE_GIVEN, which also wants 0 <= orientation <= 2 pi — a
    detection's angle of the last histogram bin can exceed (float)(2 pi) by a few ulps, and such a feature is not taken back."""
    octs = ND.octaves_for(w, h, ups)
    c = ND.classify(as_keypoints(feats), octs, ND.sigma_steps(SEED_SIGMA, S), keep_orientation)
    oi = np.array([octs[o][2] for o in c["oct"]], np.int32)
    same_cell = c["adm"] & (oi == feats["octave_idx"]) & (c["scale_idx"] == feats["scale_idx"])
    same_pos = (c["scale_x"].view(u32) == feats["scale_x"].view(u32)) & (c["scale_y"].view(u32) == feats["scale_y"].view(u32))
    return same_cell, same_pos


@pytest.mark.parametrize("name", list(SETS))
def test_round_trip_on_the_golden_sets(name):
    w, h, ups, S = SETS[name]
    feats = np.load(os.path.join(GOLD, name + ".npy"))
    octs = ND.octaves_for(w, h, ups)
    od, sd = ND.classify_double(feats["sigma"], octs, SEED_SIGMA, S)
    cell_d = (np.array([octs[o][2] for o in od]) == feats["octave_idx"]) & (sd == feats["scale_idx"])
    for keep in (False, True):
        same_cell, same_pos = reproducible(feats, w, h, ups, S, keep)
        print(f"{name}: {len(feats)} features, keep_orientation {keep}: fp32 table {100 * same_cell.mean():.1f} %, double-precision rule {100 * cell_d.mean():.1f} %")
        assert same_cell.mean() >= ROUND_TRIP_MIN, (name, keep, same_cell.mean())
        # the power-of-two scaling is exact: every reproduced feature gets its position back in every bit
        assert same_pos[same_cell].all()
        # every feature of the sets lies inside its octave and inside the window range: without the orientation test, the table names
        # the same cell as the double-precision rule for each of them
        if not keep:
            assert np.array_equal(same_cell, cell_d)


def test_octaves_of_the_golden_images():
    assert ND.octaves_for(192, 144, True) == [(384, 288, -1), (192, 144, 0), (96, 72, 1), (48, 36, 2)]
    assert ND.octaves_for(160, 120, True) == [(320, 240, -1), (160, 120, 0), (80, 60, 1)]
    assert ND.octaves_for(192, 144, False) == [(192, 144, 0), (96, 72, 1), (48, 36, 2)]
    assert ND.octaves_for(20, 20, False) == []


def test_sigma_steps_are_the_half_way_points_between_scales():
    st = ND.sigma_steps(SEED_SIGMA, 3)
    assert st.dtype == f32 and len(st) == 4
    seed = float(f32(SEED_SIGMA))
    for j in range(4):
        assert st[j] == f32(seed * 2.0 ** ((j + 0.5) / 3))
    assert np.all(np.diff(st) > 0) and st[0] > f32(SEED_SIGMA) and st[3] < f32(2 * 1.6 * 2 ** (1 / 3))


OCTS = [(33, 17, -1), (16, 8, 0), (8, 4, 1)]   # odd sizes halving with floors
STEPS = ND.sigma_steps(SEED_SIGMA, 3)


def kp(x=4.0, y=2.0, sigma=1.6, orientation=0.0, response=0.5):
    return np.array([(x, y, sigma, orientation, response)], ND.KEYPOINT_DTYPE)


def one(**kw):
    keep = kw.pop("keep", False)
    c = ND.classify(kp(**kw), OCTS, STEPS, keep)
    return {k: v[0] for k, v in c.items()}


def test_admissibility_edges():
    assert one()["adm"]
    for bad in (np.nan, np.inf, -np.inf):
        assert not one(x=bad)["adm"] and not one(y=bad)["adm"] and not one(sigma=bad)["adm"]
    assert not one(sigma=0.0)["adm"] and not one(sigma=-1.6)["adm"]
    # octave -1 is 33 x 17 texels of half a pixel: x in [0, 16.5), y in [0, 8.5)
    assert one(x=0.0, y=0.0, sigma=0.9)["adm"] and one(x=-0.0, sigma=0.9)["adm"]
    assert not one(x=np.nextafter(f32(0), f32(-1)), sigma=0.9)["adm"]
    assert not one(x=16.5, sigma=0.9)["adm"] and one(x=np.nextafter(f32(16.5), f32(0)), sigma=0.9)["adm"]
    assert not one(y=8.5, sigma=0.9)["adm"] and one(y=np.nextafter(f32(8.5), f32(0)), sigma=0.9)["adm"]
    # octave 1 is 8 x 4 texels of two pixels: x = w of the octave in texels is outside, just below is inside
    c = one(x=np.nextafter(f32(16), f32(0)), y=7.9, sigma=4.0)
    assert c["adm"] and c["oct"] == 2 and c["scale_x"] == np.nextafter(f32(8), f32(0))
    assert not one(x=16.0, y=7.9, sigma=4.0)["adm"]
    # the window range: 0.02 <= rel <= 29, both ends included
    assert one(sigma=0.01, x=1.0, y=1.0)["adm"] and one(sigma=0.01, x=1.0, y=1.0)["rel"] == f32(0.02)
    assert not one(sigma=np.nextafter(f32(0.01), f32(0)), x=1.0, y=1.0)["adm"]
    assert one(sigma=58.0)["adm"] and not one(sigma=np.nextafter(f32(58), f32(100)))["adm"]


def test_first_and_last_octave_clamps():
    # below the first octave's scale 0: still the first octave, scale_idx 0
    c = one(sigma=0.3, x=1.0, y=1.0)
    assert c["oct"] == 0 and c["scale_idx"] == 0 and c["adm"]
    # at and beyond the top threshold of the last octave: the last octave, scale_idx S + 1
    top = f32(STEPS[3] * f32(2.0))
    c = one(sigma=top)
    assert c["oct"] == 2 and c["scale_idx"] == 4 and c["adm"]
    c = one(sigma=np.nextafter(top, f32(0)))
    assert c["oct"] == 2 and c["scale_idx"] == 3
    # the same threshold one octave lower hands over to the next octave, where it is scale 0's upper threshold (to the bit or one ulp beside
    # it): never scale_idx S + 1 in front of the last octave
    c = one(sigma=STEPS[3])
    assert c["oct"] == 2 and c["scale_idx"] == (1 if f32(STEPS[3] * f32(0.5)) >= STEPS[0] else 0)
    c = one(sigma=np.nextafter(STEPS[3], f32(0)))
    assert c["oct"] == 1 and c["scale_idx"] == 3
    # a threshold itself belongs to the scale above it
    c = one(sigma=STEPS[1])
    assert c["oct"] == 1 and c["scale_idx"] == 2
    # one octave only: everything lands in it
    c = ND.classify(kp(sigma=0.05, x=1.0, y=1.0), OCTS[1:2], STEPS)
    assert c["oct"][0] == 0 and c["scale_idx"][0] == 0 and c["adm"][0]
    c = ND.classify(kp(sigma=20.0), OCTS[1:2], STEPS)
    assert c["oct"][0] == 0 and c["scale_idx"][0] == 4 and c["adm"][0]


def test_orientation_range():
    two_pi = ND.TWO_PI32
    assert one(orientation=0.0, keep=True)["adm"] and one(orientation=two_pi, keep=True)["adm"] and one(orientation=-0.0, keep=True)["adm"]
    assert not one(orientation=np.nextafter(two_pi, f32(10)), keep=True)["adm"]
    assert not one(orientation=-1e-6, keep=True)["adm"] and not one(orientation=np.nan, keep=True)["adm"]
    # without keep_orientation the field is not looked at, and the record carries 0
    k = kp(orientation=np.nan)
    sec, found, placed, _ = ND.place(k, OCTS, [4, 4, 4], STEPS, False)
    assert placed == 1 and found == [1, 0, 0] and sec[0][0, 7] == 0 and sec[0][0, 4] == 3   # sigma 1.6 is scale 3 of the up-sampled octave
    k = kp(orientation=1.25)
    sec, _, _, _ = ND.place(k, OCTS, [4, 4, 4], STEPS, True)
    assert sec[0][0, 7] == f32(1.25).view(u32)


def test_order_capacity_and_counters():
    rng = np.random.default_rng(5)
    n = 40
    k = np.zeros(n, ND.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 16, n), rng.uniform(0, 8, n)
    k["sigma"] = np.exp(rng.uniform(np.log(0.5), np.log(12), n))
    k["response"] = rng.uniform(-1, 1, n)
    k["x"][::3] = np.nan     # a third inadmissible, interleaved
    caps = [4, 100, 3]
    sec, found, placed, index = ND.place(k, OCTS, caps, STEPS)
    c = ND.classify(k, OCTS, STEPS)
    assert sum(found) == int(c["adm"].sum()) and found[0] > 4 and found[2] > 3
    assert placed == 4 + found[1] + 3 and [len(s) for s in sec] == [4, found[1], 3]
    for o in range(3):
        want = np.flatnonzero(c["adm"] & (c["oct"] == o))[:caps[o]]
        assert np.array_equal(index[o], want) and np.all(np.diff(index[o]) > 0)
        # x, y, sigma and response travel bit for bit: the caller's join key
        assert np.array_equal(sec[o][:, 0], k["x"][want].view(u32)) and np.array_equal(sec[o][:, 6], k["sigma"][want].view(u32))
        assert np.array_equal(sec[o][:, 8], k["response"][want].view(u32)) and np.all(sec[o][:, 5].view(np.int32) == OCTS[o][2])
    empty = ND.place(k[:0], OCTS, caps, STEPS)
    assert empty[1] == [0, 0, 0] and empty[2] == 0


def test_public_keypoint_struct_is_20_bytes(tmp_path):
    src = tmp_path / "kp.c"
    src.write_text('#include <stddef.h>\n#include "vksift_ext.h"\n#include "vksift_hip.h"\n'
                   '_Static_assert(sizeof(vksift_ext_Keypoint) == 20, "size");\n_Static_assert(sizeof(vksift_hip_Keypoint) == 20, "size");\n'
                   '_Static_assert(offsetof(vksift_ext_Keypoint, response) == 16 && offsetof(vksift_hip_Keypoint, response) == 16, "layout");\n'
                   '_Static_assert(VKSIFT_EXT_DESCRIBE_ORIENT == 0u && VKSIFT_EXT_DESCRIBE_GIVEN == 1u, "modes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "kp")], check=True)
    assert ND.KEYPOINT_DTYPE.itemsize == 20


def test_the_cases_cover_what_they_are_for():
    """the launcher test's case table (tests/hip_place.py, laid out without a GPU) holds the shapes it claims: inadmissible keypoints of every kind next to admissible ones, every octave
    used, scale_idx S + 1 in the last octave, an overflowing section"""
    h = HPL.Place(HPL.case_named(f"{4 * HPL.WG + 3} keypoints, five octaves"), device="cpu")
    sections, found, placed, _ = h.spec(0)
    n = h.case["counts"][0]
    assert all(f > 0 for f in found) and 0.5 * n < sum(found) < 0.8 * n
    assert sections[-1][:, 4].max() == h.case["S"] + 1 and sections[0][:, 4].min() == 0
    h = HPL.Place(HPL.case_named("capacity 4 receiving 10"), device="cpu")
    sections, found, placed, index = h.spec(0)
    assert found == [0, 10] and placed == 4 and list(index[1]) == [0, 1, 2, 3]
    h = HPL.Place(HPL.case_named("three images, unequal, an empty one"), device="cpu")
    assert h.spec(1)[1] == [0] * 5 and h.spec(1)[2] == 0
    exp = h.expected()
    assert np.count_nonzero(exp != h.host) > 0
