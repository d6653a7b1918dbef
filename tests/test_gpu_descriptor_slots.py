"""The pair-slot enumeration of the descriptor launch (features.hip desc_row_prefix / desc_run / desc_next_slot / desc_step_pair): a lane walks
slots of two row neighbours, a span of cnt samples is (cnt + 1) / 2 slots, the second half of an odd span's last slot is dead. The cases are the
windows at which that enumeration can go wrong: fewer slots than lanes and than phases (R = 1, 2, 3), slot totals P with P mod 64 = 0, 1 and 63
(R and position chosen by the CPU restatement tests/desc_slots.py), rows of a single sample, rows clipped by a border or a corner, all-odd rows
(pi / 4), a team window beside a solo one, a window of several passes, binary16 planes; on the two-wave form (batches of 8) and the four-wave
form (batch 1).

As in tests/test_gpu_descriptor_pairs.py every case is compared BYTE FOR BYTE over its whole poisoned arena with orc_descriptor of the CPU
oracle (det math mode), at knob values 0, the built-in value and 63 of VKSIFT_TUNE_DESC_SOLO_R, with the matcher's dense rows off and on; the
expected arena is computed once per case and shared by its launches. Every case asserts on the CPU, from the restatement, that it reaches what it
is named for."""
import ctypes as C
import functools

import numpy as np
import pytest

import desc_slots as DS
import hip_features as HF

pytestmark = pytest.mark.gpu
f32 = np.float32
PI = np.pi
TUNE_DESC_SOLO_R = 14      # VKSIFT_TUNE_DESC_SOLO_R of include/vksift_hip.h
SOLO_MAX_R = 63            # features.hip DESC_SOLO_MAX_R
S = 1
THETAS = (0.0, PI / 4, PI / 2, 2.1)   # ksin == 0 (the spans' else-branch), all-odd rows, the fp32 neighbour of pi / 2, a generic angle


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HF.bind(vk.lib())


@pytest.fixture(scope="module")
def TAB(oracle):
    return HF.fp_table(oracle, 110)  # R up to 219


@pytest.fixture(scope="module")
def BUILT_IN(L):
    v = L.vksift_hip_tune_get(TUNE_DESC_SOLO_R)
    assert 0 <= v <= SOLO_MAX_R
    return v


def spans_of(row, w, h):
    x, y, R, th = row
    return DS.row_spans(x, y, HF.rel_for_R(R), th, w, h)


def slots_of(row, w, h):
    """P of every pass of the window"""
    return [DS.slots(rows) for _, rows in DS.passes(spans_of(row, w, h))]


@functools.lru_cache(maxsize=None)
def window_with_slots(w, h, residue):
    """(x, y, R, theta) of an unclipped window near the plane's centre whose slot total is residue mod 64, P >= 63: the first of a fixed scan"""
    for R in range(6, min(w, h) // 2 - 2):
        for th in THETAS + tuple(0.37 * k for k in range(1, 17)):
            for fx in (0.0, 0.3, -0.4):
                for fy in (0.0, -0.2, 0.45):
                    row = (w / 2 + fx, h / 2 + fy, R, th)
                    P = slots_of(row, w, h)
                    if len(P) == 1 and P[0] >= 63 and P[0] % 64 == residue:
                        return row
    raise AssertionError(f"no window with P mod 64 == {residue} on {w}x{h}")


def keypoints(w, h):
    """rows of (x, y, R, theta) for a w x h plane and what the restatement says of them"""
    rows = []
    for R in (1, 2, 3):                                                  # whole windows of fewer slots than lanes
        rows += [(w / 2 + 0.3 * i - 0.4, h / 2 - 0.2 * i + 0.1, R, th) for i, th in enumerate(THETAS)]
    fitted = [window_with_slots(w, h, r) for r in (0, 1, 63)]
    rows += fitted
    rows += [(x, y, R, THETAS[(i + 1) % 4]) for i, (x, y, R, _) in enumerate(fitted)]   # the same windows at another angle
    border = [(1.2, 1.2), (w - 2.2, 1.2), (1.2, h - 2.2), (w - 2.2, h - 2.2), (1.2, h / 2), (w - 2.2, h / 2 + 0.3), (w / 2, 1.2), (w / 2 - 0.3, h - 2.2)]
    rows += [(x, y, 5, THETAS[i % 4]) for i, (x, y) in enumerate(border)]
    rows += [(x, y, 9, THETAS[(i + 1) % 4]) for i, (x, y) in enumerate(border[:4])]
    # what the case is named for
    for R in (1, 2, 3):
        for row in rows[4 * (R - 1):4 * R]:
            P = slots_of(row, w, h)
            assert len(P) == 1 and 0 < P[0] < 64 and P[0] <= (2 * R + 1) * (R + 1), (row, P)
    assert min(slots_of(r, w, h)[0] for r in rows[:4]) < 4, "fewer slots than a solo wave has phases"
    assert [slots_of(r, w, h)[0] % 64 for r in fitted] == [0, 1, 63]
    nb = len(rows) - 12
    for row in rows[nb:]:
        sp = spans_of(row, w, h)
        assert len(sp) < 2 * row[2] + 1 or max(lo + c for lo, c in sp) - min(lo for lo, c in sp if c) < 2 * row[2] + 1, row   # clipped
    assert any(c == 1 for row in rows[nb:] for _, c in spans_of(row, w, h)), "a one-sample row in a clipped window"
    assert any(c == 1 for row in rows[:nb] for _, c in spans_of(row, w, h)), "a one-sample row in a whole window"
    odd = spans_of((w // 2, h // 2, 7, PI / 4), w, h)
    assert all(c & 1 for _, c in odd if c)
    big = (w / 2 + 0.2, h / 2 - 0.3, min(w, h) // 2 - 4, 2.1)                 # unclipped, steps for each of four waves
    assert slots_of(big, w, h)[0] > 3 * 64
    return rows + [(w // 2, h // 2, 7, PI / 4), big]


def records(rows):
    recs = HF.make_records([(x, y, i % (S + 2), i % 3, HF.rel_for_R(R), th) for i, (x, y, R, th) in enumerate(rows)])
    assert [HF.desc_radius(k) for k in recs] == [r[2] for r in rows]
    return recs


def planes_of(batch, w, h, seed, fp16=False):
    fams = ("smooth", "blackhalf", "periodic")
    return np.stack([HF.field(fams[b % 3], S, h, w, seed + b, fp16) for b in range(batch)])


def run_case(L, oracle, TAB, built_in, planes, recs, cap, what, fp16=False, **geom):
    """the case at knob values 0, built-in and 63, dense rows off and on; the knob goes back to what it was"""
    batch = len(planes)
    founds = [len(r) for r in recs]
    cfg = oracle.default_config(math_mode=1, nb_scales_per_octave=S, pyramid_fp16=1 if fp16 else 0)
    pyr = [oracle.Pyramid.from_planes(cfg, p) for p in planes]
    before = L.vksift_hip_tune_get(TUNE_DESC_SOLO_R)
    try:
        for dense in (None, [cap + 3, cap]):
            kw = dict(geom)
            if dense is not None:
                kw.update(dense=dense, sec_index=1, nsec=2, front=[[5 + b, 0] for b in range(batch)], found_img_stride=3, dense_strides=(1, 2, 1, 0))
            exp = None
            for knob in sorted({0, built_in, SOLO_MAX_R}):
                fa = HF.FeatureArena(planes, recs, founds, cap, fp16=fp16, tab=TAB, **kw)
                if exp is None:
                    exp = fa.expected_descriptor(pyr, dense=dense is not None)
                job = fa.job()
                assert L.vksift_hip_tune(TUNE_DESC_SOLO_R, knob) == 0
                if dense is not None:
                    d = fa.dense_rows()
                    rc = L.vksift_hip_descriptors_multi_dense(C.byref(job), 1, batch, C.byref(d), None)
                else:
                    rc = L.vksift_hip_descriptors(C.byref(job), batch, None)
                assert rc == 0, (what, knob, rc)
                fa.check(fa.read(), exp, f"{what}, knob {knob}, dense rows {'on' if dense else 'off'}")
    finally:
        L.vksift_hip_tune(TUNE_DESC_SOLO_R, before)


def batch_lists(rows, batch):
    """image b drops its first b keypoints: the same windows meet other partners and other workgroups (every second image has an odd count)"""
    return [records(rows[b:]) for b in range(batch)]


@pytest.mark.parametrize("size", [(64, 64), (40, 40)], ids=["64x64", "40x40"])
def test_two_wave_form(L, oracle, TAB, BUILT_IN, size):
    """batches of 8: solo at the knob values that allow a radius, team otherwise"""
    w, h = size
    rows = keypoints(w, h)
    assert max(r[2] for r in rows) <= SOLO_MAX_R
    recs = batch_lists(rows, 8)
    run_case(L, oracle, TAB, BUILT_IN, planes_of(8, w, h, 500 + w), recs, len(rows) + 1, f"slots, two waves, {w}x{h}", pitch=w + 3, feat_gap=7)


def test_four_wave_form(L, oracle, TAB, BUILT_IN):
    """batch 1 on one 64 x 64 plane: four shares of the slots, many of them without a step for the small windows"""
    w, h = 64, 64
    rows = keypoints(w, h)
    P = [slots_of(r, w, h)[0] for r in rows]
    assert min(P) < 4 and any(64 < p <= 3 * 64 for p in P) and any(p > 3 * 64 for p in P)   # three waves idle; one or two; every wave with steps
    run_case(L, oracle, TAB, BUILT_IN, planes_of(1, w, h, 520), [records(rows)], len(rows), "slots, four waves, 64x64", pitch=w + 1)


def test_team_window_beside_a_solo_one(L, oracle, TAB, BUILT_IN):
    """R = 64 cannot go solo at any knob value: its pair runs as a team beside workgroups whose waves go solo"""
    w, h = 64, 64
    rows = [(31.7, 32.2, 64, 0.9), (20.3, 40.1, 4, PI / 4), (30.0, 30.0, 5, 0.0), (33.3, 28.8, 6, 2.1), (w / 2, h / 2, 3, PI / 2)]
    recs0 = records(rows)
    assert HF.desc_radius(recs0[0]) == SOLO_MAX_R + 1 and all(HF.desc_radius(k) <= 6 for k in recs0[1:])
    P = slots_of(rows[0], w, h)
    assert len(P) == 1 and P[0] > 8 * 64       # clipped to the plane, still many steps for each of the two waves
    recs = [recs0[:(5, 4, 2, 1, 5, 3, 0, 5)[b]] for b in range(8)]
    run_case(L, oracle, TAB, BUILT_IN, planes_of(8, w, h, 540), recs, 6, "team beside solo", pitch=w + 2)


@pytest.mark.parametrize("batch", [8, 1], ids=["two-waves", "four-waves"])
def test_window_of_several_passes(L, oracle, TAB, BUILT_IN, batch):
    """24 x 300, R = 200: 298 window rows, more than DESC_MAX_ROWS — two passes, each with its own slot prefix"""
    w, h = 24, 300
    rows = [(12.2, 150.4, 200, 0.3), (11.0, 149.0, 200, PI / 4), (12.0, 20.0, 3, 0.0)]
    for row in rows[:2]:
        sp = spans_of(row, w, h)
        P = slots_of(row, w, h)
        assert len(sp) == h - 2 > DS.MAX_ROWS and len(P) == 2 and min(P) > 0, (row, P)
    recs = [records(rows[:(3, 1, 2, 3, 0, 3, 2, 1)[b]]) for b in range(batch)]
    run_case(L, oracle, TAB, BUILT_IN, planes_of(batch, w, h, 560), recs, 4, f"several passes, batch {batch}", pitch=w + 4)


def test_binary16_planes(L, oracle, TAB, BUILT_IN):
    """the binary16 instantiation takes its second sample's taps from sx + 1"""
    w, h = 64, 64
    rows = keypoints(w, h)
    recs = batch_lists(rows, 8)
    run_case(L, oracle, TAB, BUILT_IN, planes_of(8, w, h, 580, fp16=True), recs, len(rows) + 1, "slots, binary16 planes", fp16=True, pitch=w + 6)
