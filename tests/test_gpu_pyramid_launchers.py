"""Every pyramid launcher of include/vksift_hip.h, called directly, across the shape domain its contract allows — not only at the few
hundred shapes an instance's planner produces (pitch a multiple of 64, 16-byte aligned bases, one relation between w, h, batch and
row-segment cut). Expected values: orc_blur_plane / orc_blit_input / orc_blit_nearest of the CPU oracle (pinned by
tests/test_pyramid_reference.py), compared BIT FOR BIT. Every plane of a case lives in one poisoned arena (tests/hip_planes.py):

  * return 0  : every destination equals the reference and no byte outside the destinations' valid extents changed
  * return -1 : nothing was launched — every byte of the arena still holds its poison
  * > 0       : only for the invalid arguments of test_invalid_arguments

Sources: uniform [0, 1), and an "edge" family with exact zeros, subnormals and values up to 255; rounded through binary16 for fp16
planes. Taps: the oracle's effective_taps over a ladder of sigmas (every count 2..20; the single tap is 0.75), random signed taps
with all-distinct values, one-hot taps. Deterministic (fixed seeds). One GPU context, no subprocesses; tune knobs are restored."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import hip_planes as HP

pytestmark = pytest.mark.gpu

# read once per process by the library; they change which launcher accepts what
assert "VKSIFT_BLUR_KERNEL" not in os.environ and "VKSIFT_BLUR_PAIR" not in os.environ, "unset VKSIFT_BLUR_KERNEL / VKSIFT_BLUR_PAIR for this module"

f32 = np.float32
W4 = (list(range(4, 321, 4)) + list(range(380, 393, 4)) + list(range(508, 521, 4)) + list(range(764, 773, 4)) + list(range(1020, 1029, 4))
      + list(range(2044, 2053, 4)))
W_ODD = [1, 2, 3, 5, 17, 63, 65, 129, 255, 257, 1001]
H_LIST = list(range(1, 41)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 250]
BATCHES = [1, 2, 3, 8, 9]
PAIR_H = [63, 64, 65, 71, 72, 128, 250]
U8_SIDES = list(range(1, 41)) + [63, 64, 65] + list(range(127, 131)) + list(range(509, 516))


@pytest.fixture(scope="module")
def L(vk):
    import torch

    assert torch.cuda.is_available()
    return HP.bind(vk.lib())


@pytest.fixture(scope="module")
def T(oracle):
    """taps by count: 'gauss' from the oracle's effective_taps over a ladder of sigmas"""
    table = {1: np.array([0.75], f32)}
    for direct in (1, 0):
        for sigma in np.arange(0.2, 4.6, 0.05):
            cfg = oracle.default_config(seed_scale_sigma=float(sigma), use_input_upsampling=0, use_hardware_interpolated_blur=0 if direct else 1)
            k, n = oracle.effective_taps(cfg)
            for s in range(1, len(n)):
                table.setdefault(int(n[s]), k[s, :n[s]].copy())
    assert sorted(table) == list(range(1, 21)), sorted(table)
    return table


def make_taps(T, rng, n, family):
    if family == 0 or n == 1:
        return T[n]
    if family == 1:  # signed, all distinct (a swapped tap index changes the result), two-sided absolute sum 1.25
        while True:
            k = rng.uniform(-1, 1, n).astype(f32)
            k = (k * f32(1.25) / f32(abs(k[0]) + 2 * np.abs(k[1:]).sum())).astype(f32)
            if len(set(k.tolist())) == n and np.all(k != 0):
                return k
    k = np.zeros(n, f32)  # one-hot
    k[int(rng.integers(1, n))] = 1
    return k


def make_src(oracle, rng, family, shape, fp16):
    if family == 0:
        a = rng.random(shape, dtype=f32)
    else:
        a = (rng.random(shape, dtype=f32) * f32(255)).astype(f32)
        sel = rng.integers(0, 8, shape)
        a[sel == 0] = 0
        a[sel == 1] = (rng.random(shape, dtype=f32)[sel == 1] * f32(1e-39)).astype(f32)  # fp32 subnormals
        a[sel == 2] = f32(255)
    return oracle.store_f16(a) if fp16 else a


def geometry(rng, w, h, batch, aligned=False):
    """pitch, img_stride, base offset (texels) of one plane; aligned: what the four-texel kernels and the chain ask for"""
    up = (w + 63) // 64 * 64
    pitch = [w, w + 1, w + 4, up, up + 64][int(rng.integers(0, 5))]
    if aligned:
        pitch = [(w + 3) // 4 * 4, (w + 3) // 4 * 4 + 4, up, up + 64][int(rng.integers(0, 4))]
    ph = pitch * h
    stride = [ph, ph + 1, ph + 4, ph + 5000][int(rng.integers(0, 4))]
    offset = [0, 1, 4][int(rng.integers(0, 3))]
    if aligned:
        stride, offset = [ph, ph + 4, ph + 5000][int(rng.integers(0, 3))], [0, 4][int(rng.integers(0, 2))]
    return dict(pitch=pitch, img_stride=stride, offset=offset)


def kind_of(fp16):
    return "f16" if fp16 else "f32"


def blur_ref(oracle, src, taps, fp16):
    return np.stack([oracle.blur_plane(s, taps, fp16=fp16) for s in src])


def ok(L, rc, what):
    assert rc == 0, f"{what}: returned {rc} ({L.vksift_hip_error_string(rc).decode() if rc > 0 else 'declined'})"


@contextlib.contextmanager
def tuned(L, **knobs):
    ids = dict(wg_target=HP.TUNE_WG_TARGET, wide_mask=HP.TUNE_WIDE_MASK, multi_max=HP.TUNE_MULTI_MAX, pair_form=HP.TUNE_PAIR_FORM,
               min_march=HP.TUNE_MIN_MARCH)
    old = {k: L.vksift_hip_tune_get(ids[k]) for k in knobs}
    try:
        for k, v in knobs.items():
            assert L.vksift_hip_tune(ids[k], v) == 0
        yield
    finally:
        for k, v in old.items():
            L.vksift_hip_tune(ids[k], v)


def form_of(L, w, h, nt, batch, pitch=None, fp16=False):
    p = HP.Plane(256, w, h, pitch or w, (pitch or w) * h, 1 if fp16 else 0, 0)
    q = HP.Plane(512, w, h, pitch or w, (pitch or w) * h, 1 if fp16 else 0, 0)
    return L.vksift_hip_blur_form(p, q, nt, batch)


def boundary_widths(L, nt):
    """the three multiples of 4 on either side of the smallest width the strip march takes at this tap count"""
    for w in range(4, 400, 4):
        if form_of(L, w, 64, nt, 1) != 0:
            return [v for v in range(w - 12, w + 12, 4) if v >= 4]
    return []


def must_march(w, nt):
    return nt >= 2 and w % 4 == 0 and w >= 2 * ((nt + 2) & ~3) + 128


def blur_case(L, oracle, T, rng, w, h, nt, *, batch=None, fp16=None, aligned=False, stats=None, what="blur"):
    """one vksift_hip_blur launch with every free axis drawn from rng; returns the form the launcher reports"""
    if batch is None:
        batch = BATCHES[int(rng.integers(0, 5))] if w * h <= 65536 else int(rng.integers(1, 4))
    if fp16 is None:
        fp16 = bool(rng.integers(0, 2))
    taps = make_taps(T, rng, nt, int(rng.integers(0, 3)))
    src = make_src(oracle, rng, int(rng.integers(0, 2)), (batch, h, w), fp16)
    A = HP.Arena()
    s = A.plane("src", w, h, batch, kind=kind_of(fp16), data=src, **geometry(rng, w, h, batch, aligned))
    d = A.plane("dst", w, h, batch, kind=kind_of(fp16), **geometry(rng, w, h, batch, aligned))
    A.build()
    reverse = int(rng.integers(0, 2))
    form = L.vksift_hip_blur_form(s.c(), d.c(reverse), nt, batch)
    k, n = HP.taps_arg(taps)
    desc = f"{what} taps {nt} w {w} h {h} batch {batch} {kind_of(fp16)} reverse {reverse} form {form} src {s.pitch}/{s.img_stride}/+{s.offset} dst {d.pitch}/{d.img_stride}/+{d.offset}"
    ok(L, L.vksift_hip_blur(s.c(), d.c(reverse), k, n, batch, None), desc)
    HP.check_launch(A, [(d, blur_ref(oracle, src, taps, fp16))], desc)
    if stats is not None:
        stats["form"][form] += 1
        stats["seen"].update({("batch", batch), ("fp16", fp16), ("reverse", reverse), ("soff", s.offset), ("doff", d.offset),
                              ("pitch_eq", s.pitch == d.pitch), ("pad", s.pitch - w > 0), ("gap", s.img_stride - s.pitch * h)})
    return form


def new_stats():
    return dict(form={0: 0, 1: 0, 2: 0}, seen=set())


def report(name, accepted, declined):
    print(f"\n{name}: accepted {accepted} / declined {declined} / total {accepted + declined}")


# ------------------------------------------------------------------------------------------------------------------- vksift_hip_blur
@pytest.mark.parametrize("nt", range(1, 21))
def test_blur(L, oracle, T, nt):
    rng = np.random.default_rng(1000 + nt)
    stats = new_stats()
    bw = boundary_widths(L, nt)
    assert (nt == 1) == (bw == [])
    widths = W4 + bw + W_ODD
    for i, w in enumerate(widths):
        h = H_LIST[(7 * i + 3 * nt) % len(H_LIST)]
        form = blur_case(L, oracle, T, rng, w, h, nt, stats=stats)
        if must_march(w, nt):
            assert form in (1, 2), (w, h, nt, form)
        if w % 4 or nt == 1:
            assert form == 0, (w, h, nt, form)
    # every height: at the narrowest width the strip march takes, at a two-strip width, and through the tile kernel
    for w in ([bw[3]] if bw else []) + [160 + 4 * (nt % 7), 17]:
        for h in H_LIST:
            blur_case(L, oracle, T, rng, w, h, nt, stats=stats, batch=[1, 2, 3][h % 3])
    seen = stats["seen"]
    assert {v for k, v in seen if k == "batch"} >= {1, 2, 3, 8, 9} and {v for k, v in seen if k == "soff"} == {0, 1, 4}
    assert {("fp16", True), ("fp16", False), ("reverse", 0), ("reverse", 1), ("pitch_eq", False), ("pad", True), ("pad", False)} <= seen
    assert len({v for k, v in seen if k == "gap"}) >= 4
    if nt >= 2:
        assert stats["form"][1] + stats["form"][2] > 100
    report(f"vksift_hip_blur[{nt} taps] strip march", stats["form"][1] + stats["form"][2], stats["form"][0])


@pytest.mark.parametrize("nt", range(2, 21))
def test_blur_forced_forms(L, oracle, T, nt):
    """VKSIFT_TUNE_WIDE_MASK 0 and all ones (the four-texel form at widths and batches the built-in choice never gives it), and
    VKSIFT_TUNE_WG_TARGET / VKSIFT_TUNE_MIN_MARCH so that one plane is cut into 1, 2, 3 and the largest number of row segments"""
    rng = np.random.default_rng(2000 + nt)
    stats = new_stats()
    # (the four-texel form takes widths that waste at most 64 columns of their last 256-column strip)
    widths = (W4[::2] + boundary_widths(L, nt) + [132, 136, 140, 252, 260, 316] + list(range(192, 257, 4)) + list(range(448, 513, 8))
              + [704, 736, 768, 960, 992, 1024, 1988, 2048])
    for mask in (0, 0xFFFFF):
        with tuned(L, wide_mask=mask):
            for i, w in enumerate(widths):
                h = H_LIST[(11 * i + 5 * nt + mask) % len(H_LIST)]
                form = blur_case(L, oracle, T, rng, w, h, nt, stats=stats, aligned=bool(mask) and i % 4 != 0, fp16=False if mask and i % 3 else None,
                                 what=f"blur wide_mask {mask:#x}")
                assert mask or form != 2
                if must_march(w, nt):
                    assert form in (1, 2), (w, h, nt, form)
    if nt in (5, 7, 9, 11, 13):
        assert stats["form"][2] > 20, stats["form"]  # the four-texel kernel itself
    cuts = 0
    for mask in (0, 0xFFFFF):
        for w, h, batch in ((boundary_widths(L, nt)[3], 37, 1), (256, 65, 2), (264, 129, 1), (388, 250, 1), (512, 31, 3)):
            with tuned(L, wide_mask=mask):
                strips = (w + 255) // 256 if form_of(L, w, h, nt, batch) == 2 else (w + 127) // 128
            for nseg in (1, 2, 3, 0):
                with tuned(L, wide_mask=mask, min_march=8, wg_target=(nseg * strips * batch) if nseg else 1 << 20):
                    blur_case(L, oracle, T, rng, w, h, nt, batch=batch, aligned=True, fp16=False if mask else None, stats=stats,
                              what=f"blur wide_mask {mask:#x} segments {nseg or 'max'}")
                    cuts += 1
    assert cuts == 40
    report(f"vksift_hip_blur forced forms[{nt} taps] four-texel form", stats["form"][2], stats["form"][0] + stats["form"][1])


# -------------------------------------------------------------------------------------------------------------- vksift_hip_blur_pair
def pair_case(L, oracle, T, rng, w, h, n1, n2, batch, fp16, aligned, what):
    t1, t2 = make_taps(T, rng, n1, int(rng.integers(0, 3))), make_taps(T, rng, n2, int(rng.integers(0, 3)))
    src = make_src(oracle, rng, int(rng.integers(0, 2)), (batch, h, w), fp16)
    A = HP.Arena()
    kind = kind_of(fp16)
    s = A.plane("src", w, h, batch, kind=kind, data=src, **geometry(rng, w, h, batch, aligned))
    d1, d2, e1, e2 = (A.plane(nm, w, h, batch, kind=kind, **geometry(rng, w, h, batch, aligned)) for nm in ("dst1", "dst2", "blur1", "blur2"))
    A.build()
    (k1, m1), (k2, m2) = HP.taps_arg(t1), HP.taps_arg(t2)
    rev = int(rng.integers(0, 2))
    desc = f"{what} taps {n1}+{n2} w {w} h {h} batch {batch} {kind} pitches {s.pitch}/{d1.pitch}/{d2.pitch} offsets {s.offset}/{d1.offset}/{d2.offset}"
    rc = L.vksift_hip_blur_pair(s.c(), d1.c(), d2.c(rev), k1, m1, k2, m2, batch, None)
    if rc == -1:
        HP.check_nothing_launched(A, desc)
        return False
    ok(L, rc, desc)
    ok(L, L.vksift_hip_blur(s.c(), e1.c(), k1, m1, batch, None), desc)
    ok(L, L.vksift_hip_blur(e1.c(), e2.c(rev), k2, m2, batch, None), desc)
    r1 = blur_ref(oracle, src, t1, fp16)
    r2 = blur_ref(oracle, r1, t2, fp16)
    HP.check_launch(A, [(d1, r1), (d2, r2), (e1, r1), (e2, r2)], desc)
    return True


@pytest.mark.parametrize("pair_form", [0, 1, 2])
def test_blur_pair(L, oracle, T, pair_form):
    rng = np.random.default_rng(3000 + pair_form)
    acc = dec = 0
    with tuned(L, pair_form=pair_form):
        for i, w in enumerate(W4 + W_ODD):
            h = PAIR_H[(i + pair_form) % len(PAIR_H)]
            batch = BATCHES[int(rng.integers(0, 5))] if w * h <= 65536 else int(rng.integers(1, 3))
            got = pair_case(L, oracle, T, rng, w, h, 5, 7, batch, False, pair_form == 2 and i % 3 != 0, f"blur_pair form {pair_form}")
            if w % 4 == 0 and w >= 160 and h >= 64:
                assert got, ("must accept", w, h, batch)
            if w % 4 or h < 64:
                assert not got, ("must decline", w, h)
            acc, dec = acc + got, dec + (not got)
        # every other tap combination and fp16 decline
        for n1, n2, fp16 in ((5, 7, True), (7, 5, False), (5, 5, False), (7, 7, False), (5, 9, False), (4, 7, False), (9, 11, False), (1, 7, False), (5, 20, False)):
            assert not pair_case(L, oracle, T, rng, 256, 64, n1, n2, 2, fp16, True, "blur_pair other combination")
            dec += 1
    assert acc > 45
    report(f"vksift_hip_blur_pair[form knob {pair_form}]", acc, dec)


# ------------------------------------------------------------------------------------------------------------- vksift_hip_blur_multi
def multi_case(L, oracle, T, rng, shapes, nt, batch, kinds, what):
    taps = make_taps(T, rng, nt, int(rng.integers(0, 3)))
    A = HP.Arena()
    S, D, E, srcs = [], [], [], []
    for i, ((w, h), kind) in enumerate(zip(shapes, kinds)):
        src = make_src(oracle, rng, int(rng.integers(0, 2)), (batch, h, w), kind == "f16")
        srcs.append(src)
        S.append(A.plane(f"src{i}", w, h, batch, kind=kind, data=src, **geometry(rng, w, h, batch)))
        D.append(A.plane(f"dst{i}", w, h, batch, kind=kind, **geometry(rng, w, h, batch)))
        E.append(A.plane(f"blur{i}", w, h, batch, kind=kind, **geometry(rng, w, h, batch)))
    A.build()
    n = len(shapes)
    k, m = HP.taps_arg(taps)
    desc = f"{what} taps {nt} batch {batch} planes {shapes} {kinds[0]}"
    rc = L.vksift_hip_blur_multi((HP.Plane * n)(*[p.c() for p in S]), (HP.Plane * n)(*[p.c(i & 1) for i, p in enumerate(D)]), n, k, m, batch, None)
    if rc == -1:
        HP.check_nothing_launched(A, desc)
        return False
    ok(L, rc, desc)
    res = []
    for s, d, e, src, kind in zip(S, D, E, srcs, kinds):
        ok(L, L.vksift_hip_blur(s.c(), e.c(), k, m, batch, None), desc)
        r = blur_ref(oracle, src, taps, kind == "f16")
        res += [(d, r), (e, r)]
    HP.check_launch(A, res, desc)
    return True


@pytest.mark.parametrize("nt", [9, 11, 13, 15])
def test_blur_multi(L, oracle, T, nt):
    rng = np.random.default_rng(4000 + nt)
    acc = dec = 0
    wide = [w for w in W4 if w >= 160]
    for multi_max in (0, 1, 3):
        with tuned(L, multi_max=multi_max):
            for rep in range(10):
                for n in (1, 2, 5, 8):
                    pool = wide if rep % 2 == 0 else W4 + W_ODD
                    shapes = [(int(pool[int(rng.integers(0, len(pool)))]), int(H_LIST[int(rng.integers(0, len(H_LIST)))])) for _ in range(n)]
                    shapes = [(w, h if w < 600 else min(h, 65)) for w, h in shapes]
                    kind = kind_of((rep + n) % 3 == 0)
                    got = multi_case(L, oracle, T, rng, shapes, nt, [1, 2, 3][rep % 3], [kind] * n, f"blur_multi multi_max {multi_max}")
                    if all(w % 4 == 0 and w >= 160 for w, _ in shapes):
                        assert got, ("must accept", shapes)
                    acc, dec = acc + got, dec + (not got)
    # nine planes, other tap counts, mixed texel types: declined
    nine = [(160 + 4 * i, 20 + i) for i in range(9)]
    assert not multi_case(L, oracle, T, rng, nine, nt, 1, ["f32"] * 9, "blur_multi nine planes")
    assert not multi_case(L, oracle, T, rng, nine[:3], nt, 2, ["f32", "f16", "f32"], "blur_multi mixed types")
    assert not multi_case(L, oracle, T, rng, nine[:3], nt, 2, ["f16", "f16", "f32"], "blur_multi mixed types")
    for other in (1, 2, 5, 7, 8, 10, 12, 14, 16, 17, 20):
        assert not multi_case(L, oracle, T, rng, nine[:2], other, 1, ["f32"] * 2, "blur_multi other tap count")
        dec += 1
    assert acc >= 60
    report(f"vksift_hip_blur_multi[{nt} taps]", acc, dec + 3)


# --------------------------------------------------------------------------------- vksift_hip_blur_downsample, vksift_hip_downsample
@pytest.mark.parametrize("nt", range(1, 21))
def test_blur_downsample(L, oracle, T, nt):
    rng = np.random.default_rng(5000 + nt)
    acc = dec = 0
    widths = W4[1::3] + boundary_widths(L, nt) + [5, 17, 63, 129, 255]
    for mask in (-1, 0xFFFFF):
        with tuned(L, wide_mask=mask):
            for i, w in enumerate(widths):
                h = H_LIST[(5 * i + nt + (mask & 1)) % len(H_LIST)]
                batch = BATCHES[int(rng.integers(0, 5))] if w * h <= 65536 else 1
                fp16 = bool(rng.integers(0, 2)) and mask < 0
                aligned = mask > 0 and i % 3 != 0
                taps = make_taps(T, rng, nt, int(rng.integers(0, 3)))
                src = make_src(oracle, rng, int(rng.integers(0, 2)), (batch, h, w), fp16)
                kind = kind_of(fp16)
                nw, nh = max(w // 2, 1), max(h // 2, 1)
                A = HP.Arena()
                s = A.plane("src", w, h, batch, kind=kind, data=src, **geometry(rng, w, h, batch, aligned))
                d = A.plane("dst", w, h, batch, kind=kind, **geometry(rng, w, h, batch, aligned))
                nx = A.plane("next", nw, nh, batch, kind=kind, **geometry(rng, nw, nh, batch, aligned))
                e = A.plane("blur", w, h, batch, kind=kind, **geometry(rng, w, h, batch, aligned))
                en = A.plane("down", nw, nh, batch, kind=kind, **geometry(rng, nw, nh, batch, aligned))
                A.build()
                k, m = HP.taps_arg(taps)
                form = L.vksift_hip_blur_form(s.c(), d.c(), nt, batch)
                desc = f"blur_downsample mask {mask:#x} taps {nt} w {w} h {h} batch {batch} {kind} form {form} pitches {s.pitch}/{d.pitch}/{nx.pitch}"
                rc = L.vksift_hip_blur_downsample(s.c(), d.c(), nx.c(), k, m, batch, None)
                if rc == -1:
                    assert form == 0 or w % 2 or h % 2, ("must accept", desc)
                    HP.check_nothing_launched(A, desc)
                    dec += 1
                    continue
                ok(L, rc, desc)
                assert w % 2 == 0 and h % 2 == 0, ("odd sizes must decline", desc)
                acc += 1
                ok(L, L.vksift_hip_blur(s.c(), e.c(), k, m, batch, None), desc)
                ok(L, L.vksift_hip_downsample(e.c(), en.c(), batch, None), desc)
                r = blur_ref(oracle, src, taps, fp16)
                rn = np.stack([oracle.blit_nearest(p, nw, nh) for p in r])
                HP.check_launch(A, [(d, r), (nx, rn), (e, r), (en, rn)], desc)
    assert nt == 1 or acc > 5
    report(f"vksift_hip_blur_downsample[{nt} taps]", acc, dec)


def test_downsample_general(L, oracle):
    """vksift_hip_downsample alone: blit_nearest is general, so halved, odd-halved, equal and larger targets"""
    rng = np.random.default_rng(6000)
    n = 0
    for i, sw in enumerate(W4[::3] + W_ODD):
        sh = H_LIST[(3 * i) % len(H_LIST)]
        for dw, dh in ((max(sw // 2, 1), max(sh // 2, 1)), (sw, sh), ((sw + 1) // 2, (sh + 2) // 3), (min(sw + 3, 300), sh + 1)):
            fp16 = bool(rng.integers(0, 2))
            batch = int(rng.integers(1, 4))
            src = make_src(oracle, rng, i % 2, (batch, sh, sw), fp16)
            A = HP.Arena()
            s = A.plane("src", sw, sh, batch, kind=kind_of(fp16), data=src, **geometry(rng, sw, sh, batch))
            d = A.plane("dst", dw, dh, batch, kind=kind_of(fp16), **geometry(rng, dw, dh, batch))
            A.build()
            desc = f"downsample {sw}x{sh} -> {dw}x{dh} batch {batch} {kind_of(fp16)}"
            ok(L, L.vksift_hip_downsample(s.c(), d.c(), batch, None), desc)
            HP.check_launch(A, [(d, np.stack([oracle.blit_nearest(p, dw, dh) for p in src]))], desc)
            n += 1
    report("vksift_hip_downsample", n, 0)


# ------------------------------------------------------------------ vksift_hip_input_blit, vksift_hip_seed_upsampled, vksift_hip_seed_direct
def u8_plane(A, rng, sw, sh, batch, img):
    stride = sw * sh + [0, 1, 3, 777][int(rng.integers(0, 4))]
    return A.plane("u8", sw, sh, batch, kind="u8", pitch=sw, img_stride=max(stride, sw * sh), offset=int(rng.integers(0, 4)), data=img)


def blit_ref(oracle, img, dw, dh, fp16):
    r = np.stack([oracle.blit_input(p, dw, dh) for p in img])
    return oracle.store_f16(r) if fp16 else r


def test_input_blit(L, oracle):
    rng = np.random.default_rng(7000)
    n = 0
    for i, sw in enumerate(U8_SIDES):
        for sh in (U8_SIDES[(7 * i + 1) % len(U8_SIDES)], U8_SIDES[(13 * i + 5) % len(U8_SIDES)]):
            for f in (2, 1):
                fp16, batch = bool(rng.integers(0, 2)), int(rng.integers(1, 4))
                img = rng.integers(0, 256, (batch, sh, sw), dtype=np.uint8)
                A = HP.Arena()
                u = u8_plane(A, rng, sw, sh, batch, img)
                d = A.plane("dst", f * sw, f * sh, batch, kind=kind_of(fp16), **geometry(rng, f * sw, f * sh, batch))
                A.build()
                desc = f"input_blit {sw}x{sh} x{f} batch {batch} {kind_of(fp16)} pitch {d.pitch} offset {d.offset}"
                ok(L, L.vksift_hip_input_blit(u.ptr, sw, sh, u.img_stride, d.c(), batch, None), desc)
                HP.check_launch(A, [(d, blit_ref(oracle, img, f * sw, f * sh, fp16))], desc)
                n += 1
    report("vksift_hip_input_blit", n, 0)


def seed_sweep(L, oracle, T, nt, ups, seed):
    rng = np.random.default_rng(seed)
    f = 2 if ups else 1
    fn = L.vksift_hip_seed_upsampled if ups else L.vksift_hip_seed_direct
    limit = 12 if ups else 20
    acc = dec = 0
    sides = U8_SIDES + ([80, 84, 96, 100, 160, 256] if ups else [160, 164, 200, 256, 320])
    for i, sw in enumerate(sides):
        sh = U8_SIDES[(5 * i + nt) % len(U8_SIDES)]
        fp16, batch = bool(rng.integers(0, 2)), int(rng.integers(1, 4))
        W, H = f * sw, f * sh
        img = rng.integers(0, 256, (batch, sh, sw), dtype=np.uint8)
        taps = make_taps(T, rng, nt, int(rng.integers(0, 3)))
        kind = kind_of(fp16)
        A = HP.Arena()
        u = u8_plane(A, rng, sw, sh, batch, img)
        d = A.plane("dst", W, H, batch, kind=kind, **geometry(rng, W, H, batch))
        b = A.plane("blit", W, H, batch, kind=kind, **geometry(rng, W, H, batch))
        e = A.plane("blur", W, H, batch, kind=kind, **geometry(rng, W, H, batch))
        A.build()
        k, m = HP.taps_arg(taps)
        desc = f"seed ups {ups} taps {nt} source {sw}x{sh} batch {batch} {kind} stride {u.img_stride} +{u.offset} dst pitch {d.pitch} +{d.offset}"
        rc = fn(u.ptr, sw, sh, u.img_stride, d.c(int(rng.integers(0, 2))), k, m, batch, None)
        if rc == -1:
            assert not (W % 4 == 0 and W >= 160 and 2 <= nt <= 12), ("must accept", desc)
            HP.check_nothing_launched(A, desc)
            dec += 1
            continue
        ok(L, rc, desc)
        assert nt <= limit and W % 4 == 0, desc
        acc += 1
        ok(L, L.vksift_hip_input_blit(u.ptr, sw, sh, u.img_stride, b.c(), batch, None), desc)
        ok(L, L.vksift_hip_blur(b.c(), e.c(), k, m, batch, None), desc)
        rb = blit_ref(oracle, img, W, H, fp16)
        r = blur_ref(oracle, rb, taps, fp16)
        HP.check_launch(A, [(d, r), (b, rb), (e, r)], desc)
    return acc, dec


@pytest.mark.parametrize("nt", range(2, 15))
def test_seed_upsampled(L, oracle, T, nt):
    acc, dec = seed_sweep(L, oracle, T, nt, True, 8000 + nt)
    assert (acc == 0) if nt > 12 else (acc > 8)
    report(f"vksift_hip_seed_upsampled[{nt} taps]", acc, dec)


@pytest.mark.parametrize("nt", range(1, 21))
def test_seed_direct(L, oracle, T, nt):
    acc, dec = seed_sweep(L, oracle, T, nt, False, 9000 + nt)
    # (13 taps and more: the u8-source kernels are instantiated for 2..12 taps, the launcher may decline — nothing launched, checked above)
    assert (acc == 0) if nt < 2 else (acc >= 5 or nt > 12)
    report(f"vksift_hip_seed_direct[{nt} taps]", acc, dec)


# ----------------------------------------------------------------------------------------------------------- vksift_hip_octave_chain
CHAIN_RUNS = [  # (w, h, octaves, must accept with taps no longer than the shortest side)
    (8, 8, 1, True), (12, 8, 1, True), (8, 20, 1, True), (16, 16, 2, True), (32, 16, 2, True), (64, 32, 3, True), (128, 64, 4, True),
    (160, 120, 4, True), (200, 96, 2, True), (96, 200, 2, True), (136, 140, 1, True), (140, 137, 1, True), (64, 66, 2, True),
    (100, 60, 2, False), (200, 96, 3, False), (50, 24, 1, False), (164, 120, 1, False), (4, 8, 1, False), (8, 4, 1, False),
]


def chain_case(L, oracle, T, rng, w, h, n_oct, n_layers, S, batch, counts, what, misalign=False, pitch_odd=False):
    sizes = [(w >> o, h >> o) for o in range(n_oct)]
    taps = [make_taps(T, rng, n, int(rng.integers(0, 3))) for n in counts]
    src = make_src(oracle, rng, int(rng.integers(0, 2)), (batch, h, w), False)
    A = HP.Arena()
    layers = []
    for o, (ow, oh) in enumerate(sizes):
        g = geometry(rng, ow, oh, batch, aligned=True)
        if misalign:
            g["offset"] = 1
        if pitch_odd:
            g["pitch"], g["img_stride"] = ow + 1, (ow + 1) * oh
        layers.append([A.plane(f"o{o}l{l}", ow, oh, batch, data=src if (o, l) == (0, 0) else None, **g) for l in range(n_layers)])
    A.build()
    flat = [p.c() for row in layers for p in row]
    kt = np.zeros((n_layers, HP.MAX_TAPS), f32)
    for l, t in enumerate(taps):
        kt[l, :len(t)] = t
    nts = (C.c_uint32 * n_layers)(*counts)
    desc = f"{what} {w}x{h} octaves {n_oct} layers {n_layers} S {S} batch {batch} taps {counts} pitch {layers[0][0].pitch} stride {layers[0][0].img_stride}"
    rc = L.vksift_hip_octave_chain((HP.Plane * len(flat))(*flat), n_oct, n_layers, S, kt.ctypes.data_as(C.POINTER(C.c_float)), nts, batch, None)
    if rc == -1:
        HP.check_nothing_launched(A, desc)
        return False
    ok(L, rc, desc)
    res, g = [], src
    for o, (ow, oh) in enumerate(sizes):
        if o > 0:
            g = np.stack([oracle.blit_nearest(p, ow, oh) for p in gS])
            res.append((layers[o][0], g))
        for l in range(1, n_layers):
            g = blur_ref(oracle, g, taps[l], False)
            res.append((layers[o][l], g))
            if l == S:
                gS = g
    HP.check_launch(A, res, desc)  # (layer 0 of octave 0 is a source of the arena: unchanged, or the comparison fails)
    return True


def test_octave_chain(L, oracle, T):
    rng = np.random.default_rng(10000)
    acc = dec = 0
    for w, h, n_oct, good in CHAIN_RUNS:
        side = min(w >> (n_oct - 1), h >> (n_oct - 1))
        for n_layers in range(2, HP.CH_MAX_LAYERS + 1):
            S = int(rng.integers(1, n_layers))
            special = [n for n in (5, 7, 9, 11, 13) if n <= side]
            counts = [1] + [int(special[int(rng.integers(0, len(special)))]) if special and rng.integers(0, 2) else int(rng.integers(1, min(20, side) + 1))
                            for _ in range(n_layers - 1)]
            batch = 1 if n_layers % 2 else 3
            got = chain_case(L, oracle, T, rng, w, h, n_oct, n_layers, S, batch, counts, "octave_chain")
            assert got == good, ("accepted" if got else "declined", w, h, n_oct, n_layers, counts)
            acc, dec = acc + got, dec + (not got)
        if good and side < 20:  # a tap count above the shortest side declines
            assert not chain_case(L, oracle, T, rng, w, h, n_oct, 3, 1, 1, [1, min(side, 5), side + 1], "octave_chain long taps")
            dec += 1
    # the longest runs and layer counts, every specialised tap count and the generic path at once
    assert chain_case(L, oracle, T, rng, 160, 120, 4, 8, 3, 3, [1, 5, 7, 9, 11, 13, 15, 2], "octave_chain full")
    assert chain_case(L, oracle, T, rng, 128, 128, 4, 8, 7, 1, [1, 13, 11, 9, 7, 5, 3, 16], "octave_chain full")
    acc += 2
    # what the launcher documents as not covered: fp16 is a field of the plane (not built here), 5 octaves / 9 layers, S out of range,
    # a base that is not 16-byte aligned, a pitch that is not a multiple of 4
    assert not chain_case(L, oracle, T, rng, 32, 32, 1, 3, 3, 1, [1, 5, 5], "octave_chain S = layers")
    assert not chain_case(L, oracle, T, rng, 32, 32, 1, 3, 1, 1, [1, 5, 5], "octave_chain misaligned base", misalign=True)
    assert not chain_case(L, oracle, T, rng, 32, 32, 1, 3, 1, 1, [1, 5, 5], "octave_chain odd pitch", pitch_odd=True)
    assert not chain_case(L, oracle, T, rng, 128, 128, 5, 2, 1, 1, [1, 3], "octave_chain five octaves")
    dec += 4
    report("vksift_hip_octave_chain", acc, dec)


# -------------------------------------------------------------------------------------------------------------- vksift_hip_dog_plane
def test_dog_plane(L, oracle):
    rng = np.random.default_rng(11000)
    n = 0
    for i, w in enumerate(W4[::4] + W_ODD):
        h = H_LIST[(9 * i) % len(H_LIST)]
        for fp16 in (False, True):
            for with_hi in (True, False):
                lo_v = make_src(oracle, rng, i % 2, (1, h, w), fp16)
                hi_v = make_src(oracle, rng, (i + 1) % 2, (1, h, w), fp16)
                g = geometry(rng, w, h, 1)
                g["img_stride"] = g["pitch"] * h
                A = HP.Arena()
                lo = A.plane("lo", w, h, 1, kind=kind_of(fp16), data=lo_v, **g)
                hi = A.plane("hi", w, h, 1, kind=kind_of(fp16), data=hi_v, **g)
                out = A.plane("out", w, h, 1, kind="f32", offset=int(rng.integers(0, 2)))
                A.build()
                desc = f"dog_plane {w}x{h} pitch {lo.pitch} {kind_of(fp16)} hi {with_hi}"
                ok(L, L.vksift_hip_dog_plane(lo.ptr, hi.ptr if with_hi else None, w, h, lo.pitch, int(fp16), out.ptr, None), desc)
                ref = (hi_v - lo_v).astype(f32) if with_hi else lo_v
                if fp16 and with_hi:
                    ref = ref.astype(np.float16).astype(f32)  # numpy rounds to nearest even, like the store
                HP.check_launch(A, [(out, ref)], desc)
                n += 1
    report("vksift_hip_dog_plane", n, 0)


# ------------------------------------------------------------------------------------------------------------ one far-apart batch
def test_far_apart_batch(L, oracle, T):
    """Two images more than 4 GiB (in bytes) apart, 256 x 64 planes, through the tile, two-texel, four-texel, two-scale, multi, fused
    down-sampling and seed kernels: the 64-bit image offsets of every kernel."""
    import torch

    rng = np.random.default_rng(12000)
    W, H = 256, 64
    far = HP.FarArena()
    try:
        slot = lambda i: i * (1 << 20)
        src = make_src(oracle, rng, 0, (2, H, W), False)

        def blur_far(nt, what, **knobs):
            taps = make_taps(T, rng, nt, 1)
            k, m = HP.taps_arg(taps)
            s = far.plane("src", W, H, pitch=W + 64, room_off=slot(0), data=src)
            d = far.plane("dst", W, H, pitch=W, room_off=slot(1))
            with tuned(L, **knobs):
                form = L.vksift_hip_blur_form(s.c(), d.c(), nt, 2)
                ok(L, L.vksift_hip_blur(s.c(), d.c(1), k, m, 2, None), what)
            far.check([(d, blur_ref(oracle, src, taps, False))], what)
            return form

        assert blur_far(1, "far: tile kernel") == 0
        assert blur_far(7, "far: two-texel kernel") == 1
        assert blur_far(9, "far: four-texel kernel", wide_mask=0xFFFFF) == 2
        for pf in (1, 2):
            t1, t2 = make_taps(T, rng, 5, 1), make_taps(T, rng, 7, 1)
            (k1, m1), (k2, m2) = HP.taps_arg(t1), HP.taps_arg(t2)
            s = far.plane("src", W, H, room_off=slot(0), data=src)
            d1 = far.plane("dst1", W, H, pitch=W + 4, room_off=slot(1))
            d2 = far.plane("dst2", W, H, room_off=slot(2))
            with tuned(L, pair_form=pf):
                ok(L, L.vksift_hip_blur_pair(s.c(), d1.c(), d2.c(), k1, m1, k2, m2, 2, None), f"far: two-scale kernel form {pf}")
            r1 = blur_ref(oracle, src, t1, False)
            far.check([(d1, r1), (d2, blur_ref(oracle, r1, t2, False))], f"far: two-scale kernel form {pf}")
        # multi: two planes of different sizes, fp16
        taps = make_taps(T, rng, 11, 1)
        k, m = HP.taps_arg(taps)
        srch = make_src(oracle, rng, 0, (2, H, W), True)
        src2 = make_src(oracle, rng, 0, (2, 40, 160), True)
        s0 = far.plane("src0", W, H, kind="f16", room_off=slot(0), data=srch)
        s1 = far.plane("src1", 160, 40, kind="f16", pitch=192, room_off=slot(1), data=src2)
        d0 = far.plane("dst0", W, H, kind="f16", room_off=slot(2))
        d1 = far.plane("dst1", 160, 40, kind="f16", room_off=slot(3))
        ok(L, L.vksift_hip_blur_multi((HP.Plane * 2)(s0.c(), s1.c()), (HP.Plane * 2)(d0.c(), d1.c(1)), 2, k, m, 2, None), "far: multi kernel")
        far.check([(d0, blur_ref(oracle, srch, taps, True)), (d1, blur_ref(oracle, src2, taps, True))], "far: multi kernel")
        # fused down-sampling, both strip-march forms
        for mask, nt in ((0, 7), (0xFFFFF, 13)):
            taps = make_taps(T, rng, nt, 1)
            k, m = HP.taps_arg(taps)
            s = far.plane("src", W, H, room_off=slot(0), data=src)
            d = far.plane("dst", W, H, room_off=slot(1))
            nx = far.plane("next", W // 2, H // 2, pitch=W // 2 + 4, room_off=slot(2))
            with tuned(L, wide_mask=mask):
                ok(L, L.vksift_hip_blur_downsample(s.c(), d.c(), nx.c(), k, m, 2, None), f"far: fused down-sampling mask {mask:#x}")
            r = blur_ref(oracle, src, taps, False)
            far.check([(d, r), (nx, np.stack([oracle.blit_nearest(p, W // 2, H // 2) for p in r]))], f"far: fused down-sampling mask {mask:#x}")
        # the seed kernels: u8 images 4 GiB apart as well
        for ups in (True, False):
            f = 2 if ups else 1
            sw, sh = W // f, H // f
            img = rng.integers(0, 256, (2, sh, sw), dtype=np.uint8)
            taps = make_taps(T, rng, 8, 1)
            k, m = HP.taps_arg(taps)
            u = far.plane("u8", sw, sh, kind="u8", room_off=slot(0), data=img)
            d = far.plane("dst", W, H, room_off=slot(1))
            fn = L.vksift_hip_seed_upsampled if ups else L.vksift_hip_seed_direct
            ok(L, fn(u.ptr, sw, sh, u.img_stride, d.c(), k, m, 2, None), f"far: seed kernel ups {ups}")
            far.check([(d, blur_ref(oracle, blit_ref(oracle, img, W, H, False), taps, False))], f"far: seed kernel ups {ups}")
    finally:
        del far
        torch.cuda.empty_cache()


# -------------------------------------------------------------------------------------------------------------- invalid arguments
def test_invalid_arguments(L, oracle, T):
    """host-side checks only: nothing reaches the GPU, every destination keeps its poison"""
    rng = np.random.default_rng(13000)
    w, h, batch = 256, 64, 2
    src = make_src(oracle, rng, 0, (batch, h, w), False)
    A = HP.Arena()
    s = A.plane("src", w, h, batch, data=src)
    d, d2, nx = A.plane("dst", w, h, batch), A.plane("dst2", w, h, batch), A.plane("next", w // 2, h // 2, batch)
    A.build()
    null = HP.Plane(None, w, h, w, w * h, 0, 0)
    k5, k7, k9 = HP.taps_arg(T[5])[0], HP.taps_arg(T[7])[0], HP.taps_arg(T[9])[0]
    INV = HP.HIP_ERROR_INVALID_VALUE
    assert L.vksift_hip_blur(s.c(), s.c(), k5, 5, batch, None) == INV  # src.base == dst.base
    assert L.vksift_hip_blur(s.c(), d.c(), k5, 0, batch, None) == INV
    assert L.vksift_hip_blur(s.c(), d.c(), k5, 21, batch, None) == INV
    assert L.vksift_hip_blur(s.c(), null, k5, 5, batch, None) == INV
    assert L.vksift_hip_blur_downsample(s.c(), d.c(), nx.c(), k5, 0, batch, None) == INV
    assert L.vksift_hip_blur_downsample(s.c(), d.c(), nx.c(), k5, 21, batch, None) == INV
    assert L.vksift_hip_blur_downsample(s.c(), s.c(), nx.c(), k5, 5, batch, None) == INV
    assert L.vksift_hip_blur_downsample(s.c(), null, nx.c(), k5, 5, batch, None) == -1
    assert L.vksift_hip_blur_downsample(s.c(), d.c(), HP.Plane(None, w // 2, h // 2, w // 2, w * h // 4, 0, 0), k5, 5, batch, None) == -1
    assert L.vksift_hip_blur_pair(s.c(), null, d2.c(), k5, 5, k7, 7, batch, None) == -1
    assert L.vksift_hip_blur_pair(s.c(), d.c(), null, k5, 5, k7, 7, batch, None) == -1
    assert L.vksift_hip_blur_pair(s.c(), d.c(), d2.c(), k5, 0, k7, 7, batch, None) == -1
    assert L.vksift_hip_blur_pair(s.c(), d.c(), d2.c(), k5, 5, k7, 21, batch, None) == -1
    one = lambda p: (HP.Plane * 1)(p)
    assert L.vksift_hip_blur_multi(one(s.c()), one(null), 1, k9, 9, batch, None) == -1
    assert L.vksift_hip_blur_multi(one(s.c()), one(s.c()), 1, k9, 9, batch, None) == -1
    assert L.vksift_hip_blur_multi(one(s.c()), one(d.c()), 1, k9, 0, batch, None) == -1
    assert L.vksift_hip_blur_multi(one(s.c()), one(d.c()), 1, k9, 21, batch, None) == -1
    u = src.view(np.uint8)  # any bytes
    assert L.vksift_hip_seed_direct(s.ptr, w, h, w * h, d.c(), k5, 0, batch, None) == -1
    assert L.vksift_hip_seed_direct(s.ptr, w, h, w * h, d.c(), k5, 21, batch, None) == -1
    assert L.vksift_hip_seed_upsampled(s.ptr, w // 2, h // 2, w * h, d.c(), k5, 0, batch, None) == -1
    assert L.vksift_hip_seed_upsampled(s.ptr, w // 2, h // 2, w * h, d.c(), k5, 21, batch, None) == -1
    assert u.size
    HP.check_nothing_launched(A, "invalid arguments")
