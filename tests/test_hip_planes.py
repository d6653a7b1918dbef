"""tests/hip_planes.py on the CPU: the arena's layout and poison, and that its checks catch what the GPU sweep relies on them to catch
(a wrong texel, a store into the pitch padding, between images, into another plane or a guard zone, a write after a declined launch)."""
import ctypes as C

import numpy as np
import pytest

import hip_planes as HP


def build(kind="f32", offset=1):
    rng = np.random.default_rng(1)
    src = rng.random((2, 5, 6), dtype=np.float32)
    if kind == "f16":
        src = src.astype(np.float16).astype(np.float32)
    A = HP.Arena(device="cpu")
    s = A.plane("src", 6, 5, 2, kind=kind, pitch=9, img_stride=50, offset=offset, data=src)
    d = A.plane("dst", 6, 5, 2, kind=kind, pitch=7, img_stride=36, offset=4)
    A.build()
    return A, s, d, src


def raw(A):
    return np.frombuffer((C.c_uint8 * A.host.size).from_address(A.dev.data_ptr()), np.uint8)


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_layout_and_poison(kind):
    A, s, d, src = build(kind)
    es = HP.KINDS[kind][0]
    assert A.guard >= max(s.nbytes, d.nbytes) and s.byte_off >= A.guard and A.host.size - (d.byte_off + d.nbytes) >= A.guard
    assert (s.ptr - A.dev.data_ptr()) % 256 == es and (d.ptr - A.dev.data_ptr()) % 256 == 4 * es and d.byte_off >= s.byte_off + s.nbytes + 256
    assert np.array_equal(s.view(A.host), HP.to_bits(src, kind))
    assert np.all(d.view(A.host) == HP.KINDS[kind][2])
    # everything that is not a source texel is a NaN of the plane's type (or the guards' fp32 NaN)
    span = A.host[s.byte_off:s.byte_off + s.nbytes].view(HP.KINDS[kind][1]).copy()
    np.lib.stride_tricks.as_strided(span, (2, 5, 6), (50 * es, 9 * es, es))[...] = 0
    assert set(span.tolist()) == {0, HP.KINDS[kind][2]}
    assert np.isnan(np.array([HP.POISON_F32], np.uint32).view(np.float32)[0]) and np.isnan(np.array([HP.POISON_F16], np.uint16).view(np.float16)[0])
    c = d.c(reverse=1)
    assert (c.base, c.w, c.h, c.pitch, c.img_stride, c.fp16, c.reverse) == (d.ptr, 6, 5, 7, 36, int(kind == "f16"), 1)


def test_checks_pass_and_catch():
    A, s, d, src = build()
    ref = src * np.float32(2)
    HP.check_nothing_launched(A, "idle")
    d.view(raw(A))[...] = HP.to_bits(ref, "f32")
    HP.check_launch(A, [(d, ref)], "exact")
    with pytest.raises(AssertionError, match="returned without launching"):
        HP.check_nothing_launched(A, "declined")
    # a wrong texel: named by image, row and column
    d.view(raw(A))[1, 3, 2] ^= 1
    with pytest.raises(AssertionError, match=r"1 of 60 texels differ, first at image 1 y 3 x 2"):
        HP.check_launch(A, [(d, ref)], "one bit")
    d.view(raw(A))[1, 3, 2] ^= 1
    # a NaN carried in from poisoned padding differs from any finite reference
    d.view(raw(A))[0, 0, 0] = HP.POISON_F32
    with pytest.raises(AssertionError, match="image 0 y 0 x 0"):
        HP.check_launch(A, [(d, ref)], "nan")
    d.view(raw(A))[...] = HP.to_bits(ref, "f32")
    words = raw(A).view(np.uint32)
    for byte, where in ((d.byte_off + 4 * 6, "pitch padding"), (d.byte_off + 4 * 35, "between images"), (s.byte_off + 4 * 7, "plane 'src'"),
                        (8, "guard zone"), (A.host.size - 4, "guard zone"), (s.byte_off, "plane 'src' image 0 y 0 x 0 .valid extent")):
        old = int(words[byte // 4])
        words[byte // 4] = 0
        with pytest.raises(AssertionError, match=where):
            HP.check_launch(A, [(d, ref)], "stray store")
        words[byte // 4] = old
    HP.check_launch(A, [(d, ref)], "restored")


def test_to_bits_refuses_inexact_binary16():
    with pytest.raises(AssertionError):
        HP.to_bits(np.array([1 / 3], np.float32), "f16")
    assert HP.to_bits(np.array([0.5], np.float32), "f16").tolist() == [0x3800]
