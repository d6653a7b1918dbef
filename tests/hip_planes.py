"""Plane-level access to the pyramid launchers of include/vksift_hip.h for tests (plain module, no fixtures).

  * Plane / bind(): the ctypes vksift_hip_Plane and the argtypes of every launcher of the header's "pyramid" section
  * Arena: ONE byte tensor on the GPU that holds every plane of a case. Whatever is not a valid source texel holds a poison
    pattern — a quiet NaN with a recognisable payload for fp32 and binary16 texels, 0xA5 for u8 — and guard zones at least as large
    as the largest plane lie in front of the first plane and behind the last one. A kernel that USES a texel outside a valid extent
    carries the NaN into its result; a kernel that STORES outside the valid extent of its destination changes a poisoned byte.
  * FarArena: the same for two images more than 4 GiB apart (filled and checked on the device)
  * assert_plane_equal / assert_untouched: bit comparisons that name the first differing texel or byte

Contract checked by assert_untouched (vksift_hip_Plane): a launch writes the valid w x h extent of every image of its destination
planes and nothing else — not the pitch padding, not the rows below h, not the gap between images, not another plane.
"""
import ctypes as C

import numpy as np

MAX_TAPS = 20
HIP_ERROR_INVALID_VALUE = 1
TUNE_WG_TARGET, TUNE_WIDE_MASK, TUNE_MULTI_MAX, TUNE_PAIR_FORM, TUNE_MIN_MARCH = 0, 1, 2, 5, 12
CH_MAX_OCT, CH_MAX_LAYERS, CH_LDS_FLOATS = 4, 8, 19200 * 2  # vksift_hip_octave_chain (pyramid.hip)

POISON_F32 = 0x7FC5A5A5  # quiet NaN, payload 0x05A5A5
POISON_F16 = 0x7EA5      # quiet NaN, payload 0xA5
POISON_U8 = 0xA5
KINDS = {"f32": (4, np.uint32, POISON_F32), "f16": (2, np.uint16, POISON_F16), "u8": (1, np.uint8, POISON_U8)}
ALIGN = 256


class Plane(C.Structure):
    _fields_ = [("base", C.c_void_p), ("w", C.c_uint32), ("h", C.c_uint32), ("pitch", C.c_uint32), ("img_stride", C.c_uint64),
                ("fp16", C.c_uint32), ("reverse", C.c_uint32)]


def bind(L):
    """argtypes / restype of the pyramid launchers (and the two knobs they read) on a loaded libvulkansift."""
    f32p, u32p, u8p, pp, u32, u64, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(Plane), C.c_uint32, C.c_uint64, C.c_void_p
    sigs = {
        "vksift_hip_input_blit": [u8p, u32, u32, u64, Plane, u32, vp],
        "vksift_hip_blur": [Plane, Plane, f32p, u32, u32, vp],
        "vksift_hip_blur_pair": [Plane, Plane, Plane, f32p, u32, f32p, u32, u32, vp],
        "vksift_hip_blur_form": [Plane, Plane, u32, u32],
        "vksift_hip_blur_multi": [pp, pp, u32, f32p, u32, u32, vp],
        "vksift_hip_blur_downsample": [Plane, Plane, Plane, f32p, u32, u32, vp],
        "vksift_hip_seed_upsampled": [u8p, u32, u32, u64, Plane, f32p, u32, u32, vp],
        "vksift_hip_seed_direct": [u8p, u32, u32, u64, Plane, f32p, u32, u32, vp],
        "vksift_hip_downsample": [Plane, Plane, u32, vp],
        "vksift_hip_octave_chain": [pp, u32, u32, u32, f32p, u32p, u32, vp],
        "vksift_hip_dog_plane": [vp, vp, u32, u32, u32, u32, vp, vp],
        "vksift_hip_tune": [C.c_int, C.c_int],
        "vksift_hip_tune_get": [C.c_int],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


def taps_arg(taps):
    """one-sided taps (centre first) as the float[VKSIFT_HIP_MAX_TAPS] the launchers read, and their number"""
    taps = np.asarray(taps, np.float32)
    assert taps.ndim == 1 and len(taps) <= MAX_TAPS + 1
    buf = (C.c_float * (MAX_TAPS + 4))(*taps.tolist())
    return buf, len(taps)


def to_bits(values, kind):
    """what a plane of this texel type holds for these float32 values (already exact in the type), as unsigned integers"""
    values = np.asarray(values)
    if kind == "f32":
        return np.ascontiguousarray(values, np.float32).view(np.uint32)
    if kind == "f16":
        h = np.ascontiguousarray(values, np.float32).astype(np.float16)
        assert np.array_equal(h.astype(np.float32).view(np.uint32), np.ascontiguousarray(values, np.float32).view(np.uint32)), "not binary16 values"
        return h.view(np.uint16)
    return np.ascontiguousarray(values, np.uint8)


class PlaneRef:
    """One batch of same-sized planes inside an arena: `data` (batch, h, w) makes it a source, None leaves it all poison."""

    def __init__(self, name, kind, w, h, batch, pitch, img_stride, offset, data):
        self.name, self.kind, self.w, self.h, self.batch = name, kind, int(w), int(h), int(batch)
        self.pitch = int(pitch if pitch is not None else w)
        self.img_stride = int(img_stride if img_stride is not None else self.pitch * self.h)
        self.offset = int(offset)
        assert self.pitch >= self.w and self.img_stride >= self.pitch * self.h and self.w > 0 and self.h > 0 and self.batch > 0
        self.es, self.utype, self.poison = KINDS[kind]
        self.texels = (self.batch - 1) * self.img_stride + self.pitch * self.h  # every image spans pitch * h texels
        self.data = None if data is None else to_bits(data, kind).reshape(self.batch, self.h, self.w)
        self.byte_off = None
        self.ptr = None

    @property
    def nbytes(self):
        return self.texels * self.es

    def view(self, raw, base=None):
        """the (batch, h, w) valid texels inside the arena bytes `raw`"""
        off = self.byte_off if base is None else base
        flat = raw[off:off + self.nbytes].view(self.utype)
        return np.lib.stride_tricks.as_strided(flat, (self.batch, self.h, self.w), (self.img_stride * self.es, self.pitch * self.es, self.es))

    def c(self, reverse=0, w=None, h=None):
        assert self.ptr is not None, "arena not built"
        assert self.kind != "u8"
        return Plane(self.ptr, self.w if w is None else w, self.h if h is None else h, self.pitch, self.img_stride, 1 if self.kind == "f16" else 0, reverse)


class Arena:
    """planes are declared with plane(), then build() lays them out between two guard zones, poisons everything, writes the sources
    and uploads; read() downloads the whole arena."""

    def __init__(self, device="cuda"):
        self.device, self.planes, self.host, self.dev = device, [], None, None

    def plane(self, name, w, h, batch=1, *, kind="f32", pitch=None, img_stride=None, offset=0, data=None):
        p = PlaneRef(name, kind, w, h, batch, pitch, img_stride, offset, data)
        self.planes.append(p)
        return p

    def build(self):
        import torch

        up = lambda n: (n + ALIGN - 1) // ALIGN * ALIGN
        self.guard = up(max(p.nbytes for p in self.planes) + ALIGN)
        pos = self.guard
        for p in self.planes:
            p.byte_off = pos + p.offset * p.es
            pos = up(p.byte_off + p.nbytes) + ALIGN  # a poisoned gap between neighbours
        total = pos + self.guard
        host = np.empty(total, np.uint8)
        host.view(np.uint32)[:] = POISON_F32
        for p in self.planes:
            host[p.byte_off:p.byte_off + p.nbytes].view(p.utype)[:] = p.poison
            if p.data is not None:
                p.view(host)[...] = p.data
        self.host = host
        self.dev = torch.from_numpy(host).to(self.device, copy=True)
        base = self.dev.data_ptr()
        for p in self.planes:
            p.ptr = base + p.byte_off
        return self

    def read(self):
        import torch

        if self.dev.is_cuda:
            torch.cuda.synchronize()
        return self.dev.cpu().numpy().copy()

    def expected(self, results):
        """the arena as it must look after a launch: `results` = [(destination PlaneRef, values (batch, h, w))]"""
        exp = self.host.copy()
        for p, values in results:
            p.view(exp)[...] = to_bits(values, p.kind).reshape(p.batch, p.h, p.w)
        return exp

    def where(self, byte):
        for p in self.planes:
            if p.byte_off <= byte < p.byte_off + p.nbytes:
                t = (byte - p.byte_off) // p.es
                img, r = divmod(t, p.img_stride)
                y, x = divmod(r, p.pitch)
                part = "valid extent" if (x < p.w and y < p.h) else ("pitch padding" if y < p.h else "between images")
                return f"plane {p.name!r} image {img} y {y} x {x} ({part}; w {p.w} h {p.h} pitch {p.pitch} img_stride {p.img_stride})"
        return "guard zone / gap between planes"


def assert_plane_equal(got, ref, what):
    """bit patterns of two (batch, h, w) arrays; reports the first differing (image, y, x) and the number of differing texels"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(got != ref)
    if len(bad):
        i, y, x = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} texels differ, first at image {i} y {y} x {x}: "
                             f"got 0x{int(got[i, y, x]):x}, expected 0x{int(ref[i, y, x]):x}")


def assert_untouched(arena, planes, after):
    """every byte of the arena outside the valid w x h extents of the destination `planes` still holds what build() put there"""
    exp = arena.host.copy()
    for p in planes:
        p.view(exp)[...] = p.view(after)
    bad = np.flatnonzero(after != exp)
    if len(bad):
        b = int(bad[0])
        raise AssertionError(f"{len(bad)} bytes outside the destination extents were overwritten, first at arena byte {b}: {arena.where(b)}: "
                             f"0x{int(exp[b]):02x} -> 0x{int(after[b]):02x}")


def check_launch(arena, results, what):
    """after a launch that returned 0: every destination equals its reference bit for bit and nothing else changed"""
    after = arena.read()
    if np.array_equal(after, arena.expected(results)):
        return
    for p, values in results:
        assert_plane_equal(p.view(after), to_bits(values, p.kind).reshape(p.batch, p.h, p.w), f"{what}: plane {p.name!r}")
    assert_untouched(arena, [p for p, _ in results], after)
    raise AssertionError(f"{what}: arena differs")  # (not reached)


def check_nothing_launched(arena, what):
    """after a launch that declined (-1) or refused its arguments: every byte still holds what build() put there"""
    after = arena.read()
    if not np.array_equal(after, arena.host):
        b = int(np.flatnonzero(after != arena.host)[0])
        raise AssertionError(f"{what}: returned without launching, yet arena byte {b} changed: {arena.where(b)}")


class FarArena:
    """Two images whose bytes lie more than 4 GiB apart: one device allocation, poisoned and checked on the device. Planes are placed
    at explicit byte offsets of image 0; image 1 follows `gap_bytes` later."""

    def __init__(self, gap_bytes=(1 << 32) + (1 << 20), room_bytes=1 << 26, guard_bytes=1 << 28, device="cuda"):
        import torch

        self.gap, self.room, self.guard = gap_bytes, room_bytes, guard_bytes
        self.total = 2 * guard_bytes + gap_bytes + room_bytes
        self.dev = torch.empty(self.total, dtype=torch.uint8, device=device)
        self.words = self.dev.view(torch.int32)
        self.poison = int(np.uint32(POISON_F32).view(np.int32))
        self.words.fill_(self.poison)
        self.placed = []

    def plane(self, name, w, h, *, kind="f32", pitch=None, room_off=0, data=None):
        """a batch of two; room_off: byte offset of image 0 inside the room (256-byte aligned offsets keep every alignment)"""
        import torch

        es = KINDS[kind][0]
        pitch = int(pitch if pitch is not None else w)
        assert self.gap % es == 0 and room_off % es == 0 and room_off + pitch * h * es <= self.room
        p = PlaneRef(name, kind, w, h, 2, pitch, self.gap // es, 0, data)
        p.byte_off = self.guard + room_off
        p.ptr = self.dev.data_ptr() + p.byte_off
        one = PlaneRef(name, kind, w, h, 1, pitch, None, 0, None)
        p.spans = []
        for b in range(2):
            span = np.empty(one.nbytes, np.uint8)
            span.view(one.utype)[:] = one.poison
            if p.data is not None:
                one.view(span, 0)[0] = p.data[b]
            p.spans.append(span)
            lo = p.byte_off + b * self.gap
            self.dev[lo:lo + one.nbytes] = torch.from_numpy(span).to(self.dev.device)
        p.one = one
        self.placed.append(p)
        return p

    def check(self, results, what):
        """destinations equal their references, every other byte of every placed span is unchanged; then the spans are poisoned again
        and the WHOLE allocation must hold the poison (the guards, the 4 GiB between the images, the rest of the room)"""
        import torch

        torch.cuda.synchronize()
        want = {id(p): v for p, v in results}
        for p in self.placed:
            for b in range(2):
                lo = p.byte_off + b * self.gap
                got = self.dev[lo:lo + p.one.nbytes].cpu().numpy()
                exp = p.spans[b].copy()
                if id(p) in want:
                    ref = to_bits(want[id(p)], p.kind).reshape(2, p.h, p.w)
                    assert_plane_equal(p.one.view(got, 0), ref[b:b + 1], f"{what}: plane {p.name!r} image {b}")
                    p.one.view(exp, 0)[0] = ref[b]
                assert np.array_equal(got, exp), f"{what}: plane {p.name!r} image {b}: bytes outside the valid extent changed"
                self.dev[lo:lo + p.one.nbytes].view(torch.int32).fill_(self.poison)
        stray = int((self.words != self.poison).sum().item())
        assert stray == 0, f"{what}: {stray} words outside every plane were overwritten"
        self.placed = []
