"""vksift_hip_place_keypoints called directly, in the manner of tests/hip_records.py (plain module, no fixtures): the ctypes mirror of
vksift_hip_PlaceOctave, the case table, and a Launch that turns a case into ONE poisoned arena — the keypoints and their offsets, the SIFT
buffers of the batch with canary records behind every section, the counters and the placed words — and states the whole arena as the
contract expects it afterwards, from tests/np_describe.py: words 0..8 of the stored records, found, placed, and every other byte as it
went in (bytes 36..163 of every record, the records at and beyond a capacity, the gaps, the guards).

A case is small: counts around the wave (64) and the workgroup (256, a chunk of the walk), several chunks, several images with an empty one
among them, one and five octaves of odd sizes, the scale counts at both ends, a section that overflows, and keypoints that are not
admissible interleaved with the rest."""
import ctypes as C

import numpy as np

import hip_records as HR
import np_describe as ND
from hip_features import POISON_BYTE, POISON_WORD

REC = 164
WG = 256   # VKSIFT_HIP_PLACE_WG
f32, u32 = np.float32, np.uint32
SEED_SIGMA = 1.6


class PlaceOctave(C.Structure):
    """vksift_hip_PlaceOctave"""
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("octave_idx", C.c_int32), ("feats", C.c_void_p), ("feat_img_stride", C.c_uint64), ("cap", C.c_uint32),
                ("found", C.c_void_p), ("found_img_stride", C.c_uint32)]


def bind(L):
    L.vksift_hip_place_keypoints.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PlaceOctave), C.c_uint32, C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_void_p, C.c_void_p]
    L.vksift_hip_place_keypoints.restype = C.c_int
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


def halving(w, h, n, first_idx=-1):
    """n octaves from w x h, halving with floors"""
    return [(max(w >> o, 1), max(h >> o, 1), first_idx + o) for o in range(n)]


ODD5 = halving(33, 17, 5)    # 33x17, 16x8, 8x4, 4x2, 2x1
BAD = ("nan x", "inf y", "sigma 0", "sigma < 0", "x beyond", "y < 0", "rel > 29", "orientation 7", "-inf sigma", "nan sigma")


def make_keypoints(n, octs, S, kind, rng):
    """n keypoints over the image of octs[0]: positions up to both borders, sigma over the whole scale-space and beyond both of its ends. kind
    "mixed": every third one made inadmissible, the ways in turn; "one octave": all in the second octave, all admissible"""
    steps = ND.sigma_steps(SEED_SIGMA, S)
    w0, h0, i0 = octs[0]
    img_w, img_h = w0 * 2.0 ** i0, h0 * 2.0 ** i0
    k = np.zeros(n, ND.KEYPOINT_DTYPE)
    lo, hi = 0.4 * steps[0] * 2.0 ** i0, 2.5 * steps[S] * 2.0 ** octs[-1][2]
    k["sigma"] = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    o_of = rng.integers(0, len(octs), n)
    if kind == "one octave":
        o = min(1, len(octs) - 1)
        k["sigma"] = rng.uniform(steps[0], steps[S - 1], n) * 2.0 ** octs[o][2]
        o_of[:] = o
    # inside the octave the sigma will most likely fall in (a coarse octave of floored size covers less than the image)
    for i in range(n):
        c = ND.classify(k[i:i + 1], octs, steps)
        w, h, oi = octs[int(c["oct"][0])]
        k["x"][i], k["y"][i] = rng.uniform(0, w * 2.0 ** oi), rng.uniform(0, h * 2.0 ** oi)
    if n:
        k["x"][0], k["y"][0] = 0.0, 0.0
    k["orientation"] = rng.uniform(0, float(ND.TWO_PI32), n)
    k["response"] = rng.uniform(-0.3, 0.3, n)
    if kind == "mixed":
        for t, i in enumerate(range(1, n, 3)):
            bad = BAD[t % len(BAD)]
            if bad == "nan x":
                k["x"][i] = np.nan
            elif bad == "inf y":
                k["y"][i] = np.inf
            elif bad == "sigma 0":
                k["sigma"][i] = 0.0
            elif bad == "sigma < 0":
                k["sigma"][i] = -k["sigma"][i]
            elif bad == "x beyond":
                k["x"][i] = img_w + 1.0
            elif bad == "y < 0":
                k["y"][i] = -0.25
            elif bad == "rel > 29":
                k["sigma"][i] = 30.0 * 2.0 ** octs[-1][2]
            elif bad == "orientation 7":     # only looked at with keep_orientation
                k["orientation"][i] = 7.0
            elif bad == "-inf sigma":
                k["sigma"][i] = -np.inf
            elif bad == "nan sigma":
                k["sigma"][i] = np.nan
    return k


def case(name, counts, *, octs=ODD5, S=3, caps=None, keep=0, kind="mixed", seed=1):
    caps = list(caps) if caps is not None else [max(counts) + 3] * len(octs)
    assert len(caps) == len(octs)
    return dict(name=name, counts=list(counts), octs=list(octs), S=S, caps=caps, keep=keep, kind=kind, seed=seed)


CASES = []
for _i, _n in enumerate((0, 1, 63, 64, 65, WG - 1, WG, WG + 1, 4 * WG + 3)):
    CASES.append(case(f"{_n} keypoints, five octaves", [_n], keep=_i % 2, seed=10 + _i))
CASES += [
    case("three images, unequal, an empty one", [70, 0, 300], seed=30),
    case("three images, supplied orientations", [WG + 5, 3, 0], keep=1, seed=31),
    case("one octave", [130], octs=ODD5[:1], seed=32),
    case("one octave, S 1", [90], octs=halving(33, 17, 1, 0), S=1, keep=1, seed=33),
    case("five octaves, S 1", [200], S=1, seed=34),
    case("five octaves, S 13", [300], S=13, keep=1, seed=35),
    case("every keypoint in one octave", [2 * WG + 9], kind="one octave", seed=36),
    case("sixteen octaves", [500], octs=halving(1 << 15, 1 << 14, 16, -1), seed=37),
    case("capacities 4, 0 and 1", [400, 37], caps=[4, 0, 1, 400, 2], seed=38),
]
# a section of capacity 4 that receives ten: the first four in input order, found 10, placed counts 4
CASES.append(case("capacity 4 receiving 10", [10], octs=ODD5[:2], caps=[20, 4], kind="one octave", seed=39))
assert len({c["name"] for c in CASES}) == len(CASES)


def case_named(name):
    (c,) = [c for c in CASES if c["name"] == name]
    return c


CANARY = 2   # records behind every section that must stay as they were


class Place(HR.Launch):
    entry = "place_keypoints"

    def __init__(self, c, device="cuda"):
        super().__init__(c, device)
        rng = np.random.default_rng(c["seed"])
        self.batch, self.n_oct = len(c["counts"]), len(c["octs"])
        self.lists = [make_keypoints(n, c["octs"], c["S"], c["kind"], rng) for n in c["counts"]]
        # a keypoint behind the last list that would be stored if it were read
        decoy = np.array([(1.0, 1.0, 1.0, 0.5, 0.9)], ND.KEYPOINT_DTYPE)
        self.kps = self.block("keypoints", np.concatenate(self.lists + [decoy]), row_bytes=20)
        first = np.concatenate([[0], np.cumsum(c["counts"])]).astype(u32)
        self.first = self.block("offsets", np.concatenate([first, [POISON_WORD]]).astype(u32), row_bytes=4)
        self.sec_off = np.concatenate([[0], np.cumsum([cap + CANARY for cap in c["caps"]])]).astype(np.int64)
        self.img_stride = int(self.sec_off[-1]) * REC + 12
        self.feats = self.poison("SIFT buffers", self.batch * self.img_stride, slot_bytes=self.img_stride, row_bytes=REC)
        self.fstride = self.n_oct + 2
        self.found = self.poison("section counters", self.batch * self.fstride * 4, slot_bytes=4 * self.fstride, row_bytes=4)
        self.placed = self.poison("placed", (self.batch + 2) * 4, row_bytes=4)
        self.build()
        self.steps = ND.sigma_steps(SEED_SIGMA, c["S"])
        octs = (PlaceOctave * 20)()
        for o, (w, h, oi) in enumerate(c["octs"]):
            octs[o] = PlaceOctave(w, h, oi, self.feats.ptr + int(self.sec_off[o]) * REC, self.img_stride, c["caps"][o], self.found.ptr + 4 * o, self.fstride)
        self.args = dict(kps=self.kps.ptr, kp_first=self.first.ptr, oct=octs, n_oct=self.n_oct, sigma_steps=(C.c_float * 16)(*[float(s) for s in self.steps]),
                         S=c["S"], keep_orientation=c["keep"], batch=self.batch, placed=self.placed.ptr)

    def spec(self, b):
        c = self.case
        return ND.place(self.lists[b], c["octs"], c["caps"], self.steps, bool(c["keep"]))

    def expected(self):
        exp = self.host.copy()
        feats, found, placed = self.view(exp, self.feats), self.view(exp, self.found, u32), self.view(exp, self.placed, u32)
        for b in range(self.batch):
            sections, cnt, stored, _ = self.spec(b)
            for o, words in enumerate(sections):
                for r in range(len(words)):
                    at = b * self.img_stride + (int(self.sec_off[o]) + r) * REC
                    feats[at:at + 36] = words[r].astype("<u4").view(np.uint8)
                found[b * self.fstride + o] = cnt[o]
            placed[b] = stored
        return exp


# (a case of the table, the arguments changed): hipErrorInvalidValue, and the arena as it was
_R = "three images, unequal, an empty one"
REFUSALS = [(_R, {"n_oct": 0}), (_R, {"n_oct": 17}), (_R, {"S": 0}), (_R, {"S": 14}), (_R, {"oct": None}), (_R, {"sigma_steps": None})]
