"""Plain numpy statement of the keypoint placement (vksift_hip_place_keypoints, vksift_ext_describeKeypoints): the specification. fp32, every
operation rounded once, in the order of include/vksift_hip.h; the kernel only compares against the host-made table, and so does this.

  sigma_steps(seed_sigma, S)        the S + 1 thresholds (float)(seed_sigma * 2^((j + 0.5) / S)), evaluated in double
  octaves_for(w, h, ups)            the octaves of an image: [(w, h, octave_idx)] (vksift_hostmath.c: vksift_hm_octaves_for)
  classify(kps, octs, steps, keep)  per keypoint: octave, scale_idx, scale_x, scale_y, admissible
  place(kps, octs, caps, steps, keep)   the sections' header words in input order, the un-clamped counters, the records stored
  classify_double(...)              the same rule with the logarithm in double precision: what the table approximates

TEST INFRASTRUCTURE ONLY."""
import numpy as np

f32 = np.float32
u32 = np.uint32
TWO_PI32 = f32(f32(2.0) * f32(3.14159265358979323846))
REL_MIN, REL_MAX = f32(0.02), f32(29.0)     # the window range the orientation and descriptor launchers are specified for
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("sigma", "<f4"), ("orientation", "<f4"), ("response", "<f4")])
HEAD_WORDS = 9
assert KEYPOINT_DTYPE.itemsize == 20


def sigma_steps(seed_sigma, S):
    seed = float(f32(seed_sigma))
    return np.array([f32(seed * 2.0 ** ((j + 0.5) / S)) for j in range(S + 1)], f32)


def octaves_for(w, h, ups=True, max_octaves=16):
    """[(w_o, h_o, octave_idx)]: float arithmetic as in vksift_hm_octaves_for"""
    fn = f32(f32(np.log2(f32(min(w, h)))) - f32(4) + f32(1 if ups else 0))
    n = int(fn) if fn >= 1 else 0
    n = min(n, max_octaves)
    first = f32(0.5 if ups else 1.0)
    out = []
    for o in range(n):
        inv = f32(f32(1.0) / f32(f32(2.0 ** o) * first))
        out.append((int(f32(inv * f32(w))), int(f32(inv * f32(h))), o - (1 if ups else 0)))
    return out


def _pow2(n):
    return f32(2.0 ** int(n))   # exact


def classify(kps, octs, steps, keep_orientation=False):
    """kps: KEYPOINT_DTYPE array; octs: [(w, h, octave_idx)]; steps: sigma_steps(). Returns a dict of arrays: oct (index into octs), scale_idx,
    scale_x, scale_y, rel (all per keypoint) and adm (bool)."""
    kps = np.asarray(kps, KEYPOINT_DTYPE)
    steps = np.asarray(steps, f32)
    S, n, n_oct = len(steps) - 1, len(kps), len(octs)
    assert 1 <= n_oct <= 16 and 1 <= S <= 13
    sigma, x, y, ori = kps["sigma"], kps["x"], kps["y"], kps["orientation"]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        oct_ = np.full(n, n_oct - 1, np.int64)
        chosen = np.zeros(n, bool)
        for o in range(n_oct):
            r = (sigma * _pow2(-octs[o][2])).astype(f32)
            take = ~chosen & (r < steps[S])
            oct_[take] = o
            chosen |= take
        inv = np.array([_pow2(-octs[o][2]) for o in oct_], f32).reshape(n)
        wf = np.array([f32(octs[o][0]) for o in oct_], f32).reshape(n)
        hf = np.array([f32(octs[o][1]) for o in oct_], f32).reshape(n)
        rel = (sigma * inv).astype(f32)
        scale_idx = np.zeros(n, u32)
        for j in range(S + 1):
            scale_idx += (rel >= steps[j]).astype(u32)
        sx, sy = (x * inv).astype(f32), (y * inv).astype(f32)
        adm = np.isfinite(x) & np.isfinite(y) & np.isfinite(sigma) & (rel >= REL_MIN) & (rel <= REL_MAX) & (sx >= 0) & (sx < wf) & (sy >= 0) & (sy < hf)
        if keep_orientation:
            adm &= (ori >= 0) & (ori <= TWO_PI32)
    return dict(oct=oct_, scale_idx=scale_idx, scale_x=sx, scale_y=sy, rel=rel, adm=adm)


def header_words(kps, octs, c, keep_orientation):
    """(n, 9) uint32: the record head of every keypoint as the placement writes it (admissible or not)"""
    kps = np.asarray(kps, KEYPOINT_DTYPE)
    n = len(kps)
    w = np.zeros((n, HEAD_WORDS), u32)
    w[:, 0], w[:, 1] = kps["x"].view(u32), kps["y"].view(u32)
    w[:, 2], w[:, 3] = c["scale_x"].view(u32), c["scale_y"].view(u32)
    w[:, 4] = c["scale_idx"]
    w[:, 5] = np.array([octs[o][2] for o in c["oct"]], np.int32).reshape(n).view(u32)
    w[:, 6] = kps["sigma"].view(u32)
    w[:, 7] = kps["orientation"].view(u32) if keep_orientation else 0
    w[:, 8] = kps["response"].view(u32)
    return w


def place(kps, octs, caps, steps, keep_orientation=False):
    """-> (sections, found, placed, index): sections[o] = (min(found[o], caps[o]), 9) uint32 header words in input order; found[o] un-clamped;
    placed = records stored; index[o] = the input indices of the stored keypoints of octave o"""
    c = classify(kps, octs, steps, keep_orientation)
    words = header_words(kps, octs, c, keep_orientation)
    sections, found, index = [], [], []
    for o in range(len(octs)):
        idx = np.flatnonzero(c["adm"] & (c["oct"] == o))
        found.append(len(idx))
        idx = idx[:caps[o]]
        index.append(idx)
        sections.append(words[idx])
    return sections, found, sum(len(s) for s in sections), index


def classify_double(sigma, octs, seed_sigma, S):
    """(octave index into octs, scale_idx) of every sigma by the rule the table stands for, with the logarithm in double precision:
    ss = S * log2(sigma / (seed_sigma * 2^octave_idx)); the first octave with ss < S + 0.5 (the last otherwise); scale_idx = the number of
    j in 0 .. S with ss >= j + 0.5"""
    sigma = np.asarray(sigma, np.float64)
    n_oct = len(octs)
    seed = float(f32(seed_sigma))
    oct_ = np.full(len(sigma), n_oct - 1, np.int64)
    chosen = np.zeros(len(sigma), bool)
    for o in range(n_oct):
        ss = S * np.log2(sigma / (seed * 2.0 ** octs[o][2]))
        take = ~chosen & (ss < S + 0.5)
        oct_[take] = o
        chosen |= take
    oi = np.array([octs[o][2] for o in oct_], np.float64).reshape(len(sigma))
    ss = S * np.log2(sigma / (seed * 2.0 ** oi))
    scale_idx = np.zeros(len(sigma), np.int64)
    for j in range(S + 1):
        scale_idx += ss >= j + 0.5
    return oct_, scale_idx
