"""Planes for the direct tests of vksift_hip_extract_keypoints (tests/test_gpu_extract_launcher.py launches them, tests/test_extract_reference.py
pins on the CPU what each of them reaches). Plain module, no fixtures, deterministic.

The extraction stage only ever sees a Gaussian stack through its differences, so the planes are built DoG-first: a target DoG stack D[0..S+1] of
small dyadic values (multiples of Q = 2^-10, magnitudes below 2) and Gaussian layers G[anchor] = base, G[l+1] = G[l] + D[l], so that the
subtraction the kernels perform gives back D bit for bit — in fp32, and in binary16 after the rounding the binary16 pyramid applies to a DoG
texel. gauss_from_dog() asserts that. Exact values are what lets a case place TIES on purpose: blurred images almost never hold one.

  * bump(): an isolated, refinable extremum at a chosen (x, y, s): the separable quadratic peak P - 8 dx^2 - 8 dy^2 - 16 ds^2 (in units of Q,
    cut at 0), of either sign; gradient 0 at its centre, so the refinement converges at once and accepts it. plateau = (dx, dy, ds): the
    pointwise maximum of two such peaks one step apart — two EQUAL texels, neither of which is a strict extremum: the 26 strict comparisons
    yield no candidate, a `>=` anywhere yields one or two (which the refinement accepts: tests/test_extract_reference.py proves it per case).
  * skew(): a peak whose refined value lies 50 % above its centre texel (both in-plane neighbours on one side far below it), for the cases
    around the candidate threshold |c| > 0.8 * dog_threshold, where the acceptance test |value| > dog_threshold must still pass
  * ridge(): a peak with a principal-curvature ratio of 30 (rejected by the edge test unless edge_limit is infinite)
  * noise(): seeded integer noise (full of ties, of candidates that walk in x, y and s, run into the clamps and read the missing DoG layer
    S + 2 of quirk Q1), periodic(): the 2x2-periodic stack that holds the most candidates an octave can have (tests/test_extraction_limits.py)
  * candidates() / refine_trace(): the 26 strict comparisons and the refinement of ExtractKeypoints.comp restated in numpy fp32 scalars, for the
    facts the oracle does not report: which texels are candidates, where each one walks, which clamp it meets. The records themselves always
    come from the oracle; test_extract_reference.py checks that this restatement accepts exactly the oracle's keypoints, bit for bit.
"""
import functools

import numpy as np

f32 = np.float32
Q = 2.0 ** -10
P = 64  # peak height of a bump in units of Q: 0.0625 > the default dog_threshold 0.04 / S for every S


# ---------------------------------------------------------------------------------------------------------------- DoG -> Gaussian layers
def base_plane(h, w):
    """a non-constant layer 0 in multiples of Q below 1/16: a kernel that reads the wrong texel of a layer reads another value"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx * 3 + yy * 5) % 61) * Q).astype(f32)


def gauss_from_dog(D, *, fp16=False, anchor=0, base=None):
    """(S + 3, h, w) float32 Gaussian layers with G[l + 1] - G[l] == D[l] exactly (asserted)"""
    D = np.asarray(D, f32)
    n, h, w = D.shape
    G = np.empty((n + 1, h, w), f32)
    G[anchor] = base_plane(h, w) if base is None else base
    r16 = (lambda v: v.astype(np.float16).astype(f32)) if fp16 else (lambda v: v)   # (a layer next to a subnormal difference absorbs it)
    for l in range(anchor, n):
        G[l + 1] = r16(G[l] + D[l])
    for l in range(anchor - 1, -1, -1):
        G[l] = r16(G[l + 1] - D[l])
    diff = G[1:] - G[:-1]
    assert np.isfinite(G).all()
    if fp16:
        assert np.array_equal(G.astype(np.float16).astype(f32).view(np.uint32), G.view(np.uint32)), "the layers are not binary16 values"
        diff = diff.astype(np.float16).astype(f32)
    assert np.array_equal(diff.view(np.uint32), D.view(np.uint32)), "the layers do not give the DoG stack back bit for bit"
    return G


# ---------------------------------------------------------------------------------------------------------------- peaks
def _peak(dx, dy, ds):
    return np.maximum(P - 8 * dx * dx - 8 * dy * dy - 16 * ds * ds, 0)


def _stamp(D, x, y, s, fn, sign, rx=2, ry=2, rs=1, q=Q):
    """adds sign * q * fn(dx, dy, ds) on the box around (x, y, s), clipped to the stack; the box must still be empty"""
    n, h, w = D.shape
    s0, s1, y0, y1, x0, x1 = max(s - rs, 0), min(s + rs + 1, n), max(y - ry, 0), min(y + ry + 1, h), max(x - rx, 0), min(x + rx + 1, w)
    ds, dy, dx = np.mgrid[s0 - s:s1 - s, y0 - y:y1 - y, x0 - x:x1 - x]
    assert not D[s0:s1, y0:y1, x0:x1].any(), ("peaks overlap", x, y, s)
    D[s0:s1, y0:y1, x0:x1] = (sign * q * fn(dx, dy, ds)).astype(f32) + f32(0)   # (no -0: G + -0 - G is +0)


def bump(D, x, y, s, sign=1, plateau=None):
    """an isolated maximum (sign 1) or minimum (-1) at texel (x, y) of DoG layer s; plateau (dx, dy, ds): the texel one step further holds the
    same value"""
    if plateau is None:
        _stamp(D, x, y, s, _peak, sign)
        return
    px, py, ps = plateau
    _stamp(D, x, y, s, lambda dx, dy, ds: np.maximum(_peak(dx, dy, ds), _peak(dx - px, dy - py, ds - ps)), sign, 2 + abs(px), 2 + abs(py), 1 + abs(ps))


def skew(D, x, y, s, c, sign=1):
    """centre value c (any fp32 value), x + 1 and y + 1 one Q below it, x - 1 and y - 1 at c - 2c = -c: the refined value is c + c / 2 with
    offsets just below 0.5; layers s - 1 and s + 1 stay zero (no coupling between the axes). Needs anchor = s and base = 0 in
    gauss_from_dog: then G[s + 1] = G[s + 2] = D[s] and G[s - 1] = 0 are exact whatever c is. (The corner at c - 4c is an extremum of the
    other sign, the same for every c.)"""
    c = f32(c)
    fx = {-1: f32(2) * c, 0: f32(0), 1: f32(Q)}
    pat = np.empty((3, 3), f32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            pat[dy + 1, dx + 1] = f32(f32(c - fx[dx]) - fx[dy])
    assert not D[s - 1:s + 2, y - 1:y + 2, x - 1:x + 2].any()
    D[s, y - 1:y + 2, x - 1:x + 2] = f32(sign) * pat


def ridge(D, x, y, s, sign=1):
    """curvature 2 Q along x and 60 Q along y: edgeness 32, above (10 + 1)^2 / 10"""
    _stamp(D, x, y, s, lambda dx, dy, ds: np.maximum(P - dx * dx - 30 * dy * dy - 32 * ds * ds, 0), sign, rx=7, ry=1, rs=1)


def inverted(D, x, y, s, centre):
    """a pit (the negated peak) whose centre texel alone is `centre` > 0, a value as small as a denormal: a strict maximum of its 26
    neighbours, all of them below -40 Q, with |c| above a threshold of 0 only if nothing flushes it to zero"""
    _stamp(D, x, y, s, _peak, -1)
    D[s, y, x] = f32(centre)


def noise(S, h, w, seed, amp=96):
    """integers -amp .. amp times Q: about one texel in eight of a scale is a candidate, and ties are everywhere"""
    return (np.random.default_rng(seed).integers(-amp, amp + 1, (S + 2, h, w)) * Q).astype(f32)


def periodic(S, h, w):
    """+64 Q on (odd, odd), -64 Q on (even, even) texels, at full amplitude on the odd DoG layers and at half on the even ones: every 2x2 block
    of the interior of an odd layer holds a maximum and a minimum, all of them accepted"""
    yy, xx = np.mgrid[0:h, 0:w]
    alt = np.where((yy % 2 == 1) & (xx % 2 == 1), 64.0, np.where((yy % 2 == 0) & (xx % 2 == 0), -64.0, 0.0)) * Q
    return np.stack([alt * (1.0 if l % 2 else 0.5) for l in range(S + 2)]).astype(f32)


# ---------------------------------------------------------------------------------------------------------------- the stage restated
def thresholds(S, intensity_threshold=0.04, edge_threshold=10.0):
    """(dog_threshold, edge_limit) as the host and the oracle form them in fp32"""
    thr = f32(f32(intensity_threshold) / f32(S))
    e = f32(edge_threshold)
    with np.errstate(divide="ignore"):
        lim = f32(f32(f32(e + f32(1)) * f32(e + f32(1))) / e)
    return thr, lim


def candidates(D, S, thr, strict=True):
    """(s, y, x) of the texels that pass the 26 comparisons and |c| > thr * 0.8f, in raster order"""
    D = np.asarray(D, f32)
    _, h, w = D.shape
    if h < 3 or w < 3:
        return np.zeros((0, 3), np.int64)
    pre = f32(f32(thr) * f32(0.8))
    c = D[1:S + 1, 1:h - 1, 1:w - 1]
    is_max = np.ones(c.shape, bool)
    is_min = np.ones(c.shape, bool)
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if ds == 0 and dy == 0 and dx == 0:
                    continue
                v = D[1 + ds:S + 1 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                is_max &= (c > v) if strict else (c >= v)
                is_min &= (c < v) if strict else (c <= v)
    out = np.argwhere((is_max | is_min) & (np.abs(c) > pre))
    return out + 1


def refine_trace(D, S, x, y, s, thr, edge_limit):
    """ExtractKeypoints.comp:121-206 for one candidate in fp32 scalars: dict(ok, rx, ry, rs, sx, sy, ss, nv, moved_x, moved_y, moved_s, clamps)
    where clamps is the set of limits a wanted step ran into ('x1', 'xw', 'y1', 'yh', 's1', 'sS')"""
    D = np.asarray(D, f32)
    n, H, W = D.shape
    z = f32(0)

    def ld(ls, lx, ly):
        return D[ls, ly, lx] if 0 <= ls < n else z

    rx, ry, rs = x, y, s
    clamps = set()
    h, q, two = f32(0.5), f32(0.25), f32(2)
    oX = oY = oS = gX = gY = gS = z
    with np.errstate(all="ignore"):
        for step in range(5):
            vc = ld(rs, rx, ry)
            sp, sm = ld(rs + 1, rx, ry), ld(rs - 1, rx, ry)
            xp, xm = ld(rs, rx + 1, ry), ld(rs, rx - 1, ry)
            yp, ym = ld(rs, rx, ry + 1), ld(rs, rx, ry - 1)
            gS, gX, gY = h * (sp - sm), h * (xp - xm), h * (yp - ym)
            h11, h22, h33 = sp + sm - two * vc, xp + xm - two * vc, yp + ym - two * vc
            h12 = q * (ld(rs + 1, rx + 1, ry) - ld(rs + 1, rx - 1, ry) - ld(rs - 1, rx + 1, ry) + ld(rs - 1, rx - 1, ry))
            h13 = q * (ld(rs + 1, rx, ry + 1) - ld(rs + 1, rx, ry - 1) - ld(rs - 1, rx, ry + 1) + ld(rs - 1, rx, ry - 1))
            h23 = q * (ld(rs, rx + 1, ry + 1) - ld(rs, rx + 1, ry - 1) - ld(rs, rx - 1, ry + 1) + ld(rs, rx - 1, ry - 1))
            det = h11 * ((h22 * h33) - (h23 * h23)) - h12 * ((h12 * h33) - (h13 * h23)) + h13 * ((h12 * h23) - (h13 * h22))
            if det == 0:
                return dict(ok=False, rx=rx, ry=ry, rs=rs, clamps=clamps, moved_x=rx != x, moved_y=ry != y, moved_s=rs != s)
            i11 = ((h22 * h33) - (h23 * h23)) / det
            i12 = f32(-1) * ((h12 * h33) - (h13 * h23)) / det
            i13 = ((h12 * h23) - (h13 * h22)) / det
            i22 = ((h11 * h33) - (h13 * h13)) / det
            i23 = f32(-1) * ((h11 * h23) - (h13 * h12)) / det
            i33 = ((h11 * h22) - (h12 * h12)) / det
            oS = -i11 * gS - i12 * gX - i13 * gY
            oX = -i12 * gS - i22 * gX - i23 * gY
            oY = -i13 * gS - i23 * gX - i33 * gY
            lim = f32(0.6)
            if abs(oX) < lim and abs(oY) < lim and abs(oS) < lim:
                break
            if step < 4:
                for o, pos, hi, lo_name, hi_name in ((oX, rx, W - 2, "x1", "xw"), (oY, ry, H - 2, "y1", "yh"), (oS, rs, S + 1, "s1", "sS")):
                    if o >= lim and not pos < hi:
                        clamps.add(hi_name)
                    if o <= -lim and not pos > 1:
                        clamps.add(lo_name)
                rx += (1 if (oX >= lim and rx < W - 2) else 0) - (1 if (oX <= -lim and rx > 1) else 0)
                ry += (1 if (oY >= lim and ry < H - 2) else 0) - (1 if (oY <= -lim and ry > 1) else 0)
                rs += (1 if (oS >= lim and rs < S + 1) else 0) - (1 if (oS <= -lim and rs > 1) else 0)
        sx, sy, ss = f32(rx) + oX, f32(ry) + oY, f32(rs) + oS
        vc = ld(rs, rx, ry)
        nv = vc + h * (gX * oX + gY * oY + gS * oS)
        out = dict(ok=False, rx=rx, ry=ry, rs=rs, sx=sx, sy=sy, ss=ss, nv=nv, clamps=clamps, moved_x=rx != x, moved_y=ry != y, moved_s=rs != s)
        big = f32(1.5)
        if not (abs(nv) > f32(thr) and abs(oX) < big and abs(oY) < big and abs(oS) < big and sx >= 0 and sx < f32(W) and sy >= 0 and sy < f32(H)
                and ss >= 0 and ss <= f32(S + 1)):
            return out
        e11 = ld(rs, rx + 1, ry) + ld(rs, rx - 1, ry) - two * vc
        e22 = ld(rs, rx, ry + 1) + ld(rs, rx, ry - 1) - two * vc
        e12 = q * (ld(rs, rx + 1, ry + 1) - ld(rs, rx + 1, ry - 1) - ld(rs, rx - 1, ry + 1) + ld(rs, rx - 1, ry - 1))
        edgeness = ((e11 + e22) * (e11 + e22)) / ((e11 * e22) - (e12 * e12))
        out["ok"] = bool(edgeness < f32(edge_limit) and edgeness >= 0)
    return out


def traces(D, S, thr, edge_limit, strict=True):
    """[(s, y, x, trace)] of every candidate, in raster order"""
    return [(int(s), int(y), int(x), refine_trace(D, S, int(x), int(y), int(s), thr, edge_limit)) for s, y, x in candidates(D, S, thr, strict)]


# ---------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """One launch: per image a DoG stack, the texel type, the thresholds. planes: (batch, S + 3, h, w)."""

    def __init__(self, name, dogs, *, fp16=False, anchor=0, zero_base=False, intensity_threshold=0.04, edge_threshold=10.0, seed_sigma=1.6, **marks):
        self.name, self.dogs, self.fp16 = name, [np.asarray(d, f32) for d in dogs], bool(fp16)
        self.S = self.dogs[0].shape[0] - 2
        self.h, self.w = self.dogs[0].shape[1:]
        self.batch = len(self.dogs)
        self.it, self.et, self.seed_sigma = intensity_threshold, edge_threshold, seed_sigma
        self.thr, self.edge_limit = thresholds(self.S, intensity_threshold, edge_threshold)
        base = np.zeros((self.h, self.w), f32) if zero_base else None
        self.planes = np.stack([gauss_from_dog(d, fp16=fp16, anchor=anchor, base=base) for d in self.dogs])
        self.marks = marks  # what the case is built to reach: test_extract_reference.py asserts every entry

    def cfg(self, oracle, **over):
        kw = dict(math_mode=1, nb_scales_per_octave=self.S, pyramid_fp16=1 if self.fp16 else 0, intensity_threshold=self.it, edge_threshold=self.et,
                  seed_scale_sigma=self.seed_sigma, use_input_upsampling=0)
        kw.update(over)
        return oracle.default_config(**kw)

    def pyramids(self, oracle, **over):
        cfg = self.cfg(oracle, **over)
        return [oracle.Pyramid.from_planes(cfg, p) for p in self.planes]

    def job_kw(self):
        return dict(seed_sigma=float(self.seed_sigma), dog_threshold=float(self.thr), edge_limit=float(self.edge_limit))

    def oracle_records(self, oracle, b=0):
        p = self.pyramids(oracle)[b]
        return p.extract_keypoints(0, cap=1 << 20)

    def traces(self, b=0, strict=True):
        return traces(self.dogs[b], self.S, self.thr, self.edge_limit, strict)

    def accepted(self, b=0):
        """(s, y, x) of the candidates the restated refinement accepts"""
        return [(s, y, x) for s, y, x, t in self.traces(b) if t["ok"]]


def _place(cols, bands, gap=5):
    """column -> row band: the first band that holds no peak within `gap` columns"""
    used = [[] for _ in bands]
    out = []
    for c in cols:
        for i, u in enumerate(used):
            if all(abs(c - o) >= gap for o in u):
                u.append(c)
                out.append((c, bands[i]))
                break
        else:
            raise AssertionError(("no room for column", c))
    return out


COLS = [1, 2, 62, 63, 64, 65, 126, 127, 128, 129]
WIDTHS = [3, 4, 64, 65, 66, 127, 128, 129, 130, 193, 258]
X_PLATEAUS = [(10, "one lane's pair"), (21, "two lanes"), (63, "segments 0 / 1"), (127, "lane 63's halo / lane 0's halo")]


@functools.lru_cache(maxsize=None)
def columns_case(w, fp16, plateaus=True):
    """S = 1, h = 44: accepted keypoints of alternating sign on every column of COLS that is interior, on w - 3 and w - 2, and in the lower half
    plateaus of two along x at the positions of X_PLATEAUS, one of each sign"""
    S, h = 1, 44 if plateaus else 22
    D = np.zeros((S + 2, h, w), f32)
    cols = sorted({c for c in COLS + [w - 3, w - 2] if 1 <= c <= w - 2})
    want = _place(cols, [3, 8, 13, 18])
    for i, (c, r) in enumerate(want):
        bump(D, c, r, 1, 1 if i % 2 == 0 else -1)
    plats = []
    if plateaus and w > 4 and h == 44:
        for i, (c, what) in enumerate(X_PLATEAUS):
            if c + 1 <= w - 2:
                for sign, r in ((1, 26), (-1, 32)):
                    if not any(abs(c - o) < 7 for o, rr in plats if rr == r):
                        bump(D, c, r, 1, sign, plateau=(1, 0, 0))
                        plats.append((c, r))
    return Case(f"columns w={w}", [D], fp16=fp16, want=[(1, r, c) for c, r in want], plateaus=plats)


ROWS = [1, 15, 16, 17, 31, 32, 47, 48, 49]


@functools.lru_cache(maxsize=None)
def rows_case(h, fp16=False, S=1):
    """w = 100: accepted keypoints on every row of ROWS that is interior and on h - 2, one column block each; vertical plateaus across the
    16-, 32- and 48-row band edges (rows 15/16, 31/32, 47/48) where they fit"""
    w = 100
    D = np.zeros((S + 2, h, w), f32)
    rows = sorted({r for r in ROWS + [h - 2] if 1 <= r <= h - 2})
    want = []
    for i, r in enumerate(rows):
        bump(D, 3 + 6 * i, r, 1 + i % S, 1 if i % 2 == 0 else -1)
        want.append((1 + i % S, r, 3 + 6 * i))
    plats = []
    for i, r in enumerate((15, 31, 47)):
        if r + 1 <= h - 2:
            bump(D, 70 + 8 * i, r, 1, 1 if i % 2 else -1, plateau=(0, 1, 0))
            plats.append((70 + 8 * i, r))
    return Case(f"rows h={h}", [D], fp16=fp16, want=want, plateaus=plats)


@functools.lru_cache(maxsize=None)
def find_noise(S, h, w, fp16, need, first_seed=0):
    """the first seed whose noise stack holds what `need` names: 'q1' an accepted record that walked to rs = S + 1, 'moves' candidates that move
    in x, in y and in s and one that meets a clamp"""
    thr, lim = thresholds(S)
    for seed in range(first_seed, first_seed + 60):
        D = noise(S, h, w, seed)
        tr = traces(D, S, thr, lim)
        ok = True
        if "q1" in need:
            ok &= any(t["ok"] and t["rs"] == S + 1 and t["ss"] > S + 0.6 for _, _, _, t in tr)
        if "moves" in need:
            ok &= any(t["moved_x"] for *_, t in tr) and any(t["moved_y"] for *_, t in tr) and any(t["moved_s"] for *_, t in tr)
            ok &= any(t["clamps"] for *_, t in tr)
        if ok:
            return seed
    raise AssertionError(("no seed", S, h, w, need))


@functools.lru_cache(maxsize=None)
def scales_case(S, fp16):
    """112 x 20: an accepted keypoint on every scale 1 .. S (columns 3, 8, ..), a plateau across layers S - 1 / S (S = 1: 1 / 2) of either sign,
    and a 40-column noise strip whose seed is chosen so that an accepted record walks to rs = S + 1 (quirk Q1); seed_sigma 1.25, 1.6 or 2"""
    h, w = 20, 112
    D = np.zeros((S + 2, h, w), f32)
    want = []
    for s in range(1, S + 1):
        bump(D, 3 + 5 * (s - 1), 4, s, 1 if s % 2 else -1)
        want.append((s, 4, 3 + 5 * (s - 1)))
    s0 = max(S - 1, 1)
    bump(D, 4, 12, s0, 1, plateau=(0, 0, 1))
    bump(D, 12, 12, s0, -1, plateau=(0, 0, 1))
    thr, lim = thresholds(S)
    for seed in range(60):   # the first seed with which an accepted record of the strip walks to rs = S + 1
        D[:, :, 72:] = noise(S, h, 40, seed)
        if any(t["ok"] and t["rs"] == S + 1 and t["ss"] > S + 0.6 for s, y, x, t in traces(D, S, thr, lim) if s == S and x >= 72):
            break
    else:
        raise AssertionError(("no seed", S))
    return Case(f"scales S={S}", [D], fp16=fp16, seed_sigma=(1.6, 1.25, 2.0)[S % 3], want=want, plateaus=[(4, 12), (12, 12)], q1=True)


def pre_for(thr):
    return f32(f32(thr) * f32(0.8))


@functools.lru_cache(maxsize=None)
def threshold_case():
    """S = 1, fp32: skewed peaks of both signs whose centre is exactly 0.8f * dog_threshold, one ulp above and one ulp below it; only the
    middle one is a candidate, and its refined value 1.2 * dog_threshold is accepted"""
    c = f32(40 * Q)
    thr = f32(c / f32(0.8))
    for _ in range(64):   # the fp32 threshold whose product with 0.8f is c itself
        if pre_for(thr) == c:
            break
        thr = np.nextafter(thr, f32(1) if pre_for(thr) < c else f32(0))
    assert pre_for(thr) == c
    D = np.zeros((3, 12, 40), f32)
    vals = [c, np.nextafter(c, f32(1)), np.nextafter(c, f32(0))]
    for i, v in enumerate(vals):
        skew(D, 4 + 6 * i, 3, 1, v, 1)
        skew(D, 4 + 6 * i, 8, 1, v, -1)
    return Case("threshold", [D], anchor=1, zero_base=True, intensity_threshold=float(thr), at=[(4, 3), (4, 8)], above=[(10, 3), (10, 8)],
                below=[(16, 3), (16, 8)])


@functools.lru_cache(maxsize=None)
def tiny_case(fp16):
    """dog_threshold = 0: maxima whose value is an fp32 denormal (binary16: a binary16 subnormal difference of two layers) above a pit of
    ordinary depth; a scan that flushes them to zero loses the keypoint"""
    tiny = [2.0 ** -24, 3 * 2.0 ** -24] if fp16 else [2.0 ** -149, 5 * 2.0 ** -140]
    D = np.zeros((3, 12, 40), f32)
    for i, v in enumerate(tiny):
        inverted(D, 5 + 8 * i, 5, 1, v)
    bump(D, 30, 5, 1, -1)
    return Case("tiny values", [D], fp16=fp16, anchor=1, zero_base=True, intensity_threshold=0.0, tiny=[(5, 5), (13, 5)])


@functools.lru_cache(maxsize=None)
def edge_case(infinite):
    D = np.zeros((3, 12, 40), f32)
    ridge(D, 10, 3, 1, 1)
    ridge(D, 10, 8, 1, -1)
    bump(D, 30, 5, 1, 1)
    return Case("edge", [D], edge_threshold=0.0 if infinite else 10.0, ridges=[(10, 3), (10, 8)])


@functools.lru_cache(maxsize=None)
def constant_case(batch, fp16=False):
    """every image but the first and the last is constant (batch 1: the only one): no candidate, found = 0 over the poison"""
    dogs = []
    for b in range(batch):
        D = np.zeros((3, 20, 70), f32)
        if batch > 1 and b in (0, batch - 1):
            bump(D, 9 + b, 6, 1, 1)
            bump(D, 40, 12, 1, -1)
        dogs.append(D)
    return Case(f"constant batch {batch}", dogs, fp16=fp16)


@functools.lru_cache(maxsize=None)
def noise_case(S, h, w, seed, fp16=False, batch=1):
    return Case(f"noise {w}x{h} S={S}", [noise(S, h, w, seed + 7 * b) for b in range(batch)], fp16=fp16)


@functools.lru_cache(maxsize=None)
def moves_case(fp16=False):
    """the small noise stack of the capacity and layout cases: candidates that move in x, y and s and meet a clamp"""
    S, h, w = 2, 24, 70
    return noise_case(S, h, w, find_noise(S, h, w, False, ("moves", "q1")), fp16)


@functools.lru_cache(maxsize=None)
def periodic_case(h, w, fp16=False):
    return Case(f"periodic {w}x{h}", [periodic(1, h, w)], fp16=fp16)


def refine_grid_rows(S, w, h, batch=1):
    """workgroup rows of the refinement launches per image (extract_run in extrema.hip): candidates beyond 256 * rows are reached by striding"""
    rcap = min(max(65536 // batch, 16), 512)
    return min((S * w * h // 4 + 64 + 255) // 256, rcap)


MANY = dict(S=13, w=129, h=13600)


@functools.lru_cache(maxsize=None)
def many_chunks_case():
    """S = 13, 129 x 13600, flat except for peaks: 530 400 segments = 130 scan chunks; peaks whose segments lie in chunk 0, in chunk 66 and in chunk 129
    (k_cand_list adds up the chunk totals in front of a segment 64 at a time: one, two and three rounds)"""
    S, w, h = MANY["S"], MANY["w"], MANY["h"]
    D = np.zeros((S + 2, h, w), f32)
    want = [(1, 5, 5), (1, 700, 127), (7, 9000, 64), (7, 9010, 3), (13, 13500, 100), (13, h - 2, w - 2)]
    for i, (s, y, x) in enumerate(want):
        bump(D, x, y, s, 1 if i % 2 == 0 else -1)
    return Case("many chunks", [D], want=want)


def seg_chunk(case, s, y, x):
    nseg = (case.w + 63) // 64
    return (((s - 1) * case.h + y) * nseg + x // 64) // 4096
