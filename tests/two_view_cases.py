"""The cases tests/test_gpu_two_view_launchers.py runs the two-view launchers of include/vksift_hip.h on — vksift_hip_ransac_homography,
_ransac_fundamental, _refit_homography, _refit_fundamental and _match_guided — as plain data (no GPU import), and what the numpy restatements
(np_verify, np_verify_f, np_refine, np_refine_f, np_guided) give for them, computed once per case and to be left unchanged.

  RANSAC[m]   m = "h" (four-point samples, 13-word records) or "f" (seven-point, 14 words). A case: max_n, the launch arguments, the slack of
              every stride, and per slot the raw counter n_dev and the rows the arena holds for it — min(n_dev, max_n) correspondences and,
              where the case says so, DECOYS behind them: copies of true inliers of the planted model, which a kernel that read or counted
              one row too many would count. Layout cases, hypothesis counts (ties at 65 536, a better hypothesis just outside nb_hypotheses)
              and the degenerate inputs (NaN rows, one point, collinear, duplicated, infinite, subnormal, huge).
  REFIT[m]    the layout cases again, start records and masks from the RANSAC restatement of the same slot, and slots edited AFTER that
              verification: mask bytes 2 and 0xff, a valid word of 2, NaN / inf coordinates on marked and unmarked rows, marked duplicates.
  GUIDED      layouts (shared cache entries, padded strides, clamped counters, degenerate models, NaN coordinates) crossed with
              GUIDED_MODES: model kind x cross_check x threshold.
  REFUSALS    (launch, case name, changes): every refusal the header lists; the arena must come back byte for byte.
tests/test_two_view_cases.py pins which edge each case reaches."""
import numpy as np

import np_guided as G
import np_refine as R
import np_refine_f as RF
import np_verify as V
import np_verify_f as VF
import quality as Q

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)
JUNK_COUNTER = 0x7FFFFFF1   # the counter words between the strided ones: never to be read (a count a clamp would turn into max_n)
W, H = 640, 480
SAMPLE = {"h": 4, "f": 7}
RANSAC_WORDS = {"h": 13, "f": 14}
REFIT_WORDS = 13
NP_RANSAC = {"h": V, "f": VF}
NP_REFIT = {"h": R, "f": RF}
MODEL_KEY = {"h": "H", "f": "F"}
_MEMO = {}


def planted(m, n, seed, exact=None):
    """n correspondences of a planted model of kind m in a W x H image: half outliers and 0.5 px noise, or (exact; the default for n <= 9)
    exact images without outliers, so that a model with enough inliers exists -> (rows float32 [n, 4], is_true bool [n])"""
    exact = n <= 9 if exact is None else exact
    out, noise = (0.0, 0.0) if exact else (0.5, 0.5)
    if m == "h":
        c, true = V.synthetic_case(Q.homography(W, H, **Q.WARPS[seed % 4]), W, H, n=n, outliers=out, noise=noise, seed=seed)
    else:
        c, true, _ = VF.two_view_case(n, out, noise, seed, W, H)
    return c, true


def slot(m, n_dev, n, seed, decoys=0):
    """a slot of n planted correspondences whose counter reads n_dev, `decoys` copies of true inliers behind them"""
    c, true = planted(m, n + decoys, seed)
    if decoys:
        src = np.flatnonzero(true[:n]) if true[:n].any() else np.arange(max(n, 1))[:n]
        c = np.concatenate([c[:n], c[src[np.arange(decoys) % max(len(src), 1)]]]) if len(src) else c[:n]
    return dict(n_dev=int(n_dev), rows=np.ascontiguousarray(c, f32))


def ransac_case(name, m, slots, max_n, *, corr_extra=0, mask_extra=0, n_stride=1, nb_hyp=256, thr=2.5, seed=9, strides=None):
    """corr_extra: rows, mask_extra: bytes a slot's stride lies above max_n; strides: (corr_slot_stride, mask_slot_stride) to pass instead
    of those (the single-slot case)"""
    assert all(len(s["rows"]) <= max_n + corr_extra and len(s["rows"]) >= min(s["n_dev"], max_n) for s in slots)
    return dict(name=name, model=m, slots=slots, max_n=max_n, corr_extra=corr_extra, mask_extra=mask_extra, n_stride=n_stride, nb_hyp=nb_hyp, thr=thr, seed=seed,
                strides=strides)


def slot_n(case, s):
    return min(s["n_dev"], case["max_n"])


# ---- the hypothesis-count cases: slot 1 of two holds 40 correspondences (slot 0 none: the keys of slot 1 lie one slot's workgroups into the
# scratch). Seeds found by search on the CPU (tests/test_two_view_cases.py asserts what they were chosen for).
HYP_N = 40
HYP_DATA_SEED = {"h": 23, "f": 24}
HYP_SEED = {"h": 4, "f": 2}         # the sampler seed of the hypothesis-count cases
J_STAR = {"h": 52, "f": 94}         # the first hypothesis in [1, 1024), not a multiple of 256, that beats every earlier one at threshold 2.5
HYP_COUNTS = [1, 255, 256, 257, 65536]


def hypothesis_counts(m, nb, thr=2.5):
    """inlier counts of hypotheses 0 .. nb-1 of the hypothesis-count slot (for "f": the best of a hypothesis's roots) and per model id"""
    key = ("hyp counts", m, nb, thr)
    if key not in _MEMO:
        c, mod = planted(m, HYP_N, HYP_DATA_SEED[m])[0], NP_RANSAC[m]
        hyps = mod.hypotheses(c, nb, HYP_SEED[m], 1)
        ids = mod.inliers(hyps[1], c, V.threshold2(thr)).sum(axis=1)
        _MEMO[key] = (ids if m == "h" else ids.reshape(nb, 4).max(axis=1)), ids
    return _MEMO[key]


def j_star(m):
    c = hypothesis_counts(m, 1024)[0]
    for j in range(1, 1024):
        if j % 256 and c[j] > c[:j].max():
            return j
    return None


# ---- the degenerate inputs ------------------------------------------------------------------------------------------------------------------
DEGENERATE = ["every third row NaN", "all rows NaN", "all rows one point", "all zeros", "both sides collinear", "side A on a horizontal line, integer x",
              "second half duplicates the first", "+inf and -inf", "side B equals side A", "scaled by 1e-41 (subnormal)", "scaled by 1e30"]
DEGENERATE_N = 300


def degenerate_rows(m):
    base = planted(m, DEGENERATE_N, 41)[0]
    t = np.arange(DEGENERATE_N, dtype=f32)
    out = []
    for name in DEGENERATE:
        c = base.copy()
        if name == "every third row NaN":
            c[::3] = NAN
        elif name == "all rows NaN":
            c[:] = NAN
        elif name == "all rows one point":
            c[:] = base[7]
        elif name == "all zeros":
            c[:] = 0
        elif name == "both sides collinear":
            c = np.stack([10 + 2 * t, 20 + 1.5 * t, 30 + t, 400 - t], axis=1).astype(f32)
        elif name.startswith("side A on a horizontal line"):
            c[:, 0], c[:, 1] = t, 100
        elif name.startswith("second half"):
            c[DEGENERATE_N // 2:] = c[:DEGENERATE_N // 2]
        elif name == "+inf and -inf":
            c[5, 0], c[77, 3] = INF, -INF
        elif name == "side B equals side A":
            c[:, 2:] = c[:, :2]
        elif name.startswith("scaled by 1e-41"):
            c = c * f32(1e-41)
        else:
            assert name == "scaled by 1e30"
            c = c * f32(1e30)
        out.append(np.ascontiguousarray(c, f32))
    return out


def _ransac_cases(m):
    K = SAMPLE[m]
    cases = [
        ransac_case("padded strides", m, [slot(m, n, n, 100 + i) for i, n in enumerate((300, 65, K))], 300, corr_extra=5, mask_extra=13, n_stride=3),
        ransac_case("decoys beyond n", m, [slot(m, n, n, 110 + i, decoys=305 - n) for i, n in enumerate((200, 65, 20))], 300, corr_extra=5, mask_extra=13,
                    n_stride=2),
        ransac_case("clamp", m, [slot(m, nd, 257, 120 + i, decoys=3) for i, nd in enumerate((258, 0xFFFFFFFF, 257))], 257, corr_extra=3, mask_extra=3),
        # nslots == 1: the strides address nothing and are not held to max_n (the header says so); both are passed as 0
        ransac_case("one slot, strides 0", m, [slot(m, 100, 100, 130, decoys=4)], 100, corr_extra=4, mask_extra=4, strides=(0, 0)),
        ransac_case("many slots", m, [slot(m, n, n, 200 + i) for i, n in enumerate([(0, K - 1, K, K + 1, 63, 64)[i % 6] for i in range(70)])], 64, nb_hyp=300),
    ]
    for nb in HYP_COUNTS + [J_STAR[m]]:
        hyp_slot = dict(n_dev=HYP_N, rows=planted(m, HYP_N, HYP_DATA_SEED[m])[0])
        cases.append(ransac_case(f"{nb} hypotheses" + (" (j*)" if nb == J_STAR[m] else ""), m, [slot(m, 0, 0, 140), hyp_slot], HYP_N, nb_hyp=nb, seed=HYP_SEED[m]))
    for thr in (2.5, 0.5):
        cases.append(ransac_case(f"degenerate data, threshold {thr}", m, [dict(n_dev=DEGENERATE_N, rows=c) for c in degenerate_rows(m)], DEGENERATE_N, thr=thr))
    return cases


RANSAC = {m: _ransac_cases(m) for m in "hf"}


def ransac_expected(case):
    """the restatement's result of every slot, on rows [0, min(n_dev, max_n))"""
    key = ("ransac", case["model"], case["name"])
    if key not in _MEMO:
        mod = NP_RANSAC[case["model"]]
        _MEMO[key] = [mod.ransac(s["rows"][:slot_n(case, s)], case["nb_hyp"], case["thr"], case["seed"], slot=i) for i, s in enumerate(case["slots"])]
    return _MEMO[key]


# ---- refits ---------------------------------------------------------------------------------------------------------------------------------
REFIT_SPECIAL = ["plain", "mask bytes 2 and 0xff on true inliers", "start valid word 2", "NaN on a marked row", "inf on a marked row", "NaN on an unmarked row",
                 "inf on an unmarked row", "marked duplicates"]
REFIT_SPECIAL_N = 300
REFIT_START_HYP = {"h": 64, "f": 256}


def case_named(cases, name):
    (c,) = [c for c in cases if c["name"] == name]
    return c


def _special_base(m):
    return ransac_case("refit special slots", m, [slot(m, REFIT_SPECIAL_N, REFIT_SPECIAL_N, 300 + i, decoys=2) for i in range(len(REFIT_SPECIAL))],
                       REFIT_SPECIAL_N, corr_extra=2, mask_extra=7, n_stride=2, nb_hyp=REFIT_START_HYP[m])


def refit_case(name, m, base, nb_rounds, *, special=False, start_slack=5, out_slack=29):
    """base: the RANSAC case whose layout, slots and results the refit starts from; start_slack / out_slack: bytes behind the last slot's stride
    of start_masks / masks_out (the two have one stride and different room)"""
    return dict(name=name, model=m, base=base, nb_rounds=nb_rounds, special=special, thr=base["thr"], start_slack=start_slack, out_slack=out_slack)


def _refit_cases(m):
    layout = lambda name: case_named(RANSAC[m], name)
    special = _special_base(m)
    return [refit_case("padded strides", m, layout("padded strides"), 3), refit_case("clamp", m, layout("clamp"), 3),
            refit_case("many slots", m, layout("many slots"), 3), refit_case("special slots, 1 round", m, special, 1, special=True),
            refit_case("special slots, 8 rounds", m, special, 8, special=True)]


REFIT = {m: _refit_cases(m) for m in "hf"}


def refit_slots(case):
    """per slot dict(n_dev, rows, start: the RANSAC record as a dict, start_mask: uint8 [n]) — the RANSAC restatement of the base case's slot, then
    (special) the edit the slot is named for"""
    key = ("refit slots", case["model"], case["base"]["name"], case["special"])
    if key in _MEMO:
        return _MEMO[key]
    base, out = case["base"], []
    for i, (s, r) in enumerate(zip(base["slots"], ransac_expected(base))):
        n = slot_n(base, s)
        rows, start, mask = s["rows"].copy(), dict(r), r["mask"].astype(np.uint8)
        if case["special"]:
            assert start["valid"] == 1 and n == REFIT_SPECIAL_N
            on, off = np.flatnonzero(mask == 1), np.flatnonzero(mask == 0)
            what = REFIT_SPECIAL[i]
            if what.startswith("mask bytes"):
                mask[on[0]], mask[on[1]] = 2, 0xFF
            elif what == "start valid word 2":
                start["valid"] = 2
            elif what == "NaN on a marked row":
                rows[on[3], 0] = NAN
            elif what == "inf on a marked row":
                rows[on[3], 3] = INF
            elif what == "NaN on an unmarked row":
                rows[off[3], 2] = NAN
            elif what == "inf on an unmarked row":
                rows[off[3], 1] = -INF
            elif what == "marked duplicates":
                rows[on[1::2][:len(on[0::2])]] = rows[on[0::2][:len(on[1::2])]]
            else:
                assert what == "plain"
        out.append(dict(n_dev=s["n_dev"], rows=rows, start=start, start_mask=mask))
    _MEMO[key] = out
    return out


def refit_expected(case):
    key = ("refit", case["model"], case["name"])
    if key not in _MEMO:
        mod, mx = NP_REFIT[case["model"]], case["base"]["max_n"]
        _MEMO[key] = [mod.refit(s["rows"][:min(s["n_dev"], mx)], s["start"], s["start_mask"], case["nb_rounds"], case["thr"]) for s in refit_slots(case)]
    return _MEMO[key]


# ---- guided matching ------------------------------------------------------------------------------------------------------------------------
KIND = {"h": G.HOMOGRAPHY, "f": G.FUNDAMENTAL}
# the wide threshold admits every pair (it fills the wave queues); it runs without a ratio test or a distance limit, which would leave nothing of a
# plain 2-NN matching over repeated structure
GUIDED_MODES = [dict(kind=k, cross_check=x, thr=t, ratio=r, max_distance=d) for k in "hf" for x in (0, 1) for t, r, d in ((2.5, 0.8, 200.0), (1e6, 1.01, float("inf")))]
GUIDED_SIZES = [(0, 5), (1, 63), (64, 65), (257, 300)]
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], f32)


def mode_name(mode):
    return f"{mode['kind']}, cross_check {mode['cross_check']}, threshold {mode['thr']:g}"


def pair(size, seed):
    """np_guided.slot_case of one of GUIDED_SIZES; odd seeds two views of a scene (F fits), even seeds a plane (H fits)"""
    assert size in GUIDED_SIZES
    key = ("pair", size, seed)
    if key not in _MEMO:
        _MEMO[key] = G.slot_case(size[0], size[1], seed, planar=seed % 2 == 0)
    return _MEMO[key]


def xy_of(p, side):
    return np.stack([p["x" + side], p["y" + side]], axis=1).astype(f32)


def gslot(tab, n_dev, xy_a, xy_b, models, valid=1):
    """tab: the cache entries of A and B; models: {"h": float32 [9], "f": float32 [9]}"""
    return dict(tab=tuple(tab), n_dev=tuple(int(v) for v in n_dev), xy=(np.ascontiguousarray(xy_a, f32), np.ascontiguousarray(xy_b, f32)),
                models={k: np.ascontiguousarray(v, f32).reshape(9) for k, v in models.items()}, valid=int(valid))


def own_slot(p, ea, eb, **kw):
    return gslot((ea, eb), (len(p["xa"]), len(p["xb"])), xy_of(p, "a"), xy_of(p, "b"), dict(h=p["H"], f=p["F"]), **kw)


def guided_layout(name, entries, slots, max_n, *, desc_extra=0, norm_extra=0, xy_extra=0, out_extra=0, tab_stride=2, n_stride=2, model_stride=9, valid_stride=1):
    """entries: the cache entries, uint8 [rows, 128] (None: an entry no slot names, all poison); desc_extra: rows, norm_extra: words, xy_extra:
    rows, out_extra: 4-byte words above the minimal strides"""
    for s in slots:
        for t in (0, 1):
            n = min(s["n_dev"][t], max_n)
            assert len(entries[s["tab"][t]]) >= n and len(s["xy"][t]) >= n
            assert len(entries[s["tab"][t]]) <= max_n + desc_extra and len(s["xy"][t]) <= max_n + xy_extra
    return dict(name=name, entries=entries, slots=slots, max_n=max_n, desc_extra=desc_extra, norm_extra=norm_extra, xy_extra=xy_extra, out_extra=out_extra,
                tab_stride=tab_stride, n_stride=n_stride, model_stride=model_stride, valid_stride=valid_stride)


def _guided_layouts():
    p0, p1, p2, p3 = pair((64, 65), 500), pair((257, 300), 501), pair((1, 63), 502), pair((0, 5), 503)
    out = []
    # several slots name entry 3 (A of pair 0), one names the pair swapped, one entry 3 twice; entry 1 belongs to nobody
    entries = [p0["desc_b"], None, p1["desc_a"], p0["desc_a"], p1["desc_b"], p2["desc_b"], p2["desc_a"]]
    slots = [own_slot(p0, 3, 0), gslot((0, 3), (65, 64), xy_of(p0, "b"), xy_of(p0, "a"), dict(h=p0["H"], f=p0["F"])),
             gslot((3, 3), (64, 64), xy_of(p0, "a"), xy_of(p0, "a"), dict(h=IDENTITY, f=p0["F"])),
             gslot((3, 4), (64, 300), xy_of(p0, "a"), xy_of(p1, "b"), dict(h=p0["H"], f=p0["F"])), own_slot(p1, 2, 4), own_slot(p2, 6, 5),
             gslot((3, 0), (0, 5), xy_of(p0, "a"), xy_of(p0, "b"), dict(h=p0["H"], f=p0["F"]))]
    out.append(guided_layout("shared entries", entries, slots, 300))
    out.append(guided_layout("padded strides", [p0["desc_a"], p0["desc_b"], p2["desc_a"], p2["desc_b"], p3["desc_a"], p3["desc_b"], p1["desc_a"], p1["desc_b"]],
                             [own_slot(p0, 0, 1), own_slot(p2, 2, 3), own_slot(p3, 4, 5), own_slot(p1, 6, 7)], 300, desc_extra=1, norm_extra=3, xy_extra=2, out_extra=3,
                             tab_stride=3, n_stride=3, model_stride=12, valid_stride=2))
    # counters above max_n = 60 on either side; rows 60 .. 119 of B are exact copies (descriptor and coordinates) of rows 0 .. 59 of B: every
    # candidate has an admissible look-alike there that would tie with it
    db, xb = np.concatenate([p0["desc_b"][:60], p0["desc_b"][:60]]), np.concatenate([xy_of(p0, "b")[:60], xy_of(p0, "b")[:60]])
    mods = dict(h=p0["H"], f=p0["F"])
    out.append(guided_layout("clamp", [p0["desc_a"], db], [gslot((0, 1), (64, 65), xy_of(p0, "a"), xb, mods), gslot((0, 1), (0xFFFFFFFF, 61), xy_of(p0, "a"), xb, mods),
                                                            gslot((0, 1), (60, 0xFFFFFFFF), xy_of(p0, "a"), xb, mods)], 60, desc_extra=60, norm_extra=5, xy_extra=60))
    models = [("all NaN", np.full(9, NAN, f32)), ("all zero", np.zeros(9, f32)), ("an inf entry", None), ("negated", None)]
    slots = []
    for what, M in models:
        mh, mf = (p0["H"].copy(), p0["F"].copy()) if M is None else (M, M)
        if what == "an inf entry":
            mh[4], mf[4] = INF, INF
        elif what == "negated":
            mh, mf = -mh, -mf
        slots.append(gslot((0, 1), (64, 65), xy_of(p0, "a"), xy_of(p0, "b"), dict(h=mh, f=mf)))
    slots.append(own_slot(p0, 0, 1, valid=2))
    slots.append(own_slot(p0, 0, 1, valid=0))
    slots.append(own_slot(p0, 0, 1))
    out.append(guided_layout("degenerate models", [p0["desc_a"], p0["desc_b"]], slots, 65))
    xa0, xb0, xa1, xb1 = xy_of(p0, "a"), xy_of(p0, "b"), xy_of(p1, "a"), xy_of(p1, "b")
    xa0[3, 0], xa0[40, 1], xb0[0, 1], xb0[64, 0], xa1[::5, 0], xb1[256:, 1] = NAN, NAN, NAN, NAN, NAN, NAN
    out.append(guided_layout("NaN coordinates", [p0["desc_a"], p0["desc_b"], p1["desc_a"], p1["desc_b"]],
                             [gslot((0, 1), (64, 65), xa0, xb0, dict(h=p0["H"], f=p0["F"])), gslot((2, 3), (257, 300), xa1, xb1, dict(h=p1["H"], f=p1["F"]))], 300))
    return out


GUIDED_LAYOUTS = _guided_layouts()
DEGENERATE_MODEL_SLOTS = 4      # the first slots of "degenerate models"
GUIDED = [dict(lay, name=f"{lay['name']}: {mode_name(mode)}", layout=lay["name"], **mode) for lay in GUIDED_LAYOUTS for mode in GUIDED_MODES]


def guided_expected(case):
    """the records of every slot (np_guided.RECORD_DTYPE)"""
    key = ("guided", case["name"])
    if key not in _MEMO:
        out, mx = [], case["max_n"]
        for s in case["slots"]:
            na, nb = min(s["n_dev"][0], mx), min(s["n_dev"][1], mx)
            (xa, xb), (da, db) = s["xy"], (case["entries"][s["tab"][0]], case["entries"][s["tab"][1]])
            out.append(G.guided(KIND[case["kind"]], s["models"][case["kind"]], s["valid"], xa[:na, 0], xa[:na, 1], da[:na], xb[:nb, 0], xb[:nb, 1], db[:nb], case["thr"],
                                case["ratio"], case["max_distance"], case["cross_check"]))
        _MEMO[key] = out
    return _MEMO[key]


# ---- refusals: hipErrorInvalidValue and not a byte of the arena changed -----------------------------------------------------------------------
BIG = 1 << 40
_RANSAC_REFUSALS = [{"nslots": 0}, {"nb_hypotheses": 0}, {"nb_hypotheses": 65537}, {"threshold_px": 0.0}, {"threshold_px": -1.0}, {"threshold_px": float("inf")},
                    {"threshold_px": float("nan")}, {"+scratch_u32": -1}, {"+corr": 8}, {"+corr_slot_stride": 8}, {"+results": 2}, {"corr_slot_stride": 16 * 299},
                    {"mask_slot_stride": 299},
                    # nslots * ceil(nb_hypotheses / 256) = 2^31 workgroups: refused before anything is touched, whatever the scratch claims to hold
                    {"nslots": 1 << 23, "nb_hypotheses": 65536, "scratch_u32": BIG}]
_REFIT_REFUSALS = [{"nslots": 0}, {"nb_rounds": 0}, {"nb_rounds": 9}, {"threshold_px": 0.0}, {"threshold_px": -1.0}, {"threshold_px": float("inf")},
                   {"threshold_px": float("nan")}, {"threshold_px": 1e-30}, {"threshold_px": 1e20},   # t2 zero, t2 infinite
                   {"+corr": 8}, {"+corr_slot_stride": 8}, {"+results": 2}, {"+start_results": 2}, {"corr_slot_stride": 16 * 299}, {"mask_slot_stride": 299},
                   {"masks_out": "start_masks"}, {"masks_out": "start_masks+1"}, {"masks_out": "start_masks-1"}]
_M24 = (1 << 24) + 1
_GUIDED_REFUSALS = [{"model_kind": 2}, {"t2": 0.0}, {"t2": -1.0}, {"t2": float("inf")}, {"t2": float("nan")}, {"ratio": 0.0}, {"ratio": float("nan")}, {"max_distance": 0.0},
                    {"+scratch_u32": -1}, {"+cache_desc_stride": -16}, {"+cache_norm_stride": -1}, {"+xy_side_stride": -1}, {"+out_slot_stride": -4},
                    {"max_n": _M24, "cache_desc_stride": 128 * _M24, "cache_norm_stride": _M24, "xy_side_stride": _M24, "out_slot_stride": 16 * _M24, "scratch_u32": BIG},
                    {"nslots": 0}, {"nslots": 65536, "scratch_u32": BIG}, {"slot_tab_stride": 1}, {"n_stride": 1}, {"model_stride": 8}, {"valid_stride": 0},
                    {"+scratch": 4}, {"+cache_desc": 8}, {"+cache_desc_stride": 8}, {"+xy": 4}, {"+out": 2}, {"+out_slot_stride": 2}]
REFUSALS = ([("ransac_" + full, "padded strides", ch) for full in ("homography", "fundamental") for ch in _RANSAC_REFUSALS] +
            [("refit_" + full, "padded strides", ch) for full in ("homography", "fundamental") for ch in _REFIT_REFUSALS] +
            [("match_guided", "shared entries: h, cross_check 1, threshold 2.5", ch) for ch in _GUIDED_REFUSALS])
CASES = {"ransac_homography": RANSAC["h"], "ransac_fundamental": RANSAC["f"], "refit_homography": REFIT["h"], "refit_fundamental": REFIT["f"], "match_guided": GUIDED}

for _launch, _cases in CASES.items():
    assert len({c["name"] for c in _cases}) == len(_cases), f"{_launch}: case names repeat"
