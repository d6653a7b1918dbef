"""The scale-space accessors (vksift_getScaleSpaceNbOctaves, vksift_getScaleSpaceOctaveResolution, vksift_downloadScaleSpaceImage,
vksift_downloadDoGImage) under every launch schedule a caller can produce.

The reference keeps ONE scale-space per instance and every detection rewrites it, so the accessors show the last image detected
(vulkansift.c:480-518). Here a run of plain vksift_detectFeatures calls may be staged and launched as one batch (deferred submission,
vksift_internal.h: defer_enabled): the accessors must still show the run's last image — with VKSIFT_DEFER=0 and =1 alike — and image 0
after a vksift_ext_detectFeaturesBatch call (include/vksift_ext.h). Each schedule is played with both settings, and what the accessors
return is compared bit for bit with the oracle's scale-space of the image the reference would show. The batches of these schedules take
every batched launch form: the forked scale-space with the LDS chain (2-4 images), the per-scale launches, the multi-octave tail (8 images
and more), binary16 planes and the ping-pong pyramid; the planes of their images 1..n-1 are read here, not only image 0's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TUNE_TAIL_MULTI = 10
W, H = 320, 240
MAX_PX = 640 * 480
SWITCHES = ("VKSIFT_DEFER_CHUNK", "VKSIFT_DEFER_MAX", "VKSIFT_PYR_PINGPONG", "VKSIFT_FORK_SCALES", "VKSIFT_LDS_CHAIN")


def _images(vk, seed, n, w=W, h=H):
    return [vk.gen_synthetic_image_family(seed + i, w, h, i % 3) for i in range(n)]


def _run(first_img, n, first_buf=0):
    """n plain detect calls of consecutive images into consecutive SIFT buffers"""
    return [("detect", first_img + i, first_buf + i) for i in range(n)]


def _oracle_kw(cfg, max_px):
    okw = {"input_image_max_size": max_px}
    for k, v in cfg.items():
        if k == "pyramid_precision_mode":
            okw["pyramid_fp16"] = v
        else:
            okw[k] = int(v) if isinstance(v, bool) else v
    return okw


def _oracle_scale_space(oracle, okw, img):
    pyr = oracle.Pyramid(oracle.default_config(math_mode=1, **okw), img)
    try:
        n = pyr.nb_octaves
        return (n, [pyr.resolution(o) for o in range(n)], [[pyr.gauss(o, s) for s in range(pyr.S + 3)] for o in range(n)],
                [[pyr.dog(o, s) for s in range(pyr.S + 2)] for o in range(n)])
    finally:
        pyr.close()


def _oracle_top(oracle, okw, img):
    """octave 0's top Gaussian plane"""
    pyr = oracle.Pyramid(oracle.default_config(math_mode=1, **okw), img)
    try:
        return pyr.gauss(0, pyr.S + 2)
    finally:
        pyr.close()


def _scale_space(inst, S):
    n = inst.getScaleSpaceNbOctaves()
    return (n, [inst.getScaleSpaceOctaveResolution(o) for o in range(n)], [[inst.downloadScaleSpaceImage(o, s) for s in range(S + 3)] for o in range(n)],
            [[inst.downloadDoGImage(o, s) for s in range(S + 2)] for o in range(n)])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _diff(got, exp):
    """None when the two scale-spaces are the same bit for bit, else where they first differ"""
    if got[0] != exp[0] or got[1] != exp[1]:
        return ("octaves", got[0], exp[0], got[1], exp[1])
    for o in range(exp[0]):
        for kind, g, e in (("gauss", got[2][o], exp[2][o]), ("dog", got[3][o], exp[3][o])):
            for s in range(len(e)):
                if not _same(g[s], e[s]):
                    return (kind, o, s)
    return None


def _model(script):
    """the image the reference would show at every ("read",) and at the end: the last valid plain detection, image 0 of an ext batch"""
    shown, reads = None, []
    for op in script:
        if op[0] == "detect":
            shown = op[1]
        elif op[0] == "batch":
            shown = op[1][0]
        elif op[0] == "read":
            reads.append(shown)
    return reads + [shown]


def _play(vk, inst, imgs, script, nbuf, max_px, S):
    snaps = []
    for op in script:
        if op[0] == "detect":
            inst.detectFeatures(imgs[op[1]], op[2])
        elif op[0] == "batch":
            inst.detectFeaturesBatch([imgs[k] for k in op[1]], op[2])
        elif op[0] == "bad_buffer":
            with pytest.raises(vk.VksiftError):
                inst.detectFeatures(imgs[0], nbuf)
        elif op[0] == "too_large":
            side = int(np.ceil(np.sqrt(max_px))) + 1
            with pytest.raises(vk.VksiftError):
                inst.detectFeatures(np.full((side, side), 77, np.uint8), 0)
        elif op[0] == "read":
            snaps.append(_scale_space(inst, S))
        else:
            raise ValueError(op)
    snaps.append(_scale_space(inst, S))
    return snaps


def _check(vk, oracle, monkeypatch, imgs, script, nbuf, cap=1, cfg=None, env=None, max_px=MAX_PX, knob=None, min_staged=1):
    """play `script` with VKSIFT_DEFER=0 and =1 on a fresh instance each; every read has to show, bit for bit, the oracle's scale-space
    of the image the model names, both times"""
    cfg, env = cfg or {}, env or {}
    okw = _oracle_kw(cfg, max_px)
    S = cfg.get("nb_scales_per_octave", 3)
    shown = _model(script)
    out = {}
    L = vk.lib()
    try:
        if knob is not None:
            L.vksift_hip_tune(TUNE_TAIL_MULTI, knob)
        for defer in (False, True):
            monkeypatch.setenv("VKSIFT_DEFER", "1" if defer else "0")
            for k in SWITCHES:
                if k in env:
                    monkeypatch.setenv(k, str(env[k]))
                else:
                    monkeypatch.delenv(k, raising=False)
            with vk.Instance(vk.default_config(input_image_max_size=max_px, sift_buffer_count=nbuf, **cfg), batch_capacity=cap) as inst:
                out[defer] = _play(vk, inst, imgs, script, nbuf, max_px, S)
                stats = inst.getDeferredStats()
            if defer:
                assert stats[1] >= min_staged, stats        # the schedule did stage images
            else:
                assert stats == (0, 0)
    finally:
        if knob is not None:
            L.vksift_hip_tune(TUNE_TAIL_MULTI, 0)
    cache = {}
    for r, k in enumerate(shown):
        if k not in cache:
            cache[k] = _oracle_scale_space(oracle, okw, imgs[k])
        exp = cache[k]
        assert exp[0] > 0
        # the case can tell the expected image from its neighbour
        nb = k - 1 if k > 0 else k + 1
        assert not _same(exp[2][0][S + 2], _oracle_top(oracle, okw, imgs[nb])), (k, nb)
        for defer in (False, True):
            d = _diff(out[defer][r], exp)
            if d is not None:
                top = out[defer][r][2][0][S + 2] if out[defer][r][0] else None
                shows = [j for j in range(len(imgs)) if top is not None and _same(top, _oracle_top(oracle, okw, imgs[j]))]
                pytest.fail(f"read {r}, VKSIFT_DEFER={int(defer)}: expected image {k}, the accessors show image(s) {shows}; first difference {d}")
    for r in range(len(shown)):
        assert _diff(out[False][r], out[True][r]) is None, r


# ---- run lengths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", ["plain", "batch"])
@pytest.mark.parametrize("n", [2, 3, 5, 8, 9, 17])
def test_run_of_plain_detections_shows_its_last_image(vk, oracle, monkeypatch, n, capacity):
    """VKSIFT_DEFER_CHUNK=0: each run is one deterministic schedule. A fresh instance launches the first call at once and stages the rest;
    a batch instance (capacity n) takes them as ONE batch of n - 1, a plain one in batches that double with its capacity"""
    imgs = _images(vk, 1000 + 50 * n, n)
    _check(vk, oracle, monkeypatch, imgs, _run(0, n), nbuf=n, cap=1 if capacity == "plain" else n, env={"VKSIFT_DEFER_CHUNK": 0})


@pytest.mark.parametrize("n", [17, 24])
def test_run_split_by_the_default_chunk_shows_its_last_image(vk, oracle, monkeypatch, n):
    """the default chunk (16) launches the first staged images while the GPU is idle: where the run splits depends on timing, what the
    accessors show does not"""
    imgs = _images(vk, 2000 + 50 * n, n)
    _check(vk, oracle, monkeypatch, imgs, _run(0, n), nbuf=n, cap=n)


@pytest.mark.parametrize("capacity", [1, 8])
def test_second_run_in_batch_mode_shows_its_last_image(vk, oracle, monkeypatch, capacity):
    """after a run of two calls or more the next run is staged from its first call on (batch_mode)"""
    imgs = _images(vk, 3000 + capacity, 6)
    script = _run(0, 3) + [("read",)] + _run(3, 3)
    _check(vk, oracle, monkeypatch, imgs, script, nbuf=8, cap=capacity)


@pytest.mark.parametrize("capacity", ["plain", "batch"])
@pytest.mark.parametrize("n", [7, 8])
def test_small_defer_max_gives_several_full_flushes(vk, oracle, monkeypatch, n, capacity):
    imgs = _images(vk, 4000 + 10 * n, n)
    _check(vk, oracle, monkeypatch, imgs, _run(0, n), nbuf=n, cap=1 if capacity == "plain" else n,
           env={"VKSIFT_DEFER_MAX": 3, "VKSIFT_DEFER_CHUNK": 0})


# ---- runs ended early (instances with room for the whole run: the staged images are still pending when the run ends) ------------
def test_run_ended_by_a_resolution_switch(vk, oracle, monkeypatch):
    imgs = _images(vk, 5000, 3) + _images(vk, 5100, 3, 257, 131)
    script = _run(0, 3) + _run(3, 3, first_buf=3)
    _check(vk, oracle, monkeypatch, imgs, script, nbuf=6, cap=6)


def test_run_ended_by_a_buffer_named_twice(vk, oracle, monkeypatch):
    imgs = _images(vk, 5200, 5)
    script = [("detect", 0, 0), ("detect", 1, 1), ("detect", 2, 2), ("detect", 3, 1), ("detect", 4, 2)]
    _check(vk, oracle, monkeypatch, imgs, script, nbuf=4, cap=4)


@pytest.mark.parametrize("bad", ["bad_buffer", "too_large"])
def test_run_ended_by_an_invalid_call_keeps_the_last_valid_image(vk, oracle, monkeypatch, bad):
    imgs = _images(vk, 5300, 3)
    script = _run(0, 3) + [(bad,)]
    _check(vk, oracle, monkeypatch, imgs, script, nbuf=4, cap=4, max_px=W * H)


# ---- ext batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after_run", [False, True])
def test_ext_batch_shows_image_0_then_a_plain_detection_its_own(vk, oracle, monkeypatch, after_run):
    imgs = _images(vk, 5400, 8)
    script = (_run(0, 3) if after_run else []) + [("batch", [3, 4, 5, 6], 4), ("read",), ("detect", 7, 0)]
    _check(vk, oracle, monkeypatch, imgs, script, nbuf=8, cap=4, min_staged=2 if after_run else 0)


# ---- configurations, shapes and switches: a deferred run of 3 (forked form) and one of 9 (tail-batch form) ----------------------------
VARIANTS = [
    # id, w, h, max_px, cfg, env, knob
    ("fp16", W, H, MAX_PX, {"pyramid_precision_mode": 1}, {}, None),
    ("no_upsampling", W, H, MAX_PX, {"use_input_upsampling": False}, {}, None),
    ("S2", W, H, MAX_PX, {"nb_scales_per_octave": 2}, {}, None),
    ("S4", W, H, MAX_PX, {"nb_scales_per_octave": 4}, {}, None),
    ("odd_width", 257, 131, MAX_PX, {}, {}, None),
    ("97x61", 97, 61, MAX_PX, {}, {}, None),
    ("min_side", 61, 17, MAX_PX, {}, {}, None),                    # one octave, the shortest side just above 16
    ("at_max_size", W, H, W * H, {}, {}, None),                     # exactly input_image_max_size
    ("pingpong2", W, H, MAX_PX, {}, {"VKSIFT_PYR_PINGPONG": 2}, None),
    ("no_fork", W, H, MAX_PX, {}, {"VKSIFT_FORK_SCALES": 0}, None),
    ("no_lds_chain", W, H, MAX_PX, {}, {"VKSIFT_LDS_CHAIN": 0}, None),
    ("tail_per_octave", W, H, MAX_PX, {}, {}, 1),
]


@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("name,w,h,max_px,cfg,env,knob", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_run_forms_show_the_last_image(vk, oracle, monkeypatch, n, name, w, h, max_px, cfg, env, knob):
    imgs = _images(vk, 6000 + 100 * [v[0] for v in VARIANTS].index(name) + n, n, w, h)
    _check(vk, oracle, monkeypatch, imgs, _run(0, n), nbuf=n, cap=n, cfg=cfg, env=dict(env, VKSIFT_DEFER_CHUNK=0), max_px=max_px, knob=knob)


# ---- random operation sequences ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("defer", [0, 1])
def test_random_scale_space_reads_follow_the_model(vk, oracle, monkeypatch, defer, seed):
    """plain detects (mostly in runs into consecutive buffers), ext batches, feature reads and reads of a random scale-space plane; the
    model is the buffer contents and the last shown image. Features and planes against the oracle."""
    rng = np.random.default_rng(seed)
    shapes = [(160, 120), (136, 100)]
    pool = [vk.gen_synthetic_image_family(7000 + 40 * seed + k, *shapes[k % 2], k % 3) for k in range(8)]
    nbuf, cap, max_px = 8, 4, 160 * 120
    okw = _oracle_kw({}, max_px)
    ocfg = oracle.default_config(math_mode=1, **okw)
    pyrs, feats_ref = {}, {}
    monkeypatch.setenv("VKSIFT_DEFER", str(defer))
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    content = [None] * nbuf
    shown = None
    steps = 0
    with vk.Instance(vk.default_config(input_image_max_size=max_px, sift_buffer_count=nbuf), batch_capacity=cap) as inst:
        while steps < 150:
            r = rng.integers(0, 100)
            if r < 35:
                n = int(rng.integers(1, 6))
                b = int(rng.integers(0, nbuf - n + 1))
                shape = int(rng.integers(0, 2))
                for j in range(n):
                    k = int(rng.choice([i for i in range(len(pool)) if i % 2 == shape]))
                    inst.detectFeatures(pool[k], b + j)
                    content[b + j], shown = k, k
                steps += n
                continue
            if r < 45:
                k, b = int(rng.integers(0, len(pool))), int(rng.integers(0, nbuf))
                inst.detectFeatures(pool[k], b)
                content[b], shown = k, k
            elif r < 55:
                n = int(rng.integers(1, cap + 1))
                b = int(rng.integers(0, nbuf - n + 1))
                shape = int(rng.integers(0, 2))
                ks = [int(rng.choice([i for i in range(len(pool)) if i % 2 == shape])) for _ in range(n)]
                inst.detectFeaturesBatch([pool[k] for k in ks], b)
                content[b:b + n] = ks
                shown = ks[0]
            elif r < 75:
                b = int(rng.integers(0, nbuf))
                f = inst.downloadFeatures(b)
                if content[b] is None:
                    assert len(f) == 0, (steps, b)
                else:
                    k = content[b]
                    if k not in feats_ref:
                        feats_ref[k] = oracle.detect(ocfg, pool[k])[0].tobytes()
                    assert f.tobytes() == feats_ref[k], (steps, b, k)
            elif shown is not None:
                if shown not in pyrs:
                    pyrs[shown] = oracle.Pyramid(ocfg, pool[shown])
                pyr = pyrs[shown]
                assert inst.getScaleSpaceNbOctaves() == pyr.nb_octaves, steps
                o = int(rng.integers(0, pyr.nb_octaves))
                assert inst.getScaleSpaceOctaveResolution(o) == pyr.resolution(o), (steps, o)
                if rng.integers(0, 2):
                    s = int(rng.integers(0, pyr.S + 3))
                    got, ref = inst.downloadScaleSpaceImage(o, s), pyr.gauss(o, s)
                else:
                    s = int(rng.integers(0, pyr.S + 2))
                    got, ref = inst.downloadDoGImage(o, s), pyr.dog(o, s)
                assert _same(got, ref), (steps, shown, o, s)
            steps += 1
        stats = inst.getDeferredStats()
    for p in pyrs.values():
        p.close()
    assert len(pyrs) >= 2 and len(feats_ref) >= 2
    assert (stats[1] > 0) if defer else stats == (0, 0)


# ---- the launch form of a batch ------------------------------------------------------------------------------------------------------
def test_batch_of_8_takes_the_tail_launches_deterministically(vk):
    """a batch of 8 images with two tail octaves or more queues scales S+1, S+2 of its coarser octaves as multi-octave launches
    (DetectCtx::tail_batch, plan_detection in vksift_detect.c), unless VKSIFT_TUNE_TAIL_MULTI = 1: fewer blur launches, the same launches on every call, the same
    feature bytes as the per-octave form"""
    w, h, n = 1536, 1024, 8
    imgs = [vk.gen_synthetic_image_family(7700 + i, w, h, i % 3) for i in range(n)]
    L = vk.lib()
    out = {}
    try:
        for knob in (1, 0):
            L.vksift_hip_tune(TUNE_TAIL_MULTI, knob)
            launches, feats = [], []
            with vk.Instance(vk.default_config(input_image_max_size=w * h, sift_buffer_count=n), batch_capacity=n) as inst:
                inst.setProfiling(True)
                for _ in range(3):
                    inst.detectFeaturesBatch(imgs, 0)
                    feats.append([inst.downloadFeatures(i).tobytes() for i in range(n)])
                    t = inst.getAccumulatedDetectTimings(reset=True)
                    assert t["nb_calls"] == 1, t
                    launches.append(t["nb_blur_launches_all"])
            out[knob] = (launches, feats)
    finally:
        L.vksift_hip_tune(TUNE_TAIL_MULTI, 0)
    per_scale, per_octave = out[0], out[1]
    assert len(set(per_scale[0])) == 1 and len(set(per_octave[0])) == 1, (per_scale[0], per_octave[0])
    assert 0 < per_scale[0][0] < per_octave[0][0], (per_scale[0], per_octave[0])
    ref = per_octave[1][0]
    assert all(len(f) > 164 * 100 for f in ref) and len(set(ref)) == n      # distinct images, features in every buffer
    assert all(f == ref for f in per_scale[1] + per_octave[1])
