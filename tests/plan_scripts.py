"""Scripts of API calls that drive the detection graph cache to its edges — data only: this module imports neither a GPU library nor the built
library. tests/test_detect_plan.py runs them on the simulated device (tests/native/plan_harness.c) and proves from its log that each reaches
its edge; tests/test_gpu_graph_cache.py runs the same calls on the real library and compares bytes with a VKSIFT_GRAPH=0 instance.

A script is a dict: env (VKSIFT_* switches), create (batch_capacity, input_image_max_size, max_nb_sift_per_buffer, sift_buffer_count,
use_input_upsampling, fp16) and ops, a list of tuples:
    ("detect", w, h, buffer)                      vksift_detectFeatures
    ("batch", w, h, first, count)                 vksift_ext_detectFeaturesBatch
    ("batchdev", w, h, first, count, which)       vksift_ext_detectFeaturesBatchDevice from device input block `which` (0 or 1)
    ("num", buffer) ("download", buffer) ("avail", buffer) ("match", a, b) ("prof", 0 | 1) ("describe", w, h, buffer, n_keypoints)
and, for the simulated device alone (the GPU executor skips them):
    ("busy", 0 | 1) ("drain",) ("covered", 0 | 1) ("counts", v)
"""
GRAPH_CACHE = 8       # VKSIFT_GRAPH_CACHE
GIVE_UP_AFTER = 32    # 4 * VKSIFT_GRAPH_CACHE consecutive misses are tolerated: the next one switches the replay off
POST_IDLE = 16        # VKSIFT_POST_IDLE
BIG, SMALL, NARROW = (160, 120), (96, 64), (33, 580)   # NARROW: the area of BIG; its rows, padded to 64 floats on every octave, outgrow the reservation
MAX_PX, MAX_FEATS = 160 * 120, 600
LIMIT, OVER, TINY = (640, 480), (800, 600), (64, 24)   # graph_max_pixels exactly, above it, and (without up-sampling) below a single octave
SIM_ONLY = ("busy", "drain", "covered", "counts")


def create(bc=1, nbuf=12, ups=1, fp16=0, max_px=MAX_PX, max_feats=MAX_FEATS):
    return dict(bc=bc, max_px=max_px, max_feats=max_feats, nbuf=nbuf, ups=ups, fp16=fp16)


def _det(b, size=BIG):
    return ("detect", size[0], size[1], b)


def _cycle10(download):
    ops = []
    for r in range(9):                  # 4 rounds reach the give-up (the 33rd miss is detection 33), 5 more follow it
        for b in range(10):
            ops.append(_det(b))
            if download:
                ops.append(("download", b))
        if not download and r in (3, 8):
            ops += [("download", b) for b in range(10)]   # the stretches in between have no download and no query at all
    return ops


def _hit_resets(misses):
    """`misses` consecutive misses (ten buffers in turn never hit a cache of eight), a hit, `misses` more, a hit"""
    ops, b = [], 0
    for _ in range(2):
        for _ in range(misses):
            ops += [_det(b % 10), ("download", b % 10)]
            b += 1
        ops += [_det((b - 1) % 10), ("download", (b - 1) % 10)]
    return ops


def _miss_run(miss, ineligible):
    """20 misses (ten buffers in turn never hit a cache of eight), the ineligible calls, 12 more misses — the 32nd capture —, the 33rd miss, 3 more"""
    step = lambda k: [("detect", miss[0], miss[1], k % 10), ("num", k % 10)]
    return [op for k in range(20) for op in step(k)] + ineligible + [op for k in range(20, 36) for op in step(k)]


SCRIPTS = {
    # single detections cycling over ten buffers: every call misses, every miss from the ninth on evicts an exec
    "cycle10": dict(env={"VKSIFT_DEFER": "0"}, create=create(), ops=_cycle10(True)),
    # ... with nothing between the detections: the evicted exec may still be executing when it is destroyed
    "cycle10_unsync": dict(env={"VKSIFT_DEFER": "0"}, create=create(), ops=_cycle10(False)),
    # the same from device memory: no staging buffer to wait for, so nothing at all orders the host behind the launches it evicts
    # (device_pool: on the GPU every detection reads a region of its own, written before the first call — nothing may wait in between)
    "cycle10_device": dict(env={"VKSIFT_DEFER": "0"}, create=create(), device_pool=True,
                           ops=[("batchdev", BIG[0], BIG[1], b, 1, 0) for _ in range(2) for b in range(10)] + [("download", b) for b in range(10)]),
    # nine keys, then the first again (evicted: recaptured), and again (replayed)
    "comeback": dict(env={"VKSIFT_DEFER": "0"}, create=create(),
                     ops=[op for b in list(range(9)) + [0, 0] for op in (_det(b), ("download", b))]),
    # 30 misses, a hit, 30 misses, a hit: the counter never passes 32
    "hit_resets": dict(env={"VKSIFT_DEFER": "0"}, create=create(), ops=_hit_resets(30)),
    "hit_resets_short": dict(env={"VKSIFT_DEFER": "0"}, create=create(), ops=_hit_resets(10)),
    # a capture, then a narrow image of the same area: the scratch grows, every exec holds freed addresses and is dropped
    "grow_drop": dict(env={"VKSIFT_DEFER": "0"}, create=create(),
                      ops=[_det(0), ("download", 0), _det(1, SMALL), ("download", 1), _det(0, NARROW), ("download", 0), _det(0), ("download", 0),
                           _det(0), ("download", 0), _det(1, SMALL), ("download", 1)]),
    # a run of plain detections is staged and launched as batches whose capacity doubles to 8: every growth drops the cache
    "defer_grow": dict(env={"VKSIFT_DEFER": "1"}, create=create(),
                       ops=[_det(0), ("download", 0), _det(0), ("download", 0)] + [_det(b) for b in range(12)] + [("download", b) for b in range(12)] +
                           [_det(0), ("download", 0), _det(0), ("download", 0), _det(0), ("download", 0), _det(1), ("download", 1)]),
    # the first matching creates the matcher's cache blocks: the detections after it write dense rows, a different launch sequence
    "dense_flip": dict(env={"VKSIFT_DEFER": "0"}, create=create(),
                       ops=[_det(0), ("download", 0), _det(1), ("download", 1), ("match", 0, 1), _det(0), _det(0), ("download", 0), ("match", 0, 1),
                            _det(1), ("download", 1), ("match", 1, 0)]),
    # posted detections nobody fetches: after POST_IDLE of them the posting is switched off, by the next download on again
    "post_flip": dict(env={"VKSIFT_DEFER": "0"}, create=create(),
                      ops=[_det(0), ("download", 0)] + [_det(0)] * (POST_IDLE + 2) + [("download", 0), _det(0), ("download", 0)]),
    # device input from two blocks in turn: the input pointer is part of the key
    "two_pointers": dict(env={"VKSIFT_DEFER": "0"}, create=create(),
                         ops=[op for k in range(6) for op in (("batchdev", BIG[0], BIG[1], 0, 1, k & 1), ("download", 0))]),
    # the first describe call extends the descriptor scale table, whose length is an argument of every descriptor launch
    "describe_table": dict(env={"VKSIFT_DEFER": "0"}, create=create(),
                           ops=[_det(0), ("download", 0), _det(0), ("download", 0), ("describe", BIG[0], BIG[1], 1, 20), ("download", 1), _det(0),
                                ("download", 0), _det(0), ("download", 0), ("describe", BIG[0], BIG[1], 1, 20), _det(0), ("download", 0)]),
    # ---- ineligible calls neither capture nor count as misses (CPU only)
    # an instance reserved above graph_max_pixels under the default VKSIFT_GRAPH: detections above, exactly at and below the limit, per image and per batch
    "above_limit": dict(env={"VKSIFT_DEFER": "0"}, create=create(bc=2, max_px=OVER[0] * OVER[1]),
                        ops=[_det(0, OVER), ("download", 0), _det(0, OVER), ("download", 0), _det(0, LIMIT), ("download", 0), _det(0, LIMIT), ("download", 0),
                             ("batch", 480, 360, 0, 2), ("download", 0), ("batch", 480, 360, 0, 2), ("download", 1), ("batch", 480, 360, 0, 1), ("download", 0),
                             ("batch", 480, 360, 0, 1), ("download", 0), _det(0, OVER), ("download", 0), _det(0, LIMIT), ("download", 0)]),
    # two pyramid buffers: a detection without an octave does not overlap, so the two-buffer clause alone keeps it from being captured ...
    "two_buffers": dict(env={"VKSIFT_DEFER": "0", "VKSIFT_PYR_PINGPONG": "2"}, create=create(ups=0),
                        ops=[_det(0, TINY), ("num", 0), _det(0, TINY), ("num", 0), _det(0), ("download", 0), _det(0), ("download", 0), _det(0, TINY), ("num", 0)]),
    # ... as the same calls on the one-buffer overlap instance show: there it is captured and replayed, the overlapped detections are not
    "one_buffer_overlap": dict(env={"VKSIFT_DEFER": "0", "VKSIFT_PYR_PINGPONG": "1"}, create=create(ups=0),
                               ops=[_det(0, TINY), ("num", 0), _det(0, TINY), ("num", 0), _det(0), ("download", 0), _det(0), ("download", 0), _det(0, TINY), ("num", 0)]),
    # profiled detections, a describe call and detections above the limit in the middle of a run of misses: the give-up comes at the 33rd MISS
    "miss_run": dict(env={"VKSIFT_DEFER": "0"}, create=create(max_px=OVER[0] * OVER[1]),
                     ops=_miss_run(BIG, [("prof", 1), _det(10), ("num", 10), _det(10), ("num", 10), ("prof", 0), ("describe", BIG[0], BIG[1], 11, 20), ("num", 11),
                                         _det(10, OVER), ("num", 10), _det(10, OVER), ("num", 10), _det(11, OVER), ("num", 11)])),
    # ... and overlapped detections (one-buffer overlap instance: only images without an octave are eligible, and they are the misses)
    "miss_run_overlap": dict(env={"VKSIFT_DEFER": "0", "VKSIFT_PYR_PINGPONG": "1"}, create=create(ups=0),
                             ops=_miss_run(TINY, [_det(10), ("num", 10), _det(10), ("num", 10), _det(11), ("num", 11), _det(10, SMALL), ("num", 10)])),
    # the environment, capacity and sizes of api_model.PROFILES["batch"] (tests/test_detect_plan.py holds them to that table)
    "batch_profile": dict(env={"VKSIFT_GRAPH": "1"}, create=create(bc=8, nbuf=12, max_px=256 * 192, max_feats=100000),
                          ops=[("detect", 160, 120, 0), ("download", 0), ("detect", 160, 120, 0), ("download", 0), ("batch", 256, 192, 0, 8),
                               ("download", 3), ("download", 4), ("detect", 200, 160, 9), ("num", 9), ("detect", 200, 160, 9), ("num", 9),
                               ("batch", 160, 120, 2, 2), ("download", 2), ("batch", 160, 120, 2, 2), ("download", 3), ("batch", 256, 192, 1, 1),
                               ("download", 1), ("batch", 256, 192, 1, 1), ("download", 1), ("match", 0, 1), ("detect", 160, 120, 0), ("download", 0),
                               ("detect", 160, 120, 0), ("download", 0)]),
}
GPU_SCRIPTS = ("cycle10", "cycle10_unsync", "cycle10_device", "comeback", "hit_resets_short", "grow_drop", "defer_grow", "dense_flip", "post_flip", "two_pointers")
