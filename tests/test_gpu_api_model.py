"""Random walks over every stateful entry of the API on real instances, checked against the model of tests/api_model.py: three profiles (plain
detections staged and launched as batches; overlapped batches of 8 with the packed download — no graph replay: overlapped detections are never
captured, tests/test_gpu_graph_cache.py covers the replay —; clamped sections without record posting), two
seeds each. This test checks STATE — which launch reads which rows, and when —, not kernels: the expected records come from the oracle and the
numpy restatements, those of the describe calls from describe calls on a fresh quiet instance made before the walk (tests/test_gpu_describe.py holds
the describe kernels to their restatement). tests/test_api_model.py pins on the CPU which edges these walks reach and that the executor notices
planted bookkeeping faults. VKSIFT_TEST_SEQUENCE_SEEDS adds seeds for a soak, as in tests/test_gpu_api_scenarios.py."""
import os

import numpy as np
import pytest

import api_model as A

pytestmark = pytest.mark.gpu

STEPS, SEEDS = A.STEPS, A.SEEDS


def _cases():
    extra = os.environ.get("VKSIFT_TEST_SEQUENCE_SEEDS")
    more = [int(x) for x in extra.split(",")] if extra else []
    return [(p, s) for p in A.PROFILES for s in SEEDS[p] + more]


def instance(vk, profile):
    p = A.PROFILES[profile]
    kw = {} if p["cap"] is None else {"max_nb_sift_per_buffer": p["cap"]}
    cfg = vk.default_config(sift_buffer_count=p["nbuf"], input_image_max_size=max(w * h for w, h in A.SIZES), **kw)
    return vk.Instance(cfg, batch_capacity=p["bc"])


_WORLDS = {}


def world(vk, oracle, profile):
    """the profile's images, oracle detections and describe table; the table from describe calls on a quiet instance of the profile's configuration"""
    if profile not in _WORLDS:
        def describe(img, kps, mode):
            with instance(vk, profile) as inst:
                inst.describeKeypoints(img, kps, 0, mode)
                return inst.downloadFeatures(0), inst.getPlacedKeypointsNumber(0)
        _WORLDS[profile] = A.World(profile, oracle, vk, describe)
    return _WORLDS[profile]


@pytest.fixture(scope="module")
def scratch(vk):
    """device memory for vksift_ext_exportDescriptorsDevice, as large as any buffer's descriptors (made here, so that the first walk of a process is not
    the one timed with torch's start-up)"""
    import torch

    return torch.zeros(vk.default_config().max_nb_sift_per_buffer * 128, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("profile,seed", _cases())
def test_random_walks_over_the_whole_api_follow_the_model(vk, oracle, monkeypatch, scratch, profile, seed):
    for k, v in A.PROFILES[profile]["env"].items():
        monkeypatch.setenv(k, v)
    level = vk.lib().vksift_log_get_level()                  # (the logger's own getter; its levels are those of vksift_setLogLevel)
    vk.lib().vksift_setLogLevel(vk.VKSIFT_NO_LOG)            # clamped sections warn and refused calls log, by the hundred
    try:
        w = world(vk, oracle, profile)
        if profile == "clamped":
            assert all(w.clamps)
        # the table the CPU test generates its walks from is this one: the reach pinned there is the reach of this walk
        rec = np.load(A.GOLDEN)
        for d, (recs, placed) in enumerate(w.desc):
            assert recs.tobytes() == rec[f"{profile}_{d}_records"].tobytes() and placed == int(rec[f"{profile}_{d}_placed"]) and placed > 10, d
        ops, _ = A.generate(seed, STEPS, profile, w)
        with instance(vk, profile) as inst:
            A.run(A.Real(vk, inst, scratch), ops, A.Model(w), (profile, seed))
    finally:
        vk.lib().vksift_setLogLevel(level)
