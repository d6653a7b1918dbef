"""Results through the churn of the detection graph cache (vksift_detect.c: graph_lookup, launch_detection): the scripts of tests/plan_scripts.py
on the real library. tests/test_detect_plan.py proves on the simulated device that each script reaches its edge — eviction, the give-up, a key
that comes back, the drop after the scratch grew, the dense and the posting flip, two input pointers —; here every downloaded buffer, match
list and feature count must be byte-identical to the same script on an instance created under VKSIFT_GRAPH=0, the path the other tests pin to
the oracle. Every detection gets a different synthetic image, so a replay that was skipped, stale or taken for the wrong key shows up.
"""
import numpy as np
import pytest

import plan_scripts as PS

pytestmark = pytest.mark.gpu

_IMAGES = {}


def image(vk, seed, w, h):
    if (seed, w, h) not in _IMAGES:
        _IMAGES[(seed, w, h)] = np.ascontiguousarray(vk.gen_synthetic_image(seed, w, h), dtype=np.uint8)
    return _IMAGES[(seed, w, h)]


def run_script(vk, script, d_in):
    """every result the script's calls return, in order; images numbered by the detection that takes them"""
    import torch
    c = script["create"]
    pool = None
    if script.get("device_pool"):     # every device-input detection has its own region, filled up front: the run itself never synchronises
        devs = [op for op in script["ops"] if op[0] == "batchdev"]
        pool = torch.from_numpy(np.concatenate([image(vk, 5000 + k, op[1], op[2]).reshape(-1) for k, op in enumerate(devs)])).cuda()
        offs = np.cumsum([0] + [op[1] * op[2] for op in devs])
        assert len(devs) == len([op for op in script["ops"] if op[0] in ("detect", "batch", "batchdev")])
        torch.cuda.synchronize()
    assert not c["fp16"]
    cfg = vk.default_config(sift_buffer_count=c["nbuf"], input_image_max_size=c["max_px"], max_nb_sift_per_buffer=c["max_feats"],
                            use_input_upsampling=bool(c["ups"]))
    out, seed = [], 5000
    with vk.Instance(cfg, batch_capacity=c["bc"]) as inst:
        for op in script["ops"]:
            name = op[0]
            if name == "detect":
                inst.detectFeatures(image(vk, seed, op[1], op[2]), op[3])
                seed += 1
            elif name == "batch":
                inst.detectFeaturesBatch([image(vk, seed + i, op[1], op[2]) for i in range(op[4])], op[3])
                seed += op[4]
            elif name == "batchdev":
                assert op[4] == 1
                if pool is not None:
                    inst.detectFeaturesBatchDevice(pool.data_ptr() + int(offs[seed - 5000]), 1, op[1], op[2], op[3])
                else:                         # one of two blocks, refilled: the script has fetched the previous detection's results
                    d_in[op[5]][:op[1] * op[2]].copy_(torch.from_numpy(image(vk, seed, op[1], op[2]).reshape(-1)))
                    torch.cuda.synchronize()  # the library reads the block on its own stream
                    inst.detectFeaturesBatchDevice(d_in[op[5]].data_ptr(), 1, op[1], op[2], op[3])
                seed += 1
            elif name == "num":
                out.append(("num", op[1], inst.getFeaturesNumber(op[1])))
            elif name == "download":
                f = inst.downloadFeatures(op[1])
                out.append(("download", op[1], len(f), f.tobytes()))
            elif name == "avail":
                inst.isBufferAvailable(op[1])   # (its answer is a matter of timing)
            elif name == "match":
                inst.matchFeatures(op[1], op[2])
                out.append(("match", op[1], op[2], inst.getMatchesNumber(), inst.downloadMatches().tobytes()))
            else:
                assert name in PS.SIM_ONLY, name
    return out


@pytest.fixture(scope="module")
def d_in():
    import torch
    return [torch.zeros(PS.MAX_PX, dtype=torch.uint8, device="cuda") for _ in range(2)]


def check(vk, monkeypatch, name, d_in):
    script = PS.SCRIPTS[name]
    for k, v in script["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VKSIFT_GRAPH", "0")
    ref = run_script(vk, script, d_in)
    monkeypatch.delenv("VKSIFT_GRAPH")          # the default: on for these sizes
    got = run_script(vk, script, d_in)
    assert len(got) == len(ref) > 0
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (name, i, g[:3], r[:3])
    # the script means something here: its detections find features, and different ones for different images
    downloads = [r for r in ref if r[0] == "download"]
    full = [r for r in downloads if r[2] > 5]
    assert len(full) >= len(downloads) // 2 and len({r[3] for r in full}) > len(full) * 3 // 4, (len(downloads), len(full))


# cycle10 (a download behind every call) runs in front of cycle10_unsync and cycle10_device, which evict execs with work in flight
@pytest.mark.parametrize("name", PS.GPU_SCRIPTS)
def test_results_through_cache_churn_equal_the_graphless_instance(vk, monkeypatch, d_in, name):
    check(vk, monkeypatch, name, d_in)
