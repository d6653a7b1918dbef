"""Time vksift_ext_keepStrongestFeatures on the benchmark workload: B frames 640x480 detected in one batch, every buffer cut to its N strongest
features. Per repetition, after a fresh detection into buffers [0, B):
  1. the selection of the B buffers, by its HIP events (vksift_ext_getKeepStrongestTime);
  2. the same result the only way the API offered before: vksift_downloadFeatures, a stable sort on the host, vksift_uploadFeatures into
     buffers [B, 2B) — host wall time, through the public API, same process;
  3. vksift_ext_getMatchTime of the B self-matches in front of the selection and behind it.
Warm-ups, then repetitions; median, minimum and maximum of each. Then one buffer of --big uploaded features cut to --big-n (the kernel is one
workgroup per buffer: this is the single-CU case)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from vulkansift_amd import api

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("frames", nargs="?", type=int, default=512)
ap.add_argument("repeats", nargs="?", type=int, default=10)
ap.add_argument("warmups", nargs="?", type=int, default=2)
ap.add_argument("-n", "--max-features", type=int, default=1000)
ap.add_argument("--big", type=int, default=100000)
ap.add_argument("--big-n", type=int, default=8192)
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, W, H, N = opt.frames, 640, 480, opt.max_features
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)


def host_select(f, n):
    """what a caller writes: strongest n by |intensity|, ties by index, in the original order"""
    if len(f) <= n:
        return f
    keys = np.abs(f["intensity"]).view(np.uint32).astype(np.int64)
    return f[np.sort(np.argsort(-keys, kind="stable")[:n])]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


gen = np.stack([api.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(min(B, 64))])
frames = list(np.ascontiguousarray(np.concatenate([gen] * ((B + len(gen) - 1) // len(gen)))[:B]))
cfg = api.default_config(sift_buffer_count=2 * B, gpu_device_index=0, input_image_max_size=W * H)
ids = list(range(B))
out = {"frames": B, "max_features": N, "repeats": opt.repeats}
with api.Instance(cfg, batch_capacity=B) as inst:
    inst.setProfiling(True)
    sel_ms, host_ms, before_ms, after_ms = [], [], [], []
    for it in range(opt.warmups + opt.repeats):
        inst.detectFeaturesBatch(frames, 0)
        n_feat = np.array([inst.getFeaturesNumber(k) for k in ids])
        t0 = time.perf_counter()
        for k in ids:
            inst.uploadFeatures(host_select(inst.downloadFeatures(k), N), B + k)
        inst.getFeaturesNumber(2 * B - 1)
        t_host = (time.perf_counter() - t0) * 1e3
        inst.matchFeaturesBatch(ids, ids)
        t_before = inst.getMatchTime()
        inst.keepStrongestFeatures(0, B, N)
        t_sel = inst.getKeepStrongestTime()
        inst.matchFeaturesBatch(ids, ids)
        t_after = inst.getMatchTime()
        if it >= opt.warmups:
            sel_ms.append(t_sel), host_ms.append(t_host), before_ms.append(t_before), after_ms.append(t_after)
    same = all(inst.downloadFeatures(k).tobytes() == inst.downloadFeatures(B + k).tobytes() for k in ids[:: max(1, B // 16)])
    out.update(features_per_frame_mean=float(n_feat.mean()), features_per_frame_max=int(n_feat.max()), frames_above_budget=int((n_feat > N).sum()),
               selection_ms=stats(sel_ms), download_sort_upload_ms=stats(host_ms), match_before_ms=stats(before_ms), match_after_ms=stats(after_ms),
               host_path_gives_the_same_records=bool(same))

if opt.big:
    rng = np.random.default_rng(7)
    big = np.zeros(opt.big, api.FEATURE_DTYPE)
    big["intensity"] = (rng.uniform(0.005, 0.2, opt.big) * rng.choice([-1.0, 1.0], opt.big)).astype(np.float32)
    big["descriptor"] = rng.integers(0, 256, (opt.big, 128), dtype=np.uint8)
    cfg = api.default_config(sift_buffer_count=2, gpu_device_index=0, input_image_max_size=W * H, max_nb_sift_per_buffer=opt.big)
    with api.Instance(cfg) as inst:
        inst.setProfiling(True)
        ms = []
        for it in range(opt.warmups + opt.repeats):
            inst.uploadFeatures(big, 0)
            inst.keepStrongestFeatures(0, 1, opt.big_n)
            t = inst.getKeepStrongestTime()
            if it >= opt.warmups:
                ms.append(t)
        ok = inst.downloadFeatures(0).tobytes() == host_select(big, opt.big_n).tobytes()
        out["one_buffer"] = {"features": opt.big, "max_features": opt.big_n, "selection_ms": stats(ms), "same_as_host": bool(ok)}
print(json.dumps(out))
if opt.json:
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
