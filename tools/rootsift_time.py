"""Time vksift_ext_convertToRootSift on the benchmark workload: B frames 640x480 detected in one batch, every buffer converted in place. Per
repetition, after a fresh detection into buffers [0, B):
  1. the conversion of the B buffers before the instance has a matcher cache (first pass only: 256 bytes per row) and with it (388 bytes per
     row), by its HIP events (vksift_ext_getRootSiftTime);
  2. for scale, vksift_ext_getMatchTime of the B self-matches behind the conversion and vksift_ext_getKeepStrongestTime of a budget of N;
  3. once, the same result the only way the API offered before: vksift_downloadFeatures, the conversion on the host, vksift_uploadFeatures
     into buffers [B, 2B) — host wall time, through the public API, same process.
Warm-ups, then repetitions; median, minimum and maximum of each, and the rate the median implies for the bytes moved.
--quality: the metrics of tests/quality.py over its five warps with and without the conversion, same ratio threshold (asserts nothing)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from vulkansift_amd import api

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("frames", nargs="?", type=int, default=512)
ap.add_argument("repeats", nargs="?", type=int, default=10)
ap.add_argument("warmups", nargs="?", type=int, default=2)
ap.add_argument("-n", "--max-features", type=int, default=1000)
ap.add_argument("--quality", action="store_true")
ap.add_argument("--ratio", type=float, default=0.75)
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, W, H = opt.frames, 640, 480
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)


def host_root(f):
    """what a caller writes (COLMAP's L1_ROOT): L1-normalise, square root, round(512 x), saturate"""
    d = f["descriptor"].astype(np.float32)
    s = d.sum(1, keepdims=True)
    out = f.copy()
    out["descriptor"] = np.minimum(np.floor(512.0 * np.sqrt(d / np.maximum(s, 1.0)) + 0.5), 255).astype(np.uint8)
    return out


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


out = {"frames": B, "repeats": opt.repeats}
if B:
    gen = np.stack([api.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(min(B, 64))])
    frames = list(np.ascontiguousarray(np.concatenate([gen] * ((B + len(gen) - 1) // len(gen)))[:B]))
    cfg = api.default_config(sift_buffer_count=2 * B, gpu_device_index=0, input_image_max_size=W * H)
    ids = list(range(B))
    with api.Instance(cfg, batch_capacity=B) as inst:
        inst.setProfiling(True)
        plain_ms = []
        for it in range(opt.warmups + opt.repeats):     # no matching yet: the instance has no cache, the launch converts the records only
            inst.detectFeaturesBatch(frames, 0)
            inst.convertToRootSift(0, B)
            t = inst.getRootSiftTime()
            if it >= opt.warmups:
                plain_ms.append(t)
        rows = int(sum(inst.getFeaturesNumber(k) for k in ids))
        cache_ms, match_ms, budget_ms = [], [], []
        for it in range(opt.warmups + opt.repeats):
            inst.detectFeaturesBatch(frames, 0)
            if it == 0:
                inst.matchFeaturesBatch(ids, ids)           # the cache exists from here on
            inst.convertToRootSift(0, B)
            t_conv = inst.getRootSiftTime()
            inst.matchFeaturesBatch(ids, ids)
            t_match = inst.getMatchTime()
            inst.keepStrongestFeatures(0, B, opt.max_features)
            t_budget = inst.getKeepStrongestTime()
            if it >= opt.warmups:
                cache_ms.append(t_conv), match_ms.append(t_match), budget_ms.append(t_budget)
        inst.detectFeaturesBatch(frames, 0)
        inst.getFeaturesNumber(B - 1)
        t0 = time.perf_counter()
        for k in ids:
            inst.uploadFeatures(host_root(inst.downloadFeatures(k)), B + k)
        inst.getFeaturesNumber(2 * B - 1)
        t_host = (time.perf_counter() - t0) * 1e3
        inst.convertToRootSift(0, B)
        probe = ids[:: max(1, B // 16)]
        diff = sum(int((inst.downloadFeatures(k)["descriptor"] != inst.downloadFeatures(B + k)["descriptor"]).sum()) for k in probe)
        out.update(rows=rows, rows_per_frame=rows / B, conversion_ms=stats(plain_ms), conversion_with_cache_ms=stats(cache_ms), match_ms=stats(match_ms),
                   budget_ms=stats(budget_ms), download_convert_upload_ms=t_host, bytes_per_row={"records": 256, "with_cache": 388},
                   tb_per_s={"records": rows * 256 / (np.median(plain_ms) * 1e-3) / 1e12, "with_cache": rows * 388 / (np.median(cache_ms) * 1e-3) / 1e12},
                   bins_where_the_fp32_host_formula_differs=diff, bins_compared=int(sum(inst.getFeaturesNumber(k) for k in probe)) * 128)

if opt.quality:
    import quality

    img1 = api.gen_synthetic_image(35, W, H)
    table = []
    with api.Instance(api.default_config(sift_buffer_count=4, input_image_max_size=W * H)) as inst:
        for k, kw in enumerate(quality.WARPS):
            Hm = quality.homography(W, H, **kw)
            img2 = quality.warp(img1, Hm)
            for first in (0, 2):
                inst.detectFeatures(img1, first)
                inst.detectFeatures(img2, first + 1)
            inst.convertToRootSift(2, 2)
            f1, f2 = inst.downloadFeatures(0), inst.downloadFeatures(1)
            for name, first in (("sift", 0), ("rootsift", 2)):
                inst.matchFeaturesFiltered([first], [first + 1], opt.ratio, True)
                fm = inst.downloadFilteredMatches(0)
                s = quality.score(f1, f2, fm["idx_a"], fm["idx_b"], Hm, W, H)
                table.append(dict(warp=k + 1, form=name, **{key: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for key, v in s.items()}))
    out["quality"] = {"ratio": opt.ratio, "rows": table}

print(json.dumps(out))
if opt.json:
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
