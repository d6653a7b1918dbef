"""Time vksift_ext_keepStrongestFeaturesGrid on the benchmark workload: B frames 640x480 detected in one batch, every buffer cut to N features
spread over a cols x rows grid. Per repetition, after a fresh detection into buffers [0, B) and a second one into [B, 2B):
  1. the grid selection of buffers [0, B), by its HIP events (vksift_ext_getKeepStrongestGridTime);
  2. the plain budget (vksift_ext_keepStrongestFeatures, same N) on buffers [B, 2B), the same features, by its HIP events, same process;
  3. the same result the only way the API offered before: vksift_downloadFeatures, bucketing and stable sorts on the host,
     vksift_uploadFeatures into buffers [2B, 3B) — host wall time, through the public API, same process.
Warm-ups, then repetitions; median, minimum and maximum of each. Then one buffer of --big uploaded features, scattered over the frame, cut to
--big-n (the kernel is one workgroup per buffer: this is the single-CU case), grid rule and plain budget."""
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
ap.add_argument("--cols", type=int, default=8)
ap.add_argument("--rows", type=int, default=6)
ap.add_argument("--big", type=int, default=100000)
ap.add_argument("--big-n", type=int, default=8192)
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, W, H, N, COLS, ROWS = opt.frames, 640, 480, opt.max_features, opt.cols, opt.rows
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)


def strongest(keys, n):
    """the first n of keys by (key descending, index ascending), as sorted indices"""
    return np.sort(np.argsort(-keys, kind="stable")[:n])


def host_select(f, n):
    """what a caller writes: bucket by cell, the strongest n // cells of every cell, then the strongest of the rest, in the original order"""
    if len(f) <= n:
        return f
    keys = np.abs(f["intensity"]).view(np.uint32).astype(np.int64)
    bx = np.array([np.float32(float(j) * W / COLS) for j in range(1, COLS)], np.float32)
    by = np.array([np.float32(float(j) * H / ROWS) for j in range(1, ROWS)], np.float32)
    cell = (f["y"][:, None] >= by[None, :]).sum(1) * COLS + (f["x"][:, None] >= bx[None, :]).sum(1)
    keep = np.zeros(len(f), bool)
    q = n // (COLS * ROWS)
    order = np.argsort(cell, kind="stable")
    starts = np.searchsorted(cell[order], np.arange(COLS * ROWS + 1))
    for c in range(COLS * ROWS if q else 0):
        idx = order[starts[c]:starts[c + 1]]
        keep[idx[strongest(keys[idx], q)]] = True
    rest = np.flatnonzero(~keep)
    keep[rest[strongest(keys[rest], n - int(keep.sum()))]] = True
    return f[keep]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


gen = np.stack([api.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(min(B, 64))])
frames = list(np.ascontiguousarray(np.concatenate([gen] * ((B + len(gen) - 1) // len(gen)))[:B]))
cfg = api.default_config(sift_buffer_count=3 * B, gpu_device_index=0, input_image_max_size=W * H)
ids = list(range(B))
out = {"frames": B, "max_features": N, "grid": [COLS, ROWS], "repeats": opt.repeats}
with api.Instance(cfg, batch_capacity=B) as inst:
    inst.setProfiling(True)
    grid_ms, plain_ms, host_ms = [], [], []
    for it in range(opt.warmups + opt.repeats):
        inst.detectFeaturesBatch(frames, 0)
        inst.detectFeaturesBatch(frames, B)
        n_feat = np.array([inst.getFeaturesNumber(k) for k in ids])
        t0 = time.perf_counter()
        for k in ids:
            inst.uploadFeatures(host_select(inst.downloadFeatures(k), N), 2 * B + k)
        inst.getFeaturesNumber(3 * B - 1)
        t_host = (time.perf_counter() - t0) * 1e3
        inst.keepStrongestFeaturesGrid(0, B, N, W, H, COLS, ROWS)
        t_grid = inst.getKeepStrongestGridTime()
        inst.keepStrongestFeatures(B, B, N)
        t_plain = inst.getKeepStrongestTime()
        if it >= opt.warmups:
            grid_ms.append(t_grid), plain_ms.append(t_plain), host_ms.append(t_host)
    step = max(1, B // 16)
    same = all(inst.downloadFeatures(k).tobytes() == inst.downloadFeatures(2 * B + k).tobytes() for k in ids[::step])
    differs = sum(inst.downloadFeatures(k).tobytes() != inst.downloadFeatures(B + k).tobytes() for k in ids[::step])
    out.update(features_per_frame_mean=float(n_feat.mean()), features_per_frame_max=int(n_feat.max()), frames_above_budget=int((n_feat > N).sum()),
               grid_selection_ms=stats(grid_ms), plain_budget_ms=stats(plain_ms), download_bucket_sort_upload_ms=stats(host_ms),
               host_path_gives_the_same_records=bool(same), sampled_frames_where_the_grid_rule_differs_from_the_plain_budget=int(differs))

if opt.big:
    rng = np.random.default_rng(7)
    big = np.zeros(opt.big, api.FEATURE_DTYPE)
    big["x"], big["y"] = rng.uniform(0, W, opt.big).astype(np.float32), rng.uniform(0, H, opt.big).astype(np.float32)
    big["intensity"] = (rng.uniform(0.005, 0.2, opt.big) * rng.choice([-1.0, 1.0], opt.big)).astype(np.float32)
    big["descriptor"] = rng.integers(0, 256, (opt.big, 128), dtype=np.uint8)
    cfg = api.default_config(sift_buffer_count=2, gpu_device_index=0, input_image_max_size=W * H, max_nb_sift_per_buffer=opt.big)
    with api.Instance(cfg) as inst:
        inst.setProfiling(True)
        ms, ms_plain = [], []
        for it in range(opt.warmups + opt.repeats):
            inst.uploadFeatures(big, 0)
            inst.uploadFeatures(big, 1)
            inst.keepStrongestFeaturesGrid(0, 1, opt.big_n, W, H, COLS, ROWS)
            inst.keepStrongestFeatures(1, 1, opt.big_n)
            t, tp = inst.getKeepStrongestGridTime(), inst.getKeepStrongestTime()
            if it >= opt.warmups:
                ms.append(t), ms_plain.append(tp)
        ok = inst.downloadFeatures(0).tobytes() == host_select(big, opt.big_n).tobytes()
        out["one_buffer"] = {"features": opt.big, "max_features": opt.big_n, "grid_selection_ms": stats(ms), "plain_budget_ms": stats(ms_plain), "same_as_host": bool(ok)}
print(json.dumps(out))
if opt.json:
    os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
