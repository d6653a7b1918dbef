"""Time vksift_ext_matchFeaturesGuided on the benchmark workload beside the filtered matching it follows: B frames 640x480, self-pairs (i, i),
matchFeaturesFiltered(0.8, True) timed by vksift_ext_getMatchTime, a verification of the model asked for, then the guided matching (2.5 px, 0.8,
no distance limit, cross-check) timed by HIP events (vksift_ext_getGuidedMatchTime): warm-ups, then repetitions; median and spread of both on the same
run. The share of the (a, b) pairs that the model admits is counted by the numpy restatement (tests/np_guided.py) on four of the pairs.
--once: one guided matching and nothing else, for a kernel trace."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from vulkansift_amd import api

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("pairs", nargs="?", type=int, default=512)
ap.add_argument("repeats", nargs="?", type=int, default=20)
ap.add_argument("warmups", nargs="?", type=int, default=3)
ap.add_argument("--model", choices=("h", "f"), default="f")
ap.add_argument("--json", metavar="OUT")
ap.add_argument("--once", action="store_true")
opt = ap.parse_args()
B, W, H = opt.pairs, 640, 480
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)
gen = np.stack([api.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(min(B, 64))])
frames = np.ascontiguousarray(np.concatenate([gen] * ((B + len(gen) - 1) // len(gen)))[:B])
cfg = api.default_config(sift_buffer_count=B, gpu_device_index=0, input_image_max_size=W * H)
a = list(range(B))
fundamental = opt.model == "f"
kind = api.GUIDE_FUNDAMENTAL if fundamental else api.GUIDE_HOMOGRAPHY
with api.Instance(cfg, batch_capacity=B) as inst:
    inst.setProfiling(True)
    inst.detectFeaturesBatch(list(frames), 0)
    n_feat = np.array([inst.getFeaturesNumber(k) for k in range(B)])
    match_ms, guided_ms = [], []
    for it in range(1 if opt.once else opt.warmups + opt.repeats):
        inst.matchFeaturesFiltered(a, a, 0.8, True)
        tm = inst.getMatchTime()
        (inst.verifyFundamental if fundamental else inst.verifyHomography)(1024, 2.5, it)
        inst.matchFeaturesGuided(kind, None, 2.5, 0.8, float("inf"), True)
        tg = inst.getGuidedMatchTime()
        if opt.once or it >= opt.warmups:
            match_ms.append(tm), guided_ms.append(tg)
    n_f = np.array([len(inst.downloadFilteredMatches(k)) for k in range(B)])
    n_g = np.array([len(inst.downloadGuidedMatches(k)) for k in range(B)])
    out = {"model": opt.model, "pairs": B, "threshold_px": 2.5, "ratio": 0.8, "cross_check": True, "repeats": len(guided_ms),
           "features_per_frame_mean": float(n_feat.mean()), "guided_ms_median": float(np.median(guided_ms)), "guided_ms_min": float(np.min(guided_ms)),
           "guided_ms_max": float(np.max(guided_ms)), "filtered_match_ms_median": float(np.median(match_ms)), "filtered_match_ms_min": float(np.min(match_ms)),
           "filtered_match_ms_max": float(np.max(match_ms)), "filtered_matches_per_pair_mean": float(n_f.mean()), "guided_matches_per_pair_mean": float(n_g.mean())}
    if not opt.once:
        import np_guided as G

        admitted, tested = 0, 0
        for k in list(range(0, B, max(1, B // 4)))[:4]:
            f, m = inst.downloadFeatures(k), (inst.getFundamental if fundamental else inst.getHomography)(k)
            if int(m["valid"]):
                M = np.asarray(m["F" if fundamental else "H"], np.float32).reshape(9)
                adm = G.admissible(kind, M, f["x"], f["y"], f["x"], f["y"], G.threshold2(2.5))
                admitted, tested = admitted + int(np.count_nonzero(adm)), tested + adm.size
        out["admissible_share"] = admitted / tested if tested else None
print(json.dumps(out))
if opt.json:
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
