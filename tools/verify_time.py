"""Time vksift_ext_verifyHomography (--model h, the default) or vksift_ext_verifyFundamental (--model f) on the benchmark workload: B frames
640x480, consecutive pairs, matchFeaturesFiltered(0.8, True), then the verification (nb_hypotheses, 2.5) timed by HIP events
(vksift_ext_getVerifyTime): warm-ups, then repetitions; median and spread. The only other RANSAC on the box is the numpy restatement
(tests/np_verify.py, tests/np_verify_f.py), timed on a few of the same pairs for scale. With --refine ROUNDS every verification is
followed by vksift_ext_refineHomography(ROUNDS, 2.5) or, with --model f, vksift_ext_refineFundamental(ROUNDS, 2.5), timed by its own events
(vksift_ext_getRefineTime, vksift_ext_getRefineFundamentalTime). In every mode the host wall time
from the verify call to the first record read back (the verified one, or the refined one with --refine) is reported as
wall_ms_to_first_record_median: each iteration reads record 0, a host wait, before it asks for the event times, which that wait does not change.

usage: verify_time.py [B=512] [nb_hypotheses=1024] [repeats=20] [warmups=3] [--model h|f] [--refine ROUNDS] [--json out.json] [--once]
       (--once: one verification, for a kernel trace)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from vulkansift_amd import api

MODEL = "h"
REFINE = 0
argv = []
for i, arg in enumerate(sys.argv[1:], 1):
    if sys.argv[i - 1] in ("--model", "--json", "--refine"):
        if sys.argv[i - 1] == "--model":
            MODEL = arg
        if sys.argv[i - 1] == "--refine":
            REFINE = int(arg)
        continue
    argv.append(arg)
assert MODEL in ("h", "f"), "--model h|f"
args = [a for a in argv if not a.startswith("--")]
B = int(args[0]) if len(args) > 0 else 512
NH = int(args[1]) if len(args) > 1 else 1024
REP = int(args[2]) if len(args) > 2 else 20
WARM = int(args[3]) if len(args) > 3 else 3
once = "--once" in sys.argv
W, H = 640, 480
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)
gen = np.stack([api.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(min(B, 64))])
frames = np.ascontiguousarray(np.concatenate([gen] * ((B + len(gen) - 1) // len(gen)))[:B])
cfg = api.default_config(sift_buffer_count=B, gpu_device_index=0, input_image_max_size=W * H)
a = list(range(B))
b = [(i + 1) % B for i in a]
with api.Instance(cfg, batch_capacity=B) as inst:
    verify, get = (inst.verifyFundamental, inst.getFundamental) if MODEL == "f" else (inst.verifyHomography, inst.getHomography)
    refine, get_refined, refine_time = ((inst.refineFundamental, inst.getRefinedFundamental, inst.getRefineFundamentalTime) if MODEL == "f" else
                                        (inst.refineHomography, inst.getRefinedHomography, inst.getRefineTime))
    inst.setProfiling(True)
    inst.detectFeaturesBatch(list(frames), 0)
    inst.matchFeaturesFiltered(a, b, 0.8, True)
    n_f = np.array([len(inst.downloadFilteredMatches(k)) for k in range(B)])
    ms, rms, wall = [], [], []
    for it in range(1 if once else WARM + REP):
        t0 = time.perf_counter()
        verify(NH, 2.5, it)
        if REFINE:
            refine(REFINE, 2.5)
            get_refined(0)
        else:
            get(0)
        t1 = time.perf_counter()
        t = inst.getVerifyTime()
        if once or it >= WARM:
            ms.append(t)
            wall.append((t1 - t0) * 1e3)
            if REFINE:
                rms.append(refine_time())
    valid = sum(int(get(k)["valid"]) for k in range(B))
    out = {"model": MODEL, "pairs": B, "nb_hypotheses": NH, "threshold_px": 2.5, "repeats": len(ms), "verify_ms_median": float(np.median(ms)), "verify_ms_min": float(np.min(ms)),
           "verify_ms_max": float(np.max(ms)), "filtered_matches_per_pair_mean": float(n_f.mean()), "filtered_matches_per_pair_min": int(n_f.min()),
           "filtered_matches_per_pair_max": int(n_f.max()), "valid_pairs": valid, "match_ms": float(inst.getMatchTime()),
           "wall_ms_to_first_record_median": float(np.median(wall))}
    if REFINE:
        ref = [get_refined(k) for k in range(B)]
        hom = [get(k) for k in range(B)]
        out.update({"refine_rounds": REFINE, "refine_ms_median": float(np.median(rms)), "refine_ms_min": float(np.min(rms)), "refine_ms_max": float(np.max(rms)),
                    "pairs_with_an_accepted_round": sum(int(r["rounds"]) > 0 for r in ref),
                    "inliers_per_pair_mean_ransac": float(np.mean([int(h["nb_inliers"]) for h in hom])),
                    "inliers_per_pair_mean_refined": float(np.mean([int(r["nb_inliers"]) for r in ref]))})
    if not once:
        if MODEL == "f":
            import np_verify_f as V
        else:
            import np_verify as V

        ks = list(range(0, B, max(1, B // 4)))[:4]
        t0 = time.perf_counter()
        for k in ks:
            fa, fb, fm = inst.downloadFeatures(a[k]), inst.downloadFeatures(b[k]), inst.downloadFilteredMatches(k)
            c = np.stack([fa["x"][fm["idx_a"]], fa["y"][fm["idx_a"]], fb["x"][fm["idx_b"]], fb["y"][fm["idx_b"]]], axis=1).astype(np.float32).reshape(-1, 4)
            V.ransac(c, NH, 2.5, 0, slot=k)
        out["numpy_restatement_ms_per_pair"] = (time.perf_counter() - t0) / len(ks) * 1e3
print(json.dumps(out))
for i, arg in enumerate(sys.argv):
    if arg == "--json" and i + 1 < len(sys.argv):
        with open(sys.argv[i + 1], "w") as f:
            json.dump(out, f, indent=1)
