#!/usr/bin/env python3
"""Sweep of VKSIFT_TUNE_DESC_SOLO_R (pair mode of the two-wave descriptor launch, features.hip) on the bench's 512 x 640x480 frames. Per knob value a
fresh instance (a cached graph keeps the launch it was captured with), 2 warm-up calls, 8 timed calls (wall time per call) and 5 calls with stage
timing (descriptor_ms, orientation_ms, total_ms), and the sha1 of four downloaded feature buffers: every setting must give the same bytes.
usage (on the GPU box): python tools/descriptor_sweep.py <value,value,...> [repetitions [out.json]]
VKSIFT_LIB=<variant> selects another build (tools/build_variant.sh <name> features -DDESC_SOLO_PHASES=<n>: the phases of a solo wave)."""
import hashlib, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vulkansift_amd.api as api
W, H, B = 640, 480, 512
vals = [int(v) for v in sys.argv[1].split(",")]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
out = sys.argv[3] if len(sys.argv) > 3 else None  # without it the rows are only printed
dev = torch.device("cuda:0")
ngen = 128
gen = np.stack([api.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(ngen)])
variants = [gen, gen[:, :, ::-1], gen[:, ::-1, :], gen[:, ::-1, ::-1]]
host = np.ascontiguousarray(np.concatenate([variants[(k // ngen) % 4][: min(ngen, B - k)] for k in range(0, B, ngen)]))
d = torch.from_numpy(host).to(dev)
rows = []
for rep in range(reps):
    for v in vals:
        assert api.lib().vksift_hip_tune(14, v) == 0
        inst = api.Instance(api.default_config(sift_buffer_count=B, input_image_max_size=W * H), batch_capacity=B)
        for _ in range(2):
            inst.detectFeaturesBatchDevice(d.data_ptr(), B, W, H, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            inst.detectFeaturesBatchDevice(d.data_ptr(), B, W, H, 0)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / 8 * 1e3
        inst.setProfiling(True)
        for _ in range(5):
            inst.detectFeaturesBatchDevice(d.data_ptr(), B, W, H, 0)
        torch.cuda.synchronize()
        acc = inst.getAccumulatedDetectTimings()
        inst.setProfiling(False)
        n = max(acc["nb_calls"], 1)
        hsh = hashlib.sha1(b"".join(inst.downloadFeatures(b).tobytes() for b in (0, 1, 200, 511))).hexdigest()[:12]
        row = {"rep": rep, "solo_r": v, "wall_ms_per_call": round(wall, 3), "descriptor_ms": round(acc["descriptor_ms"] / n, 3),
               "orientation_ms": round(acc["orientation_ms"] / n, 3), "total_ms": round(acc["total_ms"] / n, 3), "features_sha": hsh}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del inst
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(rows, open(out, "w"), indent=1)
