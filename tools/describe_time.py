"""Time vksift_ext_describeKeypointsBatch on the benchmark workload: B frames 640x480, each described at the keypoints its own detection found.
Per repetition, host wall time from the call to the completion of its last buffer (vksift_getFeaturesNumber of buffer B - 1 waits for it), through
the public API, same process, nothing else queued:
  1. vksift_ext_detectFeaturesBatch of the B frames;
  2. vksift_ext_describeKeypointsBatch of the same frames in VKSIFT_EXT_DESCRIBE_ORIENT mode, the distinct (x, y, sigma) of each frame's features;
  3. the same in VKSIFT_EXT_DESCRIBE_GIVEN mode, every feature with its orientation.
Warm-ups, then repetitions; median, minimum and maximum of each, and how many of the detection's records come back byte for byte. Two more
figures say where a difference between 1 and 2 / 3 comes from: the same describe call with empty keypoint lists (upload, scale-space and the
fixed cost of the stages alone), and the host time the binding spends laying the B lists out as one array before the C call.
--detect-only: step 1 alone (a build without the describe entry points: the figure to compare with)."""
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
ap.add_argument("frames", nargs="?", type=int, default=64)
ap.add_argument("repeats", nargs="?", type=int, default=10)
ap.add_argument("warmups", nargs="?", type=int, default=2)
ap.add_argument("--detect-only", action="store_true")
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, W, H = opt.frames, 640, 480
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(inst, call, last):
    t0 = time.perf_counter()
    call()
    inst.getFeaturesNumber(last)
    return (time.perf_counter() - t0) * 1e3


def keypoints_of(f, distinct):
    if distinct:
        key = np.stack([f["x"].view(np.uint32), f["y"].view(np.uint32), f["sigma"].view(np.uint32)], axis=1)
        f = f[np.sort(np.unique(key, axis=0, return_index=True)[1])]
    k = np.zeros(len(f), api.KEYPOINT_DTYPE)
    k["x"], k["y"], k["sigma"], k["orientation"], k["response"] = f["x"], f["y"], f["sigma"], f["orientation"], f["intensity"]
    return k


gen = np.stack([api.gen_synthetic_image(0x5EED0000 + i, W, H) for i in range(min(B, 64))])
frames = list(np.ascontiguousarray(np.concatenate([gen] * ((B + len(gen) - 1) // len(gen)))[:B]))
cfg = api.default_config(sift_buffer_count=2 * B, gpu_device_index=0, input_image_max_size=W * H)
out = {"frames": B, "repeats": opt.repeats, "warmups": opt.warmups}
with api.Instance(cfg, batch_capacity=B) as inst:
    inst.detectFeaturesBatch(frames, 0)
    feats = [inst.downloadFeatures(k) for k in range(B)]
    out["features_per_frame_mean"] = float(np.mean([len(f) for f in feats]))
    det_ms, ori_ms, giv_ms, empty_ms, prep_ms = [], [], [], [], []
    if not opt.detect_only:
        kp_ori, kp_giv = [keypoints_of(f, True) for f in feats], [keypoints_of(f, False) for f in feats]
        out["keypoints_per_frame_mean"] = {"orient": float(np.mean([len(k) for k in kp_ori])), "given": float(np.mean([len(k) for k in kp_giv]))}
    for it in range(opt.warmups + opt.repeats):
        t_det = timed(inst, lambda: inst.detectFeaturesBatch(frames, 0), B - 1)
        if not opt.detect_only:
            t_ori = timed(inst, lambda: inst.describeKeypointsBatch(frames, kp_ori, B, api.DESCRIBE_ORIENT), 2 * B - 1)
            n_ori = [inst.getFeaturesNumber(B + k) for k in range(B)]
            t_empty = timed(inst, lambda: inst.describeKeypointsBatch(frames, [k[:0] for k in kp_giv], B, api.DESCRIBE_GIVEN), 2 * B - 1)
            t_giv = timed(inst, lambda: inst.describeKeypointsBatch(frames, kp_giv, B, api.DESCRIBE_GIVEN), 2 * B - 1)
            t0 = time.perf_counter()
            np.concatenate([np.ascontiguousarray(k, dtype=api.KEYPOINT_DTYPE) for k in kp_giv])
            t_prep = (time.perf_counter() - t0) * 1e3
        if it >= opt.warmups:
            det_ms.append(t_det)
            if not opt.detect_only:
                ori_ms.append(t_ori), giv_ms.append(t_giv), empty_ms.append(t_empty), prep_ms.append(t_prep)
    out["detect_batch_ms"] = stats(det_ms)
    if not opt.detect_only:
        out["describe_orient_ms"], out["describe_given_ms"] = stats(ori_ms), stats(giv_ms)
        out["describe_no_keypoints_ms"], out["binding_list_layout_ms"] = stats(empty_ms), stats(prep_ms)
        back, total = 0, 0
        for k in range(0, B, max(1, B // 16)):
            have = {r.tobytes() for r in np.ascontiguousarray(inst.downloadFeatures(B + k)).view(np.uint8).reshape(-1, 164)}
            back += sum(r.tobytes() in have for r in np.ascontiguousarray(feats[k]).view(np.uint8).reshape(-1, 164))
            total += len(feats[k])
        out["given_records_identical_to_the_detection"] = back / max(total, 1)
        out["orient_features_per_frame_mean"] = float(np.mean(n_ori))
print(json.dumps(out))
if opt.json:
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
