"""Time vksift_ext_selectTrackObservations on the multi-view workload of tools/tracks_time.py: B buffers of 640x480 frames — B / 8 synthetic scenes,
each seen by 8 views, about 1.9 k features per view — and P pairs in one filtered matching, tracks from the filtered matches.
  1. the GPU figures: vksift_ext_getObservationsTime (HIP events around the launch sequence and the posting of the statistics) beside
     vksift_ext_getTracksTime, warm-ups then repetitions of build + selection; and the host wall time of the selection with its three downloads
     (statistics, offsets + track ids, observations) through the public API;
  2. the host figure on the same instance: what a caller does without the stage — vksift_ext_downloadFeatureTracks and vksift_downloadFeatures for all B
     buffers, a numpy stable argsort of the words, the filter on the downloaded track records — host wall time, the downloads and the grouping reported
     apart, warm-ups then repetitions; its result is compared with the device's, byte for byte;
  3. the bytes of device memory the stage holds for this configuration, as DESIGN.md states them.
The per-launch split comes from a kernel trace of this tool with --trace-run (one build and selection after the warm-ups and nothing else)."""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from vulkansift_amd import api

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("buffers", nargs="?", type=int, default=64)
ap.add_argument("pairs", nargs="?", type=int, default=512)
ap.add_argument("repeats", nargs="?", type=int, default=20)
ap.add_argument("warmups", nargs="?", type=int, default=3)
ap.add_argument("--trace-run", action="store_true", help="warm-ups, one build and selection, no host path")
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, P, W, H = opt.buffers, opt.pairs, 640, 480
assert B % 8 == 0 and B >= 8
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)
OFFSETS = [(0, 0), (16, 8), (32, 24), (48, 40), (64, 64), (8, 56), (40, 16), (56, 32)]
PARAMS = (2, 0, api.OBS_DROP_CONFLICTING)        # what OpenMVG's TracksBuilder::Filter keeps: at least two members, no conflicting track

frames = []
for s in range(B // 8):
    scene = api.gen_synthetic_image(0x5EED0000 + s, W + 64, H + 64)
    frames += [np.ascontiguousarray(scene[y:y + H, x:x + W]) for x, y in OFFSETS]
pairs = [(8 * s + a, 8 * s + b) for s in range(B // 8) for a, b in itertools.combinations(range(8), 2)]
pairs += [(a, b) for a, b in itertools.combinations(range(B), 2) if a // 8 != b // 8][:max(0, P - len(pairs))]
pairs = pairs[:P]
ids_a, ids_b = [a for a, _ in pairs], [b for _, b in pairs]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def host_observations(inst, min_length, max_length, conflicts):
    """(download ms, grouping ms, offsets, track ids, observations): the path without the stage"""
    t0 = time.perf_counter()
    rec = inst.downloadTracks()
    words = [inst.downloadFeatureTracks(b) for b in range(B)]
    feats = [inst.downloadFeatures(b) for b in range(B)]
    t1 = time.perf_counter()
    keep = rec["length"] >= min_length
    if max_length:
        keep &= rec["length"] <= max_length
    if conflicts == api.OBS_DROP_CONFLICTING:
        keep &= rec["length"] == rec["nb_buffers"]
    ids = np.flatnonzero(keep).astype(np.uint32)
    number = np.full(len(rec) + 1, -1, np.int64)
    number[ids] = np.arange(len(ids))
    word = np.concatenate(words).astype(np.int64)
    new = number[np.minimum(word, len(rec))]                    # NO_TRACK -> the spare entry
    member = np.flatnonzero(new >= 0)
    member = member[np.argsort(new[member], kind="stable")]
    obs = np.zeros(len(member), api.OBSERVATION_DTYPE)
    obs["gpu_buffer_id"] = np.concatenate([np.full(len(w), b, np.uint32) for b, w in enumerate(words)])[member]
    obs["row"] = np.concatenate([np.arange(len(w), dtype=np.uint32) for w in words])[member]
    obs["x"], obs["y"] = np.concatenate([f["x"] for f in feats])[member], np.concatenate([f["y"] for f in feats])[member]
    offsets = np.zeros(len(ids) + 1, np.uint32)
    offsets[1:] = np.cumsum(rec["length"][ids])
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, offsets, ids, obs


cfg = api.default_config(sift_buffer_count=max(B, len(pairs)), gpu_device_index=0, input_image_max_size=W * H)
out = {"buffers": B, "pairs": len(pairs), "repeats": opt.repeats, "params": {"min_length": PARAMS[0], "max_length": PARAMS[1], "conflicts": PARAMS[2]}}
with api.Instance(cfg, batch_capacity=max(B, len(pairs))) as inst:
    inst.setProfiling(True)
    inst.detectFeaturesBatch(frames, 0)
    inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
    rows = {b: inst.getFeaturesNumber(b) for b in range(B)}
    gpu_tracks, gpu_obs, wall = [], [], []
    for it in range(opt.warmups + (1 if opt.trace_run else opt.repeats)):
        inst.buildTracks(api.TRACKS_FILTERED)
        inst.getTrackStats()                                  # (the build has run: the wall time below is the selection's alone)
        t0 = time.perf_counter()
        inst.selectTrackObservations(*PARAMS)
        got = inst.downloadObservationOffsets(), inst.downloadObservationTrackIds(), inst.downloadObservations()
        t1 = time.perf_counter()
        if it >= opt.warmups:
            gpu_tracks.append(inst.getTracksTime()), gpu_obs.append(inst.getObservationsTime()), wall.append((t1 - t0) * 1e3)
    nb, cap = cfg.max_nb_sift_per_buffer, min(2 * max(B, len(pairs)), cfg.sift_buffer_count)
    out.update(rows=int(sum(rows.values())), rows_per_buffer=sum(rows.values()) / B, max_nb_sift_per_buffer=nb, track_stats=inst.getTrackStats(),
               stats=inst.getObservationStats(), gpu_tracks_ms=stats(gpu_tracks), gpu_observations_ms=stats(gpu_obs), select_and_download_wall_ms=stats(wall),
               device_bytes={"scratch": 4 * int(api.lib().vksift_hip_observations_scratch_u32(cap, nb, nb)), "observations": 16 * cap * nb,
                             "offsets_and_track_ids": 8 * (cap * nb // 2) + 4})
    if not opt.trace_run:
        dl, group = [], []
        for it in range(opt.warmups + opt.repeats):
            d, g, offsets, ids, obs = host_observations(inst, *PARAMS)
            if it >= opt.warmups:
                dl.append(d), group.append(g)
        for mine, theirs in zip((offsets, ids, obs), got):
            assert mine.tobytes() == theirs.tobytes()
        out.update(host_download_ms=stats(dl), host_grouping_ms=stats(group), host_total_ms=stats(np.add(dl, group)))

print(json.dumps(out))
if opt.json:
    os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
