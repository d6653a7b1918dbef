"""Time tracks across matching calls on the multi-view workload of tools/tracks_time.py: B buffers of 640x480 frames (B / 8 synthetic scenes, each seen by 8
views, about 1.9 k features per view) and ALL B (B - 1) / 2 pairs, matched in calls of P pairs — the pairs of views of one scene first, so that the first call
is the pair list tools/tracks_time.py times.
  1. the GPU figures (HIP events, warm-ups then repetitions): vksift_ext_getAccumulateTime of each call's accumulate and vksift_ext_getTracksTime of the
     accumulated build over all calls; and for the first call alone, on one matching and alternating: vksift_ext_buildTracks (what the parent commit has for
     these P pairs) against one accumulate + the accumulated build;
  2. the host figure, once: what a caller has without the store — after every call vksift_ext_downloadFilteredMatches for its pairs (and, for source
     verified_h, the masks and records), then ONE union-find of tests/np_tracks.py over everything — host wall time through the public API, same process; the
     downloads and the union-find are reported apart, and the union-find's statistics must equal the accumulated build's;
  3. the bytes of device memory the store holds.
The per-launch split comes from a kernel trace of this tool with --trace-run (the warm-ups, one repetition, no host path), a run of its own."""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import np_tracks as NT
from vulkansift_amd import api

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("buffers", nargs="?", type=int, default=64)
ap.add_argument("pairs_per_call", nargs="?", type=int, default=512)
ap.add_argument("repeats", nargs="?", type=int, default=20)
ap.add_argument("warmups", nargs="?", type=int, default=3)
ap.add_argument("--source", choices=("filtered", "verified_h"), default="filtered")
ap.add_argument("--max-edges", type=int, default=1 << 22)
ap.add_argument("--trace-run", action="store_true", help="warm-ups, one repetition, no host path")
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, P, W, H = opt.buffers, opt.pairs_per_call, 640, 480
assert B % 8 == 0 and B >= 8
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)
OFFSETS = [(0, 0), (16, 8), (32, 24), (48, 40), (64, 64), (8, 56), (40, 16), (56, 32)]
SOURCE = {"filtered": api.TRACKS_FILTERED, "verified_h": api.TRACKS_VERIFIED_H}[opt.source]

frames = []
for s in range(B // 8):
    scene = api.gen_synthetic_image(0x5EED0000 + s, W + 64, H + 64)
    frames += [np.ascontiguousarray(scene[y:y + H, x:x + W]) for x, y in OFFSETS]
pairs = [(8 * s + a, 8 * s + b) for s in range(B // 8) for a, b in itertools.combinations(range(8), 2)]
pairs += [(a, b) for a, b in itertools.combinations(range(B), 2) if a // 8 != b // 8]
calls = [pairs[i:i + P] for i in range(0, len(pairs), P)]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def match(inst, call):
    inst.matchFeaturesFiltered([a for a, _ in call], [b for _, b in call], 0.8, True)
    if SOURCE == api.TRACKS_VERIFIED_H:
        inst.verifyHomography(1024, 2.5, 7)


def download(inst, call):
    """the edges of the present matching on the host: the route without the store"""
    out = []
    for k, (a, b) in enumerate(call):
        fm = inst.downloadFilteredMatches(k)
        if SOURCE == api.TRACKS_VERIFIED_H:
            out.append((a, b, NT.pair_edges(fm, inst.downloadInlierMask(k), bool(int(inst.getHomography(k)["valid"])))))
        else:
            out.append((a, b, NT.pair_edges(fm)))
    return out


cfg = api.default_config(sift_buffer_count=max(B, P), gpu_device_index=0, input_image_max_size=W * H)
out = {"buffers": B, "pairs": len(pairs), "pairs_per_call": P, "calls": len(calls), "source": opt.source, "repeats": opt.repeats, "max_edges": opt.max_edges}
with api.Instance(cfg, batch_capacity=max(B, P)) as inst:
    inst.setProfiling(True)
    inst.detectFeaturesBatch(frames, 0)
    rows = {b: inst.getFeaturesNumber(b) for b in range(B)}
    reps = opt.warmups + (1 if opt.trace_run else opt.repeats)
    acc_ms, build_ms = [[] for _ in calls], []
    for it in range(reps):
        inst.beginTrackAccumulation(opt.max_edges)
        for k, call in enumerate(calls):
            match(inst, call)
            inst.accumulateTrackEdges(SOURCE)
            t = inst.getAccumulateTime()
            if it >= opt.warmups:
                acc_ms[k].append(t)
        inst.buildTracksAccumulated()
        t = inst.getTracksTime()
        if it >= opt.warmups:
            build_ms.append(t)
    all_stats, edge_stats = inst.getTrackStats(), inst.getTrackEdgeStats()
    out.update(rows=int(sum(rows.values())), rows_per_buffer=sum(rows.values()) / B, accumulate_ms=[stats(v) for v in acc_ms], accumulated_build_ms=stats(build_ms),
               stats=all_stats, edge_stats=edge_stats, device_bytes={"edges": 16 * opt.max_edges, "row_table": 4 * cfg.sift_buffer_count,
                                                                     "append_scratch": 4 * int(api.lib().vksift_hip_track_edges_scratch_u32(max(B, P), cfg.max_nb_sift_per_buffer))})
    # the first call alone, both ways on one matching
    match(inst, calls[0])
    plain, one_acc, one_build = [], [], []
    for it in range(reps):
        inst.buildTracks(SOURCE)
        t_plain = inst.getTracksTime()
        plain_stats = inst.getTrackStats()
        inst.beginTrackAccumulation(opt.max_edges)
        inst.accumulateTrackEdges(SOURCE)
        inst.buildTracksAccumulated()
        t_acc, t_build = inst.getAccumulateTime(), inst.getTracksTime()
        assert inst.getTrackStats() == plain_stats
        if it >= opt.warmups:
            plain.append(t_plain), one_acc.append(t_acc), one_build.append(t_build)
    out["one_call"] = {"pairs": len(calls[0]), "plain_build_ms": stats(plain), "accumulate_ms": stats(one_acc), "accumulated_build_ms": stats(one_build),
                       "accumulate_plus_build_ms": stats(np.add(one_acc, one_build)), "stats": plain_stats}
    if not opt.trace_run:
        dl, edges = [], []
        for call in calls:
            match(inst, call)
            inst.downloadFilteredMatches(0)      # the matching has run: only the downloads are timed
            t0 = time.perf_counter()
            edges += download(inst, call)
            dl.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        _, _, st = NT.build(rows, edges)
        out.update(host_download_ms=dl, host_union_find_ms=(time.perf_counter() - t0) * 1e3)
        assert st == all_stats, (st, all_stats)

print(json.dumps(out))
if opt.json:
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
