"""Time vksift_ext_buildTracks on a multi-view workload of the benchmark's frame size: B buffers of 640x480 frames — B / 8 synthetic scenes of
704x544 pixels (the benchmark's blob density), each seen by 8 views cropped at 8 offsets, about 1.9 k features per view — and P pairs in one
filtered matching: every pair of views of one scene first (they share features), pairs across scenes behind them (they share none) up to P.
  1. the GPU figure: vksift_ext_getTracksTime (HIP events around the launch sequence and the posting of the statistics) for source FILTERED
     and for REFINED_H, warm-ups then repetitions of each, alternating;
  2. the host figure, once per source: what a caller has today on the same data — vksift_ext_downloadFilteredMatches (and the mask and record
     downloads) for the P pairs, then the union-find of tests/np_tracks.py — host wall time through the public API, same process; the downloads and
     the union-find are reported apart;
  3. the bytes of device memory the stage holds for this configuration, as DESIGN.md states them.
The per-launch split comes from a kernel trace of this tool with --trace-run (one build of each source after the warm-ups and nothing else)."""
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
ap.add_argument("pairs", nargs="?", type=int, default=512)
ap.add_argument("repeats", nargs="?", type=int, default=20)
ap.add_argument("warmups", nargs="?", type=int, default=3)
ap.add_argument("--trace-run", action="store_true", help="warm-ups, one build of each source, no host path")
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, P, W, H = opt.buffers, opt.pairs, 640, 480
assert B % 8 == 0 and B >= 8
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)
OFFSETS = [(0, 0), (16, 8), (32, 24), (48, 40), (64, 64), (8, 56), (40, 16), (56, 32)]

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


def host_tracks(inst, source, rows):
    """(download ms, union-find ms, stats): the path without the stage"""
    t0 = time.perf_counter()
    edges = []
    for k in range(len(pairs)):
        fm = inst.downloadFilteredMatches(k)
        if source == api.TRACKS_REFINED_H:
            edges.append(NT.pair_edges(fm, inst.downloadRefinedInlierMask(k), bool(int(inst.getRefinedHomography(k)["valid"]))))
        else:
            edges.append(NT.pair_edges(fm))
    t1 = time.perf_counter()
    _, _, st = NT.build(rows, [(a, b, e) for (a, b), e in zip(pairs, edges)])
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, st


cfg = api.default_config(sift_buffer_count=max(B, len(pairs)), gpu_device_index=0, input_image_max_size=W * H)
out = {"buffers": B, "pairs": len(pairs), "repeats": opt.repeats}
with api.Instance(cfg, batch_capacity=max(B, len(pairs))) as inst:
    inst.setProfiling(True)
    inst.detectFeaturesBatch(frames, 0)
    inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
    inst.verifyHomography(1024, 2.5, 7)
    inst.refineHomography(3, 2.5)
    rows = {b: inst.getFeaturesNumber(b) for b in range(B)}
    sources = (("filtered", api.TRACKS_FILTERED), ("refined_h", api.TRACKS_REFINED_H))
    ms = {name: [] for name, _ in sources}
    for it in range(opt.warmups + (1 if opt.trace_run else opt.repeats)):
        for name, source in sources:
            inst.buildTracks(source)
            t = inst.getTracksTime()
            if it >= opt.warmups:
                ms[name].append(t)
    nb, cap = cfg.max_nb_sift_per_buffer, min(2 * max(B, len(pairs)), cfg.sift_buffer_count)
    out.update(rows=int(sum(rows.values())), rows_per_buffer=sum(rows.values()) / B, max_nb_sift_per_buffer=nb,
               device_bytes={"scratch": 4 * int(api.lib().vksift_hip_tracks_scratch_u32(cap, nb)), "node_words": 4 * cap * nb, "records": 16 * (cap * nb // 2),
                             "sift_buffers": 164 * nb * cfg.sift_buffer_count})
    for name, source in sources:
        inst.buildTracks(source)
        gpu = inst.getTrackStats()
        entry = {"gpu_ms": stats(ms[name]), "stats": gpu}
        if not opt.trace_run:
            dl, uf, st = host_tracks(inst, source, rows)
            assert st == gpu, (name, st, gpu)
            entry.update(host_download_ms=dl, host_union_find_ms=uf)
        out[name] = entry

print(json.dumps(out))
if opt.json:
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
