"""Time vksift_ext_indexObservationsByView and vksift_ext_refineCameras on the multi-view workload of tools/triangulate_time.py: B buffers of 640x480
frames — B / 8 synthetic scenes, each seen by 8 views (crops of one image at 8 offsets), about 1.9 k features per view — and P pairs in one filtered
matching, tracks from the filtered matches, the observations of the consistent tracks of at least two members, triangulated under the crops' cameras
(the crop at (x0, y0) is an exact perspective view of the plane Z = 256 under P = [[256, 0, 0, -256 x0], [0, 256, 0, -256 y0], [0, 0, 1, 0]]), each camera
moved by a fixed small translation so that the refinement has something to do.
  1. the GPU figures: vksift_ext_getIndexViewsTime and vksift_ext_getRefineCamerasTime (HIP events around the launches and the posting of the
     statistics), warm-ups then repetitions of triangulation + index + refinement; and the host wall time of each stage with its downloads through the
     public API (the index: statistics, offsets, records; the refinement: statistics, records);
  2. the host route this replaces, on the same instance: the downloads of the observation table (offsets, observations) and of the points, a numpy
     inversion of the table by view (stable argsort) and a float64 Gauss-Newton per view (tests/np_cameras.py's estimator, up to NB_STEPS steps), host
     wall time, the three parts reported apart; the final costs of the two routes are compared per view;
  3. the bytes that leave the device on either route."""
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

import np_cameras as NC
from vulkansift_amd import api

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("buffers", nargs="?", type=int, default=64)
ap.add_argument("pairs", nargs="?", type=int, default=512)
ap.add_argument("repeats", nargs="?", type=int, default=20)
ap.add_argument("warmups", nargs="?", type=int, default=3)
ap.add_argument("--host-repeats", type=int, default=3)
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, P, W, H = opt.buffers, opt.pairs, 640, 480
assert B % 8 == 0 and B >= 8
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)
OFFSETS = [(0, 0), (16, 8), (32, 24), (48, 40), (64, 64), (8, 56), (40, 16), (56, 32)]
PARAMS = (2, 0, api.OBS_DROP_CONFLICTING)
THRESHOLD_PX, COS_MIN_ANGLE, NB_STEPS = 2.0, 1.0, 4

frames = []
for s in range(B // 8):
    scene = api.gen_synthetic_image(0x5EED0000 + s, W + 64, H + 64)
    frames += [np.ascontiguousarray(scene[y:y + H, x:x + W]) for x, y in OFFSETS]
pairs = [(8 * s + a, 8 * s + b) for s in range(B // 8) for a, b in itertools.combinations(range(8), 2)]
pairs += [(a, b) for a, b in itertools.combinations(range(B), 2) if a // 8 != b // 8][:max(0, P - len(pairs))]
pairs = pairs[:P]
ids_a, ids_b = [a for a, _ in pairs], [b for _, b in pairs]
NBUF = max(B, len(pairs))
cameras = np.zeros((NBUF, 3, 4), np.float32)
for b in range(B):
    x0, y0 = OFFSETS[b % 8]
    dx, dy = 0.25 * ((b % 5) - 2), 0.125 * ((b % 3) - 1)        # the camera's centre moved by up to half a pixel at the scene's depth
    cameras[b] = [[256, 0, 0, -256 * (x0 + dx)], [0, 256, 0, -256 * (y0 + dy)], [0, 0, 1, 0]]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def host_refinement(inst):
    """(download ms, inversion ms, Gauss-Newton ms, final cost per buffer): the route without the stages"""
    t0 = time.perf_counter()
    offsets, obs, pts = inst.downloadObservationOffsets(), inst.downloadObservations(), inst.downloadPoints()
    t1 = time.perf_counter()
    point = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.argsort(obs["gpu_buffer_id"], kind="stable")
    bounds = np.searchsorted(obs["gpu_buffer_id"][order], np.arange(B + 1))
    t2 = time.perf_counter()
    cost = np.zeros(B)
    for b in range(B):
        sel = order[bounds[b]:bounds[b + 1]]
        sel = sel[pts["status"][point[sel]] == 0]
        if len(sel) >= NC.MIN_OBSERVATIONS:
            cost[b] = NC.refine_f64(cameras[b], pts["X"][point[sel]], np.stack([obs["x"][sel], obs["y"][sel]], axis=1), NB_STEPS)[1]
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3, cost


cfg = api.default_config(sift_buffer_count=NBUF, gpu_device_index=0, input_image_max_size=W * H)
out = {"buffers": B, "pairs": len(pairs), "repeats": opt.repeats, "warmups": opt.warmups,
       "params": {"min_length": PARAMS[0], "max_length": PARAMS[1], "conflicts": PARAMS[2]}, "threshold_px": THRESHOLD_PX, "nb_steps": NB_STEPS}
with api.Instance(cfg, batch_capacity=NBUF) as inst:
    inst.setProfiling(True)
    inst.detectFeaturesBatch(frames, 0)
    inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
    inst.buildTracks(api.TRACKS_FILTERED)
    inst.selectTrackObservations(*PARAMS)
    gpu_index, gpu_refine, gpu_tri, wall_index, wall_refine = [], [], [], [], []
    for it in range(opt.warmups + opt.repeats):
        inst.triangulateTracks(cameras, THRESHOLD_PX, COS_MIN_ANGLE)
        inst.getPointStats()                                  # (the triangulation has run: the wall times below are the new stages' alone)
        t0 = time.perf_counter()
        inst.indexObservationsByView()
        view_offsets, view_obs = inst.downloadViewOffsets(), inst.downloadViewObservations()
        t1 = time.perf_counter()
        inst.refineCameras(NB_STEPS)
        rec = inst.downloadRefinedCameras()
        t2 = time.perf_counter()
        if it >= opt.warmups:
            gpu_index.append(inst.getIndexViewsTime()), gpu_refine.append(inst.getRefineCamerasTime()), gpu_tri.append(inst.getTriangulateTime())
            wall_index.append((t1 - t0) * 1e3), wall_refine.append((t2 - t1) * 1e3)
    ostats, pstats, vstats, cstats = inst.getObservationStats(), inst.getPointStats(), inst.getViewStats(), inst.getCameraStats()
    live = rec["status"][:B] == 0
    out.update(observation_stats=ostats, point_stats=pstats, view_stats=vstats, camera_stats=cstats, gpu_index_ms=stats(gpu_index), gpu_refine_ms=stats(gpu_refine),
               gpu_triangulate_ms=stats(gpu_tri), index_and_downloads_wall_ms=stats(wall_index), refine_and_download_wall_ms=stats(wall_refine),
               steps_histogram=np.bincount(rec["steps"][:B][live], minlength=NB_STEPS + 1).tolist(),
               used_observations={"median": float(np.median(rec["nb_observations"][:B])), "max": int(rec["nb_observations"][:B].max())},
               cost_start_sum=float(rec["cost_start"][:B].astype(np.float64).sum()), cost_sum=float(rec["cost"][:B].astype(np.float64).sum()),
               bytes_off_device={"refined_cameras": 72 * NBUF + 16, "view_index": 16 * vstats["nb_observations"] + 4 * (NBUF + 1) + 16,
                                 "host_route": 16 * ostats["nb_observations"] + 4 * (ostats["nb_tracks"] + 1) + 32 * pstats["nb_points"] + 32})
    dl, inv, gn = [], [], []
    for it in range(1 + opt.host_repeats):
        d, i, g, cost = host_refinement(inst)
        if it >= 1:
            dl.append(d), inv.append(i), gn.append(g)
    rel = np.abs(rec["cost"][:B][live].astype(np.float64) - cost[live]) / np.maximum(cost[live], 1e-12)
    out.update(host_download_ms=stats(dl), host_inversion_ms=stats(inv), host_gauss_newton_ms=stats(gn), host_total_ms=stats(np.add(np.add(dl, inv), gn)),
               host_repeats=opt.host_repeats, worst_relative_cost_difference_to_host=float(rel.max()) if live.any() else None)

print(json.dumps(out))
if opt.json:
    os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
