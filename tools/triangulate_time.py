"""Time vksift_ext_triangulateTracks on the multi-view workload of tools/observations_time.py: B buffers of 640x480 frames — B / 8 synthetic scenes,
each seen by 8 views (crops of one image at 8 offsets), about 1.9 k features per view — and P pairs in one filtered matching, tracks from the filtered
matches, the observations of the consistent tracks of at least two members. The crop at (x0, y0) is an exact perspective view of the plane Z = 256 under
P = [[256, 0, 0, -256 x0], [0, 256, 0, -256 y0], [0, 0, 1, 0]]: those are the cameras.
  1. the GPU figures: vksift_ext_getTriangulateTime (HIP events around the camera upload, the launches and the posting of the statistics) beside
     vksift_ext_getObservationsTime of the same runs, warm-ups then repetitions of selection + triangulation; and the host wall time of the triangulation
     with its two downloads (statistics, points) through the public API;
  2. the host route this replaces, on the same instance: the three observation downloads (offsets, track ids, observations) and a float64 numpy DLT per
     track (the SVD of the 2n x 4 system of unit rows), host wall time, the downloads and the loop reported apart; the two sets of points are compared
     (median over the accepted points of the distance between the device's point and the host's; with baselines of a few pixels the linear solution and
     the reprojection minimum differ mostly in depth);
  3. the bytes that leave the device on either route.
The per-launch split comes from a kernel trace of this tool with --trace-run (one selection and triangulation after the warm-ups and nothing else)."""
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
ap.add_argument("--host-repeats", type=int, default=3)
ap.add_argument("--trace-run", action="store_true", help="warm-ups, one selection and triangulation, no host route")
ap.add_argument("--json", metavar="OUT")
opt = ap.parse_args()
B, P, W, H = opt.buffers, opt.pairs, 640, 480
assert B % 8 == 0 and B >= 8
api.lib().vksift_setLogLevel(api.VKSIFT_LOG_ERROR)
OFFSETS = [(0, 0), (16, 8), (32, 24), (48, 40), (64, 64), (8, 56), (40, 16), (56, 32)]
PARAMS = (2, 0, api.OBS_DROP_CONFLICTING)
THRESHOLD_PX, COS_MIN_ANGLE = 1.0, 1.0

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
    cameras[b] = [[256, 0, 0, -256 * x0], [0, 256, 0, -256 * y0], [0, 0, 1, 0]]


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def host_triangulation(inst):
    """(download ms, loop ms, points float64 [tracks, 3]): the route without the stage"""
    t0 = time.perf_counter()
    offsets, _, obs = inst.downloadObservationOffsets(), inst.downloadObservationTrackIds(), inst.downloadObservations()
    t1 = time.perf_counter()
    Pd = cameras.astype(np.float64)
    X = np.zeros((len(offsets) - 1, 3))
    for m in range(len(offsets) - 1):
        o = obs[offsets[m]:offsets[m + 1]]
        Pm = Pd[o["gpu_buffer_id"]]
        A = np.concatenate([o["x"].astype(np.float64)[:, None] * Pm[:, 2] - Pm[:, 0], o["y"].astype(np.float64)[:, None] * Pm[:, 2] - Pm[:, 1]])
        A /= np.linalg.norm(A[:, :3], axis=1, keepdims=True)
        h = np.linalg.svd(A)[2][-1]
        X[m] = h[:3] / h[3]
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, X


cfg = api.default_config(sift_buffer_count=NBUF, gpu_device_index=0, input_image_max_size=W * H)
out = {"buffers": B, "pairs": len(pairs), "repeats": opt.repeats, "params": {"min_length": PARAMS[0], "max_length": PARAMS[1], "conflicts": PARAMS[2]},
       "threshold_px": THRESHOLD_PX, "cos_min_angle": COS_MIN_ANGLE}
with api.Instance(cfg, batch_capacity=NBUF) as inst:
    inst.setProfiling(True)
    inst.detectFeaturesBatch(frames, 0)
    inst.matchFeaturesFiltered(ids_a, ids_b, 0.8, True)
    inst.buildTracks(api.TRACKS_FILTERED)
    gpu_obs, gpu_tri, wall = [], [], []
    for it in range(opt.warmups + (1 if opt.trace_run else opt.repeats)):
        inst.selectTrackObservations(*PARAMS)
        inst.getObservationStats()                            # (the selection has run: the wall time below is the triangulation's alone)
        t0 = time.perf_counter()
        inst.triangulateTracks(cameras, THRESHOLD_PX, COS_MIN_ANGLE)
        pts = inst.downloadPoints()
        t1 = time.perf_counter()
        if it >= opt.warmups:
            gpu_obs.append(inst.getObservationsTime()), gpu_tri.append(inst.getTriangulateTime()), wall.append((t1 - t0) * 1e3)
    ostats, pstats = inst.getObservationStats(), inst.getPointStats()
    ok = pts["status"] == 0
    out.update(track_stats=inst.getTrackStats(), observation_stats=ostats, point_stats=pstats, gpu_observations_ms=stats(gpu_obs), gpu_triangulate_ms=stats(gpu_tri),
               triangulate_and_download_wall_ms=stats(wall), steps_histogram=np.bincount(pts["steps"][ok], minlength=3).tolist(),
               median_z_accepted=float(np.median(pts["X"][ok][:, 2])) if ok.any() else None,
               worst_error_px_accepted=float(np.sqrt(pts["max_sq_error"][ok].max())) if ok.any() else None,
               bytes_off_device={"points": 32 * pstats["nb_points"] + 16, "observation_table": 16 * ostats["nb_observations"] + 8 * ostats["nb_tracks"] + 4 + 16})
    if not opt.trace_run:
        dl, loop = [], []
        for it in range(1 + opt.host_repeats):
            d, g, X = host_triangulation(inst)
            if it >= 1:
                dl.append(d), loop.append(g)
        out.update(host_download_ms=stats(dl), host_dlt_loop_ms=stats(loop), host_total_ms=stats(np.add(dl, loop)), host_repeats=opt.host_repeats,
                   median_distance_to_host_dlt=float(np.median(np.abs(pts["X"][ok].astype(np.float64) - X[ok]).max(axis=1))) if ok.any() else None)

print(json.dumps(out))
if opt.json:
    os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
    with open(opt.json, "w") as f:
        json.dump(out, f, indent=1)
