/*
 * vksift_triangulate.c — the selected tracks of the last vksift_ext_selectTrackObservations triangulated under caller-supplied cameras
 * (vksift_ext_triangulateTracks and its accessors): one point per selected track, computed where the observation table lies. No counterpart in the
 * reference: its callers download the table and triangulate track by track on the host. Same contract as the selection it follows
 * (vksift_observations.c): queued on the instance stream, the tracks' participating buffers busy, the accessors wait; results in storage of its own.
 */
#include "vksift_internal.h"

#define TRI_FN "vksift_ext_triangulateTracks()"
#define CAMERA_FLOATS 12u

_Static_assert(sizeof(vksift_ext_Point) == 32u, "vksift_ext_Point is the kernel's eight-word record");
_Static_assert(sizeof(vksift_ext_PointStats) == 16u, "vksift_ext_PointStats is the kernel's four statistics words");

/* The entry of hip/triangulate.hip is a weak reference here, like those of vksift_observations.c: the simulated device of the host scheduler's tests does
 * not define it. Without the launcher the address is NULL and the call fails like any launch failure (VKSIFT_VULKAN_ERROR through the stage's error
 * exit); in the library it is always there (hip/triangulate.hip is linked into it). */
extern __typeof__(vksift_hip_triangulate_tracks) vksift_hip_triangulate_tracks __attribute__((weak));

/* the points an observation table of this instance can ask for: one per possible track (ensure_observation_storage) */
static uint64_t points_cap(const struct vksift_Instance_T *inst) { return ((uint64_t)inst->tracks.cap_bufs * inst->cfg.max_nb_sift_per_buffer) / 2u; }

/* Allocated by the first triangulation. A camera per SIFT buffer, whichever took part. */
static bool ensure_point_storage(vksift_Instance inst)
{
  TriangulateResults *p = &inst->tri;
  const size_t cam_bytes = sizeof(float) * CAMERA_FLOATS * inst->cfg.sift_buffer_count;
  const bool ok = mem_ensure(&p->d_points, sizeof(vksift_ext_Point) * points_cap(inst) + 32u, MEM_DEVICE) && mem_ensure(&p->d_stats, sizeof(uint32_t) * 4u, MEM_DEVICE) &&
                  mem_ensure(&p->h_stats, sizeof(uint32_t) * 4u, MEM_PINNED) && mem_ensure(&p->h_cameras, cam_bytes, MEM_PINNED) &&
                  mem_ensure(&p->d_cameras, cam_bytes, MEM_DEVICE);
  if (!inst->ev_ctab)
    inst->ev_ctab = vksift_hip_event_create();
  return ok && inst->ev_ctab;
}

/* the cameras of the buffers that took part in the last build, and no others, are all finite */
static bool cameras_finite(const struct vksift_Instance_T *inst, const float *cameras)
{
  for (uint32_t b = 0; b < inst->cfg.sift_buffer_count; b++)
    if (inst->tracks.rank_of[b] != VKSIFT_EXT_NO_TRACK)
      for (uint32_t k = 0; k < CAMERA_FLOATS; k++)
        if (!isfinite(cameras[(size_t)CAMERA_FLOATS * b + k]))
          return false;
  return true;
}

void vksift_ext_triangulateTracks(vksift_Instance instance, const float *cameras, float threshold_px, float cos_min_angle)
{
  vksift_Instance inst = instance;
  const ObservationResults *o = &inst->obs;
  TriangulateResults *p = &inst->tri;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const TrackResults *t = &inst->tracks;
  const float t2 = threshold_px * threshold_px;
  if (!o->valid || !t->valid || cameras == NULL || !(threshold_px > 0.f) || !isfinite(threshold_px) || !(t2 > 0.f) || !isfinite(t2) ||
      isnan(cos_min_angle) || !cameras_finite(inst, cameras))
  {
    logError(LOG_TAG, TRI_FN " error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!vksift_hip_triangulate_tracks)
  {
    logError(LOG_TAG, TRI_FN " error: the device layer has no triangulation launcher.");
    goto gpu_error;
  }
  if (!ensure_point_storage(inst))
  {
    logError(LOG_TAG, TRI_FN " error: out of device memory for the points.");
    goto gpu_error;
  }
  /* the cameras are copied out of pinned memory on the stream: the previous call's copy must be through with them */
  if (p->cam_pending)
  {
    HIP_CHECK(vksift_hip_event_sync(inst->ev_ctab), "event synchronisation");
    p->cam_pending = false;
  }
  /* the caller's table is copied here, before the call returns: the cameras that are read, zeros for every other buffer */
  for (uint32_t b = 0; b < inst->cfg.sift_buffer_count; b++)
  {
    float *dst = p->h_cameras + (size_t)CAMERA_FLOATS * b;
    if (inst->tracks.rank_of[b] != VKSIFT_EXT_NO_TRACK)
      memcpy(dst, cameras + (size_t)CAMERA_FLOATS * b, sizeof(float) * CAMERA_FLOATS);
    else
      memset(dst, 0, sizeof(float) * CAMERA_FLOATS);
  }
  HIP_CHECK(stage_begin(inst, &frame, T_TRIANGULATE, "Triangulation"), "timer start");
  HIP_CHECK(vksift_hip_memcpy_h2d(p->d_cameras, p->h_cameras, sizeof(float) * CAMERA_FLOATS * inst->cfg.sift_buffer_count, inst->stream), "camera upload");
  HIP_CHECK(vksift_hip_event_record(inst->ev_ctab, inst->stream), "event record");
  p->cam_pending = true;
  /* the table and its counts where the selection left them on the device. The grid is sized by the bound handed over as points_cap: the selection's own bound
   * on its tracks (two members at least, of at most max_rows rows in each of nbufs buffers), which the storage always holds */
  const uint64_t bound = ((uint64_t)inst->tracks.nbufs * inst->tracks.max_rows) / 2u;
  HIP_CHECK(vksift_hip_triangulate_tracks(o->d_offsets, o->d_obs, o->d_stats, p->d_cameras, inst->cfg.sift_buffer_count, t2, cos_min_angle, p->d_points,
                                          bound < points_cap(inst) ? (bound ? bound : 1u) : points_cap(inst), p->d_stats, inst->stream),
            "triangulation");
  p->valid = inst->cams.valid = false; /* the launch replaces the points: not served until the whole sequence has been queued; the cameras refined on the earlier
                                        * points are not served any more (vksift_cameras.c) */
  HIP_CHECK(vksift_hip_post_words(p->h_stats, p->d_stats, 4u, inst->stream), "point statistics read-back");
  HIP_CHECK(stage_end(inst, &frame, t->ids, t->ids, t->nbufs), "event record");
  p->valid = true;
  return;
gpu_error:
  stage_fail(inst, &frame, t->ids, t->ids, t->nbufs);
  logError(LOG_TAG, TRI_FN " error: Failed to start the triangulation.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

/* what every accessor starts with: the pipeline that posts the statistics has run, then the checks */
static bool points_served(vksift_Instance inst, bool args_ok, const char *fn)
{
  wait_match(inst);
  if (inst->tri.valid && args_ok)
    return true;
  logError(LOG_TAG, "%s() error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
  return false;
}

void vksift_ext_getPointStats(vksift_Instance instance, vksift_ext_PointStats *out)
{
  if (points_served(instance, out != NULL, "vksift_ext_getPointStats"))
    memcpy(out, instance->tri.h_stats, sizeof(*out));
}

void vksift_ext_downloadPoints(vksift_Instance instance, vksift_ext_Point *points)
{
  vksift_Instance inst = instance;
  if (!points_served(inst, points != NULL, "vksift_ext_downloadPoints") || inst->tri.h_stats[0] == 0)
    return;
  HIP_CHECK(vksift_hip_memcpy_d2h(points, inst->tri.d_points, sizeof(vksift_ext_Point) * inst->tri.h_stats[0], inst->dl_stream), "point read-back");
  HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "point read-back");
  return;
gpu_error:
  logError(LOG_TAG, "vksift_ext_downloadPoints() error when downloading the points from GPU memory.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

float vksift_ext_getTriangulateTime(vksift_Instance instance) { return timer_read(instance, T_TRIANGULATE); }
