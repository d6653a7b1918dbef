/*
 * vksift_cameras.c — the motion half of resection-intersection on the device: the per-view index of the observation table
 * (vksift_ext_indexObservationsByView and its accessors) and the refinement of every camera on the points of the last triangulation, the points held
 * fixed (vksift_ext_refineCameras and its accessors). No counterpart in the reference: its callers download the table and the points, invert the table
 * by view on the host and run a Gauss-Newton per view there. Same contract as the stages they follow (vksift_observations.c, vksift_triangulate.c):
 * queued on the instance stream, the tracks' participating buffers busy, the accessors wait; results in storage of their own.
 */
#include "vksift_internal.h"

#define IDX_FN "vksift_ext_indexObservationsByView()"
#define CAM_FN "vksift_ext_refineCameras()"

_Static_assert(sizeof(vksift_ext_ViewObservation) == 16u, "vksift_ext_ViewObservation is the kernel's four-word record");
_Static_assert(sizeof(vksift_ext_ViewStats) == 16u, "vksift_ext_ViewStats is the kernel's four statistics words");
_Static_assert(sizeof(vksift_ext_RefinedCamera) == 72u, "vksift_ext_RefinedCamera is the kernel's eighteen-word record");
_Static_assert(sizeof(vksift_ext_CameraStats) == 16u, "vksift_ext_CameraStats is the kernel's four statistics words");

/* The entries of hip/cameras.hip are weak references here, like those of vksift_observations.c: the simulated device of the host scheduler's tests does
 * not define them. Without a launcher its address is NULL and the call fails like any launch failure (VKSIFT_VULKAN_ERROR through the stage's error
 * exit); in the library they are always there (hip/cameras.hip is linked into it). */
extern __typeof__(vksift_hip_views_scratch_u32) vksift_hip_views_scratch_u32 __attribute__((weak));
extern __typeof__(vksift_hip_index_views) vksift_hip_index_views __attribute__((weak));
extern __typeof__(vksift_hip_refine_cameras) vksift_hip_refine_cameras __attribute__((weak));

/* the observations a table of this instance can hold (ensure_observation_storage) */
static uint64_t obs_cap(const struct vksift_Instance_T *inst) { return (uint64_t)inst->tracks.cap_bufs * inst->cfg.max_nb_sift_per_buffer; }
/* the last selection's own bound on its observations: at most max_rows rows in each of nbufs buffers (never 0 for the launchers) */
static uint64_t obs_bound(const struct vksift_Instance_T *inst)
{
  const uint64_t bound = (uint64_t)inst->tracks.nbufs * inst->tracks.max_rows;
  return bound < obs_cap(inst) ? (bound ? bound : 1u) : obs_cap(inst);
}
/* and on its tracks, as vksift_ext_triangulateTracks hands it over: two members at least */
static uint64_t tracks_bound(const struct vksift_Instance_T *inst)
{
  const uint64_t bound = ((uint64_t)inst->tracks.nbufs * inst->tracks.max_rows) / 2u;
  return bound < obs_cap(inst) / 2u ? (bound ? bound : 1u) : obs_cap(inst) / 2u;
}

/* Allocated by the first index: an entry per possible observation, an offset per SIFT buffer and one more. */
static bool ensure_view_storage(vksift_Instance inst)
{
  ViewResults *v = &inst->views;
  v->scratch_u32 = vksift_hip_views_scratch_u32(obs_cap(inst));
  return mem_ensure(&v->d_offsets, sizeof(uint32_t) * ((size_t)inst->cfg.sift_buffer_count + 1u) + 8u, MEM_DEVICE) &&
         mem_ensure(&v->d_obs, sizeof(vksift_ext_ViewObservation) * obs_cap(inst) + 16u, MEM_DEVICE) && mem_ensure(&v->d_stats, sizeof(uint32_t) * 4u, MEM_DEVICE) &&
         mem_ensure(&v->h_stats, sizeof(uint32_t) * 4u, MEM_PINNED) && mem_ensure(&v->d_scratch, sizeof(uint32_t) * v->scratch_u32 + 8u, MEM_DEVICE);
}

/* the launches of the index, behind whatever the stream holds; the statistics posted */
static int queue_index(vksift_Instance inst)
{
  const ObservationResults *o = &inst->obs;
  ViewResults *v = &inst->views;
  int rc = vksift_hip_index_views(o->d_offsets, o->d_obs, o->d_stats, tracks_bound(inst), obs_bound(inst), inst->cfg.sift_buffer_count, v->d_offsets, v->d_obs,
                                  v->d_stats, v->d_scratch, v->scratch_u32, inst->stream);
  v->valid = false; /* the launches replace the index: not served until the whole sequence has been queued */
  if (rc == 0)
    rc = vksift_hip_post_words(v->h_stats, v->d_stats, 4u, inst->stream);
  return rc;
}

void vksift_ext_indexObservationsByView(vksift_Instance instance)
{
  vksift_Instance inst = instance;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const TrackResults *t = &inst->tracks;
  if (!inst->obs.valid || !t->valid)
  {
    logError(LOG_TAG, IDX_FN " error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!vksift_hip_views_scratch_u32 || !vksift_hip_index_views)
  {
    logError(LOG_TAG, IDX_FN " error: the device layer has no view index launcher.");
    goto gpu_error;
  }
  if (!ensure_view_storage(inst))
  {
    logError(LOG_TAG, IDX_FN " error: out of device memory for the view index.");
    goto gpu_error;
  }
  HIP_CHECK(stage_begin(inst, &frame, T_VIEWS, "View index"), "timer start");
  HIP_CHECK(queue_index(inst), "view indexing");
  HIP_CHECK(stage_end(inst, &frame, t->ids, t->ids, t->nbufs), "event record");
  inst->views.valid = true;
  return;
gpu_error:
  stage_fail(inst, &frame, t->ids, t->ids, t->nbufs);
  logError(LOG_TAG, IDX_FN " error: Failed to start the view indexing.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

/* what every accessor starts with: the pipeline that posts the statistics has run, then the checks */
static bool served(vksift_Instance inst, bool valid, bool args_ok, const char *fn)
{
  wait_match(inst);
  if (valid && args_ok)
    return true;
  logError(LOG_TAG, "%s() error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
  return false;
}

static void fetch(vksift_Instance inst, void *dst, const void *src, size_t bytes, const char *fn)
{
  if (bytes == 0)
    return;
  HIP_CHECK(vksift_hip_memcpy_d2h(dst, src, bytes, inst->dl_stream), "read-back");
  HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "read-back");
  return;
gpu_error:
  logError(LOG_TAG, "%s() error when downloading from GPU memory.", fn);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_ext_getViewStats(vksift_Instance instance, vksift_ext_ViewStats *out)
{
  if (served(instance, instance->views.valid, out != NULL, "vksift_ext_getViewStats"))
    memcpy(out, instance->views.h_stats, sizeof(*out));
}

void vksift_ext_downloadViewOffsets(vksift_Instance instance, uint32_t *view_offsets)
{
  if (served(instance, instance->views.valid, view_offsets != NULL, "vksift_ext_downloadViewOffsets"))
    fetch(instance, view_offsets, instance->views.d_offsets, sizeof(uint32_t) * ((size_t)instance->cfg.sift_buffer_count + 1u), "vksift_ext_downloadViewOffsets");
}

void vksift_ext_downloadViewObservations(vksift_Instance instance, vksift_ext_ViewObservation *obs)
{
  if (served(instance, instance->views.valid, obs != NULL, "vksift_ext_downloadViewObservations"))
    fetch(instance, obs, instance->views.d_obs, sizeof(vksift_ext_ViewObservation) * instance->views.h_stats[1], "vksift_ext_downloadViewObservations");
}

float vksift_ext_getIndexViewsTime(vksift_Instance instance) { return timer_read(instance, T_VIEWS); }

/* Allocated by the first refinement: a record per SIFT buffer, whichever took part. */
static bool ensure_camera_storage(vksift_Instance inst)
{
  CameraResults *c = &inst->cams;
  return mem_ensure(&c->d_refined, sizeof(vksift_ext_RefinedCamera) * inst->cfg.sift_buffer_count + 8u, MEM_DEVICE) &&
         mem_ensure(&c->d_stats, sizeof(uint32_t) * 4u, MEM_DEVICE) && mem_ensure(&c->h_stats, sizeof(uint32_t) * 4u, MEM_PINNED);
}

void vksift_ext_refineCameras(vksift_Instance instance, uint32_t nb_steps)
{
  vksift_Instance inst = instance;
  const TrackResults *t = &inst->tracks;
  CameraResults *c = &inst->cams;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  if (!inst->tri.valid || !inst->obs.valid || !t->valid || nb_steps == 0 || nb_steps > VKSIFT_EXT_CAMERA_MAX_STEPS)
  {
    logError(LOG_TAG, CAM_FN " error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!vksift_hip_views_scratch_u32 || !vksift_hip_index_views || !vksift_hip_refine_cameras)
  {
    logError(LOG_TAG, CAM_FN " error: the device layer has no camera refinement launcher.");
    goto gpu_error;
  }
  if (!ensure_view_storage(inst) || !ensure_camera_storage(inst))
  {
    logError(LOG_TAG, CAM_FN " error: out of device memory for the refined cameras.");
    goto gpu_error;
  }
  HIP_CHECK(stage_begin(inst, &frame, T_CAMERAS, "Camera refinement"), "timer start");
  if (!inst->views.valid) /* the present observation table has no index yet: built in front, and served like one asked for */
    HIP_CHECK(queue_index(inst), "view indexing");
  /* the index, the points and their cameras, and the buffer table of the build, where the earlier stages left them on the device (tracks.d_tab is
   * rewritten by the next build only, tri.d_cameras by the next triangulation only: both invalidate this) */
  HIP_CHECK(vksift_hip_refine_cameras(inst->views.d_offsets, inst->views.d_obs, inst->views.d_stats, obs_bound(inst), inst->tri.d_points, tracks_bound(inst),
                                      inst->tri.d_cameras, inst->cfg.sift_buffer_count, t->d_tab + (size_t)2u * inst->batch_cap, t->nbufs, nb_steps, c->d_refined,
                                      c->d_stats, inst->stream),
            "camera refinement");
  c->valid = false; /* the launch replaces the records: not served until the whole sequence has been queued */
  HIP_CHECK(vksift_hip_post_words(c->h_stats, c->d_stats, 4u, inst->stream), "camera statistics read-back");
  HIP_CHECK(stage_end(inst, &frame, t->ids, t->ids, t->nbufs), "event record");
  inst->views.valid = c->valid = true;
  return;
gpu_error:
  stage_fail(inst, &frame, t->ids, t->ids, t->nbufs);
  logError(LOG_TAG, CAM_FN " error: Failed to start the camera refinement.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_ext_getCameraStats(vksift_Instance instance, vksift_ext_CameraStats *out)
{
  if (served(instance, instance->cams.valid, out != NULL, "vksift_ext_getCameraStats"))
    memcpy(out, instance->cams.h_stats, sizeof(*out));
}

void vksift_ext_downloadRefinedCameras(vksift_Instance instance, vksift_ext_RefinedCamera *cameras)
{
  if (served(instance, instance->cams.valid, cameras != NULL, "vksift_ext_downloadRefinedCameras"))
    fetch(instance, cameras, instance->cams.d_refined, sizeof(vksift_ext_RefinedCamera) * instance->cfg.sift_buffer_count, "vksift_ext_downloadRefinedCameras");
}

float vksift_ext_getRefineCamerasTime(vksift_Instance instance) { return timer_read(instance, T_CAMERAS); }
