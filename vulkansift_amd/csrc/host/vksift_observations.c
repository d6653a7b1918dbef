/*
 * vksift_observations.c — the observation table of the tracks of the last vksift_ext_buildTracks (vksift_ext_selectTrackObservations and its
 * accessors): which tracks a caller keeps, and their members with positions, grouped by track on the device. No counterpart in the reference:
 * its callers download the per-feature words and every feature record of every buffer and group them with a host sort. Same contract as the
 * build it follows (vksift_tracks.c): queued on the instance stream, the tracks' participating buffers busy, the accessors wait; results in storage of its own.
 */
#include "vksift_internal.h"

#define OBS_FN "vksift_ext_selectTrackObservations()"

_Static_assert(sizeof(vksift_ext_Observation) == 16u, "vksift_ext_Observation is the kernel's four-word record");
_Static_assert(sizeof(vksift_ext_ObservationStats) == 16u, "vksift_ext_ObservationStats is the kernel's four statistics words");

/* The two entries of hip/observations.hip are weak references here: the harness of the host scheduler's tests (tests/plan_build.py) links every host
 * file against a simulated device that defines the launchers it knew when it was written, and these two are not among them. Without the launcher the
 * addresses are NULL and the selection fails like any launch failure (VKSIFT_VULKAN_ERROR through the stage's error exit); in the library they are
 * always there (hip/observations.hip is linked into it). */
extern __typeof__(vksift_hip_observations_scratch_u32) vksift_hip_observations_scratch_u32 __attribute__((weak));
extern __typeof__(vksift_hip_track_observations) vksift_hip_track_observations __attribute__((weak));

/* Sized like the tracks (ensure_track_storage): at most cap_bufs buffers of max_nb_sift_per_buffer nodes, every node an observation, two per track
 * at least. Allocated by the first selection. */
static bool ensure_observation_storage(vksift_Instance inst)
{
  ObservationResults *o = &inst->obs;
  const uint32_t nb = inst->cfg.max_nb_sift_per_buffer, cap_bufs = inst->tracks.cap_bufs;
  const uint64_t nodes = (uint64_t)cap_bufs * nb;
  o->scratch_u32 = vksift_hip_observations_scratch_u32(cap_bufs, nb, nb);
  const bool ok = mem_ensure(&o->d_offsets, sizeof(uint32_t) * (nodes / 2u + 1u) + 8u, MEM_DEVICE) &&
                  mem_ensure(&o->d_track_ids, sizeof(uint32_t) * (nodes / 2u) + 8u, MEM_DEVICE) &&
                  mem_ensure(&o->d_obs, sizeof(vksift_ext_Observation) * nodes + 16u, MEM_DEVICE) && mem_ensure(&o->d_stats, sizeof(uint32_t) * 4u, MEM_DEVICE) &&
                  mem_ensure(&o->h_stats, sizeof(uint32_t) * 4u, MEM_PINNED) && mem_ensure(&o->d_scratch, sizeof(uint32_t) * o->scratch_u32 + 8u, MEM_DEVICE) &&
                  mem_ensure(&o->h_tab, sizeof(uint32_t) * ((size_t)VKSIFT_LAYOUT_WORDS + 1u) * cap_bufs, MEM_PINNED);
  if (!inst->ev_otab)
    inst->ev_otab = vksift_hip_event_create();
  return ok && inst->ev_otab;
}

void vksift_ext_selectTrackObservations(vksift_Instance instance, uint32_t min_length, uint32_t max_length, uint32_t conflicts)
{
  vksift_Instance inst = instance;
  const TrackResults *t = &inst->tracks;
  ObservationResults *o = &inst->obs;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const uint32_t nb = inst->cfg.max_nb_sift_per_buffer;
  if (!t->valid || min_length < 2u || (max_length != 0u && max_length < min_length) || conflicts > VKSIFT_EXT_OBS_DROP_CONFLICTING)
  {
    logError(LOG_TAG, OBS_FN " error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!vksift_hip_observations_scratch_u32 || !vksift_hip_track_observations)
  {
    logError(LOG_TAG, OBS_FN " error: the device layer has no observation launcher.");
    goto gpu_error;
  }
  if (!ensure_observation_storage(inst))
  {
    logError(LOG_TAG, OBS_FN " error: out of device memory for the observations.");
    goto gpu_error;
  }
  /* the tables are read by the launches out of pinned memory: the previous selection must be through with them */
  if (o->tab_pending)
  {
    HIP_CHECK(vksift_hip_event_sync(inst->ev_otab), "event synchronisation");
    o->tab_pending = false;
  }
  /* one layout word per rank and the section tables they name, for the participating buffers of the build (the sides of the last pair list, or every
   * buffer an accumulation named) */
  uint32_t *layouts = o->h_tab, *rank_layouts = o->h_tab + (size_t)VKSIFT_LAYOUT_WORDS * t->cap_bufs;
  buffer_layouts(inst, t->ids, t->nbufs, rank_layouts, layouts);
  const uint64_t cap_nodes = (uint64_t)t->cap_bufs * nb;
  HIP_CHECK(stage_begin(inst, &frame, T_OBSERVATIONS, "Track observations"), "timer start");
  /* the tables and counts of the build, where it left them on the device (tracks.d_tab is rewritten by the next build only, which invalidates this) */
  HIP_CHECK(vksift_hip_track_observations(t->d_node_words, t->d_records, t->d_stats, t->d_tab + (size_t)2u * inst->batch_cap, t->nbufs, t->d_rows, nb, t->max_rows,
                                          inst->d_feats, inst->buf_stride, inst->d_found, VKSIFT_MAX_OCTAVES, rank_layouts, layouts, min_length,
                                          max_length, conflicts, o->d_offsets, o->d_track_ids, cap_nodes / 2u, o->d_obs, cap_nodes, o->d_stats, o->d_scratch,
                                          o->scratch_u32, inst->stream),
            "observation building");
  o->valid = inst->tri.valid = inst->views.valid = inst->cams.valid = false; /* the launch replaces the observations: not served until the whole sequence has
                                                                              * been queued; the points of the earlier observations, their view index and the
                                                                              * cameras refined on them are not served any more (vksift_triangulate.c,
                                                                              * vksift_cameras.c) */
  HIP_CHECK(vksift_hip_event_record(inst->ev_otab, inst->stream), "event record");
  o->tab_pending = true;
  HIP_CHECK(vksift_hip_post_words(o->h_stats, o->d_stats, 4u, inst->stream), "observation statistics read-back");
  HIP_CHECK(stage_end(inst, &frame, t->ids, t->ids, t->nbufs), "event record");
  o->valid = true;
  return;
gpu_error:
  stage_fail(inst, &frame, t->ids, t->ids, t->nbufs);
  logError(LOG_TAG, OBS_FN " error: Failed to start the observation building.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

/* what every accessor starts with: the pipeline that posts the statistics has run, then the checks */
static bool observations_served(vksift_Instance inst, bool args_ok, const char *fn)
{
  wait_match(inst);
  if (inst->obs.valid && args_ok)
    return true;
  logError(LOG_TAG, "%s() error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
  return false;
}

static void observations_fetch(vksift_Instance inst, void *dst, const void *src, size_t bytes, const char *fn)
{
  if (bytes == 0)
    return;
  HIP_CHECK(vksift_hip_memcpy_d2h(dst, src, bytes, inst->dl_stream), "observation read-back");
  HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "observation read-back");
  return;
gpu_error:
  logError(LOG_TAG, "%s() error when downloading the observations from GPU memory.", fn);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_ext_getObservationStats(vksift_Instance instance, vksift_ext_ObservationStats *out)
{
  if (observations_served(instance, out != NULL, "vksift_ext_getObservationStats"))
    memcpy(out, instance->obs.h_stats, sizeof(*out));
}

void vksift_ext_downloadObservationOffsets(vksift_Instance instance, uint32_t *offsets)
{
  if (observations_served(instance, offsets != NULL, "vksift_ext_downloadObservationOffsets"))
    observations_fetch(instance, offsets, instance->obs.d_offsets, sizeof(uint32_t) * ((size_t)instance->obs.h_stats[0] + 1u), "vksift_ext_downloadObservationOffsets");
}

void vksift_ext_downloadObservationTrackIds(vksift_Instance instance, uint32_t *track_ids)
{
  if (observations_served(instance, track_ids != NULL, "vksift_ext_downloadObservationTrackIds"))
    observations_fetch(instance, track_ids, instance->obs.d_track_ids, sizeof(uint32_t) * instance->obs.h_stats[0], "vksift_ext_downloadObservationTrackIds");
}

void vksift_ext_downloadObservations(vksift_Instance instance, vksift_ext_Observation *obs)
{
  if (observations_served(instance, obs != NULL, "vksift_ext_downloadObservations"))
    observations_fetch(instance, obs, instance->obs.d_obs, sizeof(vksift_ext_Observation) * instance->obs.h_stats[1], "vksift_ext_downloadObservations");
}

float vksift_ext_getObservationsTime(vksift_Instance instance) { return timer_read(instance, T_OBSERVATIONS); }
