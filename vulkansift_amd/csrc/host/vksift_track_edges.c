/*
 * vksift_track_edges.c — tracks across matching calls: the device-resident edge store (vksift_ext_beginTrackAccumulation, vksift_ext_accumulateTrackEdges
 * and its accessors) and the build that turns it into the instance's tracks (vksift_ext_buildTracksAccumulated). No counterpart in the reference: its
 * callers keep the matches of every call on the host and run a union-find there. Same contract as the build of one matching (vksift_tracks.c): queued on
 * the instance stream, the accessors wait; results in storage of its own, which no matching and no build clears — only the next begin.
 */
#include "vksift_internal.h"

#define BEGIN_FN "vksift_ext_beginTrackAccumulation()"
#define ACC_FN "vksift_ext_accumulateTrackEdges()"
#define BUILD_FN "vksift_ext_buildTracksAccumulated()"
#define ROW_UNSET 0xFFu /* the byte the row table is filled with: a word of it is 0xFFFFFFFF until a call records a count */

_Static_assert(sizeof(vksift_ext_TrackEdge) == 16u, "vksift_ext_TrackEdge is the kernel's four-word record");
_Static_assert(sizeof(vksift_ext_TrackEdgeStats) == 16u, "vksift_ext_TrackEdgeStats is the kernel's four statistics words");

/* The entries of hip/track_edges.hip are weak references here, like those of vksift_cameras.c: the simulated device of the host scheduler's tests does not
 * define them. Without a launcher its address is NULL and the call fails like any launch failure (VKSIFT_VULKAN_ERROR through the stage's error exit); in
 * the library they are always there (hip/track_edges.hip is linked into it). */
extern __typeof__(vksift_hip_track_edges_scratch_u32) vksift_hip_track_edges_scratch_u32 __attribute__((weak));
extern __typeof__(vksift_hip_append_track_edges) vksift_hip_append_track_edges __attribute__((weak));
extern __typeof__(vksift_hip_build_tracks_from_edges) vksift_hip_build_tracks_from_edges __attribute__((weak));

static void refuse(vksift_Instance inst, const char *fn)
{
  logError(LOG_TAG, "%s error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
}

/* An accumulation can involve every SIFT buffer, and mem_ensure never grows a block: the storage of the tracks and of what is computed from them, if it was
 * allocated for min(2 batch_cap, sift_buffer_count) buffers and that is fewer than sift_buffer_count, is released here (the caller has drained the
 * streams) and allocated again, for sift_buffer_count, by whoever needs it next. */
static void size_for_all_buffers(vksift_Instance inst)
{
  TrackResults *t = &inst->tracks;
  if (t->all_bufs)
    return;
  t->all_bufs = true;
  if (2u * inst->batch_cap >= inst->cfg.sift_buffer_count)
    return;
  tracks_invalidate(inst);
  t->tab_pending = inst->obs.tab_pending = false;
  void *const device[] = {&t->d_node_words, &t->d_records, &t->d_scratch, &t->d_tab, &inst->obs.d_offsets, &inst->obs.d_track_ids, &inst->obs.d_obs, &inst->obs.d_scratch,
                          &inst->tri.d_points, &inst->views.d_obs, &inst->views.d_scratch};
  for (size_t i = 0; i < sizeof(device) / sizeof(device[0]); i++)
    mem_release(device[i], MEM_DEVICE);
  mem_release(&t->h_tab, MEM_PINNED);
  mem_release(&inst->obs.h_tab, MEM_PINNED);
  mem_release(&t->count_word, MEM_HEAP);
  mem_release(&t->ids, MEM_HEAP);
}

void vksift_ext_beginTrackAccumulation(vksift_Instance instance, uint32_t max_edges)
{
  vksift_Instance inst = instance;
  EdgeStore *e = &inst->edges;
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  if (max_edges == 0)
  {
    refuse(inst, BEGIN_FN);
    return;
  }
  /* nothing of the instance is in flight from here on: the store's blocks may be replaced, its pinned words written */
  HIP_CHECK(wait_all(inst), "synchronisation");
  e->begun = false, e->tab_pending = false;
  size_for_all_buffers(inst);
  const uint32_t bc = inst->batch_cap, sbc = inst->cfg.sift_buffer_count;
  if (e->max_edges != max_edges)
    mem_release(&e->d_edges, MEM_DEVICE);
  e->max_edges = max_edges;
  const size_t tab_words = 2u * ((size_t)bc + sbc);
  if (!inst->ev_etab)
    inst->ev_etab = vksift_hip_event_create();
  if (!inst->ev_etab || !mem_ensure(&e->d_edges, sizeof(vksift_ext_TrackEdge) * (size_t)max_edges + 16u, MEM_DEVICE) ||
      !mem_ensure(&e->d_stats, sizeof(uint32_t) * 4u, MEM_DEVICE) || !mem_ensure(&e->h_stats, sizeof(uint32_t) * 4u, MEM_PINNED) ||
      !mem_ensure(&e->d_rows, sizeof(uint32_t) * sbc, MEM_DEVICE) || !mem_ensure(&e->h_tab, sizeof(uint32_t) * tab_words, MEM_PINNED) ||
      !mem_ensure(&e->d_tab, sizeof(uint32_t) * tab_words, MEM_DEVICE) || !mem_ensure(&e->rank_of, sizeof(uint32_t) * sbc, MEM_HEAP) ||
      !mem_ensure(&e->named, sizeof(bool) * sbc, MEM_HEAP))
  {
    logError(LOG_TAG, BEGIN_FN " error: out of memory for the edge store.");
    goto gpu_error;
  }
  HIP_CHECK(vksift_hip_memset(e->d_stats, 0, sizeof(uint32_t) * 4u, inst->stream), "statistics reset");
  HIP_CHECK(vksift_hip_memset(e->d_rows, ROW_UNSET, sizeof(uint32_t) * sbc, inst->stream), "row table reset");
  memset(e->h_stats, 0, sizeof(uint32_t) * 4u);
  memset(e->named, 0, sizeof(bool) * sbc);
  e->max_rows = 1, e->nb_calls = 0;
  e->failed = false, e->begun = true;
  return;
gpu_error:
  e->failed = true;
  logError(LOG_TAG, BEGIN_FN " error: Failed to begin the accumulation.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

/* the store takes calls: begun, and no call on it has failed since */
static bool store_open(const struct vksift_Instance_T *inst) { return inst->edges.begun && !inst->edges.failed; }

void vksift_ext_accumulateTrackEdges(vksift_Instance instance, uint32_t source)
{
  vksift_Instance inst = instance;
  EdgeStore *e = &inst->edges;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const uint32_t count = inst->res[PR_FILTERED].slots_used, nb = inst->cfg.max_nb_sift_per_buffer, sbc = inst->cfg.sift_buffer_count;
  const PairResults *rec, *sel;
  const bool valid = store_open(inst) && track_source(inst, source, &rec, &sel);
  if (!valid)
  {
    refuse(inst, ACC_FN);
    return;
  }
  if (!vksift_hip_track_edges_scratch_u32 || !vksift_hip_append_track_edges)
  {
    logError(LOG_TAG, ACC_FN " error: the device layer has no edge store launcher.");
    goto gpu_error;
  }
  e->scratch_u32 = vksift_hip_track_edges_scratch_u32(inst->batch_cap, nb);
  if (!mem_ensure(&e->d_scratch, sizeof(uint32_t) * e->scratch_u32 + 8u, MEM_DEVICE))
  {
    logError(LOG_TAG, ACC_FN " error: out of device memory for the edge store.");
    goto gpu_error;
  }
  /* the tables are copied out of pinned memory on the stream: the previous call's copy must be through with them */
  if (e->tab_pending)
  {
    HIP_CHECK(vksift_hip_event_sync(inst->ev_etab), "event synchronisation");
    e->tab_pending = false;
  }
  /* the tables of a plain build of this pair list: the launches take the edges that build would take */
  const size_t buf_tab_at = (size_t)2u * inst->batch_cap;
  uint32_t rows;
  const uint32_t nbufs = pair_list_ranks(inst, count, e->rank_of, e->h_tab, e->h_tab + buf_tab_at, NULL, NULL, &rows);
  const uint32_t max_rows = rows < nb ? rows : nb;
  HIP_CHECK(stage_begin(inst, &frame, T_ACCUMULATE, "Track edge accumulation"), "timer start");
  HIP_CHECK(vksift_hip_memcpy_h2d(e->d_tab, e->h_tab, sizeof(uint32_t) * (buf_tab_at + 2u * nbufs), inst->stream), "table upload");
  HIP_CHECK(vksift_hip_event_record(inst->ev_etab, inst->stream), "event record");
  e->tab_pending = true;
  HIP_CHECK(vksift_hip_append_track_edges(rec->d_payload, rec->stride, rec->d_words, rec->words, max_rows, sel ? sel->d_payload : NULL, sel ? sel->stride : 0,
                                          sel ? sel->d_words + sel->words - 1u : NULL, sel ? sel->words : 0, e->d_tab, 2u, count, e->d_tab + buf_tab_at, nbufs,
                                          inst->d_match_n, max_rows, e->d_rows, sbc, e->d_edges, e->max_edges, e->d_stats, e->d_scratch, e->scratch_u32, inst->stream),
            "edge accumulation");
  e->failed = true; /* the launches change the store: not served until the whole sequence has been queued */
  HIP_CHECK(vksift_hip_post_words(e->h_stats, e->d_stats, 4u, inst->stream), "edge statistics read-back");
  HIP_CHECK(stage_end(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count), "event record");
  for (uint32_t r = 0; r < nbufs; r++)
    e->named[e->h_tab[buf_tab_at + 2u * r]] = true;
  e->max_rows = max_rows > e->max_rows ? max_rows : e->max_rows;
  e->nb_calls++;
  e->failed = false;
  return;
gpu_error:
  e->failed = true;
  stage_fail(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count);
  logError(LOG_TAG, ACC_FN " error: Failed to start the edge accumulation.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_ext_buildTracksAccumulated(vksift_Instance instance)
{
  vksift_Instance inst = instance;
  EdgeStore *e = &inst->edges;
  TrackResults *t = &inst->tracks;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const uint32_t nb = inst->cfg.max_nb_sift_per_buffer, sbc = inst->cfg.sift_buffer_count;
  uint32_t nbufs = 0;
  if (!store_open(inst) || e->nb_calls == 0)
  {
    refuse(inst, BUILD_FN);
    return;
  }
  if (!vksift_hip_build_tracks_from_edges)
  {
    logError(LOG_TAG, BUILD_FN " error: the device layer has no edge store launcher.");
    goto gpu_error;
  }
  if (!track_storage_ensure(inst) || !mem_ensure(&t->d_rows_acc, sizeof(uint32_t) * sbc, MEM_DEVICE) || !mem_ensure(&t->h_rows_acc, sizeof(uint32_t) * sbc, MEM_PINNED))
  {
    logError(LOG_TAG, BUILD_FN " error: out of device memory for the tracks.");
    goto gpu_error;
  }
  if (t->tab_pending)
  {
    HIP_CHECK(vksift_hip_event_sync(inst->ev_ttab), "event synchronisation");
    t->tab_pending = false;
  }
  /* ranks: every buffer a call of the store named, in increasing gpu_buffer_id. A buffer's row count is its word of the row table, which the build copies:
   * the tracks do not depend on the store afterwards */
  const size_t buf_tab_at = (size_t)2u * inst->batch_cap, rank_tab_at = buf_tab_at + 2u * t->cap_bufs;
  uint32_t *buf_tab = t->h_tab + buf_tab_at, *rank_tab = t->h_tab + rank_tab_at;
  for (uint32_t b = 0; b < sbc; b++)
  {
    t->rank_of[b] = rank_tab[b] = e->named[b] ? nbufs : VKSIFT_EXT_NO_TRACK;
    if (e->named[b])
      buf_tab[2u * nbufs] = t->ids[nbufs] = b, buf_tab[2u * nbufs + 1u] = t->count_word[nbufs] = b, nbufs++;
  }
  t->nbufs = nbufs;
  t->d_rows = t->d_rows_acc, t->h_rows = t->h_rows_acc;
  HIP_CHECK(stage_begin(inst, &frame, T_TRACKS, "Tracks (accumulated)"), "timer start");
  HIP_CHECK(vksift_hip_memcpy_h2d(t->d_tab + buf_tab_at, buf_tab, sizeof(uint32_t) * (2u * t->cap_bufs + sbc), inst->stream), "table upload");
  HIP_CHECK(vksift_hip_event_record(inst->ev_ttab, inst->stream), "event record");
  t->tab_pending = true;
  tracks_invalidate(inst); /* the copy replaces the tracks' row counts, the launches the tracks: not served until the whole sequence has been queued */
  HIP_CHECK(vksift_hip_memcpy_d2d(t->d_rows_acc, e->d_rows, sizeof(uint32_t) * sbc, inst->stream), "row table copy");
  HIP_CHECK(vksift_hip_post_words(t->h_rows_acc, t->d_rows_acc, sbc, inst->stream), "row table read-back");
  HIP_CHECK(vksift_hip_build_tracks_from_edges(e->d_edges, e->d_stats, e->max_edges, t->d_tab + rank_tab_at, sbc, t->d_tab + buf_tab_at, nbufs, t->d_rows, nb, e->max_rows,
                                               t->d_node_words, t->d_records, ((uint64_t)t->cap_bufs * nb) / 2u, t->d_stats, t->d_scratch, t->scratch_u32, inst->stream),
            "track building");
  HIP_CHECK(vksift_hip_post_words(t->h_stats, t->d_stats, 4u, inst->stream), "track statistics read-back");
  HIP_CHECK(stage_end(inst, &frame, t->ids, t->ids, nbufs), "event record");
  t->max_rows = e->max_rows;
  t->valid = true;
  return;
gpu_error:
  e->failed = true;
  stage_fail(inst, &frame, t->ids, t->ids, nbufs);
  logError(LOG_TAG, BUILD_FN " error: Failed to start the track building.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

/* what every accessor starts with: the pipeline that posts the statistics has run, then the checks */
static bool store_served(vksift_Instance inst, bool args_ok, const char *fn)
{
  wait_match(inst);
  if (store_open(inst) && args_ok)
    return true;
  logError(LOG_TAG, "%s() error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
  return false;
}

void vksift_ext_getTrackEdgeStats(vksift_Instance instance, vksift_ext_TrackEdgeStats *out)
{
  if (store_served(instance, out != NULL, "vksift_ext_getTrackEdgeStats"))
    memcpy(out, instance->edges.h_stats, sizeof(*out));
}

void vksift_ext_downloadTrackEdges(vksift_Instance instance, vksift_ext_TrackEdge *edges)
{
  vksift_Instance inst = instance;
  if (!store_served(inst, edges != NULL, "vksift_ext_downloadTrackEdges") || inst->edges.h_stats[0] == 0)
    return;
  HIP_CHECK(vksift_hip_memcpy_d2h(edges, inst->edges.d_edges, sizeof(vksift_ext_TrackEdge) * inst->edges.h_stats[0], inst->dl_stream), "edge read-back");
  HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "edge read-back");
  return;
gpu_error:
  logError(LOG_TAG, "vksift_ext_downloadTrackEdges() error when downloading the edges from GPU memory.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

float vksift_ext_getAccumulateTime(vksift_Instance instance) { return timer_read(instance, T_ACCUMULATE); }
