/*
 * vksift_tracks.c — feature tracks over the pairs of the last filtered matching (vksift_ext_buildTracks and its accessors). No counterpart in
 * the reference: its callers download the matches (and masks) of every pair and run a union-find on the host. The only stage that looks at
 * more than one pair at a time, so what it keeps is not a PairResults but a record of its own (TrackResults). Same contract as the guided
 * matching (vksift_guided.c): queued on the instance stream, the pairs' buffers busy, the accessors wait.
 */
#include "vksift_internal.h"

#define TRACKS_FN "vksift_ext_buildTracks()"

_Static_assert(sizeof(vksift_ext_Track) == 16u, "vksift_ext_Track is the kernel's four-word record");
_Static_assert(sizeof(vksift_ext_TrackStats) == 16u, "vksift_ext_TrackStats is the kernel's four statistics words");

/* where a source's edges are: the set whose records and counts they come from, the set whose masks and valid words select them (PR_COUNT: none) */
typedef struct
{
  uint32_t records, masked_by;
} TrackSource;
static const TrackSource sources[] = {
    [VKSIFT_EXT_TRACKS_FILTERED] = {PR_FILTERED, PR_COUNT},   [VKSIFT_EXT_TRACKS_VERIFIED_H] = {PR_FILTERED, PR_VERIFY_H},
    [VKSIFT_EXT_TRACKS_VERIFIED_F] = {PR_FILTERED, PR_VERIFY_F}, [VKSIFT_EXT_TRACKS_REFINED_H] = {PR_FILTERED, PR_REFINE_H},
    [VKSIFT_EXT_TRACKS_REFINED_F] = {PR_FILTERED, PR_REFINE_F},  [VKSIFT_EXT_TRACKS_GUIDED] = {PR_GUIDED, PR_COUNT},
};

bool track_source(vksift_Instance inst, uint32_t source, const PairResults **rec, const PairResults **sel)
{
  const uint32_t count = inst->res[PR_FILTERED].slots_used;
  if (count == 0 || source >= sizeof(sources) / sizeof(sources[0]))
    return false;
  *rec = &inst->res[sources[source].records];
  *sel = sources[source].masked_by == PR_COUNT ? NULL : &inst->res[sources[source].masked_by];
  return (*rec)->slots_used == count && (*sel == NULL || (*sel)->slots_used == count);
}

/* Everything is sized by what the host knows when the call is queued: at most cap_bufs buffers take part — min(2 batch_cap, sift_buffer_count), or
 * sift_buffer_count once an accumulation has been begun (tracks.all_bufs, vksift_track_edges.c) — each with max_nb_sift_per_buffer nodes; a track has two
 * members at least. Allocated by the first build. The tables: {rank A, rank B} per slot of batch_cap, {gpu_buffer_id, count word} per rank, and a rank per
 * SIFT buffer for the accumulated build's edges. */
bool track_storage_ensure(vksift_Instance inst)
{
  TrackResults *t = &inst->tracks;
  const uint32_t bc = inst->batch_cap, nb = inst->cfg.max_nb_sift_per_buffer, sbc = inst->cfg.sift_buffer_count;
  t->cap_bufs = (2u * bc < sbc && !t->all_bufs) ? 2u * bc : sbc;
  const uint64_t nodes = (uint64_t)t->cap_bufs * nb;
  const size_t tab_words = 2u * ((size_t)bc + t->cap_bufs) + sbc;
  t->scratch_u32 = vksift_hip_tracks_scratch_u32(t->cap_bufs, nb);
  const bool ok = nodes < 0xFFFFFFFFull && mem_ensure(&t->d_node_words, sizeof(uint32_t) * nodes + 8u, MEM_DEVICE) &&
                  mem_ensure(&t->d_records, sizeof(vksift_ext_Track) * (nodes / 2u) + 16u, MEM_DEVICE) && mem_ensure(&t->d_stats, sizeof(uint32_t) * 4u, MEM_DEVICE) &&
                  mem_ensure(&t->h_stats, sizeof(uint32_t) * 4u, MEM_PINNED) && mem_ensure(&t->d_scratch, sizeof(uint32_t) * t->scratch_u32 + 8u, MEM_DEVICE) &&
                  mem_ensure(&t->h_tab, sizeof(uint32_t) * tab_words, MEM_PINNED) && mem_ensure(&t->d_tab, sizeof(uint32_t) * tab_words, MEM_DEVICE) &&
                  mem_ensure(&t->rank_of, sizeof(uint32_t) * sbc, MEM_HEAP) && mem_ensure(&t->count_word, sizeof(uint32_t) * t->cap_bufs, MEM_HEAP) &&
                  mem_ensure(&t->ids, sizeof(uint32_t) * t->cap_bufs, MEM_HEAP);
  if (!inst->ev_ttab)
    inst->ev_ttab = vksift_hip_event_create();
  return ok && inst->ev_ttab;
}

/* ranks: the buffers of the pair list in increasing gpu_buffer_id. A buffer's row count is the word the matching left in d_match_n for the first pair
 * that names it ({N_A, N_B, spare, spare} per slot): on the device, so nothing here waits for it */
uint32_t pair_list_ranks(vksift_Instance inst, uint32_t count, uint32_t *rank_of, uint32_t *slot_tab, uint32_t *buf_tab, uint32_t *ids, uint32_t *count_word, uint32_t *max_rows)
{
  const uint32_t *ids_a = inst->filt_ids, *ids_b = inst->filt_ids + inst->batch_cap;
  for (uint32_t b = 0; b < inst->cfg.sift_buffer_count; b++)
    rank_of[b] = VKSIFT_EXT_NO_TRACK;
  for (uint32_t i = 0; i < count; i++)
    rank_of[ids_a[i]] = rank_of[ids_b[i]] = 0;
  uint32_t nbufs = 0;
  for (uint32_t b = 0; b < inst->cfg.sift_buffer_count; b++)
    if (rank_of[b] == 0)
      rank_of[b] = nbufs++;
  (void)detect_running(inst); /* polls the detections in flight: rows_bound() uses the counts that have arrived */
  uint32_t rows = 1;
  for (uint32_t i = count; i-- > 0;) /* (downwards: the first pair that names a buffer has the last word) */
    for (uint32_t side = 0; side < 2u; side++)
    {
      const uint32_t id = side ? ids_b[i] : ids_a[i], r = rank_of[id];
      slot_tab[2u * i + side] = r;
      buf_tab[2u * r] = id, buf_tab[2u * r + 1u] = 4u * i + side;
      if (ids)
        ids[r] = id, count_word[r] = 4u * i + side;
      rows = rows_bound(inst, id) > rows ? rows_bound(inst, id) : rows;
    }
  *max_rows = rows;
  return nbufs;
}

void vksift_ext_buildTracks(vksift_Instance instance, uint32_t source)
{
  vksift_Instance inst = instance;
  TrackResults *t = &inst->tracks;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const uint32_t count = inst->res[PR_FILTERED].slots_used, nb = inst->cfg.max_nb_sift_per_buffer;
  const PairResults *rec, *sel;
  const bool valid = track_source(inst, source, &rec, &sel);
  if (!valid)
  {
    logError(LOG_TAG, TRACKS_FN " error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!track_storage_ensure(inst))
  {
    logError(LOG_TAG, TRACKS_FN " error: out of device memory for the tracks.");
    goto gpu_error;
  }
  /* the tables are copied out of pinned memory on the stream: the previous build's copy must be through with them */
  if (t->tab_pending)
  {
    HIP_CHECK(vksift_hip_event_sync(inst->ev_ttab), "event synchronisation");
    t->tab_pending = false;
  }
  const uint32_t *ids_a = inst->filt_ids, *ids_b = inst->filt_ids + inst->batch_cap;
  uint32_t rows;
  t->nbufs = pair_list_ranks(inst, count, t->rank_of, t->h_tab, t->h_tab + (size_t)2u * inst->batch_cap, t->ids, t->count_word, &rows);
  t->d_rows = inst->d_match_n, t->h_rows = inst->h_match_n;
  const uint32_t max_rows = rows < nb ? rows : nb; /* (stored with `valid`: the tracks of an earlier build are read with theirs until then) */
  HIP_CHECK(stage_begin(inst, &frame, T_TRACKS, "Tracks"), "timer start");
  const size_t buf_tab_at = (size_t)2u * inst->batch_cap;
  HIP_CHECK(vksift_hip_memcpy_h2d(t->d_tab, t->h_tab, sizeof(uint32_t) * (buf_tab_at + 2u * t->nbufs), inst->stream), "table upload");
  HIP_CHECK(vksift_hip_event_record(inst->ev_ttab, inst->stream), "event record");
  t->tab_pending = true;
  /* a record set's first word is its count; a mask set's last word is `valid` (vksift_ext_Homography ... vksift_ext_RefinedFundamental). No pair holds
   * more records than its buffer A has rows */
  HIP_CHECK(vksift_hip_build_tracks(rec->d_payload, rec->stride, rec->d_words, rec->words, max_rows, sel ? sel->d_payload : NULL, sel ? sel->stride : 0,
                                    sel ? sel->d_words + sel->words - 1u : NULL, sel ? sel->words : 0, t->d_tab, 2u, count, t->d_tab + buf_tab_at, t->nbufs, t->d_rows, nb,
                                    max_rows, t->d_node_words, t->d_records, ((uint64_t)t->cap_bufs * nb) / 2u, t->d_stats, t->d_scratch, t->scratch_u32, inst->stream),
            "track building");
  tracks_invalidate(inst); /* the launch replaces the tracks: not served until the whole sequence has been queued; observations of the earlier tracks, their
                            * points, view index and refined cameras are not served any more */
  HIP_CHECK(vksift_hip_post_words(t->h_stats, t->d_stats, 4u, inst->stream), "track statistics read-back");
  HIP_CHECK(stage_end(inst, &frame, ids_a, ids_b, count), "event record");
  t->max_rows = max_rows;
  t->valid = true;
  return;
gpu_error:
  stage_fail(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count);
  logError(LOG_TAG, TRACKS_FN " error: Failed to start the track building.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

/* what every accessor starts with: the pipeline that posts the statistics has run, then the checks */
static bool tracks_served(vksift_Instance inst, bool args_ok, const char *fn)
{
  wait_match(inst);
  if (inst->tracks.valid && args_ok)
    return true;
  logError(LOG_TAG, "%s() error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
  return false;
}

static void tracks_fetch(vksift_Instance inst, void *dst, const void *src, size_t bytes, const char *fn)
{
  if (bytes == 0)
    return;
  HIP_CHECK(vksift_hip_memcpy_d2h(dst, src, bytes, inst->dl_stream), "track read-back");
  HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "track read-back");
  return;
gpu_error:
  logError(LOG_TAG, "%s() error when downloading the tracks from GPU memory.", fn);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_ext_getTrackStats(vksift_Instance instance, vksift_ext_TrackStats *out)
{
  if (tracks_served(instance, out != NULL, "vksift_ext_getTrackStats"))
    memcpy(out, instance->tracks.h_stats, sizeof(*out));
}

void vksift_ext_downloadTracks(vksift_Instance instance, vksift_ext_Track *tracks)
{
  if (tracks_served(instance, tracks != NULL, "vksift_ext_downloadTracks"))
    tracks_fetch(instance, tracks, instance->tracks.d_records, sizeof(vksift_ext_Track) * instance->tracks.h_stats[0], "vksift_ext_downloadTracks");
}

void vksift_ext_downloadFeatureTracks(vksift_Instance instance, uint32_t gpu_buffer_id, uint32_t *track_ids)
{
  const TrackResults *t = &instance->tracks;
  const bool known = t->valid && gpu_buffer_id < instance->cfg.sift_buffer_count && t->rank_of[gpu_buffer_id] != VKSIFT_EXT_NO_TRACK;
  if (!tracks_served(instance, known && track_ids != NULL, "vksift_ext_downloadFeatureTracks"))
    return;
  /* the rows the launches labelled: the count posted for the buffer, as the kernels clamped it */
  const uint32_t r = t->rank_of[gpu_buffer_id], n = t->h_rows[t->count_word[r]];
  tracks_fetch(instance, track_ids, t->d_node_words + (size_t)r * instance->cfg.max_nb_sift_per_buffer, sizeof(uint32_t) * (n < t->max_rows ? n : t->max_rows),
               "vksift_ext_downloadFeatureTracks");
}

float vksift_ext_getTracksTime(vksift_Instance instance) { return timer_read(instance, T_TRACKS); }
