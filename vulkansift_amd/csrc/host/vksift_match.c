/*
 * vksift_match.c — the matching pipeline (vulkansift.c:417-462, sift_memory.c:957-1058, sift_matcher.c:246-279) and GPU-side match filtering
 */
#include "vksift_internal.h"

/* ------------------------------------------------------------------------------------------------ */
/* matching (vulkansift.c:417-462, sift_memory.c:957-1058, sift_matcher.c:408-486)                  */
/* ------------------------------------------------------------------------------------------------ */
/* Launch bound on the number of stored rows of a buffer: the real total if its counters have reached the host, else the
 * sum of its section capacities. */
uint32_t rows_bound(vksift_Instance inst, uint32_t id)
{
  const BufferInfo *b = &inst->bufs[id];
  if (b->nb_sections == 0)
    return b->nb_stored;
  uint32_t known = 0, cap_sum = 0;
  const uint32_t *found = inst->h_found + (size_t)id * VKSIFT_MAX_OCTAVES;
  for (uint32_t o = 0; o < b->nb_sections; o++)
  {
    known += found[o] < b->sec_cap[o] ? found[o] : b->sec_cap[o];
    cap_sum += b->sec_cap[o];
  }
  return counts_valid(inst, id) ? known : cap_sum;
}

/* layout word of a buffer in a pair table: its section table is appended to `layouts` unless an equal one is there */
static uint32_t layout_word(const BufferInfo *b, uint32_t *layouts, uint32_t *nlay)
{
  if (b->nb_sections == 0)
    return VKSIFT_LAYOUT_DENSE | b->nb_stored; /* uploaded: one dense run of records */
  uint32_t t[VKSIFT_LAYOUT_WORDS] = {0};
  t[0] = b->nb_sections;
  for (uint32_t o = 0; o < b->nb_sections; o++)
    t[VKSIFT_LAYOUT_OFF_AT + o] = b->sec_off[o], t[VKSIFT_LAYOUT_CAP_AT + o] = b->sec_cap[o];
  for (uint32_t k = *nlay; k-- > 0;) /* the last one first: the buffers of a batched detection all share one */
    if (memcmp(layouts + (size_t)k * VKSIFT_LAYOUT_WORDS, t, sizeof(t)) == 0)
      return k;
  memcpy(layouts + (size_t)*nlay * VKSIFT_LAYOUT_WORDS, t, sizeof(t));
  return (*nlay)++;
}

void pair_tables(vksift_Instance inst, uint32_t *tab, uint32_t count, uint32_t *max_rows)
{
  uint32_t *layouts = pair_layouts(inst, tab), nlay = 0, rows = 0;
  if (max_rows)
    (void)detect_running(inst); /* polls the detections in flight: rows_bound() uses the counts that have arrived */
  for (uint32_t i = 0; i < count; i++)
    for (uint32_t side = 0; side < 2u; side++)
    {
      const uint32_t id = inst->filt_ids[side * inst->batch_cap + i];
      tab[PAIR_SLOT_WORDS * i + side] = id;
      tab[PAIR_SLOT_WORDS * i + 2u + side] = layout_word(&inst->bufs[id], layouts, &nlay);
      if (max_rows && rows_bound(inst, id) > rows)
        rows = rows_bound(inst, id);
    }
  if (max_rows)
    *max_rows = rows < inst->cfg.max_nb_sift_per_buffer ? rows : inst->cfg.max_nb_sift_per_buffer;
}

void buffer_layouts(vksift_Instance inst, const uint32_t *ids, uint32_t n, uint32_t *words, uint32_t *layouts)
{
  uint32_t nlay = 0;
  for (uint32_t i = 0; i < n; i++)
    words[i] = layout_word(&inst->bufs[ids[i]], layouts, &nlay);
}

/* The matcher's input of a SIFT buffer — dense 128-byte descriptor rows in download order, their shifted norms and the row
 * count — lives in a per-buffer cache entry, filled by ONE device-side gather the first time the buffer is matched after it
 * changed (detection, upload) and reused by every later matching: a self-match gathers once instead of twice, the two
 * directions of a pair matching gather nothing the second time. The reference physically packs the octave sections
 * (pack_BufferMemory, sift_memory.c:957-1047) after reading the counts on the host; here the gather kernel reads the
 * counters in HBM and walks the sections in the same order, so nothing waits on the host. Rows below 2 are zero-filled:
 * Get2NearestNeighbors.comp:66-67 reads b[0] and b[1] unconditionally (stale memory in the reference when B holds fewer
 * than two features); here the missing rows are defined as all-zero descriptors. */
/* first matching / descriptor export of the instance: the cache blocks (see create_instance). A failed allocation is retried by
 * the next call; nothing is leaked in between. */
static int ensure_match_cache(vksift_Instance inst)
{
  const uint32_t nb = inst->cfg.max_nb_sift_per_buffer;
  const bool desc = mem_ensure(&inst->d_cache_desc, inst->desc_slot_stride * inst->cfg.sift_buffer_count, MEM_DEVICE);
  const bool norm = mem_ensure(&inst->d_cache_norm, sizeof(uint32_t) * inst->cache_norm_stride * inst->cfg.sift_buffer_count, MEM_DEVICE);
  const bool part = nb <= VKSIFT_HIP_MATCH_SMALL_NA || mem_ensure(&inst->d_match_partial, sizeof(uint32_t) * (size_t)nb * 5u * VKSIFT_HIP_MATCH_CHUNKS, MEM_DEVICE);
  return (desc && norm && part) ? 0 : 2; /* hipErrorOutOfMemory */
}

int refresh_match_cache(vksift_Instance inst, const uint32_t *ids, uint32_t count)
{
  const int ce = ensure_match_cache(inst);
  if (ce)
    return ce;
  (void)detect_running(inst); /* polls the detections in flight: counts_valid() is up to date */
  /* Passes of at most VKSIFT_HIP_GATHER_SLOTS not-yet-cached buffers until none is left: a run of VKSIFT_HIP_MATCH_SLOTS (256) pairs may
   * name that many distinct buffers per side, and every one of them must be gathered before the matching kernels read its cache entry. */
  for (;;)
  {
    uint32_t todo[VKSIFT_HIP_GATHER_SLOTS], bound[VKSIFT_HIP_GATHER_SLOTS];
    uint32_t n = 0;
    bool more = false;
    for (uint32_t i = 0; i < count; i++)
    {
      if (inst->cache_valid[ids[i]] || inst->cache_queued[ids[i]])
        continue;
      if (n == VKSIFT_HIP_GATHER_SLOTS)
      {
        more = true; /* taken by the next pass */
        break;
      }
      inst->cache_queued[ids[i]] = true;
      todo[n++] = ids[i];
    }
    for (uint32_t k = 0; k < n; k++)
      inst->cache_queued[todo[k]] = false, bound[k] = rows_bound(inst, todo[k]);
    LayoutRun run;
    for (uint32_t pos = 0; next_layout_run(inst->bufs, todo, n, bound, &pos, &run);)
    {
      const int e = vksift_hip_gather_sections(inst->d_feats, inst->buf_stride, run.ids, run.n, run.nsec, run.off, run.cap, run.fixed, run.fixed ? NULL : inst->d_found,
                                               run.found_stride, run.max_rows, 2u, inst->d_cache_desc, inst->desc_slot_stride, inst->d_cache_norm,
                                               inst->cache_norm_stride, inst->d_cache_n, 1, inst->stream);
      if (e)
        return e;
      for (uint32_t k = 0; k < run.n; k++)
        inst->cache_valid[run.ids[k]] = true;
    }
    if (!more)
      return 0;
  }
}

MatchScratch fwd_scratch(vksift_Instance inst)
{
  MatchScratch ms = {inst->d_matches, inst->d_redo, inst->d_match_n};
  return ms;
}

static int match_slots(vksift_Instance inst, const MatchScratch *ms, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count, uint32_t first_slot)
{
  int e = refresh_match_cache(inst, ids_a, count);
  if (e == 0)
    e = refresh_match_cache(inst, ids_b, count);
  if (e)
    return e;
  uint32_t max_na = 0, max_nb = 0;
  bool nb_exact = true; /* every reference buffer's count is known on the host (uploaded, or its detection has completed) */
  for (uint32_t i = 0; i < count; i++)
  {
    const uint32_t r = rows_bound(inst, ids_a[i]), rb = rows_bound(inst, ids_b[i]);
    max_na = r > max_na ? r : max_na;
    max_nb = rb > max_nb ? rb : max_nb;
    nb_exact = nb_exact && (inst->bufs[ids_b[i]].nb_sections == 0 || counts_valid(inst, ids_b[i]));
  }
  return vksift_hip_match_2nn_async(inst->d_cache_desc, inst->d_cache_norm, inst->d_cache_n, ids_a, ids_b, max_na, max_nb, nb_exact ? 1u : 0u,
                                    ms->redo + (uint64_t)first_slot * inst->redo_slot_stride, ms->match_n + (size_t)first_slot * 4,
                                    ms->matches + (uint64_t)first_slot * inst->match_slot_stride, count, inst->desc_slot_stride, inst->cache_norm_stride,
                                    inst->redo_slot_stride, inst->match_slot_stride, 4, inst->d_match_partial, inst->stream);
}

/* reverse-matching scratch + survivor lists of vksift_ext_matchFeaturesFiltered, allocated on first use */
static bool ensure_filter_scratch(vksift_Instance inst)
{
  const uint32_t bc = inst->batch_cap;
  const uint64_t stride = (((uint64_t)inst->cfg.max_nb_sift_per_buffer * 16u) + 255u) & ~(uint64_t)255u;
  return mem_ensure(&inst->rev.matches, inst->match_slot_stride * bc, MEM_DEVICE) && mem_ensure(&inst->rev.redo, sizeof(uint32_t) * inst->redo_slot_stride * bc, MEM_DEVICE) &&
         mem_ensure(&inst->rev.match_n, sizeof(uint32_t) * 4 * bc, MEM_DEVICE) && pair_results_ensure(inst, PR_FILTERED, 1, stride, sizeof(vksift_ext_FilteredMatch), PR_FILTERED) &&
         mem_ensure(&inst->filt_ids, sizeof(uint32_t) * 2u * bc, MEM_HEAP);
}

static void match_impl(vksift_Instance inst, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count, const char *fn, bool filter, float ratio,
                       bool cross_check)
{
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  bool valid = count >= 1 && count <= inst->batch_cap;
  for (uint32_t i = 0; valid && i < count; i++)
    valid = buffer_idx_valid(inst, ids_a[i]) && buffer_idx_valid(inst, ids_b[i]);
  if (!valid)
  {
    logError(LOG_TAG, "%s error: invalid input.", fn);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  vksift_hip_set_device(inst->device);
  HIP_CHECK(stage_begin(inst, &frame, T_MATCH, "Matching"), "timer start");
  const MatchScratch fwd = fwd_scratch(inst);
  /* the matcher's view of every buffer of the call first, in one gather launch per 512 buffers (each run below would gather its own) */
  HIP_CHECK(refresh_match_cache(inst, ids_a, count), "descriptor gather");
  HIP_CHECK(refresh_match_cache(inst, ids_b, count), "descriptor gather");
  /* one launch sequence serves up to VKSIFT_HIP_MATCH_SLOTS pairs; a longer list goes in runs of that many, run r into the slots from r on */
  for (uint32_t r = 0; r < count; r += VKSIFT_HIP_MATCH_SLOTS)
  {
    HIP_CHECK(match_slots(inst, &fwd, ids_a + r, ids_b + r, count - r < VKSIFT_HIP_MATCH_SLOTS ? count - r : VKSIFT_HIP_MATCH_SLOTS, r), "2-NN matching");
    if (r == 0)
    {
      /* the first launch that overwrites the previous matching's records and counts has been queued: nothing of that matching is served any more,
       * whatever becomes of this call (it marks its own results once the whole sequence has been queued) */
      pair_results_invalidate(inst);
      tracks_invalidate(inst); /* tracks are built from the pairs of a matching (vksift_tracks.c), observations from tracks, points and the view index from observations, refined cameras from both */
      inst->match_slots_used = 0;
      inst->md_valid = false, inst->md_hits = 0, inst->md_direct = false, inst->md_asked = false;
    }
  }
  HIP_CHECK(vksift_hip_post_words(inst->h_match_n, inst->d_match_n, (size_t)4 * count, inst->stream), "match count read-back");
  if (inst->desc_start_valid && vksift_hip_tune_get(VKSIFT_TUNE_PYR_GATE) == 1)
    vksift_hip_event_record(inst->ev_desc_start, inst->stream); /* experiment: the next scale-space behind this matching, not beside it */
  if (filter)
  {
    /* the reverse matching, then cross-check + ratio test on the device; only the survivors are read back */
    if (!ensure_filter_scratch(inst))
    {
      logError(LOG_TAG, "%s error: out of device memory for the filtered-matching scratch.", fn);
      goto gpu_error;
    }
    PairResults *filt = &inst->res[PR_FILTERED];
    for (uint32_t r = 0; r < count; r += VKSIFT_HIP_MATCH_SLOTS)
    {
      const uint32_t n = count - r < VKSIFT_HIP_MATCH_SLOTS ? count - r : VKSIFT_HIP_MATCH_SLOTS;
      if (cross_check)
        HIP_CHECK(match_slots(inst, &inst->rev, ids_b + r, ids_a + r, n, r), "reverse 2-NN matching");
      HIP_CHECK(vksift_hip_filter_matches(inst->d_matches + (uint64_t)r * inst->match_slot_stride, inst->match_slot_stride,
                                          cross_check ? inst->rev.matches + (uint64_t)r * inst->match_slot_stride : NULL, inst->match_slot_stride,
                                          inst->d_match_n + (size_t)r * 4, 4, ratio, n, filt->d_payload + (uint64_t)r * filt->stride, filt->stride,
                                          filt->d_words + r, inst->stream),
                "match filtering");
    }
    HIP_CHECK(vksift_hip_post_words(filt->h_words, filt->d_words, count, inst->stream), "filtered count read-back");
    /* the pairs, for vksift_ext_verifyHomography */
    memcpy(inst->filt_ids, ids_a, sizeof(uint32_t) * count);
    memcpy(inst->filt_ids + inst->batch_cap, ids_b, sizeof(uint32_t) * count);
  }
  HIP_CHECK(stage_end(inst, &frame, ids_a, ids_b, count), "event record");
  inst->match_slots_used = count; /* (served only now: the accessors wait for the event stage_end has recorded) */
  if (filter)
    inst->res[PR_FILTERED].slots_used = count;
  return;
gpu_error:
  stage_fail(inst, &frame, ids_a, ids_b, count);
  logError(LOG_TAG, "%s error: Failed to start the matching pipeline.", fn);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_matchFeatures(vksift_Instance instance, uint32_t gpu_buffer_id_A, uint32_t gpu_buffer_id_B)
{
  match_impl(instance, &gpu_buffer_id_A, &gpu_buffer_id_B, 1, "vksift_matchFeatures()", false, 0.f, false);
}

void vksift_ext_matchFeaturesBatch(vksift_Instance instance, uint32_t count, const uint32_t *gpu_buffer_ids_A, const uint32_t *gpu_buffer_ids_B)
{
  match_impl(instance, gpu_buffer_ids_A, gpu_buffer_ids_B, count, "vksift_ext_matchFeaturesBatch()", false, 0.f, false);
}

void vksift_ext_matchFeaturesFiltered(vksift_Instance instance, uint32_t count, const uint32_t *gpu_buffer_ids_A, const uint32_t *gpu_buffer_ids_B, float ratio,
                                      bool cross_check)
{
  if (!(ratio > 0.f))
  {
    logError(LOG_TAG, "vksift_ext_matchFeaturesFiltered() error: invalid input.");
    instance->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  match_impl(instance, gpu_buffer_ids_A, gpu_buffer_ids_B, count, "vksift_ext_matchFeaturesFiltered()", true, ratio, cross_check);
}

int match_follow(vksift_Instance inst, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count)
{
  (void)match_running(inst); /* an earlier matching that has completed releases its buffers; one still in flight keeps them */
  const int e = vksift_hip_event_record(inst->ev_match, inst->stream);
  if (e)
    return e;
  inst->match_pending = true;
  for (uint32_t i = 0; i < count; i++)
    inst->match_busy[ids_a[i]] = inst->match_busy[ids_b[i]] = true; /* every pair of a batched call (vksift_isBufferAvailable) */
  return 0;
}

void wait_match(vksift_Instance inst)
{
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  if (inst->match_pending)
  {
    vksift_hip_event_sync(inst->ev_match);
    inst->match_pending = false;
  }
  inst->curr_nb_matches = inst->h_match_n[0];
}

/* The reference knows N_A on the host when vksift_matchFeatures returns (it blocks while packing); here the count is
 * produced on the device, so this accessor waits for the matching pipeline if it is still running. */
uint32_t vksift_getMatchesNumber(vksift_Instance instance)
{
  wait_match(instance);
  return instance->curr_nb_matches;
}

uint32_t vksift_ext_getMatchesNumberBatch(vksift_Instance instance, uint32_t pair)
{
  wait_match(instance);
  if (pair >= instance->match_slots_used)
  {
    logError(LOG_TAG, "vksift_ext_getMatchesNumberBatch() error: invalid input.");
    instance->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return 0;
  }
  return instance->h_match_n[(size_t)pair * 4];
}

/* all pairs of the last matching -> pinned memory (row pitch = the longest list), then `pair` out of it; false: not available */
static bool packed_match_download(vksift_Instance inst, uint32_t pair, vksift_Match_2NN *matches, uint32_t n)
{
  if (!inst->md_valid)
  {
    uint32_t max_n = 0;
    for (uint32_t i = 0; i < inst->match_slots_used; i++)
      max_n = inst->h_match_n[(size_t)i * 4] > max_n ? inst->h_match_n[(size_t)i * 4] : max_n;
    const size_t pitch = (size_t)max_n * MATCH_BYTES, bytes = pitch * inst->match_slots_used;
    if (bytes > inst->md_cap)
    {
      mem_release(&inst->h_matches, MEM_PINNED);
      inst->md_cap = mem_ensure(&inst->h_matches, bytes + bytes / 4u + 4096u, MEM_PINNED) ? bytes + bytes / 4u + 4096u : 0;
      if (!inst->md_cap)
        return false;
    }
    if (vksift_hip_memcpy2d_d2h(inst->h_matches, pitch, inst->d_matches, inst->match_slot_stride, pitch, inst->match_slots_used, inst->dl_stream) != 0 ||
        vksift_hip_stream_sync(inst->dl_stream) != 0)
      return false;
    inst->md_pitch = pitch;
    inst->md_valid = true;
  }
  memcpy(matches, inst->h_matches + (size_t)pair * inst->md_pitch, (size_t)n * MATCH_BYTES);
  return true;
}

static void download_matches(vksift_Instance inst, uint32_t pair, vksift_Match_2NN *matches, const char *fn)
{
  wait_match(inst);
  if (pair >= inst->match_slots_used && !(pair == 0 && inst->match_slots_used == 0))
  {
    logError(LOG_TAG, "%s error: invalid input.", fn);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  uint32_t n = inst->h_match_n[(size_t)pair * 4];
  if (n > 0)
  {
    /* A caller that walks the pairs of a batched matching gets them out of ONE strided copy into pinned memory instead of one
     * copy + synchronisation per pair (12 us each: 1.5 ms per 128 pairs). Like the packed feature download it starts with the
     * second download after a matching: a caller that samples one pair must not pay for all of them. */
    /* (a page-locked destination takes the records by DMA straight from the slot: vksift_ext_pinHostMemory) */
    if (inst->match_slots_used >= VKSIFT_DL_BATCH_MIN && !inst->md_asked)
      inst->md_direct = !detect_running(inst) && vksift_hip_is_pinned(matches) == 1, inst->md_asked = true; /* once per matching: the query costs a microsecond; not behind a queued detection (vksift_buffers.c) */
    if (inst->match_slots_used >= VKSIFT_DL_BATCH_MIN && !inst->md_direct && (inst->md_valid || inst->md_hits++ > 0) &&
        packed_match_download(inst, pair, matches, n))
      return;
    HIP_CHECK(vksift_hip_memcpy_d2h(matches, inst->d_matches + (uint64_t)pair * inst->match_slot_stride, (size_t)n * MATCH_BYTES, inst->dl_stream),
              "match read-back");
    HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "match read-back");
  }
  return;
gpu_error:
  logError(LOG_TAG, "%s error when downloading SIFT matches from GPU memory.", fn);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_downloadMatches(vksift_Instance instance, vksift_Match_2NN *matches) { download_matches(instance, 0, matches, "vksift_downloadMatches()"); }

uint32_t vksift_ext_getFilteredMatchesNumber(vksift_Instance instance, uint32_t pair)
{
  const uint32_t *w = pair_words(instance, PR_FILTERED, pair, true, "vksift_ext_getFilteredMatchesNumber");
  return w ? w[0] : 0;
}

void vksift_ext_downloadFilteredMatches(vksift_Instance instance, uint32_t pair, vksift_ext_FilteredMatch *matches)
{
  pair_download(instance, PR_FILTERED, pair, matches, "vksift_ext_downloadFilteredMatches", "filtered match read-back", "the filtered matches");
}

void vksift_ext_downloadMatchesBatch(vksift_Instance instance, uint32_t pair, vksift_Match_2NN *matches)
{
  download_matches(instance, pair, matches, "vksift_ext_downloadMatchesBatch()");
}

