/*
 * vksift_guided.c — guided matching of the pairs of the last filtered matching under their verified (or the caller's) models
 * (vksift_ext_matchFeaturesGuided and its accessors). No counterpart in the reference: its callers download every feature and descriptor
 * and loop on the CPU. Same contract as the verification it follows (vksift_verify.c): queued on the instance stream, the pairs' buffers
 * busy, the accessors wait; results in storage of its own.
 */
#include "vksift_internal.h"

#define GUIDED_FN "vksift_ext_matchFeaturesGuided()"

/* coordinates, keys, records and counts of batch_cap pairs, allocated by the first guided matching */
static bool ensure_guided_scratch(vksift_Instance inst)
{
  const uint32_t bc = inst->batch_cap, nb = inst->cfg.max_nb_sift_per_buffer;
  inst->gxy_side_stride = nb;
  inst->gkeys_u32 = vksift_hip_guided_scratch_u32(bc, nb);
  const bool ok = mem_ensure(&inst->d_gxy, sizeof(float) * 2u * 2u * inst->gxy_side_stride * bc + 8u, MEM_DEVICE) &&
                  mem_ensure(&inst->d_gkeys, sizeof(uint32_t) * inst->gkeys_u32 + 8u, MEM_DEVICE) &&
                  pair_results_ensure(inst, PR_GUIDED, 1, (((uint64_t)nb * 16u) + 255u) & ~(uint64_t)255u, sizeof(vksift_ext_FilteredMatch), PR_GUIDED) &&
                  mem_ensure(&inst->h_gtab, sizeof(uint32_t) * (pair_table_words(inst) + (size_t)10u * bc), MEM_PINNED);
  if (!inst->ev_gtab)
    inst->ev_gtab = vksift_hip_event_create();
  return ok && inst->ev_gtab;
}

void vksift_ext_matchFeaturesGuided(vksift_Instance instance, uint32_t model, const float *models, float threshold_px, float ratio, float max_distance,
                                    bool cross_check)
{
  vksift_Instance inst = instance;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const PairResults *ver = &inst->res[model == VKSIFT_EXT_GUIDE_HOMOGRAPHY ? PR_VERIFY_H : PR_VERIFY_F]; /* (read once `model` has been checked) */
  PairResults *own = &inst->res[PR_GUIDED];
  const uint32_t count = inst->res[PR_FILTERED].slots_used;
  /* the squared threshold in pixels, formed like the verification's (threshold_px 2^-13)^2 and brought back by the exact factor 2^26 */
  const float ts = threshold_px * (1.0f / 8192.0f), t2 = (ts * ts) * 67108864.0f;
  bool valid = count > 0 && model <= VKSIFT_EXT_GUIDE_FUNDAMENTAL && threshold_px > 0.f && isfinite(threshold_px) && t2 > 0.f && isfinite(t2) && ratio > 0.f &&
               max_distance > 0.f;
  if (valid && models == NULL)
    valid = ver->slots_used == count;
  for (size_t i = 0; valid && models != NULL && i < (size_t)9u * count; i++)
    valid = isfinite(models[i]);
  if (!valid)
  {
    logError(LOG_TAG, GUIDED_FN " error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!ensure_guided_scratch(inst))
  {
    logError(LOG_TAG, GUIDED_FN " error: out of device memory for the guided-matching scratch.");
    goto gpu_error;
  }
  /* the tables are read by the launches out of pinned memory: the previous guided matching must be through with them */
  if (inst->gtab_pending)
  {
    HIP_CHECK(vksift_hip_event_sync(inst->ev_gtab), "event synchronisation");
    inst->gtab_pending = false;
  }
  uint32_t max_rows;
  pair_tables(inst, inst->h_gtab, count, &max_rows);
  uint32_t *h_models = inst->h_gtab + pair_table_words(inst), *h_ones = h_models + (size_t)9u * inst->batch_cap;
  const float *d_models;
  const uint32_t *d_valid;
  uint32_t model_stride, valid_stride;
  if (models != NULL)
  {
    memcpy(h_models, models, sizeof(float) * 9u * count);
    for (uint32_t i = 0; i < count; i++)
      h_ones[i] = 1u;
    d_models = (const float *)h_models, model_stride = 9u, d_valid = h_ones, valid_stride = 1u;
  }
  else /* the verified records: the model's nine floats first, the word `valid` last */
    d_models = (const float *)ver->d_words, model_stride = ver->words, d_valid = ver->d_words + ver->words - 1u, valid_stride = ver->words;
  HIP_CHECK(stage_begin(inst, &frame, T_GUIDED, "Guided matching"), "timer start");
  /* the dense rows and norms: the matcher's cache, refreshed the way the matcher does it (a no-op while the buffers are unchanged) */
  HIP_CHECK(refresh_match_cache(inst, inst->filt_ids, count), "descriptor gather");
  HIP_CHECK(refresh_match_cache(inst, inst->filt_ids + inst->batch_cap, count), "descriptor gather");
  HIP_CHECK(vksift_hip_gather_xy(inst->d_feats, inst->buf_stride, inst->d_found, VKSIFT_MAX_OCTAVES, inst->h_gtab, pair_layouts(inst, inst->h_gtab), max_rows,
                                 count, inst->d_gxy, inst->gxy_side_stride, inst->stream),
            "coordinate gather");
  /* {N_A, N_B} are the words the matching left in d_match_n, rows and coordinates the buffers' present ones: the same while the buffers hold the
   * matched features, which the header asks for (as the verification does; nothing here notices a buffer refilled since). Strides are those of
   * max_nb_sift_per_buffer rows, so the reads stay inside the storage either way. One launch sequence serves 65535 pairs. */
  for (uint32_t r = 0; r < count; r += 65535u)
  {
    const uint32_t n = count - r < 65535u ? count - r : 65535u;
    HIP_CHECK(vksift_hip_match_guided(inst->d_cache_desc, inst->desc_slot_stride, inst->d_cache_norm, inst->cache_norm_stride, inst->h_gtab + (size_t)PAIR_SLOT_WORDS * r, PAIR_SLOT_WORDS,
                                      inst->d_gxy + (size_t)4u * inst->gxy_side_stride * r, inst->gxy_side_stride, inst->d_match_n + (size_t)4u * r, 4u, max_rows,
                                      d_models + (size_t)model_stride * r, model_stride, d_valid + (size_t)valid_stride * r, valid_stride, model, t2, ratio, max_distance,
                                      cross_check ? 1u : 0u, n, own->d_payload + own->stride * r, own->stride, own->d_words + r,
                                      inst->d_gkeys, inst->gkeys_u32, inst->stream),
              "guided matching");
    own->slots_used = 0; /* the launch replaces the set: not served until the whole sequence has been queued */
  }
  HIP_CHECK(vksift_hip_event_record(inst->ev_gtab, inst->stream), "event record");
  inst->gtab_pending = true;
  HIP_CHECK(vksift_hip_post_words(own->h_words, own->d_words, count, inst->stream), "guided count read-back");
  HIP_CHECK(stage_end(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count), "event record");
  own->slots_used = count;
  return;
gpu_error:
  stage_fail(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count);
  logError(LOG_TAG, GUIDED_FN " error: Failed to start the guided-matching pipeline.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

uint32_t vksift_ext_getGuidedMatchesNumber(vksift_Instance instance, uint32_t pair)
{
  const uint32_t *w = pair_words(instance, PR_GUIDED, pair, true, "vksift_ext_getGuidedMatchesNumber");
  return w ? w[0] : 0;
}

void vksift_ext_downloadGuidedMatches(vksift_Instance instance, uint32_t pair, vksift_ext_FilteredMatch *matches)
{
  pair_download(instance, PR_GUIDED, pair, matches, "vksift_ext_downloadGuidedMatches", "guided match read-back", "the guided matches");
}

float vksift_ext_getGuidedMatchTime(vksift_Instance instance) { return timer_read(instance, T_GUIDED); }
