/*
 * vksift_verify.c — geometric verification of the last filtered matching (vksift_ext_verifyHomography, vksift_ext_verifyFundamental and
 * their accessors). No counterpart in the reference: its callers download matches and features and run a CPU RANSAC per pair. A model
 * (VerifyModel) is its kernel entry, its record size and its own result set; everything else here (scratch, pair tables, posting)
 * serves both, and the frame and the accessors are those of every pair stage (vksift_pairs.c).
 */
#include "vksift_internal.h"

#define VERIFY_RES_WORDS 13u   /* sizeof(vksift_ext_Homography) / 4 */
#define VERIFY_F_RES_WORDS 14u /* sizeof(vksift_ext_Fundamental) / 4 */
#define VERIFY_MAX_HYPOTHESES 65536u

_Static_assert(sizeof(vksift_ext_Homography) == 4u * VERIFY_RES_WORDS, "vksift_ext_Homography is the kernel's 13-word result record");
_Static_assert(sizeof(vksift_ext_Fundamental) == 4u * VERIFY_F_RES_WORDS, "vksift_ext_Fundamental is the kernel's 14-word result record");

typedef int (*RansacFn)(const float *, uint64_t, const uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, float, uint64_t, uint8_t *, uint8_t *, uint64_t, uint32_t *,
                        size_t, vksift_hip_stream);

/* what differs between the models: the names, the launcher, the record, and which of the instance's result sets are the model's own and its refit's */
typedef struct
{
  const char *entry, *get_entry, *mask_entry;
  RansacFn ransac;
  uint32_t res_words;
  uint32_t set;
  uint32_t refit; /* results computed from this model's records and masks, no longer theirs once it is verified again */
} VerifyModel;

static const VerifyModel model_h = {"vksift_ext_verifyHomography", "vksift_ext_getHomography", "vksift_ext_downloadInlierMask", vksift_hip_ransac_homography,
                                    VERIFY_RES_WORDS, PR_VERIFY_H, PR_REFINE_H};
static const VerifyModel model_f = {"vksift_ext_verifyFundamental", "vksift_ext_getFundamental", "vksift_ext_downloadFundamentalInlierMask",
                                    vksift_hip_ransac_fundamental, VERIFY_F_RES_WORDS, PR_VERIFY_F, PR_REFINE_F};

/* correspondences, reduction keys and pair tables of batch_cap pairs, and the masks and results of the model asked for; allocated by the
 * first verification (detect-only and match-only users never pay, and a model that is never asked for costs nothing) */
static bool ensure_verify_scratch(vksift_Instance inst, const VerifyModel *m)
{
  const uint32_t bc = inst->batch_cap;
  const uint64_t mask_stride = ((uint64_t)inst->cfg.max_nb_sift_per_buffer + 255u) & ~(uint64_t)255u;
  inst->vscratch_u32 = vksift_hip_ransac_scratch_u32(bc, VERIFY_MAX_HYPOTHESES);
  const bool ok = mem_ensure(&inst->d_corr, inst->res[PR_FILTERED].stride * bc, MEM_DEVICE) && pair_results_ensure(inst, m->set, m->res_words, mask_stride, 1, PR_FILTERED) &&
                  mem_ensure(&inst->d_vscratch, sizeof(uint32_t) * inst->vscratch_u32, MEM_DEVICE) &&
                  mem_ensure(&inst->h_vtab, sizeof(uint32_t) * pair_table_words(inst), MEM_PINNED);
  if (!inst->ev_vtab)
    inst->ev_vtab = vksift_hip_event_create();
  return ok && inst->ev_vtab;
}

static void verify(vksift_Instance inst, const VerifyModel *m, uint32_t nb_hypotheses, float threshold_px, uint64_t seed)
{
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const PairResults *filt = &inst->res[PR_FILTERED];
  PairResults *own = &inst->res[m->set];
  const uint32_t count = filt->slots_used;
  if (count == 0 || nb_hypotheses == 0 || nb_hypotheses > VERIFY_MAX_HYPOTHESES || !(threshold_px > 0.f) || !isfinite(threshold_px))
  {
    logError(LOG_TAG, "%s() error: invalid input.", m->entry);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!ensure_verify_scratch(inst, m))
  {
    logError(LOG_TAG, "%s() error: out of device memory for the verification scratch.", m->entry);
    goto gpu_error;
  }
  /* the pair table is read by the gather launch out of pinned memory: the previous verification's launch must be through with it */
  if (inst->vtab_pending)
  {
    HIP_CHECK(vksift_hip_event_sync(inst->ev_vtab), "event synchronisation");
    inst->vtab_pending = false;
  }
  pair_tables(inst, inst->h_vtab, count, NULL);
  HIP_CHECK(stage_begin(inst, &frame, T_VERIFY, "Verification"), "timer start");
  HIP_CHECK(vksift_hip_gather_correspondences(inst->d_feats, inst->buf_stride, inst->d_found, VKSIFT_MAX_OCTAVES, inst->h_vtab,
                                              pair_layouts(inst, inst->h_vtab), filt->d_payload, filt->stride, filt->d_words,
                                              inst->cfg.max_nb_sift_per_buffer, count, inst->d_corr, filt->stride, inst->stream),
            "correspondence gather");
  HIP_CHECK(vksift_hip_event_record(inst->ev_vtab, inst->stream), "event record");
  inst->vtab_pending = true;
  HIP_CHECK(m->ransac(inst->d_corr, filt->stride, filt->d_words, 1, inst->cfg.max_nb_sift_per_buffer, count, nb_hypotheses, threshold_px, seed,
                      (uint8_t *)own->d_words, own->d_payload, own->stride, inst->d_vscratch, inst->vscratch_u32, inst->stream),
            "RANSAC");
  /* the launch replaces the model's records and masks, and with them what the refinement (vksift_refine.c) was computed from: neither is served any
   * more, whatever becomes of this call (the model's set is marked again once the whole sequence has been queued) */
  own->slots_used = inst->res[m->refit].slots_used = 0;
  HIP_CHECK(vksift_hip_post_words(own->h_words, own->d_words, (size_t)m->res_words * count, inst->stream), "verification read-back");
  HIP_CHECK(stage_end(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count), "event record");
  own->slots_used = count;
  return;
gpu_error:
  stage_fail(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count);
  logError(LOG_TAG, "%s() error: Failed to start the verification pipeline.", m->entry);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

static void get_result(vksift_Instance inst, const VerifyModel *m, uint32_t pair, void *out)
{
  const uint32_t *w = pair_words(inst, m->set, pair, out != NULL, m->get_entry);
  if (w)
    memcpy(out, w, sizeof(uint32_t) * m->res_words);
}

static void download_mask(vksift_Instance inst, const VerifyModel *m, uint32_t pair, uint8_t *mask)
{
  pair_download(inst, m->set, pair, mask, m->mask_entry, "inlier mask read-back", "the inlier mask");
}

void vksift_ext_verifyHomography(vksift_Instance instance, uint32_t nb_hypotheses, float threshold_px, uint64_t seed)
{
  verify(instance, &model_h, nb_hypotheses, threshold_px, seed);
}

void vksift_ext_getHomography(vksift_Instance instance, uint32_t pair, vksift_ext_Homography *out) { get_result(instance, &model_h, pair, out); }

void vksift_ext_downloadInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask) { download_mask(instance, &model_h, pair, mask); }

void vksift_ext_verifyFundamental(vksift_Instance instance, uint32_t nb_hypotheses, float threshold_px, uint64_t seed)
{
  verify(instance, &model_f, nb_hypotheses, threshold_px, seed);
}

void vksift_ext_getFundamental(vksift_Instance instance, uint32_t pair, vksift_ext_Fundamental *out) { get_result(instance, &model_f, pair, out); }

void vksift_ext_downloadFundamentalInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask) { download_mask(instance, &model_f, pair, mask); }

float vksift_ext_getVerifyTime(vksift_Instance instance) { return timer_read(instance, T_VERIFY); }
