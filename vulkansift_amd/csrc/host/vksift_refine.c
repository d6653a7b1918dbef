/*
 * vksift_refine.c — refit of the verified models on their inliers (vksift_ext_refineHomography, vksift_ext_refineFundamental and their
 * accessors). No counterpart in the reference: its callers download matches, features and masks and refit on the CPU. A refinement reads
 * what the last verification of its model left on the device (the correspondences, the records, the masks) and keeps results of its own.
 * A model (RefineModel) is its kernel entry, the verification's result set it starts from, its own and its timer; everything else here
 * serves both. Same contract as the guided matching (vksift_guided.c): queued on the instance stream, the pairs' buffers busy, the
 * accessors wait (vksift_pairs.c).
 */
#include "vksift_internal.h"

#define REFINE_RES_WORDS 13u /* sizeof(vksift_ext_RefinedHomography) / 4 == sizeof(vksift_ext_RefinedFundamental) / 4 */
#define REFINE_MAX_ROUNDS 8u

_Static_assert(sizeof(vksift_ext_RefinedHomography) == 4u * REFINE_RES_WORDS, "vksift_ext_RefinedHomography is the kernel's 13-word result record");
_Static_assert(sizeof(vksift_ext_RefinedFundamental) == 4u * REFINE_RES_WORDS, "vksift_ext_RefinedFundamental is the kernel's 13-word result record");

typedef int (*RefitFn)(const float *, uint64_t, const uint32_t *, uint32_t, uint32_t, uint32_t, const uint8_t *, const uint8_t *, uint64_t, uint32_t, float, uint8_t *,
                       uint8_t *, vksift_hip_stream);

/* what differs between the models: the names, the launcher, the verification's result set it starts from, its own, and its timer */
typedef struct
{
  const char *entry, *get_entry, *mask_entry;
  RefitFn refit;
  uint32_t verified, set, timer;
} RefineModel;

static const RefineModel model_h = {"vksift_ext_refineHomography", "vksift_ext_getRefinedHomography", "vksift_ext_downloadRefinedInlierMask",
                                    vksift_hip_refit_homography, PR_VERIFY_H, PR_REFINE_H, T_REFINE_H};
static const RefineModel model_f = {"vksift_ext_refineFundamental", "vksift_ext_getRefinedFundamental", "vksift_ext_downloadRefinedFundamentalInlierMask",
                                    vksift_hip_refit_fundamental, PR_VERIFY_F, PR_REFINE_F, T_REFINE_F};

static void refine(vksift_Instance inst, const RefineModel *m, uint32_t nb_rounds, float threshold_px)
{
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const PairResults *filt = &inst->res[PR_FILTERED], *start = &inst->res[m->verified];
  PairResults *own = &inst->res[m->set];
  const uint32_t count = start->slots_used;
  /* the squared threshold the launch forms (guided matching's) has to be a positive finite number too */
  const float ts = threshold_px * (1.0f / 8192.0f), t2 = (ts * ts) * 67108864.0f;
  if (count == 0 || nb_rounds == 0 || nb_rounds > REFINE_MAX_ROUNDS || !(threshold_px > 0.f) || !isfinite(threshold_px) || !(t2 > 0.f) || !isfinite(t2))
  {
    logError(LOG_TAG, "%s() error: invalid input.", m->entry);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  /* masks and records of batch_cap pairs, allocated by the model's first refinement (the mask stride is the verification's, which has run) */
  if (!pair_results_ensure(inst, m->set, REFINE_RES_WORDS, start->stride, 1, PR_FILTERED))
  {
    logError(LOG_TAG, "%s() error: out of device memory for the refinement's results.", m->entry);
    goto gpu_error;
  }
  HIP_CHECK(stage_begin(inst, &frame, m->timer, "Refinement"), "timer start");
  /* d_corr holds the correspondences of these pairs whichever model was verified last: both verifications gather the same ones */
  HIP_CHECK(m->refit(inst->d_corr, filt->stride, filt->d_words, 1, inst->cfg.max_nb_sift_per_buffer, count, (const uint8_t *)start->d_words, start->d_payload,
                     start->stride, nb_rounds, threshold_px, (uint8_t *)own->d_words, own->d_payload, inst->stream),
            "refit");
  own->slots_used = 0; /* the launch replaces the set: not served until the whole sequence has been queued */
  HIP_CHECK(vksift_hip_post_words(own->h_words, own->d_words, (size_t)REFINE_RES_WORDS * count, inst->stream), "refinement read-back");
  HIP_CHECK(stage_end(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count), "event record");
  own->slots_used = count;
  return;
gpu_error:
  stage_fail(inst, &frame, inst->filt_ids, inst->filt_ids + inst->batch_cap, count);
  logError(LOG_TAG, "%s() error: Failed to start the refinement.", m->entry);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

static void get_result(vksift_Instance inst, const RefineModel *m, uint32_t pair, void *out)
{
  const uint32_t *w = pair_words(inst, m->set, pair, out != NULL, m->get_entry);
  if (w)
    memcpy(out, w, sizeof(uint32_t) * REFINE_RES_WORDS);
}

static void download_mask(vksift_Instance inst, const RefineModel *m, uint32_t pair, uint8_t *mask)
{
  pair_download(inst, m->set, pair, mask, m->mask_entry, "refined inlier mask read-back", "the inlier mask");
}

void vksift_ext_refineHomography(vksift_Instance instance, uint32_t nb_rounds, float threshold_px) { refine(instance, &model_h, nb_rounds, threshold_px); }

void vksift_ext_getRefinedHomography(vksift_Instance instance, uint32_t pair, vksift_ext_RefinedHomography *out) { get_result(instance, &model_h, pair, out); }

void vksift_ext_downloadRefinedInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask) { download_mask(instance, &model_h, pair, mask); }

float vksift_ext_getRefineTime(vksift_Instance instance) { return timer_read(instance, T_REFINE_H); }

void vksift_ext_refineFundamental(vksift_Instance instance, uint32_t nb_rounds, float threshold_px) { refine(instance, &model_f, nb_rounds, threshold_px); }

void vksift_ext_getRefinedFundamental(vksift_Instance instance, uint32_t pair, vksift_ext_RefinedFundamental *out) { get_result(instance, &model_f, pair, out); }

void vksift_ext_downloadRefinedFundamentalInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask) { download_mask(instance, &model_f, pair, mask); }

float vksift_ext_getRefineFundamentalTime(vksift_Instance instance) { return timer_read(instance, T_REFINE_F); }
