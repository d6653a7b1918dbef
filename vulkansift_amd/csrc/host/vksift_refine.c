/*
 * vksift_refine.c — refit of the verified models on their inliers (vksift_ext_refineHomography, vksift_ext_refineFundamental and their
 * accessors). No counterpart in the reference: its callers download matches, features and masks and refit on the CPU. A refinement reads
 * what the last verification of its model left on the device (the correspondences, the records, the masks) and keeps results of its own.
 * A model (RefineModel) is its kernel entry, the verification's records and masks it starts from and its own results; everything else here
 * serves both. Same contract as the guided matching (vksift_guided.c): queued on the instance stream, the pairs' buffers busy, the
 * accessors wait.
 */
#include "vksift_internal.h"

#define REFINE_RES_WORDS 13u /* sizeof(vksift_ext_RefinedHomography) / 4 == sizeof(vksift_ext_RefinedFundamental) / 4 */
#define REFINE_MAX_ROUNDS 8u

_Static_assert(sizeof(vksift_ext_RefinedHomography) == 4u * REFINE_RES_WORDS, "vksift_ext_RefinedHomography is the kernel's 13-word result record");
_Static_assert(sizeof(vksift_ext_RefinedFundamental) == 4u * REFINE_RES_WORDS, "vksift_ext_RefinedFundamental is the kernel's 13-word result record");

typedef int (*RefitFn)(const float *, uint64_t, const uint32_t *, uint32_t, uint32_t, uint32_t, const uint8_t *, const uint8_t *, uint64_t, uint32_t, float, uint8_t *,
                       uint8_t *, vksift_hip_stream);

/* what differs between the models: the launcher, the verification it starts from, and where this instance keeps the model's refined results */
typedef struct
{
  const char *entry, *get_entry, *mask_entry;
  RefitFn refit;
  const uint32_t *verified_slots; /* pairs of the model's last verification */
  uint32_t *const *d_start_res;   /* its records ... */
  uint8_t *const *d_start_mask;   /* ... and masks */
  uint8_t **d_mask;
  uint32_t **d_res, **h_res;
  uint32_t *slots_used;
  bool *timing_valid;
  vksift_hip_event *ev; /* [2] */
} RefineModel;

static RefineModel model_h(vksift_Instance inst)
{
  return (RefineModel){"vksift_ext_refineHomography", "vksift_ext_getRefinedHomography", "vksift_ext_downloadRefinedInlierMask", vksift_hip_refit_homography,
                       &inst->verify_slots_used, &inst->d_vres, &inst->d_vmask, &inst->d_rmask, &inst->d_rres, &inst->h_rres, &inst->refine_slots_used,
                       &inst->refine_timing_valid, inst->ev_r};
}

static RefineModel model_f(vksift_Instance inst)
{
  return (RefineModel){"vksift_ext_refineFundamental", "vksift_ext_getRefinedFundamental", "vksift_ext_downloadRefinedFundamentalInlierMask",
                       vksift_hip_refit_fundamental, &inst->verify_f_slots_used, &inst->d_fres, &inst->d_fmask, &inst->d_rfmask, &inst->d_rfres, &inst->h_rfres,
                       &inst->refine_f_slots_used, &inst->refine_f_timing_valid, inst->ev_rf};
}

/* masks and records of batch_cap pairs, allocated by the model's first refinement (the strides are the verification's, which has run) */
static bool ensure_refine_scratch(vksift_Instance inst, const RefineModel *m)
{
  const uint32_t bc = inst->batch_cap;
  const bool ok = mem_ensure(m->d_mask, inst->vmask_slot_stride * bc, MEM_DEVICE) && mem_ensure(m->d_res, sizeof(uint32_t) * REFINE_RES_WORDS * bc, MEM_DEVICE) &&
                  mem_ensure(m->h_res, sizeof(uint32_t) * REFINE_RES_WORDS * bc, MEM_PINNED);
  for (int i = 0; i < 2; i++)
    if (!m->ev[i])
      m->ev[i] = vksift_hip_event_create();
  return ok && m->ev[0] && m->ev[1];
}

static void refine(vksift_Instance inst, const RefineModel *m, uint32_t nb_rounds, float threshold_px)
{
  bool range_open = false;
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const uint32_t count = *m->verified_slots;
  /* the squared threshold the launch forms (guided matching's) has to be a positive finite number too */
  const float ts = threshold_px * (1.0f / 8192.0f), t2 = (ts * ts) * 67108864.0f;
  if (count == 0 || nb_rounds == 0 || nb_rounds > REFINE_MAX_ROUNDS || !(threshold_px > 0.f) || !isfinite(threshold_px) || !(t2 > 0.f) || !isfinite(t2))
  {
    logError(LOG_TAG, "%s() error: invalid input.", m->entry);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!ensure_refine_scratch(inst, m))
  {
    logError(LOG_TAG, "%s() error: out of device memory for the refinement's results.", m->entry);
    goto gpu_error;
  }
  if (inst->profiling)
    vksift_hip_event_record(m->ev[0], inst->stream);
  vksift_hip_range_push("Refinement");
  range_open = true;
  /* d_corr holds the correspondences of these pairs whichever model was verified last: both verifications gather the same ones */
  HIP_CHECK(m->refit(inst->d_corr, inst->filtered_slot_stride, inst->d_filtered_n, 1, inst->cfg.max_nb_sift_per_buffer, count, (const uint8_t *)*m->d_start_res,
                     *m->d_start_mask, inst->vmask_slot_stride, nb_rounds, threshold_px, (uint8_t *)*m->d_res, *m->d_mask, inst->stream),
            "refit");
  HIP_CHECK(vksift_hip_post_words(*m->h_res, *m->d_res, (size_t)REFINE_RES_WORDS * count, inst->stream), "refinement read-back");
  vksift_hip_range_pop();
  range_open = false;
  if (inst->profiling)
  {
    vksift_hip_event_record(m->ev[1], inst->stream);
    *m->timing_valid = true;
  }
  HIP_CHECK(match_follow(inst, inst->filt_ids, inst->filt_ids + inst->batch_cap, count), "event record");
  *m->slots_used = count;
  return;
gpu_error:
  if (range_open)
    vksift_hip_range_pop();
  logError(LOG_TAG, "%s() error: Failed to start the refinement.", m->entry);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

static void get_result(vksift_Instance inst, const RefineModel *m, uint32_t pair, void *out)
{
  wait_match(inst);
  if (pair >= *m->slots_used || out == NULL)
  {
    logError(LOG_TAG, "%s() error: invalid input.", m->get_entry);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  memcpy(out, *m->h_res + (size_t)REFINE_RES_WORDS * pair, sizeof(uint32_t) * REFINE_RES_WORDS);
}

static void download_mask(vksift_Instance inst, const RefineModel *m, uint32_t pair, uint8_t *mask)
{
  wait_match(inst);
  if (pair >= *m->slots_used)
  {
    logError(LOG_TAG, "%s() error: invalid input.", m->mask_entry);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  const uint32_t n = inst->h_filtered_n[pair];
  if (n > 0)
  {
    HIP_CHECK(vksift_hip_memcpy_d2h(mask, *m->d_mask + (uint64_t)pair * inst->vmask_slot_stride, n, inst->dl_stream), "refined inlier mask read-back");
    HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "refined inlier mask read-back");
  }
  return;
gpu_error:
  logError(LOG_TAG, "%s() error when downloading the inlier mask from GPU memory.", m->mask_entry);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

static float refine_time(vksift_Instance inst, const RefineModel *m)
{
  defer_sync(inst);
  if (!inst->profiling || !*m->timing_valid)
    return -1.f;
  vksift_hip_set_device(inst->device);
  wait_all(inst);
  return vksift_hip_event_elapsed_ms(m->ev[0], m->ev[1]);
}

void vksift_ext_refineHomography(vksift_Instance instance, uint32_t nb_rounds, float threshold_px)
{
  const RefineModel m = model_h(instance);
  refine(instance, &m, nb_rounds, threshold_px);
}

void vksift_ext_getRefinedHomography(vksift_Instance instance, uint32_t pair, vksift_ext_RefinedHomography *out)
{
  const RefineModel m = model_h(instance);
  get_result(instance, &m, pair, out);
}

void vksift_ext_downloadRefinedInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask)
{
  const RefineModel m = model_h(instance);
  download_mask(instance, &m, pair, mask);
}

float vksift_ext_getRefineTime(vksift_Instance instance)
{
  const RefineModel m = model_h(instance);
  return refine_time(instance, &m);
}

void vksift_ext_refineFundamental(vksift_Instance instance, uint32_t nb_rounds, float threshold_px)
{
  const RefineModel m = model_f(instance);
  refine(instance, &m, nb_rounds, threshold_px);
}

void vksift_ext_getRefinedFundamental(vksift_Instance instance, uint32_t pair, vksift_ext_RefinedFundamental *out)
{
  const RefineModel m = model_f(instance);
  get_result(instance, &m, pair, out);
}

void vksift_ext_downloadRefinedFundamentalInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask)
{
  const RefineModel m = model_f(instance);
  download_mask(instance, &m, pair, mask);
}

float vksift_ext_getRefineFundamentalTime(vksift_Instance instance)
{
  const RefineModel m = model_f(instance);
  return refine_time(instance, &m);
}
