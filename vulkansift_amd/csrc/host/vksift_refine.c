/*
 * vksift_refine.c — refit of the verified homographies on their inliers (vksift_ext_refineHomography and its accessors). No counterpart in
 * the reference: its callers download matches, features and masks and refit on the CPU. It reads what the last vksift_ext_verifyHomography
 * left on the device (the correspondences, the records, the masks) and keeps results of its own. Same contract as the guided matching
 * (vksift_guided.c): queued on the instance stream, the pairs' buffers busy, the accessors wait.
 */
#include "vksift_internal.h"

#define REFINE_FN "vksift_ext_refineHomography()"
#define REFINE_RES_WORDS 13u /* sizeof(vksift_ext_RefinedHomography) / 4 */
#define REFINE_MAX_ROUNDS 8u

_Static_assert(sizeof(vksift_ext_RefinedHomography) == 4u * REFINE_RES_WORDS, "vksift_ext_RefinedHomography is the kernel's 13-word result record");

/* masks and records of batch_cap pairs, allocated by the first refinement (the strides are the verification's, which has run) */
static bool ensure_refine_scratch(vksift_Instance inst)
{
  const uint32_t bc = inst->batch_cap;
  const bool ok = mem_ensure(&inst->d_rmask, inst->vmask_slot_stride * bc, MEM_DEVICE) && mem_ensure(&inst->d_rres, sizeof(uint32_t) * REFINE_RES_WORDS * bc, MEM_DEVICE) &&
                  mem_ensure(&inst->h_rres, sizeof(uint32_t) * REFINE_RES_WORDS * bc, MEM_PINNED);
  for (int i = 0; i < 2; i++)
    if (!inst->ev_r[i])
      inst->ev_r[i] = vksift_hip_event_create();
  return ok && inst->ev_r[0] && inst->ev_r[1];
}

void vksift_ext_refineHomography(vksift_Instance instance, uint32_t nb_rounds, float threshold_px)
{
  vksift_Instance inst = instance;
  bool range_open = false;
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const uint32_t count = inst->verify_slots_used;
  /* the squared threshold the launch forms (guided matching's) has to be a positive finite number too */
  const float ts = threshold_px * (1.0f / 8192.0f), t2 = (ts * ts) * 67108864.0f;
  if (count == 0 || nb_rounds == 0 || nb_rounds > REFINE_MAX_ROUNDS || !(threshold_px > 0.f) || !isfinite(threshold_px) || !(t2 > 0.f) || !isfinite(t2))
  {
    logError(LOG_TAG, REFINE_FN " error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  if (!ensure_refine_scratch(inst))
  {
    logError(LOG_TAG, REFINE_FN " error: out of device memory for the refinement's results.");
    goto gpu_error;
  }
  if (inst->profiling)
    vksift_hip_event_record(inst->ev_r[0], inst->stream);
  vksift_hip_range_push("Refinement");
  range_open = true;
  /* d_corr holds the correspondences of these pairs whichever model was verified last: both verifications gather the same ones */
  HIP_CHECK(vksift_hip_refit_homography(inst->d_corr, inst->filtered_slot_stride, inst->d_filtered_n, 1, inst->cfg.max_nb_sift_per_buffer, count,
                                        (const uint8_t *)inst->d_vres, inst->d_vmask, inst->vmask_slot_stride, nb_rounds, threshold_px, (uint8_t *)inst->d_rres,
                                        inst->d_rmask, inst->stream),
            "homography refit");
  HIP_CHECK(vksift_hip_post_words(inst->h_rres, inst->d_rres, (size_t)REFINE_RES_WORDS * count, inst->stream), "refinement read-back");
  vksift_hip_range_pop();
  range_open = false;
  if (inst->profiling)
  {
    vksift_hip_event_record(inst->ev_r[1], inst->stream);
    inst->refine_timing_valid = true;
  }
  HIP_CHECK(match_follow(inst, inst->filt_ids, inst->filt_ids + inst->batch_cap, count), "event record");
  inst->refine_slots_used = count;
  return;
gpu_error:
  if (range_open)
    vksift_hip_range_pop();
  logError(LOG_TAG, REFINE_FN " error: Failed to start the refinement.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_ext_getRefinedHomography(vksift_Instance instance, uint32_t pair, vksift_ext_RefinedHomography *out)
{
  wait_match(instance);
  if (pair >= instance->refine_slots_used || out == NULL)
  {
    logError(LOG_TAG, "vksift_ext_getRefinedHomography() error: invalid input.");
    instance->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  memcpy(out, instance->h_rres + (size_t)REFINE_RES_WORDS * pair, sizeof(uint32_t) * REFINE_RES_WORDS);
}

void vksift_ext_downloadRefinedInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask)
{
  vksift_Instance inst = instance;
  wait_match(inst);
  if (pair >= inst->refine_slots_used)
  {
    logError(LOG_TAG, "vksift_ext_downloadRefinedInlierMask() error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  const uint32_t n = inst->h_filtered_n[pair];
  if (n > 0)
  {
    HIP_CHECK(vksift_hip_memcpy_d2h(mask, inst->d_rmask + (uint64_t)pair * inst->vmask_slot_stride, n, inst->dl_stream), "refined inlier mask read-back");
    HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "refined inlier mask read-back");
  }
  return;
gpu_error:
  logError(LOG_TAG, "vksift_ext_downloadRefinedInlierMask() error when downloading the inlier mask from GPU memory.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

float vksift_ext_getRefineTime(vksift_Instance instance)
{
  defer_sync(instance);
  if (!instance->profiling || !instance->refine_timing_valid)
    return -1.f;
  vksift_hip_set_device(instance->device);
  wait_all(instance);
  return vksift_hip_event_elapsed_ms(instance->ev_r[0], instance->ev_r[1]);
}
