/*
 * vksift_verify.c — geometric verification of the last filtered matching (vksift_ext_verifyHomography, vksift_ext_verifyFundamental and
 * their accessors). No counterpart in the reference: its callers download matches and features and run a CPU RANSAC per pair. A model
 * (VerifyModel) is its kernel entry, its record size and its own results and masks; everything else here (scratch, pair tables,
 * posting, accessors) serves both.
 */
#include "vksift_internal.h"

#define VERIFY_RES_WORDS 13u   /* sizeof(vksift_ext_Homography) / 4 */
#define VERIFY_F_RES_WORDS 14u /* sizeof(vksift_ext_Fundamental) / 4 */
#define VERIFY_MAX_HYPOTHESES 65536u

_Static_assert(sizeof(vksift_ext_Homography) == 4u * VERIFY_RES_WORDS, "vksift_ext_Homography is the kernel's 13-word result record");
_Static_assert(sizeof(vksift_ext_Fundamental) == 4u * VERIFY_F_RES_WORDS, "vksift_ext_Fundamental is the kernel's 14-word result record");

typedef int (*RansacFn)(const float *, uint64_t, const uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, float, uint64_t, uint8_t *, uint8_t *, uint64_t, uint32_t *,
                        size_t, vksift_hip_stream);

/* what differs between the models: the launcher, the record, and where this instance keeps the model's results */
typedef struct
{
  const char *entry, *get_entry, *mask_entry;
  RansacFn ransac;
  uint32_t res_words;
  uint8_t **d_mask;
  uint32_t **d_res, **h_res;
  uint32_t *slots_used;
  uint32_t *derived_slots_used; /* results computed from this model's records and masks, no longer theirs once it is verified again */
} VerifyModel;

static VerifyModel model_h(vksift_Instance inst)
{
  return (VerifyModel){"vksift_ext_verifyHomography", "vksift_ext_getHomography", "vksift_ext_downloadInlierMask", vksift_hip_ransac_homography, VERIFY_RES_WORDS,
                       &inst->d_vmask, &inst->d_vres, &inst->h_vres, &inst->verify_slots_used, &inst->refine_slots_used};
}

static VerifyModel model_f(vksift_Instance inst)
{
  return (VerifyModel){"vksift_ext_verifyFundamental", "vksift_ext_getFundamental", "vksift_ext_downloadFundamentalInlierMask", vksift_hip_ransac_fundamental,
                       VERIFY_F_RES_WORDS, &inst->d_fmask, &inst->d_fres, &inst->h_fres, &inst->verify_f_slots_used, &inst->refine_f_slots_used};
}

/* correspondences, reduction keys and pair tables of batch_cap pairs, and the masks and results of the model asked for; allocated by the
 * first verification (detect-only and match-only users never pay, and a model that is never asked for costs nothing) */
static bool ensure_verify_scratch(vksift_Instance inst, const VerifyModel *m)
{
  const uint32_t bc = inst->batch_cap;
  inst->vmask_slot_stride = ((uint64_t)inst->cfg.max_nb_sift_per_buffer + 255u) & ~(uint64_t)255u;
  inst->vscratch_u32 = vksift_hip_ransac_scratch_u32(bc, VERIFY_MAX_HYPOTHESES);
  const bool ok = mem_ensure(&inst->d_corr, inst->filtered_slot_stride * bc, MEM_DEVICE) && mem_ensure(m->d_mask, inst->vmask_slot_stride * bc, MEM_DEVICE) &&
                  mem_ensure(m->d_res, sizeof(uint32_t) * m->res_words * bc, MEM_DEVICE) &&
                  mem_ensure(&inst->d_vscratch, sizeof(uint32_t) * inst->vscratch_u32, MEM_DEVICE) &&
                  mem_ensure(m->h_res, sizeof(uint32_t) * m->res_words * bc, MEM_PINNED) &&
                  mem_ensure(&inst->h_vtab, sizeof(uint32_t) * pair_table_words(inst), MEM_PINNED);
  if (!inst->ev_vtab)
    inst->ev_vtab = vksift_hip_event_create();
  for (int i = 0; i < 2; i++)
    if (!inst->ev_v[i])
      inst->ev_v[i] = vksift_hip_event_create();
  return ok && inst->ev_vtab && inst->ev_v[0] && inst->ev_v[1];
}

static void verify(vksift_Instance inst, const VerifyModel *m, uint32_t nb_hypotheses, float threshold_px, uint64_t seed)
{
  bool range_open = false;
  vksift_hip_set_device(inst->device);
  defer_sync(inst);
  const uint32_t count = inst->filtered_slots_used;
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
  if (inst->profiling)
    vksift_hip_event_record(inst->ev_v[0], inst->stream);
  vksift_hip_range_push("Verification");
  range_open = true;
  HIP_CHECK(vksift_hip_gather_correspondences(inst->d_feats, inst->buf_stride, inst->d_found, VKSIFT_MAX_OCTAVES, inst->h_vtab,
                                              pair_layouts(inst, inst->h_vtab), inst->d_filtered, inst->filtered_slot_stride, inst->d_filtered_n,
                                              inst->cfg.max_nb_sift_per_buffer, count, inst->d_corr, inst->filtered_slot_stride, inst->stream),
            "correspondence gather");
  HIP_CHECK(vksift_hip_event_record(inst->ev_vtab, inst->stream), "event record");
  inst->vtab_pending = true;
  *m->derived_slots_used = 0; /* the launch below replaces the records and masks the refinement (vksift_refine.c) was computed from */
  HIP_CHECK(m->ransac(inst->d_corr, inst->filtered_slot_stride, inst->d_filtered_n, 1, inst->cfg.max_nb_sift_per_buffer, count, nb_hypotheses, threshold_px, seed,
                      (uint8_t *)*m->d_res, *m->d_mask, inst->vmask_slot_stride, inst->d_vscratch, inst->vscratch_u32, inst->stream),
            "RANSAC");
  HIP_CHECK(vksift_hip_post_words(*m->h_res, *m->d_res, (size_t)m->res_words * count, inst->stream), "verification read-back");
  vksift_hip_range_pop();
  range_open = false;
  if (inst->profiling)
  {
    vksift_hip_event_record(inst->ev_v[1], inst->stream);
    inst->verify_timing_valid = true;
  }
  HIP_CHECK(match_follow(inst, inst->filt_ids, inst->filt_ids + inst->batch_cap, count), "event record");
  *m->slots_used = count;
  return;
gpu_error:
  if (range_open)
    vksift_hip_range_pop();
  logError(LOG_TAG, "%s() error: Failed to start the verification pipeline.", m->entry);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

static void get_result(vksift_Instance inst, const VerifyModel *m, uint32_t pair, void *out)
{
  wait_match(inst);
  if (pair >= *m->slots_used || out == NULL)
  {
    logError(LOG_TAG, "%s() error: invalid input.", m->get_entry);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  memcpy(out, *m->h_res + (size_t)m->res_words * pair, sizeof(uint32_t) * m->res_words);
}

static void download_mask(vksift_Instance inst, const VerifyModel *m, uint32_t pair, uint8_t *mask)
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
    HIP_CHECK(vksift_hip_memcpy_d2h(mask, *m->d_mask + (uint64_t)pair * inst->vmask_slot_stride, n, inst->dl_stream), "inlier mask read-back");
    HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "inlier mask read-back");
  }
  return;
gpu_error:
  logError(LOG_TAG, "%s() error when downloading the inlier mask from GPU memory.", m->mask_entry);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void vksift_ext_verifyHomography(vksift_Instance instance, uint32_t nb_hypotheses, float threshold_px, uint64_t seed)
{
  const VerifyModel m = model_h(instance);
  verify(instance, &m, nb_hypotheses, threshold_px, seed);
}

void vksift_ext_getHomography(vksift_Instance instance, uint32_t pair, vksift_ext_Homography *out)
{
  const VerifyModel m = model_h(instance);
  get_result(instance, &m, pair, out);
}

void vksift_ext_downloadInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask)
{
  const VerifyModel m = model_h(instance);
  download_mask(instance, &m, pair, mask);
}

void vksift_ext_verifyFundamental(vksift_Instance instance, uint32_t nb_hypotheses, float threshold_px, uint64_t seed)
{
  const VerifyModel m = model_f(instance);
  verify(instance, &m, nb_hypotheses, threshold_px, seed);
}

void vksift_ext_getFundamental(vksift_Instance instance, uint32_t pair, vksift_ext_Fundamental *out)
{
  const VerifyModel m = model_f(instance);
  get_result(instance, &m, pair, out);
}

void vksift_ext_downloadFundamentalInlierMask(vksift_Instance instance, uint32_t pair, uint8_t *mask)
{
  const VerifyModel m = model_f(instance);
  download_mask(instance, &m, pair, mask);
}

float vksift_ext_getVerifyTime(vksift_Instance instance)
{
  defer_sync(instance);
  if (!instance->profiling || !instance->verify_timing_valid)
    return -1.f;
  vksift_hip_set_device(instance->device);
  wait_all(instance);
  return vksift_hip_event_elapsed_ms(instance->ev_v[0], instance->ev_v[1]);
}
