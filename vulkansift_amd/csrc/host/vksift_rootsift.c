/*
 * vksift_rootsift.c — RootSIFT descriptors (vksift_ext_convertToRootSift): the descriptors of every SIFT buffer of a range are converted in place on
 * the device (hip/rootsift.hip). No counterpart in the reference, which has no such mode; its callers download, convert on the CPU and upload. Same
 * contract as a detection and as the feature budget (vksift_strongest.c): queued on the instance stream, the buffers pending until it has run.
 */
#include "vksift_internal.h"

void vksift_ext_convertToRootSift(vksift_Instance instance, uint32_t first_gpu_buffer_id, uint32_t count)
{
  vksift_Instance inst = instance;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst); /* staged plain detections are launched first */
  if (!inplace_range_valid(inst, first_gpu_buffer_id, count))
  {
    logError(LOG_TAG, "vksift_ext_convertToRootSift() error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  uint32_t ids[VKSIFT_HIP_GATHER_SLOTS], bound[VKSIFT_HIP_GATHER_SLOTS];
  HIP_CHECK(inplace_begin(inst, first_gpu_buffer_id, count, ids), "download stream synchronisation");
  for (uint32_t i = 0; i < count; i++)
    bound[i] = rows_bound(inst, ids[i]); /* (before the new sequence number makes it the capacity bound) */
  HIP_CHECK(stage_begin(inst, &frame, T_ROOTSIFT, "ConvertToRootSift"), "timer start"); /* (nothing can fail between here and the sequence number) */
  /* the count of placed keypoints (vksift_ext_getPlacedKeypointsNumber) is still true of a converted buffer: it follows it to the new sequence number */
  for (uint32_t i = 0; i < count && inst->placed_seq; i++)
    if (inst->bufs[ids[i]].seq != 0 && inst->placed_seq[ids[i]] == inst->bufs[ids[i]].seq)
      inst->placed_seq[ids[i]] = inst->det_seq + 1u;
  take_sequence(inst, first_gpu_buffer_id, count);
  /* with the matcher's cache in place the launch leaves the converted buffer's entry as the gather pass would */
  const CacheBlocks cache = cache_blocks(inst);
  LayoutRun run;
  for (uint32_t pos = 0; next_layout_run(inst->bufs, ids, count, bound, &pos, &run);)
  {
    HIP_CHECK(vksift_hip_root_descriptors(inst->d_feats, inst->buf_stride, run.ids, run.n, run.nsec, run.off, run.cap, run.fixed, run.fixed ? NULL : inst->d_found,
                                          run.found_stride, run.max_rows, 2u, cache.desc, inst->desc_slot_stride, cache.norm, inst->cache_norm_stride, cache.n, 1,
                                          inst->stream),
              "descriptor conversion");
    /* Unlike the budget, which leaves a buffer below it alone, the launch rewrites every buffer it names, whatever its count: with a cache the
     * entry is valid afterwards (in stream order in front of every matching queued from here on) and the host knows it; without one, an entry
     * there may have been describes the old rows, and the next matching gathers it. */
    for (uint32_t k = 0; k < run.n; k++)
      inst->cache_valid[run.ids[k]] = cache.desc != NULL;
  }
  HIP_CHECK(inplace_end(inst, &frame), "event record");
  return;
gpu_error:
  inplace_fail(inst, &frame, "vksift_ext_convertToRootSift() error: Failed to start the descriptor conversion.");
}

float vksift_ext_getRootSiftTime(vksift_Instance instance) { return timer_read(instance, T_ROOTSIFT); }
