/*
 * vksift_strongest.c — the feature budget (vksift_ext_keepStrongestFeatures): each SIFT buffer of a range keeps its N strongest features, selected
 * and compacted on the device (hip/strongest.hip). No counterpart in the reference, whose only limit is the capacity of a buffer's sections; its
 * callers download, sort and upload. Same contract as a detection: queued on the instance stream, the buffers pending until it has run.
 */
#include "vksift_internal.h"

void vksift_ext_keepStrongestFeatures(vksift_Instance instance, uint32_t first_gpu_buffer_id, uint32_t count, uint32_t max_features)
{
  vksift_Instance inst = instance;
  StageFrame frame = {0};
  vksift_hip_set_device(inst->device);
  defer_sync(inst); /* staged plain detections are launched first */
  if (!inplace_range_valid(inst, first_gpu_buffer_id, count) || max_features == 0)
  {
    logError(LOG_TAG, "vksift_ext_keepStrongestFeatures() error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  uint32_t ids[VKSIFT_HIP_GATHER_SLOTS];
  HIP_CHECK(inplace_begin(inst, first_gpu_buffer_id, count, ids), "download stream synchronisation");
  bool known_changed[VKSIFT_HIP_GATHER_SLOTS]; /* the host knows that the buffer holds more than max_features (its cache entry will be rewritten) */
  for (uint32_t i = 0; i < count; i++)
    known_changed[i] = (inst->bufs[ids[i]].nb_sections == 0 || counts_valid(inst, ids[i])) && rows_bound(inst, ids[i]) > max_features;
  HIP_CHECK(stage_begin(inst, &frame, T_BUDGET, "KeepStrongest"), "timer start"); /* (nothing can fail between here and the sequence number) */
  take_sequence(inst, first_gpu_buffer_id, count);
  /* with the matcher's cache in place the launch leaves the selected buffer's entry as the gather pass would */
  const CacheBlocks cache = cache_blocks(inst);
  LayoutRun run;
  for (uint32_t pos = 0; next_layout_run(inst->bufs, ids, count, NULL, &pos, &run);)
  {
    HIP_CHECK(vksift_hip_keep_strongest(inst->d_feats, inst->buf_stride, run.ids, run.n, run.nsec, run.off, run.cap, run.fixed, run.fixed ? NULL : inst->d_found,
                                        run.found_stride, run.fixed ? NULL : inst->h_found, max_features, 2u, cache.desc, inst->desc_slot_stride, cache.norm,
                                        inst->cache_norm_stride, cache.n, 1, inst->stream),
              "feature selection");
    /* A buffer the launch leaves alone keeps its entry, valid or not. One it selects from has a valid entry afterwards (in stream order in front of
     * every matching queued from here on) if there is a cache; the host can say so only where it knows the count: elsewhere an entry that was not
     * valid stays marked so, and the next matching gathers it. An uploaded buffer's length the host knows, and keeps. */
    const bool *changed = known_changed + (run.ids - ids);
    for (uint32_t k = 0; k < run.n; k++)
    {
      BufferInfo *b = &inst->bufs[run.ids[k]];
      if (run.fixed)
        b->nb_stored = b->nb_stored < max_features ? b->nb_stored : max_features;
      if (changed[k])
        inst->cache_valid[run.ids[k]] = cache.desc != NULL;
      else if (!cache.desc)
        inst->cache_valid[run.ids[k]] = false;
    }
  }
  HIP_CHECK(inplace_end(inst, &frame), "event record");
  return;
gpu_error:
  inplace_fail(inst, &frame, "vksift_ext_keepStrongestFeatures() error: Failed to start the feature selection.");
}

float vksift_ext_getKeepStrongestTime(vksift_Instance instance) { return timer_read(instance, T_BUDGET); }
