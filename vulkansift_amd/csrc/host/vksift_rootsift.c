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
  const uint32_t nbuf = inst->cfg.sift_buffer_count;
  if (count == 0 || count > VKSIFT_HIP_GATHER_SLOTS || first_gpu_buffer_id >= nbuf || count > nbuf - first_gpu_buffer_id)
  {
    logError(LOG_TAG, "vksift_ext_convertToRootSift() error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  /* pack launches of a packed download that went straight to the caller's memory may still read the records on the download stream */
  if (inst->dl_valid && inst->dl_direct)
    HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "download stream synchronisation");
  (void)detect_running(inst); /* polls the detections in flight: rows_bound() uses the counts that have arrived */
  uint32_t ids[VKSIFT_HIP_GATHER_SLOTS], bound[VKSIFT_HIP_GATHER_SLOTS];
  for (uint32_t i = 0; i < count; i++)
  {
    ids[i] = first_gpu_buffer_id + i;
    bound[i] = rows_bound(inst, ids[i]); /* (before the new sequence number makes it the capacity bound) */
  }
  HIP_CHECK(stage_begin(inst, &frame, T_ROOTSIFT, "ConvertToRootSift"), "timer start"); /* (nothing can fail between here and the sequence number) */
  /* the count of placed keypoints (vksift_ext_getPlacedKeypointsNumber) is still true of a converted buffer: it follows it to the new sequence number */
  for (uint32_t i = 0; i < count && inst->placed_seq; i++)
    if (inst->bufs[ids[i]].seq != 0 && inst->placed_seq[ids[i]] == inst->bufs[ids[i]].seq)
      inst->placed_seq[ids[i]] = inst->det_seq + 1u;
  take_sequence(inst, first_gpu_buffer_id, count);
  /* with the matcher's cache in place the launch leaves the converted buffer's entry as the gather pass would */
  const bool cache = inst->d_cache_desc && inst->d_cache_norm;
  uint8_t *const c_desc = cache ? inst->d_cache_desc : NULL;
  uint32_t *const c_norm = cache ? inst->d_cache_norm : NULL, *const c_n = cache ? inst->d_cache_n : NULL;
  for (uint32_t i0 = 0, i1; i0 < count; i0 = i1)
  {
    /* one launch per run of buffers that share a section layout (always all of them after a batched detection) */
    const BufferInfo *b = &inst->bufs[ids[i0]];
    uint32_t max_rows = bound[i0];
    for (i1 = i0 + 1; i1 < count && same_layout(b, &inst->bufs[ids[i1]]); i1++)
      max_rows = bound[i1] > max_rows ? bound[i1] : max_rows;
    if (b->nb_sections == 0)
    {
      /* uploaded: one dense run whose length the host knows */
      const uint32_t zero_off = 0, n = b->nb_stored;
      HIP_CHECK(vksift_hip_root_descriptors(inst->d_feats, inst->buf_stride, ids + i0, i1 - i0, 1, &zero_off, &n, &n, NULL, 0, max_rows, 2u, c_desc,
                                            inst->desc_slot_stride, c_norm, inst->cache_norm_stride, c_n, 1, inst->stream),
                "descriptor conversion");
    }
    else
      HIP_CHECK(vksift_hip_root_descriptors(inst->d_feats, inst->buf_stride, ids + i0, i1 - i0, b->nb_sections, b->sec_off, b->sec_cap, NULL, inst->d_found,
                                            VKSIFT_MAX_OCTAVES, max_rows, 2u, c_desc, inst->desc_slot_stride, c_norm, inst->cache_norm_stride, c_n, 1,
                                            inst->stream),
                "descriptor conversion");
    /* Unlike the budget, which leaves a buffer below it alone, the launch rewrites every buffer it names, whatever its count: with a cache the
     * entry is valid afterwards (in stream order in front of every matching queued from here on) and the host knows it; without one, an entry
     * there may have been describes the old rows, and the next matching gathers it. */
    for (uint32_t k = i0; k < i1; k++)
      inst->cache_valid[ids[k]] = cache;
  }
  (void)stage_end(inst, &frame, NULL, NULL, 0); /* no pairs: the call ends on its detection-ring event instead */
  HIP_CHECK(vksift_hip_event_record(inst->det_ring[inst->det_seq % VKSIFT_DETECT_RING].ev, inst->stream), "event record");
  return;
gpu_error:
  if (stage_abort(&frame)) /* the buffers carry the new sequence number: its event stands behind whatever part of the call was queued */
    (void)vksift_hip_event_record(inst->det_ring[inst->det_seq % VKSIFT_DETECT_RING].ev, inst->stream);
  logError(LOG_TAG, "vksift_ext_convertToRootSift() error: Failed to start the descriptor conversion.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

float vksift_ext_getRootSiftTime(vksift_Instance instance) { return timer_read(instance, T_ROOTSIFT); }
