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
  const uint32_t nbuf = inst->cfg.sift_buffer_count;
  if (count == 0 || count > VKSIFT_HIP_GATHER_SLOTS || first_gpu_buffer_id >= nbuf || count > nbuf - first_gpu_buffer_id || max_features == 0)
  {
    logError(LOG_TAG, "vksift_ext_keepStrongestFeatures() error: invalid input.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  /* pack launches of a packed download that went straight to the caller's memory may still read the records on the download stream */
  if (inst->dl_valid && inst->dl_direct)
    HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), "download stream synchronisation");
  (void)detect_running(inst); /* polls the detections in flight: counts_valid() is up to date */
  uint32_t ids[VKSIFT_HIP_GATHER_SLOTS];
  bool known_changed[VKSIFT_HIP_GATHER_SLOTS]; /* the host knows that the buffer holds more than max_features (its cache entry will be rewritten) */
  for (uint32_t i = 0; i < count; i++)
  {
    ids[i] = first_gpu_buffer_id + i;
    const BufferInfo *b = &inst->bufs[ids[i]];
    known_changed[i] = (b->nb_sections == 0 || counts_valid(inst, ids[i])) && rows_bound(inst, ids[i]) > max_features;
  }
  HIP_CHECK(stage_begin(inst, &frame, T_BUDGET, "KeepStrongest"), "timer start"); /* (nothing can fail between here and the sequence number) */
  take_sequence(inst, first_gpu_buffer_id, count);
  /* with the matcher's cache in place the launch leaves the selected buffer's entry as the gather pass would */
  const bool cache = inst->d_cache_desc && inst->d_cache_norm;
  uint8_t *const c_desc = cache ? inst->d_cache_desc : NULL;
  uint32_t *const c_norm = cache ? inst->d_cache_norm : NULL, *const c_n = cache ? inst->d_cache_n : NULL;
  for (uint32_t i0 = 0, i1; i0 < count; i0 = i1)
  {
    /* one launch per run of buffers that share a section layout (always all of them after a batched detection) */
    BufferInfo *b = &inst->bufs[ids[i0]];
    for (i1 = i0 + 1; i1 < count && same_layout(b, &inst->bufs[ids[i1]]);)
      i1++;
    if (b->nb_sections == 0)
    {
      /* uploaded: one dense run whose length the host knows, and keeps */
      const uint32_t zero_off = 0, n = b->nb_stored;
      HIP_CHECK(vksift_hip_keep_strongest(inst->d_feats, inst->buf_stride, ids + i0, i1 - i0, 1, &zero_off, &n, &n, NULL, 0, NULL, max_features, 2u, c_desc,
                                          inst->desc_slot_stride, c_norm, inst->cache_norm_stride, c_n, 1, inst->stream),
                "feature selection");
      for (uint32_t k = i0; k < i1; k++)
        inst->bufs[ids[k]].nb_stored = n < max_features ? n : max_features;
    }
    else
      HIP_CHECK(vksift_hip_keep_strongest(inst->d_feats, inst->buf_stride, ids + i0, i1 - i0, b->nb_sections, b->sec_off, b->sec_cap, NULL, inst->d_found,
                                          VKSIFT_MAX_OCTAVES, inst->h_found, max_features, 2u, c_desc, inst->desc_slot_stride, c_norm, inst->cache_norm_stride, c_n,
                                          1, inst->stream),
                "feature selection");
    /* A buffer the launch leaves alone keeps its entry, valid or not. One it selects from has a valid entry afterwards (in stream order in front of
     * every matching queued from here on) if there is a cache; the host can say so only where it knows the count: elsewhere an entry that was not
     * valid stays marked so, and the next matching gathers it. */
    for (uint32_t k = i0; k < i1; k++)
      if (known_changed[k])
        inst->cache_valid[ids[k]] = cache;
      else if (!cache)
        inst->cache_valid[ids[k]] = false;
  }
  (void)stage_end(inst, &frame, NULL, NULL, 0); /* no pairs: the call ends on its detection-ring event instead */
  HIP_CHECK(vksift_hip_event_record(inst->det_ring[inst->det_seq % VKSIFT_DETECT_RING].ev, inst->stream), "event record");
  return;
gpu_error:
  if (stage_abort(&frame)) /* the buffers carry the new sequence number: its event stands behind whatever part of the call was queued */
    (void)vksift_hip_event_record(inst->det_ring[inst->det_seq % VKSIFT_DETECT_RING].ev, inst->stream);
  logError(LOG_TAG, "vksift_ext_keepStrongestFeatures() error: Failed to start the feature selection.");
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

float vksift_ext_getKeepStrongestTime(vksift_Instance instance) { return timer_read(instance, T_BUDGET); }
