/*
 * vksift_defer.c — deferred submission of vksift_detectFeatures (vksift_internal.h: defer_enabled) over vulkansift.c:315-344
 */
#include "vksift_internal.h"

/* the staged images as ONE batched detection. Failures are reported through the error callback of whichever call got here. */
void flush_deferred(vksift_Instance inst)
{
  const uint32_t n = inst->pend_n;
  if (n == 0)
    return;
  inst->pend_n = 0;
  inst->defer_batches++;
  inst->defer_images += n;
  vksift_hip_set_device(inst->device);
  detect_impl(inst, NULL, NULL, true, n, inst->pend_w, inst->pend_h, inst->pend_first, "vksift_detectFeatures()");
}

/* true: the image was staged (and the batch launched if that filled it); false: the caller launches it the direct way */
static bool defer_detect(vksift_Instance inst, const uint8_t *image, uint32_t w, uint32_t h, uint32_t buf)
{
  if (inst->pend_n)
  {
    /* a batch is one resolution into consecutive buffers; a buffer named twice keeps the order of its two detections */
    if (buf != inst->pend_first + inst->pend_n || w != inst->pend_w || h != inst->pend_h)
      flush_deferred(inst);
  }
  else if (inst->defer_grow && inst->det_cap < inst->defer_max)
  {
    /* the previous batch filled the capacity: twice as much for this one (the blocks follow what the caller does: an instance
     * with 1000 SIFT buffers whose caller detects two images at a time holds the scratch of two) */
    uint32_t cap = inst->det_cap * 2u;
    cap = cap > inst->defer_max ? inst->defer_max : cap;
    /* ... within a third of what the device has left */
    const uint64_t per_image = pyr_texel_bytes(inst) * inst->pyr_img_stride * inst->pyr_nbuf + 12u * inst->seg_cap + 8u * inst->cand_cap +
                               2u * (uint64_t)inst->max_image_size + (4u * VKSIFT_HIP_MAX_ORI + 4u) * inst->ori_cap;
    const uint64_t room = vksift_hip_device_free_mem() / 3u;
    inst->defer_grow = false;
    if ((uint64_t)(cap - inst->det_cap) * per_image > room || resize_detect_scratch(inst, NULL, cap) != 0)
      inst->defer_max = inst->det_cap; /* this is as far as it goes */
  }
  if (inst->det_cap < 2u || inst->h_input == NULL)
  {
    /* a single-image instance: room for two first (then doubling, see above). The second call of a run pays for it, once. */
    if (inst->h_input == NULL || resize_detect_scratch(inst, NULL, 2u) != 0)
    {
      inst->defer_enabled = false;
      return false;
    }
  }
  if (inst->pend_n == 0)
  {
    if (inst->staging_pending)
    {
      if (vksift_hip_event_sync(inst->ev_staging) != 0)
        return false;
      inst->staging_pending = false;
    }
    inst->pend_first = buf, inst->pend_w = w, inst->pend_h = h;
  }
  memcpy(inst->h_input + (size_t)inst->pend_n * w * h, image, (size_t)w * h);
  inst->pend_n++;
  const uint32_t full = inst->det_cap < inst->defer_max ? inst->det_cap : inst->defer_max;
  if (inst->pend_n >= full)
  {
    inst->defer_grow = inst->det_cap < inst->defer_max;
    flush_deferred(inst);
  }
  else if (inst->defer_chunk && inst->pend_n >= inst->defer_chunk && !detect_running(inst))
  {
    /* an idle GPU and a worthwhile number of staged images: launch them now, beside the staging of the rest of the caller's run (the
     * strictly serial pattern "detect into N buffers, then read them" otherwise leaves the GPU idle for the whole staging phase and the host
     * idle for the whole detection). With a detection in flight — the pattern with two buffer sets — nothing is launched early: whole runs
     * make the better batches. */
    inst->defer_grow = inst->det_cap < inst->defer_max; /* the caller's runs are longer than this chunk */
    flush_deferred(inst);
  }
  return true;
}

void vksift_detectFeatures(vksift_Instance instance, const uint8_t *image_data, const uint32_t image_width, const uint32_t image_height,
                           const uint32_t gpu_buffer_id)
{
  vksift_Instance inst = instance;
  const uint8_t *imgs[1] = {image_data};
  vksift_hip_set_device(inst->device);
  /* The first detection after any other call is launched at once — detect + read, the reference's own loop
   * (src/perf/wrappers/vulkansift_wrapper.cpp:30-33), and the two-buffer ping-pong keep their path and their latency — unless the
   * caller's last run of detect calls held several. From the second call of a run on the images are staged and go as one batch. */
  const bool run = inst->epoch_detects > 0 || inst->batch_mode;
  inst->epoch_detects++;
  if (inst->defer_enabled && (run || inst->pend_n) && !inst->profiling && image_data != NULL &&
      detect_args_valid(inst, 1, image_width, image_height, gpu_buffer_id, false))
  {
    if (defer_detect(inst, image_data, image_width, image_height, gpu_buffer_id))
      return;
  }
  /* invalid arguments take the direct path too: it reports them */
  if (inst->pend_n)
    flush_deferred(inst);
  detect_impl(inst, imgs, NULL, false, 1, image_width, image_height, gpu_buffer_id, "vksift_detectFeatures()");
}
