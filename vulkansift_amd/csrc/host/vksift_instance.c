/*
 * vksift_instance.c — instance creation / destruction, the environment switches, synchronisation helpers (vulkansift.c:165-313); the
 * instance's memory, streams and events are vksift_mem.c's
 */
#include "vksift_internal.h"

void set_buffer_sections(vksift_Instance inst, uint32_t buf, uint32_t n_oct, uint32_t w, uint32_t h)
{
  BufferInfo *b = &inst->bufs[buf];
  memset(b->sec_off, 0, sizeof(b->sec_off));
  memset(b->sec_cap, 0, sizeof(b->sec_cap));
  b->is_packed = false;
  b->nb_stored = 0;
  b->nb_sections = n_oct;
  b->in_w = w;
  b->in_h = h;
  vksift_hm_section_caps(inst->cfg.max_nb_sift_per_buffer, n_oct, b->sec_cap);
  uint32_t off = 0;
  for (uint32_t o = 0; o < n_oct; o++)
  {
    b->sec_off[o] = off;
    off += b->sec_cap[o];
  }
}


/* ------------------------------------------------------------------------------------------------ */
/* environment switches                                                                             */
/* ------------------------------------------------------------------------------------------------ */
static bool env_flag(const char *name) /* on unless the value starts with '0' */
{
  const char *e = getenv(name);
  return !(e && e[0] == '0');
}
static uint32_t env_u32(const char *name, uint32_t dflt)
{
  const char *e = getenv(name);
  return e ? (uint32_t)strtoul(e, NULL, 10) : dflt;
}

/* VKSIFT_DEFER          deferred submission of plain detect calls (vksift_internal.h): needs a second SIFT buffer to have anything to
 *   _DEFER_MAX, _CHUNK  batch, and a batch bound (128, at most sift_buffer_count) of at least 2; chunk: 16
 * VKSIFT_PYR_PINGPONG   Overlap mode: the (bandwidth-bound) scale-space construction of detection N+1 runs on its own stream, beside the
 *                       matching queued behind detection N's descriptors (rounds 2-3 also ran it under the descriptors themselves, out of
 *                       a second scale-space buffer: within 1 % in frames/s, and every stage interval measured the contention instead of
 *                       the kernel — vksift_detect.c, enqueue_keypoint_stages: ev_desc_start). With that gate the next scale-space starts
 *                       only when every reader of the previous one is done, so ONE buffer serves (half the memory; and the measured
 *                       placement, place_pyramid_buffers, has to find one fast range, not two). Default: instances created for batches
 *                       of 8 images and more (vksift_ext_createBatchInstance) — a single-image instance keeps the hipGraph replay of
 *                       small detections, which excludes overlapped calls. =0 / 1 forces the mode off / on, =2 is the mode with two
 *                       buffers (rounds 2-5). An instance whose detection capacity grew later (deferred submission) overlaps its batches
 *                       of 8 and more only (overlap_min_count): its single detections keep the forked scale-space and the graph replay
 * VKSIFT_FORK_SCALES    forked scale-space of small detections. One branch stream: two measured no faster in stream order and 10 % slower
 *                       in a replayed graph. (alt_order: consecutive launches of a chain walk the batch in opposite directions, +9 % on
 *                       the chain, round 3)
 * VKSIFT_LDS_CHAIN      the trailing octaves in one launch; "refuse": the chain is attempted and declines (tests of the fallback)
 *   _LDS_CHAIN_MAX      largest plane of the chain (4800 texels, at most 19200)
 * VKSIFT_GRAPH          hipGraph capture + replay of the detection launch sequence. Measured on MI355X / ROCm 7.2: 10 % faster for one
 *                       640x480 image (0.58 vs 0.65 ms), 12 % slower from 1536x1024 up (the graph runs the per-octave branches less
 *                       concurrently than the streams do) -> by default only small workloads are replayed (graph_max_pixels).
 *                       =0 never, =1 always
 * VKSIFT_POST_FEATURES  feature posting (vksift_internal.h: h_post) */
static void read_switches(vksift_Instance inst, const vksift_Config *config, uint32_t batch_cap)
{
  const char *e;
  inst->defer_max = env_u32("VKSIFT_DEFER_MAX", 128u);
  inst->defer_chunk = env_u32("VKSIFT_DEFER_CHUNK", 16u);
  if (inst->defer_max > config->sift_buffer_count)
    inst->defer_max = config->sift_buffer_count;
  inst->defer_enabled = env_flag("VKSIFT_DEFER") && config->sift_buffer_count >= 2u && inst->defer_max >= 2u;
  e = getenv("VKSIFT_PYR_PINGPONG");
  inst->pyr_pingpong = e ? (e[0] == '1' || e[0] == '2') : (batch_cap >= 8u);
  inst->pyr_nbuf = (e && e[0] == '2') ? 2u : 1u;
  inst->overlap_min_count = 1u;
  inst->overlap_forced = e != NULL;
  inst->alt_order = true;
  inst->fork_scales = env_flag("VKSIFT_FORK_SCALES");
  inst->fork_streams = 1;
  inst->fork_max_pixels = (uint64_t)16 << 20;
  e = getenv("VKSIFT_LDS_CHAIN");
  inst->lds_chain = env_flag("VKSIFT_LDS_CHAIN");
  inst->lds_chain_refuse = e && e[0] == 'r';
  inst->lds_chain_max = env_u32("VKSIFT_LDS_CHAIN_MAX", 4800u);
  if (inst->lds_chain_max > 19200u)
    inst->lds_chain_max = 19200u;
  e = getenv("VKSIFT_GRAPH");
  inst->use_graphs = env_flag("VKSIFT_GRAPH");
  inst->graph_max_pixels = (e && e[0] == '1') ? ~(uint64_t)0 : (uint64_t)640 * 480;
  inst->post_enabled = inst->post_on = env_flag("VKSIFT_POST_FEATURES");
}

/* ------------------------------------------------------------------------------------------------ */
/* instance                                                                                         */
/* ------------------------------------------------------------------------------------------------ */
static vksift_Result create_instance(vksift_Instance *instance_ptr, const vksift_Config *config, uint32_t batch_cap)
{
  assert(instance_ptr != NULL);
  assert(*instance_ptr == NULL);
  assert(config != NULL);

  if (!vksift_g_loaded)
  {
    logError(LOG_TAG, "vksift_createInstance() failure: GPU runtime not available. vksift_loadVulkan() must be called before using this function.");
    return VKSIFT_VULKAN_ERROR;
  }
  if (!config_is_valid(config))
  {
    logError(LOG_TAG, "vksift_createInstance() failed: the configuration was rejected (see above).");
    return VKSIFT_INVALID_INPUT_ERROR;
  }
  if (batch_cap == 0 || batch_cap > config->sift_buffer_count)
  {
    logError(LOG_TAG, "vksift_createInstance() failure: batch capacity (%u) must be in [1, sift_buffer_count=%u].", batch_cap, config->sift_buffer_count);
    return VKSIFT_INVALID_INPUT_ERROR;
  }

  vksift_Instance inst = (vksift_Instance)calloc(1, sizeof(struct vksift_Instance_T));
  if (!inst)
    return VKSIFT_VULKAN_ERROR;
  *instance_ptr = inst;
  inst->cfg = *config;
  inst->error_cb = config->on_error_callback_function;
  inst->S = config->nb_scales_per_octave;
  inst->batch_cap = batch_cap;
  inst->det_cap = batch_cap;
  read_switches(inst, config, batch_cap);

  int ndev = vksift_hip_device_count();
  int dev = config->gpu_device_index;
  if (dev < 0)
    dev = 0; /* all MI355X of a node are identical: "best" = first (reference scores by type/VRAM, vulkan_device.c:394-494) */
  if (dev >= ndev)
  {
    logError(LOG_TAG, "vksift_createInstance() failure: gpu_device_index %d but only %d device(s) available", dev, ndev);
    vksift_destroyInstance(instance_ptr);
    return VKSIFT_VULKAN_ERROR;
  }
  inst->device = dev;
  if (vksift_hip_set_device(dev) != 0)
  {
    vksift_destroyInstance(instance_ptr);
    return VKSIFT_VULKAN_ERROR;
  }
  /* the reference's FLOAT16 mode binds R16_SFLOAT images to shaders that declare r32f (undefined in Vulkan); this build defines it:
   * texels stored as IEEE binary16 (round to nearest even), widened exactly on every read, all arithmetic fp32 */
  inst->fp16 = config->pyramid_precision_mode == VKSIFT_PYRAMID_PRECISION_FLOAT16;
  if (config->use_gpu_debug_functions)
    logWarning(LOG_TAG, "use_gpu_debug_functions requested: there is no frame presenter in the HIP build; use rocprofv3 / roctx ranges instead.");

  inst->max_octaves = vksift_hm_max_octaves(config, &inst->max_image_size);
  vksift_hm_blur_taps(config, inst->taps, inst->ntaps);

  /* ---- reserve device memory for the configured maxima (sift_memory.c:133-360 equivalent) ---- */
  const uint32_t side = (uint32_t)ceilf(sqrtf((float)config->input_image_max_size));
  PyrLayout L;
  compute_layout(inst, side, side, &L);
  float fp_tab[DESC_FP_TAB_MAX];
  inst->desc_fp_len = vksift_hm_desc_fp_table(config, fp_tab, DESC_FP_TAB_MAX);
  if (!mem_create(inst, &L))
  {
    logError(LOG_TAG, "vksift_createInstance() failed: device / pinned memory reservation");
    vksift_destroyInstance(instance_ptr);
    return VKSIFT_VULKAN_ERROR;
  }
  memset(inst->h_found, 0, sizeof(uint32_t) * VKSIFT_MAX_OCTAVES * config->sift_buffer_count);
  memset(inst->h_match_n, 0, sizeof(uint32_t) * 4 * batch_cap);
  if (vksift_hip_memset(inst->d_found, 0, sizeof(uint32_t) * VKSIFT_MAX_OCTAVES * config->sift_buffer_count, inst->stream) != 0 ||
      vksift_hip_memcpy_h2d(inst->d_desc_fp, fp_tab, sizeof(float) * inst->desc_fp_len, inst->stream) != 0 || vksift_hip_stream_sync(inst->stream) != 0)
  {
    logError(LOG_TAG, "vksift_createInstance() failure: device initialisation failed");
    vksift_destroyInstance(instance_ptr);
    return VKSIFT_VULKAN_ERROR;
  }

  /* default scale-space = the square of maximal area, like the reference (sift_memory.c:644-662) */
  inst->cur_w = side;
  inst->cur_h = side;
  inst->cur_batch = 1;
  inst->lay = L;
  for (uint32_t b = 0; b < config->sift_buffer_count; b++)
    set_buffer_sections(inst, b, L.n_oct, side, side); /* seq 0: nothing pending, the (zeroed) counters are valid */

  logInfo(LOG_TAG, "vksift_createInstance() success");
  return VKSIFT_SUCCESS;
}

vksift_Result vksift_createInstance(vksift_Instance *instance_ptr, const vksift_Config *config) { return create_instance(instance_ptr, config, 1); }

vksift_Result vksift_ext_createInstanceBatched(vksift_Instance *instance_ptr, const vksift_Config *config, uint32_t batch_capacity)
{
  return create_instance(instance_ptr, config, batch_capacity);
}

void vksift_destroyInstance(vksift_Instance *instance_ptr)
{
  assert(instance_ptr != NULL);
  assert(*instance_ptr != NULL);
  vksift_Instance inst = *instance_ptr;
  vksift_hip_set_device(inst->device);
  inst->pend_n = 0; /* staged, never asked for: nobody can see the result of launching them */
  const vksift_hip_stream drain[] = {inst->pyr_stream, inst->side_stream, inst->dl_stream, inst->up_stream, inst->stream};
  for (int i = 0; i < 5; i++)
    if (drain[i]) /* (a half-constructed instance: creation's failure paths end here) */
      vksift_hip_stream_sync(drain[i]);
  for (int i = 0; i < VKSIFT_GRAPH_CACHE; i++)
    vksift_hip_graph_destroy(inst->graphs[i].exec);
  mem_destroy(inst);
  free(inst);
  *instance_ptr = NULL;
}

/* ------------------------------------------------------------------------------------------------ */
/* synchronisation helpers (fences of the reference)                                                */
/* ------------------------------------------------------------------------------------------------ */
/* The stream is in-order: once a detection has completed, every earlier one has too, and the host mirrors of their counters
 * are valid (counts_valid()). */
void mark_detect_done(vksift_Instance inst) { inst->det_done = inst->det_seq; }

/* polls the detections in flight; true while the LATEST one is still running */
bool detect_running(vksift_Instance inst)
{
  if (inst->det_done >= inst->det_seq)
    return false;
  for (int i = 0; i < VKSIFT_DETECT_RING; i++)
  {
    const DetectSlot *d = &inst->det_ring[i];
    if (d->seq > inst->det_done && vksift_hip_event_busy(d->ev) != 1)
      inst->det_done = d->seq;
  }
  return inst->det_done < inst->det_seq;
}

/* blocks until detection `seq` has completed. Its ring slot may have been taken over by a later detection (more than
 * VKSIFT_DETECT_RING in flight): waiting for that one is conservative, never wrong. */
int wait_detect_seq(vksift_Instance inst, uint64_t seq)
{
  if (seq <= inst->det_done)
    return 0;
  const DetectSlot *d = &inst->det_ring[seq % VKSIFT_DETECT_RING];
  const int e = vksift_hip_event_sync(d->ev);
  if (d->seq > inst->det_done)
    inst->det_done = d->seq;
  return e;
}

/* blocks until the instance stream has passed detection `seq`, waiting for as little as the ring allows: the OLDEST detection at or behind it
 * that still has a slot (the stream is in-order). A number no slot reaches — a detection that failed before it was queued — waits for nothing.
 * Returns the wait's error code: after a failed wait nothing is known about `seq`, and det_done stays what it was. */
int wait_detect_passed(vksift_Instance inst, uint64_t seq)
{
  const DetectSlot *best = NULL;
  if (seq <= inst->det_done)
    return 0;
  for (int i = 0; i < VKSIFT_DETECT_RING; i++)
  {
    const DetectSlot *d = &inst->det_ring[i];
    if (d->ev && d->seq >= seq && (!best || d->seq < best->seq))
      best = d;
  }
  if (!best)
    return 0;
  const int e = vksift_hip_event_sync(best->ev);
  if (e == 0 && best->seq > inst->det_done)
    inst->det_done = best->seq;
  return e;
}

/* A call that rewrites the records of a range of buffers in place (the feature budget, the RootSIFT conversion) is a "detection" of the buffers it
 * names as far as the waits are concerned: it takes the next sequence number and a ring slot,
 * so that counts_valid(), wait_for_buffer(), vksift_isBufferAvailable() and rows_bound() (capacity bound until the new counters have arrived)
 * hold for it without a code path of their own, and a posted or packed copy of the records as they were (post_seq, dl_seq) is no longer
 * served. The packed download of the range (download_from_batch) assumes one section table for all of it: a range that mixes tables or holds
 * uploaded buffers gets a slot that names no buffer, and its downloads take the per-buffer paths. */
void take_sequence(vksift_Instance inst, uint32_t first, uint32_t count)
{
  const uint64_t seq = inst->det_seq + 1u;
  bool uniform = inst->bufs[first].nb_sections != 0;
  for (uint32_t i = 0; i < count; i++)
  {
    uniform = uniform && same_layout(&inst->bufs[first], &inst->bufs[first + i]);
    inst->bufs[first + i].seq = seq;
  }
  DetectSlot *d = &inst->det_ring[seq % VKSIFT_DETECT_RING];
  d->seq = seq, d->first = first, d->count = uniform ? count : 0u;
  inst->det_seq = seq;
}

int inplace_begin(vksift_Instance inst, uint32_t first, uint32_t count, uint32_t *ids)
{
  /* pack launches of a packed download that went straight to the caller's memory may still read the records on the download stream */
  const int e = inst->dl_valid && inst->dl_direct ? vksift_hip_stream_sync(inst->dl_stream) : 0;
  if (e)
    return e;
  (void)detect_running(inst);
  for (uint32_t i = 0; i < count; i++)
    ids[i] = first + i;
  return 0;
}

int inplace_end(vksift_Instance inst, StageFrame *f)
{
  const int e = stage_end(inst, f, NULL, NULL, 0);
  const int r = vksift_hip_event_record(inst->det_ring[inst->det_seq % VKSIFT_DETECT_RING].ev, inst->stream);
  return e ? e : r;
}

void inplace_fail(vksift_Instance inst, StageFrame *f, const char *msg)
{
  (void)stage_abort(f);
  /* the buffers carry the new sequence number: its event stands behind whatever part of the call was queued (recorded again if it was the record
   * that failed; behind a drained stream if it fails twice) */
  if (f->begun && vksift_hip_event_record(inst->det_ring[inst->det_seq % VKSIFT_DETECT_RING].ev, inst->stream) != 0)
    (void)vksift_hip_stream_sync(inst->stream);
  logError(LOG_TAG, "%s", msg);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

bool match_running(vksift_Instance inst)
{
  if (!inst->match_pending)
    return false;
  if (vksift_hip_event_busy(inst->ev_match) == 1)
    return true;
  inst->match_pending = false;
  memset(inst->match_busy, 0, sizeof(bool) * inst->cfg.sift_buffer_count);
  return false;
}

/* Captured launch graphs hold the addresses and the launch arguments of the instance as it was when they were captured: whoever changes
 * one of them (the detection scratch, the descriptor scale table) drops them all. The caller has drained the instance's streams. */
void drop_detect_graphs(vksift_Instance inst)
{
  for (int i = 0; i < VKSIFT_GRAPH_CACHE; i++)
  {
    vksift_hip_graph_destroy(inst->graphs[i].exec);
    memset(&inst->graphs[i], 0, sizeof(inst->graphs[i]));
  }
}

/* The reservation made at creation covers `det_cap` square images of input_image_max_size pixels plus 25 %. Two things outgrow it:
 * a narrow image of the same area (every row is padded to 64 floats on every octave: 139x356 needs 1.5x; the reference re-creates its
 * images for every new input resolution, sift_memory.c:362-452) — L != NULL, the per-image strides grow to what the layout needs —
 * and a caller of the plain API who batches (deferred submission) — new_cap > det_cap, the blocks grow to new_cap images.
 * All work of the instance is drained first; captured launch graphs hold the old addresses and are dropped.
 * 0: done. 1: the larger capacity did not fit, the instance is as it was (capacity growth only). -1: out of device memory, the instance
 * holds NO detection scratch (capacities 0): the next detection retries the allocation or fails cleanly with VKSIFT_VULKAN_ERROR. */
int resize_detect_scratch(vksift_Instance inst, const PyrLayout *L, uint32_t new_cap)
{
  assert(inst->pend_n == 0);
  if (wait_all(inst) != 0)
    return -1;
  const vksift_hip_stream drain[] = {inst->pyr_stream, inst->side_stream, inst->up_stream};
  for (int i = 0; i < 3; i++)
    if (drain[i])
      vksift_hip_stream_sync(drain[i]);
  inst->staging_pending = false;
  inst->input_free_valid = false;
  drop_detect_graphs(inst);
  inst->pyr_free_valid[0] = inst->pyr_free_valid[1] = false;
  const int rc = mem_resize_scratch(inst, L, new_cap);
  inst->cur_w = inst->cur_h = 0; /* no scale-space to download until the next detection */
  inst->shown_img = 0;
  if (rc >= 0 && !inst->overlap_forced && inst->batch_cap < 8u && inst->det_cap >= 8u && !inst->pyr_pingpong)
  {
    /* a plain instance that now takes batches: they overlap like a batch instance's, its small detections stay as they were */
    inst->pyr_pingpong = true;
    inst->overlap_min_count = 8u;
  }
  return rc;
}

int grow_image_scratch(vksift_Instance inst, const PyrLayout *L) { return resize_detect_scratch(inst, L, inst->det_cap) == 0 ? 0 : -1; }

int wait_all(vksift_Instance inst)
{
  vksift_hip_set_device(inst->device);
  int e = vksift_hip_stream_sync(inst->stream);
  mark_detect_done(inst);
  inst->match_pending = false;
  memset(inst->match_busy, 0, sizeof(bool) * inst->cfg.sift_buffer_count);
  return e;
}

bool vksift_isBufferAvailable(vksift_Instance instance, const uint32_t gpu_buffer_id)
{
  vksift_hip_set_device(instance->device);
  defer_sync(instance);
  if (gpu_buffer_id >= instance->cfg.sift_buffer_count)
    return true;
  (void)detect_running(instance);
  if (!counts_valid(instance, gpu_buffer_id))
    return false;
  if (match_running(instance) && instance->match_busy[gpu_buffer_id])
    return false;
  return true;
}
