/*
 * vksift_describe.c — caller-supplied keypoints (vksift_ext_describeKeypoints, vksift_ext_describeKeypointsBatch): the launch sequence of a detection
 * (vksift_detect.c) with the placement launch (hip/place.hip) in place of the extraction stage. No counterpart in the reference, which describes only
 * what it detected. Same contract as a detection: planned by plan_detection(), queued on the same streams, a sequence number and a ring slot of its
 * own, the buffers pending until it has run. Never captured into a graph, never posted, and it leaves the detection's event sets alone: the detect
 * timings keep reporting the last detection.
 */
#include "vksift_internal.h"
#include "vksift_detect.h"

#define KP_BYTES 20u

typedef struct
{
  uint32_t mode;
  size_t off_bytes, bytes; /* the offsets' share of the staging block, and all of it */
} DescribeArgs;

/* the offsets of `count` images in front of their keypoints: count + 1 words, padded so that the keypoints start on a 256-byte boundary */
static size_t offsets_bytes(uint32_t count) { return (((size_t)count + 1u) * sizeof(uint32_t) + 255u) & ~(size_t)255u; }

/* The stage's blocks (vksift_mem.c releases them): the per-buffer counts from the first call on, the keypoint pair grown to the largest call.
 * Before anything of the call is marked or queued: a failure leaves the instance as it was. */
static int fit_keypoint_blocks(vksift_Instance inst, size_t bytes)
{
  const size_t nbuf = inst->cfg.sift_buffer_count;
  if (!mem_ensure(&inst->d_placed, sizeof(uint32_t) * nbuf, MEM_DEVICE) || !mem_ensure(&inst->h_placed, sizeof(uint32_t) * nbuf, MEM_PINNED) ||
      !mem_ensure(&inst->placed_seq, sizeof(uint64_t) * nbuf, MEM_HEAP))
    return -1;
  if (!inst->ev_kps && !(inst->ev_kps = vksift_hip_event_create()))
    return -1;
  if (bytes > inst->kps_cap)
  {
    /* a placement still in flight reads the device block, its copy the pinned one */
    if (inst->d_kps && vksift_hip_stream_sync(inst->stream) != 0)
      return -1;
    mem_release(&inst->d_kps, MEM_DEVICE);
    mem_release(&inst->h_kps, MEM_PINNED);
    inst->kps_cap = 0, inst->kps_pending = false;
    const size_t cap = bytes + bytes / 4u + 4096u;
    if (!mem_ensure(&inst->d_kps, cap, MEM_DEVICE) || !mem_ensure(&inst->h_kps, cap, MEM_PINNED))
    {
      mem_release(&inst->d_kps, MEM_DEVICE);
      mem_release(&inst->h_kps, MEM_PINNED);
      return -1;
    }
    inst->kps_cap = cap;
  }
  /* the host is about to overwrite both staging blocks */
  if (inst->kps_pending)
  {
    TRY(vksift_hip_event_sync(inst->ev_kps), "keypoint staging synchronisation");
    inst->kps_pending = false;
  }
  if (inst->staging_pending)
  {
    TRY(vksift_hip_event_sync(inst->ev_staging), "staging synchronisation");
    inst->staging_pending = false;
  }
  return 0;
}

/* A detection's keypoints have a relative sigma of at most seed_scale_sigma 2^((S + 1) / S), and the table of the descriptor's fixed-point scales
 * (vksift_hm_desc_fp_table) ends there; the launch clamps its index. Supplied keypoints reach the whole window range, so the first describe call
 * extends the table to it. The entries a detection reads stay what they were; the table's length is an argument of every descriptor launch, so
 * the detection graphs captured with the old one are dropped (the stream has been drained: none of them is in flight). */
#define DESCRIBE_MAX_REL 29.f
static int fit_desc_fp_table(vksift_Instance inst)
{
  float tab[DESC_FP_TAB_MAX];
  const uint32_t n = vksift_hm_desc_fp_table_for(DESCRIBE_MAX_REL * 1.01f, tab, DESC_FP_TAB_MAX);
  if (n <= inst->desc_fp_len)
    return 0;
  TRY(vksift_hip_memcpy_h2d(inst->d_desc_fp, tab, sizeof(float) * n, inst->stream), "descriptor scale table");
  TRY(vksift_hip_stream_sync(inst->stream), "descriptor scale table");
  inst->desc_fp_len = n;
  drop_detect_graphs(inst);
  return 0;
}

/* scale space, then place, then [orientation], then descriptors, then the counts: enqueue_detection() with the placement for the extraction */
static int enqueue_describe(DetectCtx *c, const DescribeArgs *a)
{
  vksift_Instance inst = c->inst;
  vksift_hip_stream st = inst->stream;
  vksift_hip_stream sp = c->overlap ? inst->pyr_stream : st;
  const uint32_t n_oct = c->L->n_oct;
  TRY(enqueue_upload(c, sp), "image upload");
  TRY(vksift_hip_memcpy_h2d(inst->d_kps, inst->h_kps, a->bytes, st), "keypoint upload");
  TRY(vksift_hip_event_record(inst->ev_kps, st), "event record");
  inst->kps_pending = true;
  /* the placement writes the counter of every octave it serves; an image without an octave keeps these zeros (no mask clears: nothing is scanned) */
  TRY(vksift_hip_memset(found_dev(inst, c->first_buf), 0, sizeof(uint32_t) * VKSIFT_MAX_OCTAVES * c->count, st), "counter reset");
  TRY(vksift_hip_memset(inst->d_placed + c->first_buf, 0, sizeof(uint32_t) * c->count, st), "counter reset");
  TRY(enqueue_scale_space(c, sp), "scale space construction");
  if (n_oct > 0)
  {
    vksift_hip_PlaceOctave oct[VKSIFT_MAX_OCTAVES];
    float steps[VKSIFT_MAX_SCALES + 1];
    for (uint32_t o = 0; o < n_oct; o++)
    {
      const vksift_hip_OctaveJob *j = &c->jobs[o];
      oct[o].w = j->w, oct[o].h = j->h, oct[o].octave_idx = j->octave_idx;
      oct[o].feats = j->feats, oct[o].feat_img_stride = j->feat_img_stride, oct[o].cap = j->cap;
      oct[o].found = j->found, oct[o].found_img_stride = j->found_img_stride;
    }
    /* the half-way points between the scales, in double: pow(), so that tests/np_describe.py forms the same table from the same library call */
    for (uint32_t k = 0; k <= inst->S; k++)
      steps[k] = (float)((double)inst->cfg.seed_scale_sigma * pow(2.0, ((double)k + 0.5) / (double)inst->S));
    vksift_hip_range_push("PlaceKeypoints");
    TRY_IN_RANGE(vksift_hip_place_keypoints((const vksift_hip_Keypoint *)(inst->d_kps + a->off_bytes), (const uint32_t *)inst->d_kps, oct, n_oct, steps, inst->S,
                                   a->mode == VKSIFT_EXT_DESCRIBE_GIVEN ? 1u : 0u, c->count, inst->d_placed + c->first_buf, st),
        "keypoint placement");
    vksift_hip_range_pop();
    if (a->mode == VKSIFT_EXT_DESCRIBE_ORIENT)
    {
      vksift_hip_range_push("ComputeOrientation");
      TRY_IN_RANGE(vksift_hip_orientations_multi(c->jobs, n_oct, c->count, st), "orientation");
      vksift_hip_range_pop();
    }
    vksift_hip_range_push("ComputeDescriptors");
    if (c->dense)
    {
      const vksift_hip_DenseRows dr = dense_rows(c);
      TRY_IN_RANGE(vksift_hip_descriptors_multi_dense(c->jobs, n_oct, c->count, &dr, st), "descriptor");
    }
    else
      TRY_IN_RANGE(vksift_hip_descriptors_multi(c->jobs, n_oct, c->count, st), "descriptor");
    vksift_hip_range_pop();
    if (c->overlap)
    {
      /* the next detection's scale-space may start here (vksift_detect.c: enqueue_keypoint_stages) */
      TRY(vksift_hip_event_record(inst->ev_desc_start, st), "event record");
      inst->desc_start_valid = true;
    }
  }
  if (inst->pyr_pingpong)
    TRY(pyr_last_reader(inst, st), "pyramid buffer release");
  TRY(vksift_hip_post_words(found_host(inst, c->first_buf), found_dev(inst, c->first_buf), (size_t)VKSIFT_MAX_OCTAVES * c->count, st), "count read-back");
  TRY(vksift_hip_post_words(inst->h_placed + c->first_buf, inst->d_placed + c->first_buf, c->count, st), "count read-back");
  return 0;
}

/* detect_impl() for keypoints: validate, fit, mark, plan, prepare, queue, finish */
static void describe_impl(vksift_Instance inst, const uint8_t *const *images, uint32_t count, uint32_t w, uint32_t h, const vksift_ext_Keypoint *kps,
                          const uint32_t *nb_kps, uint32_t first_buf, uint32_t mode, const char *fn)
{
  DetectCtx c;
  DescribeArgs a;
  if (!detect_args_valid(inst, count, w, h, first_buf, true))
    return invalid_input(inst, fn);
  bool ok = images != NULL && nb_kps != NULL && (mode == VKSIFT_EXT_DESCRIBE_ORIENT || mode == VKSIFT_EXT_DESCRIBE_GIVEN);
  size_t total = 0;
  for (uint32_t i = 0; ok && i < count; i++)
  {
    ok = images[i] != NULL && nb_kps[i] <= inst->cfg.max_nb_sift_per_buffer;
    total += nb_kps[i];
  }
  if (!ok || (total > 0 && kps == NULL) || total > 0xFFFFFFFFu)
    return invalid_input(inst, fn);
  a.mode = mode;
  a.off_bytes = offsets_bytes(count);
  a.bytes = a.off_bytes + total * KP_BYTES;
  if (fit_keypoint_blocks(inst, a.bytes) != 0 || fit_desc_fp_table(inst) != 0 || fit_layout(inst, w, h) != 0)
    return detect_failed(inst, NULL, fn);
  /* the keypoints are the caller's until here: offsets, then the lists back to back */
  uint32_t *first = (uint32_t *)inst->h_kps;
  first[0] = 0;
  for (uint32_t i = 0; i < count; i++)
    first[i + 1] = first[i] + nb_kps[i];
  if (total)
    memcpy(inst->h_kps + a.off_bytes, kps, total * KP_BYTES);
  for (uint32_t i = 0; i < count; i++)
  {
    set_buffer_sections(inst, first_buf + i, inst->lay.n_oct, w, h);
    inst->bufs[first_buf + i].seq = inst->det_seq + 1u;
    inst->cache_valid[first_buf + i] = false;
  }
  plan_detection(&c, inst, images, NULL, false, count, w, h, first_buf, detect_running(inst));
  /* not a detection's event set, graph or posting slot */
  c.prof = false, c.replay_ok = false, c.post_ok = false;
  if (prepare_detection(&c) != 0 || enqueue_describe(&c, &a) != 0 || finish_detection(&c) != 0)
    return detect_failed(inst, &c, fn);
  for (uint32_t i = 0; i < count; i++)
    inst->placed_seq[first_buf + i] = inst->det_seq;
}

void vksift_ext_describeKeypoints(vksift_Instance instance, const uint8_t *image_data, uint32_t image_width, uint32_t image_height,
                                  const vksift_ext_Keypoint *kps, uint32_t nb_kps, uint32_t gpu_buffer_id, uint32_t mode)
{
  const uint8_t *imgs[1] = {image_data};
  vksift_hip_set_device(instance->device);
  defer_sync(instance);
  describe_impl(instance, imgs, 1, image_width, image_height, kps, &nb_kps, gpu_buffer_id, mode, "vksift_ext_describeKeypoints()");
}

void vksift_ext_describeKeypointsBatch(vksift_Instance instance, const uint8_t *const *images, uint32_t count, uint32_t image_width, uint32_t image_height,
                                       const vksift_ext_Keypoint *kps, const uint32_t *nb_kps, uint32_t first_gpu_buffer_id, uint32_t mode)
{
  vksift_hip_set_device(instance->device);
  defer_sync(instance);
  if (ext_batch_count_valid(instance, count, "vksift_ext_describeKeypointsBatch()"))
    describe_impl(instance, images, count, image_width, image_height, kps, nb_kps, first_gpu_buffer_id, mode, "vksift_ext_describeKeypointsBatch()");
}

uint32_t vksift_ext_getPlacedKeypointsNumber(vksift_Instance instance, uint32_t gpu_buffer_id)
{
  vksift_Instance inst = instance;
  defer_sync(inst);
  if (!buffer_idx_valid(inst, gpu_buffer_id))
  {
    logError(LOG_TAG, "vksift_ext_getPlacedKeypointsNumber(): bad argument.");
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return 0;
  }
  wait_for_buffer(inst, gpu_buffer_id);
  /* the count of the describe call that filled the buffer, unless something else has filled it or a budget call has named it since (a conversion
   * takes the count along: vksift_rootsift.c) */
  const uint64_t seq = inst->bufs[gpu_buffer_id].seq;
  return inst->placed_seq && seq != 0 && inst->placed_seq[gpu_buffer_id] == seq ? inst->h_placed[gpu_buffer_id] : 0u;
}
