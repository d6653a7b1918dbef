/*
 * vksift_detect.c — the detection pipeline (vulkansift.c:315-344 + sift_memory.c:891-955 + sift_detector.c:1313-1410,1462-1542):
 * plan_detection() decides the schedule of a call, prepare_detection() readies the instance for it, enqueue_detection() queues it stage
 * by stage, detect_impl() drives them. (Image staging: vksift_stage.c; deferred submission of the plain entry point: vksift_defer.c.)
 */
#include "vksift_internal.h"
#include "vksift_detect.h"

static uint64_t algorithmic_pyramid_bytes(vksift_Instance inst, uint32_t w, uint32_t h, uint32_t nb_octaves)
{
  /* (S+3 Gaussian writes + S+2 blur reads + S+2 DoG writes) * 4 B per octave pixel,
   * plus on octave 0: input read (1 B/px of input), up-sample plane write and seed-blur read (4 B each). */
  const PyrLayout *L = &inst->lay;
  uint64_t bytes = 0;
  for (uint32_t o = 0; o < L->n_oct && o < nb_octaves; o++)
    bytes += (uint64_t)L->w[o] * L->h[o] * pyr_texel_bytes(inst) * ((inst->S + 3) + (inst->S + 2) + (inst->S + 2));
  bytes += (uint64_t)w * h + (uint64_t)L->w[0] * L->h[0] * 2u * pyr_texel_bytes(inst);
  return bytes;
}

/* fold the (completed) event timings of a detect call into the running sums */
void account_set(vksift_Instance inst, ProfSet *ps)
{
  if (!inst->profiling || !ps->valid || ps->accounted)
    return;
  vksift_hip_event *e = ps->ev_t;
  inst->acc_ms[0] += vksift_hip_event_elapsed_ms(e[0], e[1]);
  inst->acc_ms[1] += ps->overlap ? vksift_hip_event_elapsed_ms(ps->ev_pt[0], ps->ev_pt[1]) : vksift_hip_event_elapsed_ms(e[1], e[2]);
  inst->acc_ms[2] += vksift_hip_event_elapsed_ms(e[2], e[3]);
  inst->acc_ms[3] += vksift_hip_event_elapsed_ms(e[3], e[4]);
  inst->acc_ms[4] += vksift_hip_event_elapsed_ms(e[4], e[5]);
  inst->acc_ms[5] += vksift_hip_event_elapsed_ms(e[0], e[6]);
  inst->acc_ms[6] += vksift_hip_event_elapsed_ms(e[2], ps->ev_scan);
  inst->acc_ms[7] += vksift_hip_event_elapsed_ms(ps->ev_pt[0], ps->ev_pt[2]);
  inst->acc_blur_launches_all += ps->blur_launches_all;
  inst->acc_calls++;
  inst->acc_blur_launches += ps->blur_launches;
  inst->acc_alg_bytes += ps->alg_bytes;
  inst->acc_scan_bytes += ps->scan_bytes;
  ps->accounted = true;
}

/* all detections have completed (caller waited): account both event sets, oldest first */
void account_timings(vksift_Instance inst)
{
  account_set(inst, &inst->prof[inst->prof_cur ^ 1]);
  account_set(inst, &inst->prof[inst->prof_cur]);
}

/* the current pyramid buffer has a new last reader: everything queued on s so far */
int pyr_last_reader(vksift_Instance inst, vksift_hip_stream s)
{
  TRY(vksift_hip_event_record(inst->ev_pyr_free[inst->pyr_cur], s), "event record");
  inst->pyr_free_valid[inst->pyr_cur] = true;
  return 0;
}
/* the pinned staging buffer is busy until what is queued on s so far has run */
static int staging_busy_until(vksift_Instance inst, vksift_hip_stream s)
{
  TRY(vksift_hip_event_record(inst->ev_staging, s), "event record");
  inst->staging_pending = true;
  return 0;
}

static vksift_hip_Plane plane_at(const DetectCtx *c, uint32_t o, uint32_t layer)
{
  vksift_Instance inst = c->inst;
  const PyrLayout *L = c->L;
  vksift_hip_Plane p;
  p.base = (float *)((uint8_t *)c->d_pyr + (L->gauss_off[o] + (uint64_t)layer * L->plane_stride[o]) * pyr_texel_bytes(inst));
  p.fp16 = inst->fp16 ? 1u : 0u, p.reverse = 0;
  p.w = L->w[o], p.h = L->h[o], p.pitch = L->pitch[o];
  p.img_stride = inst->pyr_img_stride;
  return p;
}

/* images [first, ..) of the batch only: the same launches on a slice of the planes */
static vksift_hip_Plane plane_sub(const DetectCtx *c, uint32_t o, uint32_t layer, uint32_t first)
{
  vksift_hip_Plane p = plane_at(c, o, layer);
  p.base = (float *)((uint8_t *)p.base + (uint64_t)first * p.img_stride * pyr_texel_bytes(c->inst));
  return p;
}

static void build_jobs(DetectCtx *c)
{
  vksift_Instance inst = c->inst;
  const PyrLayout *L = c->L;
  const BufferInfo *b0 = &inst->bufs[c->first_buf];
  for (uint32_t o = 0; o < L->n_oct; o++)
  {
    vksift_hip_OctaveJob *j = &c->jobs[o];
    j->gauss = plane_at(c, o, 0).base;
    j->fp16 = inst->fp16 ? 1u : 0u;
    j->w = L->w[o], j->h = L->h[o], j->pitch = L->pitch[o];
    j->plane_stride = L->plane_stride[o];
    j->img_stride = inst->pyr_img_stride;
    j->S = inst->S;
    j->octave_idx = (int32_t)o - (inst->cfg.use_input_upsampling ? 1 : 0);
    j->seed_sigma = inst->cfg.seed_scale_sigma;
    j->dog_threshold = inst->cfg.intensity_threshold / (float)inst->S;
    j->edge_limit = ((inst->cfg.edge_threshold + 1.f) * (inst->cfg.edge_threshold + 1.f)) / inst->cfg.edge_threshold;
    j->feats = inst->d_feats + (uint64_t)c->first_buf * inst->buf_stride + (uint64_t)b0->sec_off[o] * FEAT_BYTES;
    j->feat_img_stride = inst->buf_stride;
    j->cap = b0->sec_cap[o];
    j->found = found_dev(inst, c->first_buf) + o;
    j->found_img_stride = VKSIFT_MAX_OCTAVES;
    /* segment scratch is octave-major: [octave][image][segment], so one octave's masks of the whole batch are contiguous */
    const uint64_t nsegs_o = (uint64_t)inst->S * L->h[o] * ((L->w[o] + 63) / 64);
    j->seg_mask = inst->d_seg_mask + L->seg_off[o] * c->count;
    j->seg_off = inst->d_seg_off + L->seg_off[o] * c->count;
    j->seg_img_stride = nsegs_o;
    j->cand_xy = inst->d_cand_xy + L->cand_off[o];
    j->cand_flag = inst->d_cand_flag + L->cand_off[o];
    j->cand_n = inst->d_cand_n + (size_t)o * inst->det_cap;
    j->cand_img_stride = inst->cand_cap;
    j->cand_cap = (uint32_t)L->cand_cap[o];
    j->ori_ang = inst->d_ori_ang + (size_t)b0->sec_off[o] * VKSIFT_HIP_MAX_ORI;
    j->ori_cnt = inst->d_ori_cnt + b0->sec_off[o];
    j->ori_img_stride = inst->ori_cap;
    j->max_ori = inst->cfg.max_nb_orientation_per_keypoint;
    j->use_vlfeat = inst->cfg.descriptor_format == VKSIFT_DESCRIPTOR_FORMAT_VLFEAT ? 1u : 0u;
    j->desc_fp_tab = inst->d_desc_fp;
    j->desc_fp_tab_len = inst->desc_fp_len;
    j->sec_index = o; /* (masks_cleared, scan_reverse = 0: set at launch time by enqueue_clears / enqueue_pyramid, enqueue_tail, enqueue_chain) */
  }
}

/* Everything a detection's launch sequence depends on, decided in one place. Reads the instance (layout fitted, target buffers marked, event
 * set recycled) and the arguments; gpu_busy is the one run-time observation. vksift_hip_blur_form / vksift_hip_tune_get are pure queries. */
void plan_detection(DetectCtx *c, vksift_Instance inst, const uint8_t *const *images, const uint8_t *d_images, bool prestaged, uint32_t count,
                           uint32_t w, uint32_t h, uint32_t first_buf, bool gpu_busy)
{
  const PyrLayout *L = &inst->lay;
  const BufferInfo *b0 = &inst->bufs[first_buf];
  memset(c, 0, sizeof(*c));
  c->inst = inst, c->L = L, c->PS = &inst->prof[inst->prof_cur];
  c->images = images;
  c->w = w, c->h = h, c->count = count, c->first_buf = first_buf;
  c->img_bytes = (size_t)w * h;
  c->prestaged = prestaged;
  c->prof = inst->profiling;
  /* host images are staged into pinned memory while the sequence is enqueued (enqueue_upload): the caller may reuse its
   * memory as soon as we return (sift_memory.c:943) */
  c->upload = images != NULL || prestaged;
  /* Overlapping detections (VKSIFT_PYR_PINGPONG=1): with two pyramid buffers the scale-space construction of this call
   * does not depend on anything the previous call (or a matching still in flight) reads or writes, so it runs on its own
   * stream, ordered only behind the last reader of the pyramid buffer it recycles; everything that touches the SIFT
   * buffers and the extraction scratch stays in instance-stream order. */
  c->overlap = inst->pyr_pingpong && L->n_oct > 0 && count >= inst->overlap_min_count;
  c->pyr_buf = c->overlap && inst->pyr_nbuf == 2u ? inst->pyr_cur ^ 1 : inst->pyr_cur;
  c->d_pyr = c->overlap ? inst->d_pyr_buf[c->pyr_buf] : inst->d_pyr;
  /* One host image (at most 1 MB): no copy into device memory first — the fused up-sampling + seed launch reads every source byte once, and
   * reads them out of the pinned staging buffer over the bus (300 KB: ~6 us of bus time inside a 9 us launch) instead of behind a 9 us copy */
  c->zero_copy = c->upload && count == 1u && c->img_bytes <= ((size_t)1 << 20) && vksift_hip_tune_get(VKSIFT_TUNE_ZERO_COPY) == 0;
  c->d_src = c->upload ? (c->zero_copy ? inst->h_input : inst->d_input) : d_images;
  /* forked scale-space + LDS chain are latency measures for ONE image (or a handful): a batch on a single-buffer instance
   * (batch_cap < 8 or VKSIFT_PYR_PINGPONG=0) fills the chip with its per-scale launches and takes those */
  c->fork = inst->fork_scales && !c->overlap && !c->prof && c->count <= VKSIFT_FORK_MAX_COUNT && (uint64_t)c->count * c->w * c->h <= inst->fork_max_pixels;
  /* (VKSIFT_TUNE_TAIL_MULTI = 1: every octave in full, one launch per octave and scale — A/B and the bit-identity matrix) */
  c->tail_batch = !c->fork && c->count >= 8u && L->n_oct > 1u && vksift_hip_tune_get(VKSIFT_TUNE_TAIL_MULTI) == 0;
  /* a batch: octave 0 (and every octave whose last two scales take the four-texel kernel) in full, the coarser ones up to scale S */
  for (uint32_t o = 0; o < L->n_oct; o++)
  {
    c->tail[o] = c->fork;
    if (c->tail_batch && o >= 1u)
    {
      const vksift_hip_Plane p = plane_at(c, o, 0);
      c->tail[o] = vksift_hip_blur_form(p, p, inst->ntaps[inst->S + 1u], c->count) == 1 && vksift_hip_blur_form(p, p, inst->ntaps[inst->S + 2u], c->count) == 1;
    }
  }
  /* The trailing octaves whose planes fit the LDS are built by ONE launch (vksift_hip_octave_chain: a workgroup per image walks all
   * their scales): from the first octave >= 1 behind which every octave qualifies. */
  c->chain_from = L->n_oct;
  /* (forked = small detections only: in a batch the per-scale launches are faster — one workgroup per image keeps 16 waves on a CU for
   * 80 us where the launches spread an octave over the chip: 512 x 640x480 23.3 k frames/s with the chain, 23.6 k without) */
  if (inst->lds_chain && c->fork && !inst->fp16 && inst->S + 3u <= 8u)
  {
    uint32_t f = L->n_oct;
    while (f > 1u && (L->w[f - 1u] & 3u) == 0u && (uint64_t)L->w[f - 1u] * L->h[f - 1u] <= inst->lds_chain_max && L->w[f - 1u] >= 8u && L->h[f - 1u] >= 8u &&
           L->n_oct - (f - 1u) <= 4u)
      f--;
    c->chain_from = f;
  }
  /* The upload goes in groups (enqueue_upload) ... */
  c->up_per = (uint32_t)((((size_t)4 << 20) + c->img_bytes - 1) / c->img_bytes); /* >= 4 MB per copy */
  if (c->up_per < (count + VKSIFT_UP_GROUPS - 1u) / VKSIFT_UP_GROUPS)
    c->up_per = (count + VKSIFT_UP_GROUPS - 1u) / VKSIFT_UP_GROUPS;
  if (c->up_per < 32u)
    c->up_per = 32u;
  /* ... when the GPU would otherwise wait for the bus. With the previous detection still running (a caller that queues the next
   * batch before fetching the current one) the copies are hidden anyway, and whole-batch launches are the better launches:
   * 512 frames, pipelined protocol, 21.45 -> 21.85 k frames/s */
  c->grouped = c->upload && L->n_oct > 0 && count >= 2u * c->up_per && !gpu_busy;
  /* once the instance has matched (its cache blocks exist) a detection leaves the matcher's rows of its buffers behind itself */
  c->dense = inst->d_cache_desc != NULL && inst->d_cache_norm != NULL && L->n_oct > 0 && L->n_oct == b0->nb_sections && L->n_oct <= 16u &&
             vksift_hip_tune_get(VKSIFT_TUNE_DENSE_ROWS) == 0;
  /* feature posting for single-image detections whose records fit the slot (every section is capacity-bounded) */
  c->post_ok = count == 1 && inst->post_enabled && inst->post_on && L->n_oct > 0 && b0->nb_sections > 0 && b0->nb_sections <= 16;
  for (uint32_t o = 0; c->post_ok && o < b0->nb_sections; o++)
    c->post_bytes += (uint64_t)b0->sec_cap[o] * FEAT_BYTES;
  /* host-visible events (staging, completion, profiling) stay outside a captured region; a captured graph holds the address
   * of ONE pyramid buffer, so instances with two (ping-pong) never replay, nor does a detection whose scale-space overlaps */
  c->replay_ok = inst->use_graphs && !c->prof && !c->overlap && !(inst->pyr_pingpong && inst->pyr_nbuf == 2u) && (uint64_t)count * w * h <= inst->graph_max_pixels;
  /* profiling: the scale-space interval is octave 0's (77 % of the bytes), the scan interval covers the scan launch of all octaves */
  c->alg_bytes = algorithmic_pyramid_bytes(inst, w, h, 1u) * count;
  /* "the extrema scan adds 20 B/px.octave" = one read of the S+2 DoG layers */
  for (uint32_t o = 0; o < L->n_oct; o++)
    c->scan_bytes += (uint64_t)L->w[o] * L->h[o] * pyr_texel_bytes(inst) * (inst->S + 2) * count;
  build_jobs(c);
}

/* What the plan changes on the instance before anything is queued: the feature-posting slots and their idle counter (c->post is final
 * here, and with it the graph-cache key), the accessors' view, the pyramid buffer of an overlapped call and its two gates. */
int prepare_detection(DetectCtx *c)
{
  vksift_Instance inst = c->inst;
  inst->cur_batch = c->count;
  inst->shown_img = c->prestaged ? c->count - 1u : 0u;
  if (c->post_ok)
  {
    if (!inst->h_post[0])
    {
      const size_t cap = (size_t)inst->cfg.max_nb_sift_per_buffer * FEAT_BYTES + 4096u;
      const bool p0 = mem_ensure(&inst->h_post[0], cap, MEM_PINNED), p1 = mem_ensure(&inst->h_post[1], cap, MEM_PINNED);
      inst->post_cap = (p0 && p1) ? cap : 0;
      if (!inst->post_cap)
      {
        mem_release(&inst->h_post[0], MEM_PINNED);
        mem_release(&inst->h_post[1], MEM_PINNED);
        inst->post_enabled = false;
      }
    }
    c->post = inst->post_cap != 0 && c->post_bytes <= inst->post_cap;
    if (c->post)
    {
      const uint32_t slot = c->first_buf & 1u;
      if (inst->post_seq[slot] != 0 && !inst->post_fetched[slot] && ++inst->post_idle >= VKSIFT_POST_IDLE)
        inst->post_on = false, c->post = false; /* posted and overwritten without ever being fetched, too many times in a row */
      inst->post_seq[slot] = 0; /* the slot is about to be rewritten: valid again once this detection is queued */
    }
  }
  c->PS->overlap = true; /* the scale-space interval is the one between ev_pt[0] and ev_pt[1] (octave 0) */
  prof_mark(c, c->PS->ev_t[0], inst->stream);
  if (c->overlap)
  {
    inst->pyr_cur = c->pyr_buf;
    inst->d_pyr = c->d_pyr;
    if (inst->pyr_free_valid[inst->pyr_cur])
      TRY(vksift_hip_stream_wait_event(inst->pyr_stream, inst->ev_pyr_free[inst->pyr_cur]), "pyramid buffer recycle");
    /* not before the previous detection's descriptors are done (see enqueue_keypoint_stages) */
    if (inst->desc_start_valid)
      TRY(vksift_hip_stream_wait_event(inst->pyr_stream, inst->ev_desc_start), "overlap gate");
  }
  return 0;
}

/* ------------------------------------------------------------------------------------------------ */
/* the launch sequence of one detection, stage by stage                                             */
/* ------------------------------------------------------------------------------------------------ */
enum { PYR_FIRST_GROUP = 1, PYR_LAST_GROUP = 2 };

/* Plane 0 of octave 0 for images [first, first + count): u8 -> fp32 (2x LINEAR blit when up-sampling) + seed blur: one fused pass when the
 * shape allows it, else the blit goes into the (still unused) layer-1 slot and is seed-blurred into layer 0 */
static int enqueue_seed(const DetectCtx *c, vksift_hip_stream sp, uint32_t first, uint32_t count, int group_flags)
{
  vksift_Instance inst = c->inst;
  const PyrLayout *L = c->L;
  const uint8_t *src = c->d_src + (size_t)first * c->img_bytes;
  const vksift_hip_Plane dst = plane_sub(c, 0, 0, first);
  bool fused = false;
  if (L->w[0] == 2 * c->w && L->h[0] == 2 * c->h)
    TRY(optional(vksift_hip_seed_upsampled(src, c->w, c->h, c->img_bytes, dst, scale_taps(inst, 0), inst->ntaps[0], count, sp), &fused), "fused up-sampling + seed blur");
  else if (L->w[0] == c->w && L->h[0] == c->h)
    TRY(optional(vksift_hip_seed_direct(src, c->w, c->h, c->img_bytes, dst, scale_taps(inst, 0), inst->ntaps[0], count, sp), &fused), "fused input conversion + seed blur");
  if (!fused)
  {
    const vksift_hip_Plane tmp = plane_sub(c, 0, 1, first);
    TRY(vksift_hip_input_blit(src, c->w, c->h, c->img_bytes, tmp, count, sp), "input blit");
    TRY(vksift_hip_blur(tmp, dst, scale_taps(inst, 0), inst->ntaps[0], count, sp), "seed blur");
  }
  /* d_input has been consumed: the next upload (possibly on another stream) may overwrite it after this point */
  if (!c->capturing && (group_flags & PYR_LAST_GROUP))
  {
    TRY(vksift_hip_event_record(inst->ev_input_free, sp), "event record");
    inst->input_free_valid = true;
  }
  return 0;
}

/* Scale-space construction of octave o on stream sp (sift_detector.c:881-1037), up to scale S + 2, or S when c->tail[o]. The DoG pass of the
 * reference (sift_detector.c:1039-1079) has no counterpart: the extrema stage forms D[s] = G[s+1] - G[s] from the Gaussian planes.
 * c->g0_done: plane 0 of this octave was already written by the previous octave's scale-S pass; on return it tells the same
 * for the next octave. */
static int enqueue_pyramid(DetectCtx *c, uint32_t o, vksift_hip_stream sp, uint32_t first, uint32_t count, int group_flags)
{
  vksift_Instance inst = c->inst;
  uint32_t nb_o = 0;
  vksift_hip_range_push("Scale space construction");
  if (o == 0)
  {
    if (group_flags & PYR_FIRST_GROUP)
      prof_mark(c, c->PS->ev_pt[0], sp);
    TRY_IN_RANGE(enqueue_seed(c, sp, first, count, group_flags), "seed");
    nb_o++;
  }
  else if (!c->g0_done)
    TRY_IN_RANGE(vksift_hip_downsample(plane_sub(c, o - 1, inst->S, first), plane_sub(c, o, 0, first), count, sp), "downsample");
  c->g0_done = false;
  /* consecutive launches of the chain walk the batch in opposite directions: a launch starts on the planes its predecessor wrote
   * last, which are still in the Infinity Cache (a whole-batch plane is 2.5x the cache: in the same direction every read misses);
   * the extrema scan continues the alternation */
  uint32_t li = 0;
  /* c->tail[o] (forked detections, the coarser octaves of a batch): the launches up to scale S — the path to the next octave — only;
   * scales S+1 and S+2 are queued per SCALE afterwards (enqueue_tail) */
  const uint32_t last = c->tail[o] ? inst->S : inst->S + 2u;
  for (uint32_t s = 1; s <= last; s++)
  {
    const vksift_hip_Plane srcp = plane_sub(c, o, s - 1, first);
    vksift_hip_Plane dstp = plane_sub(c, o, s, first);
    bool done = false;
    dstp.reverse = alt_dir(inst, ++li);
    nb_o++;
    /* two scales in one launch where the kernels cover the tap counts (the source plane is read once, scale s never re-read):
     * not across scale S, which also seeds the next octave */
    if (s + 1 < inst->S + 3 && s != inst->S && s + 1 != inst->S)
    {
      vksift_hip_Plane dst2 = plane_sub(c, o, s + 1, first);
      dst2.reverse = dstp.reverse;
      TRY_IN_RANGE(optional(vksift_hip_blur_pair(srcp, dstp, dst2, scale_taps(inst, s), inst->ntaps[s], scale_taps(inst, s + 1), inst->ntaps[s + 1], count, sp), &done),
          "two-scale blur");
      s += done ? 1u : 0u; /* (the single-scale launch below then has nothing left to do) */
    }
    else if (s == inst->S && o + 1 < c->L->n_oct)
    {
      /* scale S also seeds the next octave (sift_detector.c:1003-1034): stored by the same pass when the sizes halve exactly */
      TRY_IN_RANGE(optional(vksift_hip_blur_downsample(srcp, dstp, plane_sub(c, o + 1, 0, first), scale_taps(inst, s), inst->ntaps[s], count, sp), &done), "blur + down-sampling");
      c->g0_done = done;
    }
    if (!done)
      TRY_IN_RANGE(vksift_hip_blur(srcp, dstp, scale_taps(inst, s), inst->ntaps[s], count, sp), "blur");
  }
  c->jobs[o].scan_reverse = alt_dir(inst, li + 1u);
  vksift_hip_range_pop();
  c->nblur_all += nb_o;
  if (o == 0)
  {
    c->nblur += nb_o;
    if (group_flags & PYR_LAST_GROUP)
      prof_mark(c, c->PS->ev_pt[1], sp);
  }
  return 0;
}

/* Scales S+1 and S+2 of the octaves the trunk left at scale S (in_tail()): they feed nothing but the extrema scan (scale S seeds the next octave,
 * they do not), so they wait until the chain seed -> ... -> scale S has been queued for every octave and go as ONE launch per SCALE over all
 * those octaves (vksift_hip_blur_multi: a flat multi-octave grid, csrc/hip/multi.h) — 2 launches instead of 2 per octave; shapes that kernel
 * does not serve take one launch per octave and scale as before. Same kernel body either way: bit-identical planes. */
static int enqueue_tail(DetectCtx *c, vksift_hip_stream sp)
{
  vksift_Instance inst = c->inst;
  for (uint32_t s = inst->S + 1u; s < inst->S + 3u; s++)
  {
    vksift_hip_Plane src[VKSIFT_MAX_OCTAVES], dst[VKSIFT_MAX_OCTAVES];
    uint32_t n = 0;
    for (uint32_t o = 0; o < c->L->n_oct; o++)
      if (in_tail(c, o))
      {
        src[n] = plane_at(c, o, s - 1u);
        dst[n] = plane_at(c, o, s);
        dst[n].reverse = alt_dir(inst, s);
        n++;
      }
    for (uint32_t i0 = 0; i0 < n; i0 += 8u)
    {
      const uint32_t k = n - i0 < 8u ? n - i0 : 8u;
      bool done = false;
      if (vksift_hip_tune_get(VKSIFT_TUNE_TAIL_MULTI) != 1)
        TRY(optional(vksift_hip_blur_multi(src + i0, dst + i0, k, scale_taps(inst, s), inst->ntaps[s], c->count, sp), &done), "multi-octave blur");
      for (uint32_t i = i0; !done && i < i0 + k; i++)
        TRY(vksift_hip_blur(src[i], dst[i], scale_taps(inst, s), inst->ntaps[s], c->count, sp), "blur");
      c->nblur_all += done ? 1u : k;
    }
  }
  for (uint32_t o = 0; o < c->L->n_oct; o++)
    if (in_tail(c, o))
      c->jobs[o].scan_reverse = alt_dir(inst, inst->S + 3u); /* opposite to the last launch */
  return 0;
}

/* Host images -> d_input (or, zero-copy, nothing: the seed launch reads h_input), and for a grouped upload octave 0 group by group.
 * The copies run on a stream of their own, behind the previous reader of d_input only (the seed pass of the previous
 * detection, whichever stream it ran on) — not behind the gates of the scale-space stream: the staging buffer is then free
 * again (ev_staging) as soon as the bus has taken the images, and a caller that queues the next batch early is not held up
 * until this detection's turn on the GPU has come. Captured sequences keep everything on the capturing stream.
 * The batch goes in groups: stage a group, queue its copy, queue octave 0's scale-space for THAT group behind the copy, stage
 * the next group meanwhile. 128 VGA frames are 39 MB = 1.6 ms on the bus: as one copy in front of whole-batch launches that
 * is 1.6 ms of idle GPU; in 4 groups of 32 the bus and the blur chain work side by side and octave 0 is complete 0.4 ms
 * after the last byte has arrived. (Groups below 32 frames lose more in launch efficiency than they hide.) */
int enqueue_upload(DetectCtx *c, vksift_hip_stream sp)
{
  vksift_Instance inst = c->inst;
  vksift_hip_stream su = c->capturing ? sp : inst->up_stream;
  const bool grouped = upload_grouped(c);
  const uint32_t per = grouped ? c->up_per : c->count;
  if (inst->input_free_valid && !c->capturing)
    TRY(vksift_hip_stream_wait_event(su, inst->ev_input_free), "input buffer recycle");
  for (uint32_t i0 = 0, g = 0; i0 < c->count; g++)
  {
    uint32_t i1 = i0 + per;
    if (i1 >= c->count || c->count - i1 < per / 2u)
      i1 = c->count; /* a tail shorter than half a group joins the last one */
    if (!c->prestaged)
      stage_images(inst->h_input, c->images, i0, i1, c->img_bytes);
    if (!c->zero_copy)
      TRY(vksift_hip_memcpy_h2d(inst->d_input + (size_t)i0 * c->img_bytes, inst->h_input + (size_t)i0 * c->img_bytes, c->img_bytes * (i1 - i0), su), "image upload");
    if (grouped)
    {
      TRY(vksift_hip_event_record(inst->ev_up[g], su), "event record");
      TRY(vksift_hip_stream_wait_event(sp, inst->ev_up[g]), "image upload");
      TRY(enqueue_pyramid(c, 0, sp, i0, i1 - i0, (i0 == 0 ? PYR_FIRST_GROUP : 0) | (i1 == c->count ? PYR_LAST_GROUP : 0)), "scale space construction");
    }
    i0 = i1;
  }
  if (!c->capturing && !c->zero_copy)
  {
    /* the pinned staging buffer is free again as soon as these copies have run; the seed pass waits for them */
    TRY(staging_busy_until(inst, su), "image upload");
    if (!grouped)
      TRY(vksift_hip_stream_wait_event(sp, inst->ev_staging), "image upload");
  }
  return 0;
}

/* recClearBufferDataCmds (sift_detector.c:1081-1104); a forked detection clears on the side stream, beside the seed launch: the side
 * stream is ordered behind everything queued on the trunk stream so far — the previous detection's readers of the counters and masks —
 * and the trunk never waits for it (a fork in the middle of the trunk costs its next launch ~5 us) */
static int enqueue_clears(DetectCtx *c, vksift_hip_stream sp)
{
  vksift_Instance inst = c->inst;
  const size_t bytes = sizeof(uint32_t) * VKSIFT_MAX_OCTAVES * c->count;
  if (!c->fork)
    return vksift_hip_memset(found_dev(inst, c->first_buf), 0, bytes, inst->stream);
  TRY(vksift_hip_event_record(inst->ev_join[1], sp), "event record");
  TRY(vksift_hip_stream_wait_event(inst->pyr_stream, inst->ev_join[1]), "scale fork");
  TRY(vksift_hip_memset(found_dev(inst, c->first_buf), 0, bytes, inst->pyr_stream), "counter reset");
  bool cleared = false;
  if (c->L->n_oct > 0)
    TRY(optional(vksift_hip_clear_segment_masks(c->jobs, c->L->n_oct, c->count, inst->pyr_stream), &cleared), "mask reset");
  for (uint32_t o = 0; cleared && o < c->L->n_oct; o++)
    c->jobs[o].masks_cleared = 1u;
  return 0;
}

/* The LDS chain's turn (octave c->chain_from is next on the trunk): one launch for all octaves from there on, if the launcher takes them */
static int enqueue_chain(DetectCtx *c, vksift_hip_stream sp)
{
  vksift_Instance inst = c->inst;
  vksift_hip_Plane layers[4 * 8];
  const uint32_t o = c->chain_from, nl = inst->S + 3u, no = c->L->n_oct - o;
  for (uint32_t q = 0; q < no; q++)
    for (uint32_t l = 0; l < nl; l++)
      layers[q * nl + l] = plane_at(c, o + q, l);
  if (!c->g0_done)
    TRY(vksift_hip_downsample(plane_at(c, o - 1u, inst->S), layers[0], c->count, sp), "downsample");
  /* (lds_chain_refuse: test hook — S = nl is outside the shim's domain, so it declines exactly like a shape it does not cover) */
  TRY(optional(vksift_hip_octave_chain(layers, no, nl, inst->lds_chain_refuse ? nl : inst->S, inst->taps, inst->ntaps, c->count, sp), &c->chain_done),
      "coarse-octave chain");
  /* not covered after all: the octave's seed is in place, the per-scale launches follow — for a forked detection trunk AND
   * branch: in_tail() holds for these octaves again, so enqueue_tail reaches them too */
  c->g0_done = !c->chain_done;
  for (uint32_t q = o; c->chain_done && q < c->L->n_oct; q++)
    c->jobs[q].scan_reverse = 0u;
  return 0;
}

/* The scale-space of every octave (octave 0 is there already after a grouped upload): the trunk on sp — per-scale launches, then the LDS
 * chain —, the batch tail behind it, the forked branch on the side stream and its join, and the hand-over to the instance stream. */
int enqueue_scale_space(DetectCtx *c, vksift_hip_stream sp)
{
  vksift_Instance inst = c->inst;
  const PyrLayout *L = c->L;
  for (uint32_t o = upload_grouped(c) ? 1u : 0u; o < L->n_oct; o++)
  {
    if (o == c->chain_from)
    {
      TRY(enqueue_chain(c, sp), "scale space construction");
      if (c->chain_done)
        break;
    }
    TRY(enqueue_pyramid(c, o, sp, 0, c->count, PYR_FIRST_GROUP | PYR_LAST_GROUP), "scale space construction");
    if (c->fork && (o + 1u == c->chain_from || o + 1u == L->n_oct))
      TRY(vksift_hip_event_record(inst->ev_fork[0], sp), "event record"); /* scale S of the last per-scale octave is queued: the tail may follow */
  }
  if (c->tail_batch)
    TRY(enqueue_tail(c, sp), "scale space construction");
  /* the staging buffer was the seed launch's source: free again once that has run (octave 0's launches are on sp) */
  if (c->zero_copy && !c->capturing)
    TRY(staging_busy_until(inst, sp), "image upload");
  if (c->fork)
  {
    /* Branch: the scales behind S of every forked octave on the side stream (which already holds the two clears) */
    vksift_hip_stream side = inst->pyr_stream;
    if (L->n_oct > 0)
    {
      /* ONE launch per scale over all forked octaves (round 6; one per octave and scale before: eight dependent launches on this stream
       * were the end of a 640x480 detection's scale-space, 173 us after its start — with two the LDS chain of the coarsest octave is) */
      TRY(vksift_hip_stream_wait_event(side, inst->ev_fork[0]), "scale fork");
      TRY(enqueue_tail(c, side), "scale space construction");
    }
    /* the side stream rejoins (the clears at least are on it) */
    TRY(vksift_hip_event_record(inst->ev_join[0], side), "event record");
    TRY(vksift_hip_stream_wait_event(sp, inst->ev_join[0]), "scale join");
  }
  prof_mark(c, c->PS->ev_pt[2], sp); /* every octave's scale-space is queued (forked branches have joined) */
  if (c->overlap)
  {
    TRY(vksift_hip_event_record(inst->ev_pyr_done, sp), "event record");
    TRY(vksift_hip_stream_wait_event(inst->stream, inst->ev_pyr_done), "scale space ready");
  }
  return 0;
}

/* The matcher's view of the buffers comes out of the descriptor launch (pack_BufferMemory, sift_memory.c:957-1047): no gather pass;
 * so do the posted records of a single-image detection (vksift_internal.h: h_post): no pack launch behind the descriptors */
vksift_hip_DenseRows dense_rows(const DetectCtx *c)
{
  vksift_Instance inst = c->inst;
  const BufferInfo *b0 = &inst->bufs[c->first_buf];
  vksift_hip_DenseRows dr;
  memset(&dr, 0, sizeof(dr));
  if (c->dense)
  {
    dr.desc = inst->d_cache_desc + (uint64_t)c->first_buf * inst->desc_slot_stride, dr.desc_img_stride = inst->desc_slot_stride;
    dr.norm = inst->d_cache_norm + (uint64_t)c->first_buf * inst->cache_norm_stride, dr.norm_img_stride = inst->cache_norm_stride;
    dr.n = inst->d_cache_n + c->first_buf, dr.n_img_stride = 1;
  }
  if (c->post)
  {
    dr.post = inst->h_post[c->first_buf & 1u], dr.post_img_stride = 0;
    dr.found_post = found_host(inst, c->first_buf), dr.found_post_n = VKSIFT_MAX_OCTAVES;
  }
  dr.nsec = b0->nb_sections;
  for (uint32_t o = 0; o < b0->nb_sections; o++)
    dr.sec_cap[o] = b0->sec_cap[o];
  return dr;
}

/* ExtractKeypoints, ComputeOrientation, ComputeDescriptors: ONE chain of launches each for all octaves, on the instance stream */
static int enqueue_keypoint_stages(const DetectCtx *c)
{
  vksift_Instance inst = c->inst;
  vksift_hip_stream st = inst->stream;
  const uint32_t n_oct = c->L->n_oct;
  prof_mark(c, c->PS->ev_t[2], st);
  vksift_hip_range_push("ExtractKeypoints");
  TRY_IN_RANGE(vksift_hip_extract_keypoints_multi(c->jobs, n_oct, c->count, st, c->prof ? c->PS->ev_scan : NULL), "keypoint extraction");
  vksift_hip_range_pop();
  prof_mark(c, c->PS->ev_t[3], st);
  vksift_hip_range_push("ComputeOrientation");
  TRY_IN_RANGE(vksift_hip_orientations_multi(c->jobs, n_oct, c->count, st), "orientation");
  vksift_hip_range_pop();
  prof_mark(c, c->PS->ev_t[4], st);
  vksift_hip_range_push("ComputeDescriptors");
  if (c->dense || c->post)
  {
    const vksift_hip_DenseRows dr = dense_rows(c);
    TRY_IN_RANGE(vksift_hip_descriptors_multi_dense(c->jobs, n_oct, c->count, &dr, st), "descriptor");
  }
  else
    TRY_IN_RANGE(vksift_hip_descriptors_multi(c->jobs, n_oct, c->count, st), "descriptor");
  vksift_hip_range_pop();
  if (c->overlap)
  {
    /* the next detection's scale-space may start here: beside the matching that usually follows, not beside the descriptors.
     * Gates at the start of the orientation / descriptor stage, or none at all, give the same frames/s within 1 % and turn
     * every stage interval into a measurement of the contention instead of the kernel. */
    TRY(vksift_hip_event_record(inst->ev_desc_start, st), "event record");
    inst->desc_start_valid = true;
  }
  prof_mark(c, c->PS->ev_t[5], st);
  return 0;
}

/* an image too small for a single octave launches nothing: the stage events of this call are recorded here, so that its
 * (zero) intervals are not measured against the events of an earlier detection */
static void mark_no_octaves(const DetectCtx *c)
{
  vksift_hip_stream st = c->inst->stream;
  for (int i = 2; i <= 5; i++)
    prof_mark(c, c->PS->ev_t[i], st);
  prof_mark(c, c->PS->ev_scan, st);
  for (int i = 0; i <= 2; i++)
    prof_mark(c, c->PS->ev_pt[i], st);
}

/* Everything a detection puts on the GPU, from the image upload to the count read-back: the part a hipGraph captures.
 *
 * Two streams at most for a batch. The scale-space of all octaves is built on one (octave o+1 is seeded by scale S of octave o anyway;
 * small detections fork the scales behind S onto a side stream, see DetectCtx::fork: there the launch-to-launch latency is the cost,
 * not the bandwidth);
 * then every keypoint stage — ExtractKeypoints, ComputeOrientation, ComputeDescriptors — is ONE chain of launches for all
 * octaves on the instance stream (vksift_hip_*_multi), like the reference records the dispatches of all octaves of a stage into
 * one command buffer (sift_detector.c:1106-1259). With two pyramid buffers the scale-space has a stream of its own, ordered
 * behind the last reader of the buffer it recycles (prepare_detection), so that the construction for detection N+1 runs beside the
 * matching of detection N.
 * Measured on MI355X (128 x 640x480 per call): anything more concurrent is not faster — per-octave chains on per-octave
 * streams (rounds 1-2) let the coarse octaves trickle through ~50 launches too small to fill the chip (2.9 ms of a 6.5 ms step
 * for a third of the pixels), eight hardware queues instead of four cost 10 %: memory-bound and VALU-bound kernels beside each
 * other take the sum of their times (the blur launches keep the VALUs half busy themselves). */
static int enqueue_detection(DetectCtx *c)
{
  vksift_Instance inst = c->inst;
  vksift_hip_stream st = inst->stream;
  vksift_hip_stream sp = c->overlap ? inst->pyr_stream : st;
  if (c->upload)
    TRY(enqueue_upload(c, sp), "image upload");
  prof_mark(c, c->PS->ev_t[1], st);
  TRY(enqueue_clears(c, sp), "counter reset");
  TRY(enqueue_scale_space(c, sp), "scale space construction");
  if (c->L->n_oct > 0)
    TRY(enqueue_keypoint_stages(c), "keypoint stages");
  else
    mark_no_octaves(c);
  /* everything that reads this call's pyramid runs on the instance stream (also recorded by the calls that do not overlap —
   * tiny images — so that a later overlapped call never recycles the buffer under them) */
  if (inst->pyr_pingpong && !c->capturing)
    TRY(pyr_last_reader(inst, st), "pyramid buffer release");
  inst->last_blur_launches = c->nblur, inst->last_blur_launches_all = c->nblur_all;
  inst->last_alg_bytes = c->alg_bytes, inst->last_scan_bytes = c->scan_bytes;
  if (c->post)
    return 0; /* records and counters were posted by the descriptor launch */
  /* recCopySIFTCountCmds (sift_detector.c:1261-1291) */
  TRY(vksift_hip_post_words(found_host(inst, c->first_buf), found_dev(inst, c->first_buf), (size_t)VKSIFT_MAX_OCTAVES * c->count, st), "count read-back");
  return 0;
}

/* ------------------------------------------------------------------------------------------------ */
/* one detection call: validate, recycle, fit, mark, plan, prepare, launch, finish                  */
/* ------------------------------------------------------------------------------------------------ */
/* hipGraph replay (VKSIFT_GRAPH=1): the launch sequence depends only on (resolution, batch, first buffer, input pointer) —
 * counts and candidate lists live on the device — so it is captured once per such key and replayed with a single launch.
 * *out: the cache entry for the key (hit: ->exec != NULL) or the least recently used entry, emptied (miss). The evicted exec is
 * destroyed only once the stream has passed its last launch: a caller that cycles through more keys than the cache holds and never
 * waits (device input: no staging buffer to recycle) would otherwise destroy an exec that is still executing. A wait that fails is
 * the detection's failure: the exec stays, and detect_failed() drops the cache behind drained streams. */
static int graph_lookup(vksift_Instance inst, const DetectCtx *c, DetectGraph **out)
{
  DetectGraph *victim = &inst->graphs[0];
  for (int i = 0; i < VKSIFT_GRAPH_CACHE; i++)
  {
    DetectGraph *g = &inst->graphs[i];
    if (g->exec && g->w == c->w && g->h == c->h && g->count == c->count && g->first_buf == c->first_buf && g->d_src == c->d_src && g->post == c->post &&
        g->dense == c->dense)
    {
      *out = g;
      return 0;
    }
    if (g->stamp < victim->stamp)
      victim = g;
  }
  if (victim->exec)
    TRY(wait_detect_passed(inst, victim->last_seq), "detection graph retirement");
  vksift_hip_graph_destroy(victim->exec);
  memset(victim, 0, sizeof(*victim));
  *out = victim;
  return 0;
}

/* The sequence reaches the GPU: queued directly, captured and launched, or replayed from the graph cache (after prepare_detection: c->post is
 * part of the key). c->capturing is true exactly while a capture is open, so that detect_failed() can close it. */
static int launch_detection(DetectCtx *c)
{
  vksift_Instance inst = c->inst;
  vksift_hip_stream st = inst->stream;
  DetectGraph *dg = NULL;
  if (c->replay_ok)
    TRY(graph_lookup(inst, c, &dg), "detection graph lookup");
  if (dg && dg->exec)
  {
    if (c->images) /* the upload is a node of the graph: the staging buffer has to be filled before the replay */
      stage_images(inst->h_input, c->images, 0, c->count, c->img_bytes);
    TRY(vksift_hip_graph_launch(dg->exec, st), "detection graph launch");
    inst->graph_miss_run = 0;
  }
  else
  {
    if (dg && ++inst->graph_miss_run > 4u * VKSIFT_GRAPH_CACHE)
    {
      /* the caller keeps changing shape / buffer / input pointer: captures would only add cost */
      inst->use_graphs = false;
      dg = NULL;
    }
    if (dg && vksift_hip_capture_begin(st) != 0)
      dg = NULL;
    c->capturing = dg != NULL;
    const int e = enqueue_detection(c);
    if (e != 0)
      return e;
    if (c->capturing)
    {
      vksift_hip_graph exec = NULL;
      c->capturing = false;
      TRY(vksift_hip_capture_end(st, &exec), "detection graph capture");
      dg->exec = exec;
      dg->w = c->w, dg->h = c->h, dg->count = c->count, dg->first_buf = c->first_buf, dg->d_src = c->d_src, dg->post = c->post, dg->dense = c->dense;
      TRY(vksift_hip_graph_launch(dg->exec, st), "detection graph launch");
    }
  }
  if (dg)
    dg->stamp = ++inst->graph_stamp, dg->last_seq = inst->det_seq + 1u; /* (the number finish_detection gives this detection) */
  /* (recorded by enqueue_detection for every sequence that is not captured) a later overlapped detection recycles the buffer
   * behind this one's readers */
  if (dg && inst->pyr_pingpong)
    TRY(pyr_last_reader(inst, st), "pyramid buffer release");
  /* graph replay: the upload is a node of the graph, the staging buffer is busy until the graph has run */
  if (dg && c->upload)
    TRY(staging_busy_until(inst, st), "image upload");
  return 0;
}

void invalid_input(vksift_Instance inst, const char *fn)
{
  logError(LOG_TAG, "%s error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
}

/* The arguments of a detection are usable (report: say so when the image is too small, the other causes report themselves) */
bool detect_args_valid(vksift_Instance inst, uint32_t count, uint32_t w, uint32_t h, uint32_t first_buf, bool report)
{
  if (!(count >= 1 && count <= inst->det_cap && buffer_idx_valid(inst, first_buf) && buffer_idx_valid(inst, first_buf + count - 1) && resolution_valid(inst, w, h)))
    return false;
  if ((w < h ? w : h) >= 16u)
    return true;
  if (report)
    logError(LOG_TAG, "Input image %ux%u is too small to build a single octave.", w, h);
  return false;
}

/* The reference makes a new pipeline wait on the host for the running ones (vulkansift.c:326-327) because its
 * command buffers and staging memory are single-instanced. Here the instance's HIP stream is in-order, so GPU
 * work is already serialised; the host only has to wait for the resources it is about to overwrite: the pinned
 * image staging buffer, and (when profiling) the event set of the detection before the previous one. */
static int recycle_host_resources(vksift_Instance inst, bool host_images)
{
  if (inst->staging_pending && host_images) /* (prestaged images: the deferring call waited before it wrote the first one) */
  {
    TRY(vksift_hip_event_sync(inst->ev_staging), "staging synchronisation");
    inst->staging_pending = false;
  }
  if (inst->profiling)
  {
    /* recycle the older event set: the host never waits for the call it just queued */
    inst->prof_cur ^= 1;
    ProfSet *PS = &inst->prof[inst->prof_cur];
    if (PS->valid && !PS->accounted)
    {
      TRY(vksift_hip_event_sync(PS->ev_t[6]), "profiling synchronisation");
      account_set(inst, PS);
    }
    PS->valid = false;
  }
  return 0;
}

int fit_layout(vksift_Instance inst, uint32_t w, uint32_t h)
{
  if (inst->cur_w == w && inst->cur_h == h)
    return 0;
  PyrLayout L;
  compute_layout(inst, w, h, &L);
  /* n_oct == 0 (shortest side below 32 pixels, 16 with up-sampling): no scale-space, the detection finds nothing */
  if ((L.img_floats > inst->pyr_img_stride || L.seg_total > inst->seg_cap || L.cand_total > inst->cand_cap) && grow_image_scratch(inst, &L) != 0)
  {
    logError(LOG_TAG, "Failed to fit the scale-space of a %ux%u image in device memory", w, h);
    return -1;
  }
  inst->lay = L;
  inst->cur_w = w;
  inst->cur_h = h;
  return 0;
}

/* the sequence is queued: bookkeeping, ring slot, completion event */
int finish_detection(const DetectCtx *c)
{
  vksift_Instance inst = c->inst;
  ProfSet *PS = c->PS;
  const uint64_t seq = inst->det_seq + 1u;
  inst->device_input_last = !c->upload;
  if (c->dense)
    for (uint32_t i = 0; i < c->count; i++)
      inst->cache_valid[c->first_buf + i] = true; /* in stream order in front of every matching queued from here on */
  if (c->prof)
  {
    vksift_hip_event_record(PS->ev_t[6], inst->stream);
    PS->valid = true;
    PS->accounted = false;
    PS->blur_launches = inst->last_blur_launches, PS->blur_launches_all = inst->last_blur_launches_all;
    PS->alg_bytes = inst->last_alg_bytes;
    PS->scan_bytes = inst->last_scan_bytes;
  }
  DetectSlot *d = &inst->det_ring[seq % VKSIFT_DETECT_RING];
  d->seq = seq, d->first = c->first_buf, d->count = c->count;
  if (c->post)
    inst->post_seq[c->first_buf & 1u] = seq, inst->post_buf[c->first_buf & 1u] = c->first_buf, inst->post_fetched[c->first_buf & 1u] = false;
  inst->det_seq = seq; /* from here on the buffers are "pending" even if the record below fails (wait_detect_seq then syncs a stale event: harmless) */
  TRY(vksift_hip_event_record(d->ev, inst->stream), "event record");
  return 0;
}

/* c: the call's context once its buffers carry the new sequence number, NULL for a failure before that */
void detect_failed(vksift_Instance inst, const DetectCtx *c, const char *fn)
{
  vksift_hip_stream st = inst->stream;
  if (c && c->capturing)
  {
    vksift_hip_graph dead = NULL;
    (void)vksift_hip_capture_end(st, &dead);
    vksift_hip_graph_destroy(dead);
  }
  if (c)
  {
    /* The detection never got its sequence number (det_seq and the ring slot advance on success only): left as they are the
     * buffers would wait for a detection that does not exist — vksift_isBufferAvailable() false for ever, the accessors syncing
     * a foreign ring event — and the next successful detection would alias the number. They become completed, EMPTY buffers:
     * whatever part of the chain was queued may still write counters, so the stream is drained before the host mirror is zeroed. */
    (void)vksift_hip_stream_sync(st);
    if (inst->pyr_stream)
      (void)vksift_hip_stream_sync(inst->pyr_stream);
    if (inst->side_stream)
      (void)vksift_hip_stream_sync(inst->side_stream);
    /* whatever failed, no captured sequence is trusted after it: the next detection of every key captures afresh (nothing is in flight) */
    drop_detect_graphs(inst);
    for (uint32_t i = 0; i < c->count; i++)
    {
      inst->bufs[c->first_buf + i].seq = 0;
      memset(found_host(inst, c->first_buf + i), 0, sizeof(uint32_t) * VKSIFT_MAX_OCTAVES);
    }
    (void)vksift_hip_memset(found_dev(inst, c->first_buf), 0, sizeof(uint32_t) * VKSIFT_MAX_OCTAVES * c->count, st);
  }
  logError(LOG_TAG, "%s error: Failed to start the detection pipeline.", fn);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}

void detect_impl(vksift_Instance inst, const uint8_t *const *images, const uint8_t *d_images, bool prestaged, uint32_t count, uint32_t w, uint32_t h,
                 uint32_t first_buf, const char *fn)
{
  DetectCtx c;
  if (!detect_args_valid(inst, count, w, h, first_buf, true))
    return invalid_input(inst, fn);
  if (recycle_host_resources(inst, images != NULL) != 0 || fit_layout(inst, w, h) != 0)
    return detect_failed(inst, NULL, fn);
  for (uint32_t i = 0; i < count; i++)
  {
    set_buffer_sections(inst, first_buf + i, inst->lay.n_oct, w, h);
    inst->bufs[first_buf + i].seq = inst->det_seq + 1u; /* its counters are valid once the detection about to be queued has completed */
    inst->cache_valid[first_buf + i] = false;           /* the matcher's view of the buffer is rebuilt on its next matching */
  }
  plan_detection(&c, inst, images, d_images, prestaged, count, w, h, first_buf, detect_running(inst));
  if (prepare_detection(&c) != 0 || launch_detection(&c) != 0 || finish_detection(&c) != 0)
    detect_failed(inst, &c, fn);
}

bool ext_batch_count_valid(vksift_Instance inst, uint32_t count, const char *fn)
{
  if (count > inst->batch_cap)
    invalid_input(inst, fn);
  return count <= inst->batch_cap;
}

void vksift_ext_detectFeaturesBatch(vksift_Instance instance, const uint8_t *const *images, uint32_t count, uint32_t image_width, uint32_t image_height,
                                    uint32_t first_gpu_buffer_id)
{
  vksift_hip_set_device(instance->device);
  defer_sync(instance);
  if (ext_batch_count_valid(instance, count, "vksift_ext_detectFeaturesBatch()"))
    detect_impl(instance, images, NULL, false, count, image_width, image_height, first_gpu_buffer_id, "vksift_ext_detectFeaturesBatch()");
}

void vksift_ext_detectFeaturesBatchDevice(vksift_Instance instance, const uint8_t *d_images, uint32_t count, uint32_t image_width, uint32_t image_height,
                                          uint32_t first_gpu_buffer_id)
{
  vksift_hip_set_device(instance->device);
  defer_sync(instance);
  if (d_images == NULL)
    invalid_input(instance, "vksift_ext_detectFeaturesBatchDevice()");
  else if (ext_batch_count_valid(instance, count, "vksift_ext_detectFeaturesBatchDevice()"))
    detect_impl(instance, NULL, d_images, false, count, image_width, image_height, first_gpu_buffer_id, "vksift_ext_detectFeaturesBatchDevice()");
}
