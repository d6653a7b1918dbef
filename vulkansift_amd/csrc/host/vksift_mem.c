/*
 * vksift_mem.c — who owns what: every device / pinned / heap block, stream and event of an instance is listed ONCE here (blocks[],
 * handles[]), with its size where the instance decides it; reservation at creation, growth of the detection scratch, the lazily
 * allocated blocks and release all walk those two tables (sift_memory.c:133-360 equivalent). Scale-space layout and the measured
 * placement of the scale-space buffers live here too. Calls the device only through the allocation / event / stream shims and
 * vksift_hip_blur: it links against a counting stub, without the rest of the host library (tests/test_mem_ownership.py).
 */
#include "vksift_internal.h"

#include <stddef.h>

/* ------------------------------------------------------------------------------------------------ */
/* layout                                                                                           */
/* ------------------------------------------------------------------------------------------------ */
static uint32_t round_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }

void compute_layout(vksift_Instance inst, uint32_t w, uint32_t h, PyrLayout *L)
{
  memset(L, 0, sizeof(*L));
  L->n_oct = vksift_hm_octaves_for(&inst->cfg, inst->max_octaves, w, h, L->w, L->h);
  uint64_t off = 0;
  for (uint32_t o = 0; o < L->n_oct; o++)
  {
    L->pitch[o] = round_up(L->w[o], PITCH_ALIGN);
    L->plane_stride[o] = (uint64_t)L->pitch[o] * L->h[o];
    L->gauss_off[o] = off;
    off += L->plane_stride[o] * (inst->S + 3);
  }
  L->img_floats = off;
  uint64_t so = 0, co = 0;
  for (uint32_t o = 0; o < L->n_oct; o++)
  {
    L->seg_off[o] = so;
    so += (uint64_t)inst->S * L->h[o] * ((L->w[o] + 63) / 64);
    L->cand_off[o] = co;
    /* Room for every candidate any image can produce, so that they are only ever lost through the section capacity, like in the
     * reference. A strict 26-neighbour maximum is a strict maximum of its own layer's 8-neighbourhood, so the strict maxima of a
     * layer are pairwise non-adjacent (8-connectivity). Cut the (w-2) x (h-2) interior into ceil((w-2)/2) x ceil((h-2)/2) blocks
     * of at most 2x2 texels: the texels of a block are pairwise adjacent, so a block holds at most one maximum, and likewise at
     * most one minimum. A 2x2-periodic texture reaches the bound (tests/test_extraction_limits.py). ceil((n-2)/2) = (n-1)/2. */
    L->cand_cap[o] = (uint64_t)inst->S * 2u * ((L->w[o] - 1u) / 2u) * ((L->h[o] - 1u) / 2u) + 64u;
    co += L->cand_cap[o];
  }
  L->seg_total = so;
  L->cand_total = co;
}

/* what the detection scratch is sized by: images, and per image the scale-space texels, segment elements and candidates */
typedef struct
{
  uint64_t cap, pyr, seg, cand;
} ScratchDims;

/* what one image of layout L gets reserved: non-square images of the same area need a little more because of the row-pitch padding */
static ScratchDims reserve_for(const PyrLayout *L, uint32_t cap)
{
  const ScratchDims d = {cap, L->img_floats + L->img_floats / 4 + 4096, L->seg_total + L->seg_total / 4 + 1024, L->cand_total + L->cand_total / 4 + 4096u};
  return d;
}

/* ------------------------------------------------------------------------------------------------ */
/* the blocks                                                                                       */
/* ------------------------------------------------------------------------------------------------ */
/* when a block exists: from creation on with a size the configuration fixes; the detection scratch, whose size follows the per-image
 * strides (seg_cap, cand_cap) or only the capacity (det_cap) and which resize_detect_scratch re-allocates; or allocated by whoever
 * first needs it (mem_ensure, mem_fit_staging, place_pyramid_buffers), which the table only releases */
enum { AT_CREATION, PER_STRIDE, PER_CAPACITY, ELSEWHERE };
/* what the element count of a block is proportional to (block_bytes) */
enum { N_ONE, N_BUFFERS, N_FEAT_STRIDE, N_SLOTS, N_MATCH_STRIDE, N_REDO_STRIDE, N_PIXELS, N_SEG, N_CAND, N_OCTAVES, N_KEYPOINTS };
typedef struct
{
  size_t field; /* offsetof the pointer in the instance */
  uint8_t kind, when, per;
  uint32_t elem; /* bytes */
} Block;
#define FIELD(f) offsetof(struct vksift_Instance_T, f)
#define LAZY(f, kind) {FIELD(f), kind, ELSEWHERE, N_ONE, 0}
/* the three blocks of what a stage keeps per pair (PairResults, vksift_pairs.c: pair_results_ensure) */
#define PAIR_RESULTS(which) LAZY(res[which].d_payload, MEM_DEVICE), LAZY(res[which].d_words, MEM_DEVICE), LAZY(res[which].h_words, MEM_PINNED)
/* In the order create_instance() allocates (the scale-space buffers come after them, behind the stream: mem_create); a growth allocates
 * the scale-space, the PER_STRIDE blocks, then the PER_CAPACITY ones, each class in this order. A new scratch block is one line here. */
static const Block blocks[] = {
    {FIELD(d_input), MEM_DEVICE, PER_CAPACITY, N_PIXELS, 1},
    {FIELD(h_input), MEM_PINNED, PER_CAPACITY, N_PIXELS, 1},
    {FIELD(d_feats), MEM_DEVICE, AT_CREATION, N_FEAT_STRIDE, 1},
    {FIELD(d_found), MEM_DEVICE, AT_CREATION, N_BUFFERS, sizeof(uint32_t) * VKSIFT_MAX_OCTAVES},
    {FIELD(h_found), MEM_PINNED, AT_CREATION, N_BUFFERS, sizeof(uint32_t) * VKSIFT_MAX_OCTAVES},
    {FIELD(d_seg_mask), MEM_DEVICE, PER_STRIDE, N_SEG, sizeof(uint64_t)},
    {FIELD(d_seg_off), MEM_DEVICE, PER_STRIDE, N_SEG, sizeof(uint32_t)},
    {FIELD(d_cand_xy), MEM_DEVICE, PER_STRIDE, N_CAND, sizeof(uint32_t)},
    {FIELD(d_cand_flag), MEM_DEVICE, PER_STRIDE, N_CAND, sizeof(uint32_t)},
    {FIELD(d_cand_n), MEM_DEVICE, PER_CAPACITY, N_OCTAVES, sizeof(uint32_t)},
    {FIELD(d_ori_ang), MEM_DEVICE, PER_CAPACITY, N_KEYPOINTS, sizeof(float) * VKSIFT_HIP_MAX_ORI},
    {FIELD(d_ori_cnt), MEM_DEVICE, PER_CAPACITY, N_KEYPOINTS, sizeof(uint32_t)},
    {FIELD(d_desc_fp), MEM_DEVICE, AT_CREATION, N_ONE, sizeof(float) * DESC_FP_TAB_MAX},
    /* matching scratch: one slot per batch entry (slot 0 serves vksift_matchFeatures). The matcher's per-buffer cache
     * (sift_buffer_count x max_nb_sift_per_buffer x 132 B: 1.7 GB for 128 buffers of 100 000) and the partial lists of the single-pair
     * kernel are allocated by the first matching / export (ensure_match_cache): detect-only users never pay for them */
    {FIELD(d_cache_n), MEM_DEVICE, AT_CREATION, N_BUFFERS, sizeof(uint32_t)},
    {FIELD(cache_valid), MEM_HEAP, AT_CREATION, N_BUFFERS, sizeof(bool)},
    {FIELD(cache_queued), MEM_HEAP, AT_CREATION, N_BUFFERS, sizeof(bool)},
    {FIELD(d_matches), MEM_DEVICE, AT_CREATION, N_MATCH_STRIDE, 1},
    {FIELD(d_redo), MEM_DEVICE, AT_CREATION, N_REDO_STRIDE, sizeof(uint32_t)},
    {FIELD(d_match_n), MEM_DEVICE, AT_CREATION, N_SLOTS, sizeof(uint32_t) * 4},
    {FIELD(h_match_n), MEM_PINNED, AT_CREATION, N_SLOTS, sizeof(uint32_t) * 4},
    {FIELD(bufs), MEM_HEAP, AT_CREATION, N_BUFFERS, sizeof(BufferInfo)},
    {FIELD(match_busy), MEM_HEAP, AT_CREATION, N_BUFFERS, sizeof(bool)},
    LAZY(d_pyr_buf[0], MEM_DEVICE), LAZY(d_pyr_buf[1], MEM_DEVICE),
    LAZY(d_cache_desc, MEM_DEVICE), LAZY(d_cache_norm, MEM_DEVICE), LAZY(d_match_partial, MEM_DEVICE), LAZY(h_matches, MEM_PINNED),
    LAZY(rev.matches, MEM_DEVICE), LAZY(rev.redo, MEM_DEVICE), LAZY(rev.match_n, MEM_DEVICE),
    LAZY(filt_ids, MEM_HEAP), LAZY(d_corr, MEM_DEVICE), LAZY(d_vscratch, MEM_DEVICE), LAZY(h_vtab, MEM_PINNED), LAZY(d_gxy, MEM_DEVICE), LAZY(d_gkeys, MEM_DEVICE), LAZY(h_gtab, MEM_PINNED),
    LAZY(tracks.d_node_words, MEM_DEVICE), LAZY(tracks.d_records, MEM_DEVICE), LAZY(tracks.d_stats, MEM_DEVICE), LAZY(tracks.h_stats, MEM_PINNED), LAZY(tracks.d_scratch, MEM_DEVICE),
    LAZY(tracks.h_tab, MEM_PINNED), LAZY(tracks.d_tab, MEM_DEVICE), LAZY(tracks.rank_of, MEM_HEAP), LAZY(tracks.count_word, MEM_HEAP), LAZY(tracks.ids, MEM_HEAP), LAZY(tracks.d_rows_acc, MEM_DEVICE), LAZY(tracks.h_rows_acc, MEM_PINNED),
    LAZY(edges.d_edges, MEM_DEVICE), LAZY(edges.d_stats, MEM_DEVICE), LAZY(edges.h_stats, MEM_PINNED), LAZY(edges.d_rows, MEM_DEVICE), LAZY(edges.d_scratch, MEM_DEVICE),
    LAZY(edges.h_tab, MEM_PINNED), LAZY(edges.d_tab, MEM_DEVICE), LAZY(edges.rank_of, MEM_HEAP), LAZY(edges.named, MEM_HEAP),
    LAZY(obs.d_offsets, MEM_DEVICE), LAZY(obs.d_track_ids, MEM_DEVICE), LAZY(obs.d_obs, MEM_DEVICE), LAZY(obs.d_stats, MEM_DEVICE), LAZY(obs.h_stats, MEM_PINNED),
    LAZY(obs.d_scratch, MEM_DEVICE), LAZY(obs.h_tab, MEM_PINNED),
    LAZY(tri.d_points, MEM_DEVICE), LAZY(tri.d_stats, MEM_DEVICE), LAZY(tri.h_stats, MEM_PINNED), LAZY(tri.h_cameras, MEM_PINNED), LAZY(tri.d_cameras, MEM_DEVICE),
    LAZY(views.d_offsets, MEM_DEVICE), LAZY(views.d_obs, MEM_DEVICE), LAZY(views.d_stats, MEM_DEVICE), LAZY(views.h_stats, MEM_PINNED), LAZY(views.d_scratch, MEM_DEVICE),
    LAZY(cams.d_refined, MEM_DEVICE), LAZY(cams.d_stats, MEM_DEVICE), LAZY(cams.h_stats, MEM_PINNED),
    PAIR_RESULTS(PR_FILTERED), PAIR_RESULTS(PR_VERIFY_H), PAIR_RESULTS(PR_VERIFY_F), PAIR_RESULTS(PR_REFINE_H), PAIR_RESULTS(PR_REFINE_F), PAIR_RESULTS(PR_GUIDED),
    LAZY(d_dl, MEM_DEVICE), LAZY(h_dl, MEM_PINNED), LAZY(dl_row, MEM_HEAP), LAZY(h_post[0], MEM_PINNED), LAZY(h_post[1], MEM_PINNED),
    LAZY(d_kps, MEM_DEVICE), LAZY(h_kps, MEM_PINNED), LAZY(d_placed, MEM_DEVICE), LAZY(h_placed, MEM_PINNED), LAZY(placed_seq, MEM_HEAP),
};
#define N_BLOCKS (sizeof(blocks) / sizeof(blocks[0]))

static size_t block_bytes(const struct vksift_Instance_T *inst, const Block *b, const ScratchDims *d)
{
  const uint64_t per[] = {
      [N_ONE] = 1,
      [N_BUFFERS] = inst->cfg.sift_buffer_count,
      [N_FEAT_STRIDE] = inst->buf_stride * inst->cfg.sift_buffer_count,
      [N_SLOTS] = inst->batch_cap,
      [N_MATCH_STRIDE] = inst->match_slot_stride * inst->batch_cap,
      [N_REDO_STRIDE] = inst->redo_slot_stride * inst->batch_cap,
      [N_PIXELS] = (uint64_t)inst->max_image_size * d->cap,
      [N_SEG] = d->seg * d->cap,
      [N_CAND] = d->cand * d->cap,
      [N_OCTAVES] = (uint64_t)VKSIFT_MAX_OCTAVES * d->cap,
      [N_KEYPOINTS] = inst->ori_cap * d->cap,
  };
  return (size_t)(b->elem * per[b->per]);
}

/* (the fields have various pointer types: read and written as bytes) */
static void *field_get(const void *field) { void *p; memcpy(&p, field, sizeof(p)); return p; }
static void field_set(void *field, void *p) { memcpy(field, &p, sizeof(p)); }

bool mem_ensure(void *field, size_t bytes, MemKind kind)
{
  if (!field_get(field))
    field_set(field, kind == MEM_DEVICE ? vksift_hip_malloc(bytes) : kind == MEM_PINNED ? vksift_hip_host_malloc(bytes) : calloc(1, bytes));
  return field_get(field) != NULL;
}

void mem_release(void *field, MemKind kind)
{
  void (*const release[])(void *) = {[MEM_DEVICE] = vksift_hip_free, [MEM_PINNED] = vksift_hip_host_free, [MEM_HEAP] = free};
  release[kind](field_get(field));
  field_set(field, NULL);
}

static bool alloc_blocks(vksift_Instance inst, unsigned when_mask, const ScratchDims *d)
{
  for (size_t i = 0; i < N_BLOCKS; i++)
    if ((when_mask >> blocks[i].when & 1u) && !mem_ensure((uint8_t *)inst + blocks[i].field, block_bytes(inst, &blocks[i], d), (MemKind)blocks[i].kind))
      return false;
  return true;
}

static void release_blocks(vksift_Instance inst, unsigned when_mask)
{
  for (size_t i = 0; i < N_BLOCKS; i++)
    if (when_mask >> blocks[i].when & 1u)
      mem_release((uint8_t *)inst + blocks[i].field, (MemKind)blocks[i].kind);
}

bool mem_fit_staging(vksift_Instance inst, size_t bytes, bool may_shrink)
{
  /* the batch path follows the workload down as well as up: a pair more than four times what is needed (and beyond 64 MB) is released
   * instead of being kept for the life of the instance */
  const bool oversized = inst->dl_cap > ((size_t)64 << 20) && inst->dl_cap / 4u > bytes + 4096u;
  if (bytes <= inst->dl_cap && !(may_shrink && oversized))
    return true;
  mem_release(&inst->d_dl, MEM_DEVICE);
  mem_release(&inst->h_dl, MEM_PINNED);
  const size_t cap = bytes + bytes / 4u + 4096u;
  const bool d = mem_ensure(&inst->d_dl, cap, MEM_DEVICE), h = mem_ensure(&inst->h_dl, cap, MEM_PINNED);
  inst->dl_cap = (d && h) ? cap : 0;
  if (!inst->dl_cap)
  {
    mem_release(&inst->d_dl, MEM_DEVICE);
    mem_release(&inst->h_dl, MEM_PINNED);
  }
  return inst->dl_cap != 0;
}

/* ------------------------------------------------------------------------------------------------ */
/* streams and events                                                                               */
/* ------------------------------------------------------------------------------------------------ */
/* `count` handles `step` bytes apart; in the order of creation, the instance stream first (the scale-space is placed right behind it) */
typedef struct
{
  size_t field;
  uint16_t count, step;
  bool is_stream, lazy; /* lazy: created by its user (vksift_buffers.c, vksift_verify.c, vksift_guided.c, vksift_tracks.c, vksift_track_edges.c, vksift_observations.c, vksift_triangulate.c, vksift_cameras.c, vksift_pairs.c, vksift_describe.c), destroyed here */
} Handle;
#define EVENTS(f, n, step, lazy) {FIELD(f), n, step, false, lazy}
#define STREAM(f) {FIELD(f), 1, 0, true, false}
#define TIMER(which, lazy) EVENTS(timer[which].ev, 2, sizeof(vksift_hip_event), lazy) /* a StageTimer's pair (vksift_pairs.c) */
static const Handle handles[] = {
    STREAM(stream), STREAM(pyr_stream), STREAM(dl_stream), STREAM(up_stream),
    EVENTS(ev_pyr_done, 1, 0, false), EVENTS(ev_desc_start, 1, 0, false), EVENTS(ev_input_free, 1, 0, false),
    EVENTS(ev_pyr_free, 2, sizeof(vksift_hip_event), false), EVENTS(ev_fork, VKSIFT_MAX_OCTAVES, sizeof(vksift_hip_event), false),
    EVENTS(ev_join, 2, sizeof(vksift_hip_event), false), STREAM(side_stream),
    EVENTS(det_ring[0].ev, VKSIFT_DETECT_RING, sizeof(DetectSlot), false), EVENTS(ev_match, 1, 0, false), EVENTS(ev_staging, 1, 0, false),
    EVENTS(ev_up, VKSIFT_UP_GROUPS, sizeof(vksift_hip_event), false),
    EVENTS(prof[0].ev_t, 8, sizeof(vksift_hip_event), false), EVENTS(prof[1].ev_t, 8, sizeof(vksift_hip_event), false),
    EVENTS(prof[0].ev_pt, 3, sizeof(vksift_hip_event), false), EVENTS(prof[1].ev_pt, 3, sizeof(vksift_hip_event), false),
    EVENTS(prof[0].ev_scan, 2, sizeof(ProfSet), false), TIMER(T_MATCH, false),
    EVENTS(dl_ev, VKSIFT_DL_CHUNKS, sizeof(vksift_hip_event), true), EVENTS(ev_vtab, 1, 0, true), EVENTS(ev_gtab, 1, 0, true), EVENTS(ev_ttab, 1, 0, true), EVENTS(ev_etab, 1, 0, true), EVENTS(ev_otab, 1, 0, true), EVENTS(ev_ctab, 1, 0, true), EVENTS(ev_kps, 1, 0, true),
    TIMER(T_VERIFY, true), TIMER(T_REFINE_H, true), TIMER(T_REFINE_F, true), TIMER(T_GUIDED, true), TIMER(T_BUDGET, true), TIMER(T_BUDGET_GRID, true), TIMER(T_ROOTSIFT, true), TIMER(T_TRACKS, true), TIMER(T_OBSERVATIONS, true), TIMER(T_TRIANGULATE, true), TIMER(T_VIEWS, true), TIMER(T_CAMERAS, true), TIMER(T_ACCUMULATE, true),
};
#define N_HANDLES (sizeof(handles) / sizeof(handles[0]))

static void create_handles(vksift_Instance inst, size_t from, size_t to)
{
  for (size_t i = from; i < to; i++)
    for (uint32_t k = 0; k < handles[i].count && !handles[i].lazy; k++)
      field_set((uint8_t *)inst + handles[i].field + (size_t)k * handles[i].step, handles[i].is_stream ? vksift_hip_stream_create() : vksift_hip_event_create());
}

/* ------------------------------------------------------------------------------------------------ */
/* Where in HBM the scale-space lives (round 5; DESIGN.md §8, tools/microbench/stream_patterns.hip)    */
/* ------------------------------------------------------------------------------------------------ */
/* The strip-march launches of pyramid.hip and the extrema scan — thousands of waves each streaming its own row segment — run at
 * 4.9-5.0 TB/s on some ranges of the device's memory and at 5.9-6.1 TB/s on others, for the SAME kernel, sizes and strides: measured
 * with a pure copy in that access pattern sliding over a 240 GiB allocation of an idle MI355X, the first ~40 GB of a fresh process's
 * memory and a few later windows are the slow ones, ~75-170 GB the fast plateau; a linear copy runs at 6.2 TB/s everywhere. A fresh
 * process gets the low range first, so an instance that simply allocates its scale-space takes the slow memory. The two
 * scale-space buffers of a batch instance are therefore chosen by measurement: allocate a candidate, time one whole-batch blur
 * launch of octave 0 on it (the pattern that matters, 1 warm-up + 3 runs of ~1 ms), keep it, allocate the next — rejected candidates
 * stay allocated while the search runs, so that the allocator has to hand out new ranges — until `need` candidates run within
 * VKSIFT_PLACE_SPREAD of the best AND a slower range has been seen (the fast mode is identified), or everything looks alike, or the
 * candidate / memory budget is used up; then every candidate but the best `need` is freed. Nothing depends on it but speed.
 * VKSIFT_PYR_PLACEMENT=<max candidates> (default 7; 0 or 1: plain allocation). */
#define VKSIFT_PLACE_MAX 8
#define VKSIFT_PLACE_SPREAD 1.04f
/* a width the strip-march kernels take — the reservation's square layout may have one they leave to the generic tile kernel */
static uint32_t probe_width(const PyrLayout *L) { return L->w[0] >= 512u ? (L->w[0] & ~255u) : (L->w[0] & ~3u); }

static float placement_probe_ms(vksift_Instance inst, void *buf, uint64_t img_stride, const PyrLayout *L, vksift_hip_event e0, vksift_hip_event e1)
{
  vksift_hip_Plane src, dst;
  src.base = (float *)((uint8_t *)buf + L->gauss_off[0] * pyr_texel_bytes(inst));
  src.fp16 = inst->fp16 ? 1u : 0u, src.reverse = 0;
  src.w = probe_width(L);
  src.h = L->h[0], src.pitch = L->pitch[0], src.img_stride = img_stride;
  dst = src;
  dst.base = (float *)((uint8_t *)buf + (L->gauss_off[0] + L->plane_stride[0]) * pyr_texel_bytes(inst));
  float best = -1.f;
  for (int r = 0; r < 4; r++)
  {
    dst.reverse = (uint32_t)(r & 1);
    if (vksift_hip_event_record(e0, inst->stream) != 0 ||
        vksift_hip_blur(src, dst, &inst->taps[1 * VKSIFT_MAX_TAPS], inst->ntaps[1], inst->det_cap, inst->stream) != 0 ||
        vksift_hip_event_record(e1, inst->stream) != 0 || vksift_hip_event_sync(e1) != 0)
      return -1.f;
    const float ms = vksift_hip_event_elapsed_ms(e0, e1);
    if (r > 0 && ms > 0.f && (best < 0.f || ms < best))
      best = ms;
  }
  return best;
}

/* out[0 .. need): device blocks of `bytes` each for a scale-space of layout L (octave 0 is what gets timed); false: out of memory
 * (nothing is left allocated). may_search = false: plain allocation (re-allocations in the middle of a caller's detect call).
 * The rejected candidates of a search stay allocated while it runs — freed, the allocator would hand the same range out again —
 * so the search is bounded: the candidates together never hold more than VKSIFT_PLACE_MEM_FRACTION (55 %) of the memory that was
 * free when it started, and 24 GB stay free for the rest of the instance and for whoever else uses the device. */
static bool place_pyramid_buffers(vksift_Instance inst, size_t bytes, uint64_t img_stride, const PyrLayout *L, uint32_t need, float **out, bool may_search)
{
  const char *env = getenv("VKSIFT_PYR_PLACEMENT");
  int max_cand = env ? atoi(env) : 7;
  if (max_cand > VKSIFT_PLACE_MAX)
    max_cand = VKSIFT_PLACE_MAX;
  inst->place_n = 0;
  vksift_hip_event e0 = NULL, e1 = NULL;
  const bool search = may_search && max_cand > (int)need && inst->det_cap >= 8u && bytes >= ((size_t)256 << 20) && L->n_oct > 0 && inst->stream != NULL &&
                      (e0 = vksift_hip_event_create()) != NULL && (e1 = vksift_hip_event_create()) != NULL;
  const size_t budget = search ? (size_t)((double)vksift_hip_device_free_mem() * 0.55) : 0;
  void *cand[VKSIFT_PLACE_MAX] = {NULL};
  float ms[VKSIFT_PLACE_MAX];
  uint32_t n = 0;
  bool ok = true;
  while (n < need || (search && n < (uint32_t)max_cand))
  {
    if (n >= need)
    {
      /* another candidate only within the budget, and while the device still has room for it and the rest of an instance */
      if ((size_t)(n + 1u) * bytes > budget || vksift_hip_device_free_mem() < bytes + ((size_t)24 << 30))
        break;
      /* stop rules (sorted view of what has been timed) */
      float lo = ms[0], hi = ms[0];
      uint32_t near_best = 0;
      for (uint32_t i = 0; i < n; i++)
        lo = ms[i] < lo ? ms[i] : lo, hi = ms[i] > hi ? ms[i] : hi;
      for (uint32_t i = 0; i < n; i++)
        near_best += ms[i] <= lo * VKSIFT_PLACE_SPREAD ? 1u : 0u;
      if (near_best >= need && hi > lo * 1.08f)
        break; /* the fast mode has been seen `need` times, and a slow one beside it */
      if (n >= need + 5u && hi <= lo * VKSIFT_PLACE_SPREAD)
        break; /* this memory is all alike */
    }
    void *p = vksift_hip_malloc(bytes);
    if (!p)
    {
      ok = n >= need;
      break;
    }
    cand[n] = p;
    ms[n] = search ? placement_probe_ms(inst, p, img_stride, L, e0, e1) : 0.f;
    if (search && ms[n] <= 0.f)
      ms[n] = 1e9f; /* the probe failed: last choice */
    n++;
  }
  if (ok && n >= need)
  {
    /* the `need` fastest, the rest goes back */
    for (uint32_t k = 0; k < need; k++)
    {
      uint32_t b = 0;
      for (uint32_t i = 0; i < n; i++)
        if (cand[i] && (!cand[b] || ms[i] < ms[b]))
          b = i;
      out[k] = (float *)cand[b];
      inst->place_chosen[k] = b;
      cand[b] = NULL;
    }
    if (need == 1u)
      inst->place_chosen[1] = inst->place_chosen[0];
    float slowest = 0.f;
    for (uint32_t i = 0; i < n; i++)
    {
      const double px = (double)probe_width(L) * L->h[0] * inst->det_cap * 2.0 * (double)pyr_texel_bytes(inst);
      inst->place_gbps[i] = (search && ms[i] < 1e8f) ? (float)(px / (ms[i] * 1e-3) / 1e9) : 0.f;
      if (inst->place_gbps[i] > 0.f && (slowest == 0.f || inst->place_gbps[i] < slowest))
        slowest = inst->place_gbps[i];
    }
    inst->place_n = search ? n : 0;
    if (search)
      logInfo(LOG_TAG, "scale-space placement: %u candidate range(s) of %.1f GB timed, chosen %.0f GB/s, slowest %.0f GB/s", n, bytes / 1e9,
              inst->place_gbps[inst->place_chosen[0]], slowest);
  }
  else
    ok = false;
  for (uint32_t i = 0; i < n; i++)
    vksift_hip_free(cand[i]); /* NULL for the chosen ones */
  vksift_hip_event_destroy(e0);
  vksift_hip_event_destroy(e1);
  if (!ok)
    for (uint32_t k = 0; k < need; k++)
      out[k] = NULL;
  return ok;
}

/* ------------------------------------------------------------------------------------------------ */
/* creation, growth, release                                                                        */
/* ------------------------------------------------------------------------------------------------ */
/* Reserves device memory for the configured maxima (det_cap images of layout L, the square of input_image_max_size pixels) and creates the
 * streams and events. The caller has set cfg, S, fp16, batch_cap, det_cap, max_octaves, max_image_size, the taps,
 * pyr_nbuf and the switches. false: something the instance cannot do without is missing (mem_destroy releases what exists). */
bool mem_create(vksift_Instance inst, const PyrLayout *L)
{
  const vksift_Config *config = &inst->cfg;
  const ScratchDims d = reserve_for(L, inst->det_cap);
  inst->pyr_img_stride = d.pyr, inst->seg_cap = d.seg, inst->cand_cap = d.cand;
  inst->ori_cap = config->max_nb_sift_per_buffer; /* a single-octave detection gives the largest section */
  inst->buf_stride = ((uint64_t)config->max_nb_sift_per_buffer * FEAT_BYTES + 255u) & ~(uint64_t)255u;
  inst->desc_slot_stride = (((uint64_t)config->max_nb_sift_per_buffer * 128u + 256u) + 255u) & ~(uint64_t)255u;
  inst->match_slot_stride = (((uint64_t)config->max_nb_sift_per_buffer * MATCH_BYTES) + 255u) & ~(uint64_t)255u;
  inst->redo_slot_stride = (uint64_t)config->max_nb_sift_per_buffer + 32u;
  inst->cache_norm_stride = (uint64_t)config->max_nb_sift_per_buffer + 32u;
  if (!alloc_blocks(inst, 1u << AT_CREATION | 1u << PER_STRIDE | 1u << PER_CAPACITY, &d))
    return false;
  /* All streams at the default priority: a high-priority instance stream with low-priority octave streams was measured
   * 20 % slower on MI355X (11.3k vs 14.1k frames/s). */
  create_handles(inst, 0, 1);
  /* first of the large blocks after the stream: candidates need room, and everything allocated before stays where it is */
  if (!place_pyramid_buffers(inst, pyr_texel_bytes(inst) * d.pyr * d.cap, d.pyr, L, inst->pyr_nbuf, inst->d_pyr_buf, true))
    return false;
  inst->d_pyr = inst->d_pyr_buf[0];
  create_handles(inst, 1, N_HANDLES);
  if (!inst->side_stream || !inst->ev_join[0] || !inst->ev_join[1])
    inst->fork_scales = false;
  for (int i = 0; i < VKSIFT_MAX_OCTAVES; i++)
    if (!inst->ev_fork[i])
      inst->fork_scales = false;
  return inst->stream && inst->det_ring[0].ev && inst->det_ring[VKSIFT_DETECT_RING - 1].ev && inst->ev_match && inst->pyr_stream && inst->dl_stream &&
         inst->up_stream;
}

static void free_detect_scratch(vksift_Instance inst, bool cap_blocks)
{
  mem_release(&inst->d_pyr_buf[0], MEM_DEVICE);
  mem_release(&inst->d_pyr_buf[1], MEM_DEVICE);
  inst->d_pyr = NULL;
  release_blocks(inst, 1u << PER_STRIDE);
  if (cap_blocks)
    release_blocks(inst, 1u << PER_CAPACITY);
}

static bool alloc_detect_scratch(vksift_Instance inst, const PyrLayout *L, const ScratchDims *d, bool cap_blocks, bool may_search)
{
  const uint32_t old_cap = inst->det_cap;
  inst->det_cap = (uint32_t)d->cap; /* the placement probe launches on `det_cap` images */
  const bool ok = place_pyramid_buffers(inst, pyr_texel_bytes(inst) * d->pyr * d->cap, d->pyr, L, inst->pyr_nbuf, inst->d_pyr_buf, may_search);
  inst->det_cap = old_cap;
  return ok && alloc_blocks(inst, 1u << PER_STRIDE, d) && (!cap_blocks || alloc_blocks(inst, 1u << PER_CAPACITY, d));
}

/* The re-allocation of resize_detect_scratch (vksift_instance.c, which has drained the instance): L != NULL, the per-image strides grow to
 * what that layout needs; new_cap != det_cap, the blocks grow to new_cap images. Return values: see there. */
int mem_resize_scratch(vksift_Instance inst, const PyrLayout *L, uint32_t new_cap)
{
  PyrLayout cur;
  if (!L)
  {
    /* capacity growth alone: the layout the probe launch runs on is the reservation's */
    const uint32_t side = (uint32_t)ceilf(sqrtf((float)inst->cfg.input_image_max_size));
    compute_layout(inst, inst->cur_w ? inst->cur_w : side, inst->cur_h ? inst->cur_h : side, &cur);
  }
  const PyrLayout *PL = L ? L : &cur;
  ScratchDims d = L ? reserve_for(L, new_cap) : (ScratchDims){new_cap, 0, 0, 0};
  d.pyr = d.pyr > inst->pyr_img_stride ? d.pyr : inst->pyr_img_stride;
  d.seg = d.seg > inst->seg_cap ? d.seg : inst->seg_cap;
  d.cand = d.cand > inst->cand_cap ? d.cand : inst->cand_cap;
  const uint32_t old_cap = inst->det_cap;
  const bool cap_blocks = new_cap != old_cap || inst->d_input == NULL; /* (NULL: lost by an earlier attempt that ran out of memory) */
  /* old blocks first: the pyramid is the largest allocation of the instance, two generations of it may not fit */
  free_detect_scratch(inst, cap_blocks);
  int rc = 0;
  /* (a capacity growth happens once per size, outside any detection that runs: it may search for fast memory; a stride growth sits in
   * the middle of a detect call of whatever the caller is doing and takes plain allocations) */
  bool ok = alloc_detect_scratch(inst, PL, &d, cap_blocks, cap_blocks);
  if (!ok && cap_blocks)
  {
    /* the larger capacity does not fit: back to the one the instance had */
    free_detect_scratch(inst, true);
    d.cap = old_cap;
    ok = alloc_detect_scratch(inst, PL, &d, true, false);
    rc = 1;
  }
  if (!ok)
  {
    free_detect_scratch(inst, cap_blocks);
    inst->pyr_img_stride = 0, inst->seg_cap = 0, inst->cand_cap = 0;
    return -1;
  }
  inst->pyr_img_stride = d.pyr, inst->seg_cap = d.seg, inst->cand_cap = d.cand;
  inst->det_cap = (uint32_t)d.cap;
  inst->d_pyr = inst->d_pyr_buf[inst->pyr_nbuf == 2u ? inst->pyr_cur : 0];
  return rc;
}

/* every block, event and stream of the instance, whoever allocated it; the caller has drained the streams. Takes a half-constructed
 * instance (the shims and free() accept NULL). */
void mem_destroy(vksift_Instance inst)
{
  release_blocks(inst, ~0u);
  inst->d_pyr = NULL;
  for (size_t i = 0; i < N_HANDLES; i++)
    for (uint32_t k = 0; k < handles[i].count; k++)
    {
      void *field = (uint8_t *)inst + handles[i].field + (size_t)k * handles[i].step;
      (handles[i].is_stream ? vksift_hip_stream_destroy : vksift_hip_event_destroy)(field_get(field));
      field_set(field, NULL);
    }
}
