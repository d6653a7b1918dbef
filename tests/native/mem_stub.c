/*
 * mem_stub.c — vksift_mem.c against a counting stub of the device shims it calls (tests/test_mem_ownership.py; no GPU). The stub hands out
 * fake addresses that nobody dereferences, keeps a ledger of what is live (kind, bytes) and a log of the calls, and can fail the k-th
 * allocation / handle creation or enforce a device byte budget. main() is a small command interpreter over the module's entry points:
 * the scenarios and every assertion are in the Python test, this file only reports.
 */
#include "vksift_internal.h"

#include <stdio.h>

/* ------------------------------------------------------------------------------------------------ the stub */
#define MAX_ENTRIES 8192
typedef struct
{
  void *handle;
  char kind; /* D device, H pinned, E event, S stream */
  size_t bytes;
  bool live;
} Entry;
static Entry ledger[MAX_ENTRIES];
static uint32_t n_entries, bad_free;
static uintptr_t next_addr = 0x100000;
static uint64_t fail_alloc_in, fail_handle_in; /* 1: the next one fails */
static uint64_t budget, device_live;           /* budget 0: none */
static const uint64_t device_total = (uint64_t)288 << 30;
static const void *probed[16];
static uint32_t n_probed;

static void *acquire(char kind, size_t bytes)
{
  uint64_t *countdown = (kind == 'D' || kind == 'H') ? &fail_alloc_in : &fail_handle_in;
  const bool injected = *countdown && --*countdown == 0;
  if (injected || (kind == 'D' && budget && device_live + bytes > budget) || n_entries == MAX_ENTRIES)
  {
    printf("call %c %zu FAILED\n", kind, bytes);
    return NULL;
  }
  Entry *e = &ledger[n_entries++];
  e->handle = (void *)next_addr, e->kind = kind, e->bytes = bytes, e->live = true;
  next_addr += ((uintptr_t)bytes + 0xfff) & ~(uintptr_t)0xfff;
  next_addr += 0x1000;
  device_live += kind == 'D' ? bytes : 0;
  printf("call %c %zu\n", kind, bytes);
  return e->handle;
}

static Entry *find_live(const void *p)
{
  for (uint32_t i = 0; i < n_entries; i++)
    if (ledger[i].live && ledger[i].handle == p)
      return &ledger[i];
  return NULL;
}

static void release(char kind, void *p)
{
  if (!p)
    return;
  Entry *e = find_live(p);
  if (!e || e->kind != kind)
  {
    bad_free++; /* freed twice, never handed out, or through the wrong shim */
    printf("call free%c BAD\n", kind);
    return;
  }
  e->live = false;
  device_live -= kind == 'D' ? e->bytes : 0;
  printf("call free%c %zu\n", kind, e->bytes);
}

void *vksift_hip_malloc(size_t bytes) { return acquire('D', bytes); }
void vksift_hip_free(void *p) { release('D', p); }
void *vksift_hip_host_malloc(size_t bytes) { return acquire('H', bytes); }
void vksift_hip_host_free(void *p) { release('H', p); }
vksift_hip_stream vksift_hip_stream_create(void) { return acquire('S', 0); }
void vksift_hip_stream_destroy(vksift_hip_stream s) { release('S', s); }
vksift_hip_event vksift_hip_event_create(void) { return acquire('E', 0); }
void vksift_hip_event_destroy(vksift_hip_event e) { release('E', e); }
int vksift_hip_event_record(vksift_hip_event e, vksift_hip_stream s) { return (e && s) ? 0 : 1; }
int vksift_hip_event_sync(vksift_hip_event e) { return e ? 0 : 1; }
size_t vksift_hip_device_free_mem(void) { return (size_t)(device_total - device_live); }
/* the placement probe: every second range it is shown is a slow one (the first one too, like a fresh process's low memory) */
int vksift_hip_blur(vksift_hip_Plane src, vksift_hip_Plane dst, const float *taps, uint32_t ntaps, uint32_t batch, vksift_hip_stream s)
{
  (void)dst, (void)taps, (void)ntaps, (void)batch, (void)s;
  if ((n_probed == 0 || probed[n_probed - 1] != src.base) && n_probed < 16)
    probed[n_probed++] = src.base;
  return 0;
}
float vksift_hip_event_elapsed_ms(vksift_hip_event a, vksift_hip_event b)
{
  (void)a, (void)b;
  return (n_probed & 1u) ? 1.3f : 1.0f;
}

/* ------------------------------------------------------------------------------------------------ the driver */
static vksift_Instance inst;

static void new_instance(uint32_t batch_cap, uint32_t max_px, uint32_t max_feats, uint32_t nbuf, uint32_t pyr_nbuf)
{
  inst = (vksift_Instance)calloc(1, sizeof(*inst));
  vksift_Config *c = &inst->cfg;
  c->input_image_max_size = max_px, c->sift_buffer_count = nbuf, c->max_nb_sift_per_buffer = max_feats;
  c->use_input_upsampling = true, c->nb_scales_per_octave = 3, c->input_image_blur_level = 0.5f, c->seed_scale_sigma = 1.6f;
  c->use_hardware_interpolated_blur = true;
  inst->S = c->nb_scales_per_octave;
  inst->batch_cap = inst->det_cap = batch_cap;
  inst->pyr_nbuf = pyr_nbuf;
  inst->fork_scales = true;
  inst->max_octaves = vksift_hm_max_octaves(c, &inst->max_image_size);
  vksift_hm_blur_taps(c, inst->taps, inst->ntaps);
}

typedef struct
{
  const char *name;
  void *field;
  MemKind kind;
} Named;
#define NAMED(f, kind) {#f, &inst->f, kind}

int main(int argc, char **argv)
{
  setvbuf(stdout, NULL, _IOLBF, 0);
  vksift_log_set_level(VKSIFT_LOGLVL_NONE);
  for (int a = 1; a < argc; a++)
  {
    const char *cmd = argv[a];
#define ARG() strtoull(a + 1 < argc ? argv[++a] : "0", NULL, 10)
    if (!strcmp(cmd, "new"))
    {
      const uint32_t bc = (uint32_t)ARG(), px = (uint32_t)ARG(), feats = (uint32_t)ARG(), nbuf = (uint32_t)ARG(), pyr_nbuf = (uint32_t)ARG();
      new_instance(bc, px, feats, nbuf, pyr_nbuf);
    }
    else if (!strcmp(cmd, "create"))
    {
      const uint32_t side = (uint32_t)ceilf(sqrtf((float)inst->cfg.input_image_max_size));
      PyrLayout L;
      compute_layout(inst, side, side, &L);
      const bool ok = mem_create(inst, &L);
      inst->cur_w = inst->cur_h = side;
      printf("create ok=%d fork_scales=%d place_n=%u chosen=%u\n", ok, inst->fork_scales, inst->place_n, inst->place_chosen[0]);
    }
    else if (!strcmp(cmd, "fail"))
      fail_alloc_in = ARG();
    else if (!strcmp(cmd, "failh"))
      fail_handle_in = ARG();
    else if (!strcmp(cmd, "budget"))
      budget = ARG();
    else if (!strcmp(cmd, "resize"))
    {
      const uint32_t cap = (uint32_t)ARG(), w = (uint32_t)ARG(), h = (uint32_t)ARG();
      PyrLayout L;
      if (w)
        compute_layout(inst, w, h, &L);
      const int rc = mem_resize_scratch(inst, w ? &L : NULL, cap ? cap : inst->det_cap);
      printf("resize rc=%d det_cap=%u pyr=%llu seg=%llu cand=%llu d_pyr=%d\n", rc, inst->det_cap, (unsigned long long)inst->pyr_img_stride,
             (unsigned long long)inst->seg_cap, (unsigned long long)inst->cand_cap, inst->d_pyr != NULL && inst->d_pyr == inst->d_pyr_buf[0]);
    }
    else if (!strcmp(cmd, "dims")) /* what the reservation of a w x h image is, for the test's own arithmetic */
    {
      const uint32_t w = (uint32_t)ARG(), h = (uint32_t)ARG();
      PyrLayout L;
      compute_layout(inst, w, h, &L);
      printf("dims img_floats=%llu seg_total=%llu cand_total=%llu max_image_size=%u\n", (unsigned long long)L.img_floats, (unsigned long long)L.seg_total,
             (unsigned long long)L.cand_total, inst->max_image_size);
    }
    else if (!strcmp(cmd, "sizes"))
    {
      const Named scratch[] = {NAMED(d_pyr_buf[0], MEM_DEVICE), NAMED(d_pyr_buf[1], MEM_DEVICE), NAMED(d_seg_mask, MEM_DEVICE), NAMED(d_seg_off, MEM_DEVICE),
                               NAMED(d_cand_xy, MEM_DEVICE), NAMED(d_cand_flag, MEM_DEVICE), NAMED(d_input, MEM_DEVICE), NAMED(h_input, MEM_PINNED),
                               NAMED(d_cand_n, MEM_DEVICE), NAMED(d_ori_ang, MEM_DEVICE), NAMED(d_ori_cnt, MEM_DEVICE)};
      for (size_t i = 0; i < sizeof(scratch) / sizeof(scratch[0]); i++)
      {
        void *p;
        memcpy(&p, scratch[i].field, sizeof(p));
        const Entry *e = p ? find_live(p) : NULL;
        printf("size %s %lld\n", scratch[i].name, p == NULL ? -1ll : e ? (long long)e->bytes : -2ll); /* -2: points at nothing live */
      }
    }
    else if (!strcmp(cmd, "ensure") || !strcmp(cmd, "lazy"))
    {
      /* every block and event that somebody else allocates on first use (the ELSEWHERE rows of blocks[], the lazy rows of handles[]) */
      const Named lazy[] = {NAMED(d_cache_desc, MEM_DEVICE), NAMED(d_cache_norm, MEM_DEVICE), NAMED(d_match_partial, MEM_DEVICE), NAMED(h_matches, MEM_PINNED),
                            NAMED(rev.matches, MEM_DEVICE),  NAMED(rev.redo, MEM_DEVICE),     NAMED(rev.match_n, MEM_DEVICE),     NAMED(res[PR_FILTERED].d_payload, MEM_DEVICE),
                            NAMED(res[PR_FILTERED].d_words, MEM_DEVICE), NAMED(res[PR_FILTERED].h_words, MEM_PINNED), NAMED(filt_ids, MEM_HEAP), NAMED(d_corr, MEM_DEVICE),
                            NAMED(res[PR_VERIFY_H].d_payload, MEM_DEVICE), NAMED(res[PR_VERIFY_H].d_words, MEM_DEVICE), NAMED(d_vscratch, MEM_DEVICE), NAMED(res[PR_VERIFY_H].h_words, MEM_PINNED),
                            NAMED(h_vtab, MEM_PINNED),       NAMED(dl_row, MEM_HEAP),         NAMED(h_post[0], MEM_PINNED),       NAMED(h_post[1], MEM_PINNED)};
      const size_t n = sizeof(lazy) / sizeof(lazy[0]);
      if (!strcmp(cmd, "lazy"))
      {
        bool ok = mem_fit_staging(inst, 1000, false);
        for (size_t i = 0; i < n; i++)
          ok = mem_ensure(lazy[i].field, 64 + i, lazy[i].kind) && ok;
        for (uint32_t k = 0; k < VKSIFT_DL_CHUNKS; k++)
          inst->dl_ev[k] = vksift_hip_event_create();
        inst->ev_vtab = vksift_hip_event_create(), inst->timer[T_VERIFY].ev[0] = vksift_hip_event_create(), inst->timer[T_VERIFY].ev[1] = vksift_hip_event_create();
        printf("lazy ok=%d\n", ok);
      }
      else
      {
        const char *name = a + 1 < argc ? argv[++a] : "";
        const size_t bytes = (size_t)ARG();
        for (size_t i = 0; i < n; i++)
          if (!strcmp(name, lazy[i].name))
            printf("ensure %s ok=%d\n", name, mem_ensure(lazy[i].field, bytes, lazy[i].kind));
      }
    }
    else if (!strcmp(cmd, "fit"))
    {
      const size_t bytes = (size_t)ARG();
      const bool may_shrink = ARG() != 0;
      const bool ok = mem_fit_staging(inst, bytes, may_shrink);
      printf("fit ok=%d cap=%zu d_dl=%d h_dl=%d\n", ok, inst->dl_cap, inst->d_dl != NULL, inst->h_dl != NULL);
    }
    else if (!strcmp(cmd, "destroy"))
    {
      mem_destroy(inst);
      free(inst);
      inst = NULL;
    }
    else if (!strcmp(cmd, "ledger"))
    {
      uint32_t live = 0;
      for (uint32_t i = 0; i < n_entries; i++)
        if (ledger[i].live)
          live++, printf("live %c %zu\n", ledger[i].kind, ledger[i].bytes);
      printf("ledger live=%u bad_free=%u device_live=%llu\n", live, bad_free, (unsigned long long)device_live);
    }
    else
    {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  return 0;
}
