/*
 * vksift_detect.h — what the launch sequences over a scale-space share (vksift_detect.c: a detection; vksift_describe.c: caller-supplied keypoints in
 * place of the extraction stage): the plan of a call, and the steps of vksift_detect.c that both queue. Private, like vksift_internal.h.
 */
#ifndef VKSIFT_DETECT_H
#define VKSIFT_DETECT_H

#include "vksift_internal.h"

/* ------------------------------------------------------------------------------------------------ */
/* the launch sequence of one detection                                                             */
/* ------------------------------------------------------------------------------------------------ */
#define TRY(expr, what)                                                        \
  do                                                                           \
  {                                                                            \
    int _e = (expr);                                                           \
    if (_e != 0)                                                               \
    {                                                                          \
      logError(LOG_TAG, "%s failed: %s", what, vksift_hip_error_string(_e));   \
      return _e;                                                               \
    }                                                                          \
  } while (0)
/* TRY between vksift_hip_range_push and its vksift_hip_range_pop: the failure exit closes the range it leaves */
#define TRY_IN_RANGE(expr, what)                                               \
  do                                                                           \
  {                                                                            \
    int _e = (expr);                                                           \
    if (_e != 0)                                                               \
    {                                                                          \
      logError(LOG_TAG, "%s failed: %s", what, vksift_hip_error_string(_e));   \
      vksift_hip_range_pop();                                                  \
      return _e;                                                               \
    }                                                                          \
  } while (0)


/* ------------------------------------------------------------------------------------------------ */
/* the plan of one detection                                                                        */
/* ------------------------------------------------------------------------------------------------ */
/* plan_detection() fills everything down to jobs[], each field from the ones above it (named in its comment) — no GPU call, no
 * allocation, no write to the instance. After it only the last block changes: what prepare_detection(), the graph driver and the
 * answers of the optional launchers decide. Stage functions that decide nothing take a const DetectCtx *. */
typedef struct
{
  vksift_Instance inst;
  const PyrLayout *L; /* inst->lay, fitted to (w, h) before the plan */
  ProfSet *PS;        /* the event set of this call, recycled before the plan */
  const uint8_t *const *images; /* argument: the caller's host images, staged chunk by chunk while the sequence is enqueued */
  uint32_t w, h, count, first_buf; /* arguments */
  size_t img_bytes;
  bool prestaged; /* argument: the images are in h_input already (deferred vksift_detectFeatures calls): nothing to stage */
  bool prof;      /* HIP-event stage timings requested */
  bool upload;    /* images, prestaged: host images are (to be) staged in h_input and have to reach the GPU */
  bool overlap;   /* L, count: scale-space on its own stream and buffer (ping-pong), see plan_detection */
  int pyr_buf;    /* overlap: the pyramid buffer of this call (prepare_detection makes it the instance's current one) ... */
  float *d_pyr;   /* ... and its address: every plane of this call is addressed from here (plane_at) */
  bool zero_copy; /* upload, count: one host image: the seed launch reads it straight out of the pinned staging buffer (no copy to d_input in front of it) */
  const uint8_t *d_src; /* upload, zero_copy */
  bool fork;       /* overlap, prof, count: scales S+1.. of every octave on the side stream (vksift_internal.h: ev_fork) */
  bool tail_batch; /* fork, count: a batch queues scales S+1, S+2 of its coarser octaves per SCALE (enqueue_tail), like a forked detection does */
  /* "How far is octave o queued on the trunk": tail[o] = its per-scale launches stop at scale S (the path to the next octave), scales S+1, S+2
   * go with enqueue_tail; chain_from = first octave the LDS chain builds instead (L->n_oct: none). tail[] is planned for the chain's octaves
   * too: it is what they take when the chain launcher declines (in_tail()). */
  bool tail[VKSIFT_MAX_OCTAVES]; /* fork, tail_batch, L */
  uint32_t chain_from;           /* fork, L */
  uint32_t up_per; /* upload, count, gpu_busy (argument: an earlier detection was still running when this one came in): groups of this many images ... */
  bool grouped;    /* ... unless the sequence is captured (upload_grouped()) */
  bool dense;      /* L: the descriptor launch also writes the buffers' matcher cache entries (vksift_hip_DenseRows) */
  bool post_ok;    /* L, count: eligible for feature posting, post_bytes of records (vksift_internal.h: h_post) */
  uint64_t post_bytes;
  bool replay_ok;  /* prof, overlap, count: eligible for hipGraph replay */
  uint64_t alg_bytes, scan_bytes; /* L, count: profiling figures */
  vksift_hip_OctaveJob jobs[VKSIFT_MAX_OCTAVES]; /* d_pyr, L, first_buf (scan_reverse, masks_cleared: launch time) */

  /* decided after the plan */
  bool post;       /* prepare_detection: feature posting at the end of the sequence (the slots exist, the caller still fetches) */
  bool capturing;  /* launch_detection: the sequence is being captured into a hipGraph: no host-visible events inside */
  bool g0_done;    /* launchers: plane 0 of the next octave was written by the previous octave's fused scale-S pass */
  bool chain_done; /* launchers: vksift_hip_octave_chain took octaves chain_from.. */
  uint32_t nblur;     /* blur launches of octave 0 (the profiled scale-space interval) */
  uint32_t nblur_all; /* ... of every octave */
} DetectCtx;

static inline bool upload_grouped(const DetectCtx *c) { return c->grouped && !c->capturing; }
static inline bool in_tail(const DetectCtx *c, uint32_t o) { return c->tail[o] && !(c->chain_done && o >= c->chain_from); }
/* per-octave counters of SIFT buffer `buf` on the device / their host mirror */
static inline uint32_t *found_dev(vksift_Instance inst, uint32_t buf) { return inst->d_found + (size_t)buf * VKSIFT_MAX_OCTAVES; }
static inline uint32_t *found_host(vksift_Instance inst, uint32_t buf) { return inst->h_found + (size_t)buf * VKSIFT_MAX_OCTAVES; }
static inline const float *scale_taps(vksift_Instance inst, uint32_t s) { return &inst->taps[s * VKSIFT_MAX_TAPS]; }
/* dispatch direction of the n-th launch of a chain (vksift_hip_Plane::reverse) */
static inline uint32_t alt_dir(vksift_Instance inst, uint32_t n) { return inst->alt_order ? (n & 1u) : 0u; }
static inline void prof_mark(const DetectCtx *c, vksift_hip_event ev, vksift_hip_stream s) { if (c->prof) vksift_hip_event_record(ev, s); }
/* The optional launchers answer 0: launched, -1: the shape is not covered and nothing was launched, > 0: a HIP error.
 * TRY(optional(launcher(...), &done), what); if (!done) <the fall-back launches> */
static inline int optional(int e, bool *done) { *done = e == 0; return e > 0 ? e : 0; }

/* vksift_detect.c: the steps of a detection that vksift_describe.c queues as well (see there for each) */
VKSIFT_INTERNAL int pyr_last_reader(vksift_Instance inst, vksift_hip_stream s);
VKSIFT_INTERNAL void plan_detection(DetectCtx *c, vksift_Instance inst, const uint8_t *const *images, const uint8_t *d_images, bool prestaged, uint32_t count,
                                    uint32_t w, uint32_t h, uint32_t first_buf, bool gpu_busy);
VKSIFT_INTERNAL int prepare_detection(DetectCtx *c);
VKSIFT_INTERNAL int enqueue_upload(DetectCtx *c, vksift_hip_stream sp);
VKSIFT_INTERNAL int enqueue_scale_space(DetectCtx *c, vksift_hip_stream sp);
VKSIFT_INTERNAL vksift_hip_DenseRows dense_rows(const DetectCtx *c);
VKSIFT_INTERNAL void invalid_input(vksift_Instance inst, const char *fn);
VKSIFT_INTERNAL int fit_layout(vksift_Instance inst, uint32_t w, uint32_t h);
VKSIFT_INTERNAL int finish_detection(const DetectCtx *c);
VKSIFT_INTERNAL void detect_failed(vksift_Instance inst, const DetectCtx *c, const char *fn);
VKSIFT_INTERNAL bool ext_batch_count_valid(vksift_Instance inst, uint32_t count, const char *fn);

#endif
