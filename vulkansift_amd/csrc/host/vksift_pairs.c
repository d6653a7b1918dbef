/*
 * vksift_pairs.c — what the stages behind a filtered matching share on the host (vksift_match.c, vksift_verify.c, vksift_refine.c,
 * vksift_guided.c, vksift_strongest.c): the timer of a stage's interval, the frame around its launches, and the storage, lifetime and
 * accessors of what it keeps per pair (PairResults). One definition of each; a stage file holds its validation, its launches and a table
 * of names.
 */
#include "vksift_internal.h"

/* ------------------------------------------------------------------------------------------------ */
/* stage timers                                                                                     */
/* ------------------------------------------------------------------------------------------------ */
static int timer_start(vksift_Instance inst, StageTimer *t)
{
  if (!inst->profiling)
    return 0;
  for (int i = 0; i < 2; i++)
    if (!t->ev[i] && !(t->ev[i] = vksift_hip_event_create()))
      return 2; /* hipErrorOutOfMemory */
  return vksift_hip_event_record(t->ev[0], inst->stream);
}

static int timer_stop(vksift_Instance inst, StageTimer *t)
{
  if (!inst->profiling)
    return 0;
  const int e = vksift_hip_event_record(t->ev[1], inst->stream);
  t->valid = e == 0; /* (an interval whose end was never recorded is none) */
  return e;
}

float timer_read(vksift_Instance inst, uint32_t which)
{
  const StageTimer *t = &inst->timer[which];
  defer_sync(inst);
  if (!inst->profiling || !t->valid)
    return -1.f;
  vksift_hip_set_device(inst->device);
  if (wait_all(inst) != 0)
  {
    logError(LOG_TAG, "stage time: the stream synchronisation failed.");
    inst->error_cb(VKSIFT_VULKAN_ERROR);
    return -1.f;
  }
  return vksift_hip_event_elapsed_ms(t->ev[0], t->ev[1]);
}

void timers_reset(vksift_Instance inst)
{
  for (uint32_t i = 0; i < T_COUNT; i++)
    inst->timer[i].valid = false;
}

/* ------------------------------------------------------------------------------------------------ */
/* the frame around a stage's launches                                                              */
/* ------------------------------------------------------------------------------------------------ */
int stage_begin(vksift_Instance inst, StageFrame *f, uint32_t timer, const char *range)
{
  f->timer = &inst->timer[timer];
  const int e = timer_start(inst, f->timer);
  if (e)
    return e;
  vksift_hip_range_push(range);
  f->open = f->begun = true;
  return 0;
}

int stage_end(vksift_Instance inst, StageFrame *f, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count)
{
  (void)stage_abort(f);
  const int e = timer_stop(inst, f->timer);
  if (e)
    return e;
  return ids_a ? match_follow(inst, ids_a, ids_b, count) : 0;
}

void stage_fail(vksift_Instance inst, StageFrame *f, const uint32_t *ids_a, const uint32_t *ids_b, uint32_t count)
{
  (void)stage_abort(f);
  if (f->begun && match_follow(inst, ids_a, ids_b, count) != 0)
    (void)vksift_hip_stream_sync(inst->stream);
}

bool stage_abort(StageFrame *f)
{
  const bool was_open = f->open;
  if (was_open)
    vksift_hip_range_pop();
  f->open = false;
  return was_open;
}

/* ------------------------------------------------------------------------------------------------ */
/* per-pair results                                                                                 */
/* ------------------------------------------------------------------------------------------------ */
bool pair_results_ensure(vksift_Instance inst, uint32_t which, uint32_t words, uint64_t stride, uint32_t elem, uint32_t counted_by)
{
  PairResults *s = &inst->res[which];
  const uint32_t bc = inst->batch_cap;
  s->words = words, s->stride = stride, s->elem = elem, s->counted_by = counted_by;
  return mem_ensure(&s->d_payload, stride * bc, MEM_DEVICE) && mem_ensure(&s->d_words, sizeof(uint32_t) * words * bc, MEM_DEVICE) &&
         mem_ensure(&s->h_words, sizeof(uint32_t) * words * bc, MEM_PINNED);
}

void pair_results_invalidate(vksift_Instance inst)
{
  for (uint32_t i = 0; i < PR_COUNT; i++)
    inst->res[i].slots_used = 0;
}

/* what every accessor starts with: the pipeline that posts the words has run, then the checks */
static bool pair_served(vksift_Instance inst, const PairResults *s, uint32_t pair, bool out_ok, const char *fn)
{
  wait_match(inst);
  if (pair < s->slots_used && out_ok)
    return true;
  logError(LOG_TAG, "%s() error: invalid input.", fn);
  inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
  return false;
}

const uint32_t *pair_words(vksift_Instance inst, uint32_t which, uint32_t pair, bool out_ok, const char *fn)
{
  const PairResults *s = &inst->res[which];
  return pair_served(inst, s, pair, out_ok, fn) ? s->h_words + (size_t)s->words * pair : NULL;
}

void pair_download(vksift_Instance inst, uint32_t which, uint32_t pair, void *dst, const char *fn, const char *what, const char *noun)
{
  const PairResults *s = &inst->res[which];
  if (!pair_served(inst, s, pair, true, fn))
    return;
  const PairResults *c = &inst->res[s->counted_by];
  const uint32_t n = c->h_words[(size_t)c->words * pair];
  if (n == 0)
    return;
  HIP_CHECK(vksift_hip_memcpy_d2h(dst, s->d_payload + (uint64_t)pair * s->stride, (size_t)n * s->elem, inst->dl_stream), what);
  HIP_CHECK(vksift_hip_stream_sync(inst->dl_stream), what);
  return;
gpu_error:
  logError(LOG_TAG, "%s() error when downloading %s from GPU memory.", fn, noun);
  inst->error_cb(VKSIFT_VULKAN_ERROR);
}
