/*
 * vksift_stage.c — host copy of the caller's images into the pinned staging buffer (sift_memory.c:891-955)
 */
#include "vksift_internal.h"
#include <pthread.h>

/* Host copy of the caller's images into the pinned staging buffer (the caller may reuse its memory as soon as the call returns,
 * sift_memory.c:943). A batch is tens of megabytes: one thread moves ~10 GB/s, which made this copy as long as the detection
 * itself (39 MB per 128 VGA frames: 4 ms). A small pool of persistent workers shares it (creating threads per call cost as
 * much as a chunk's copy), and the batch goes chunk by chunk: the host-to-device copy of chunk i runs while chunk i+1 is staged. */
enum { STAGE_MAXT = 8 };
typedef struct
{
  uint8_t *dst;
  const uint8_t *const *images;
  uint32_t i0, i1;
  size_t img_bytes;
} StageJob;

static struct
{
  pthread_mutex_t user;     /* one staging operation at a time (instances on different threads share the pool) */
  pthread_mutex_t mu;
  pthread_cond_t cv_work, cv_done;
  pthread_t th[STAGE_MAXT];
  StageJob job[STAGE_MAXT];
  uint64_t gen[STAGE_MAXT]; /* generation each worker has to run (0: none yet) */
  uint64_t cur;
  uint32_t pending, nworkers;
  bool started;
} g_stage = {.user = PTHREAD_MUTEX_INITIALIZER, .mu = PTHREAD_MUTEX_INITIALIZER, .cv_work = PTHREAD_COND_INITIALIZER, .cv_done = PTHREAD_COND_INITIALIZER};

static void stage_copy(const StageJob *j)
{
  for (uint32_t i = j->i0; i < j->i1; i++)
    memcpy(j->dst + (size_t)i * j->img_bytes, j->images[i], j->img_bytes);
}

static void *stage_worker(void *p)
{
  const uint32_t id = (uint32_t)(uintptr_t)p;
  uint64_t seen = 0;
  pthread_mutex_lock(&g_stage.mu);
  for (;;)
  {
    while (g_stage.gen[id] == seen)
      pthread_cond_wait(&g_stage.cv_work, &g_stage.mu);
    seen = g_stage.gen[id];
    const StageJob j = g_stage.job[id];
    pthread_mutex_unlock(&g_stage.mu);
    stage_copy(&j);
    pthread_mutex_lock(&g_stage.mu);
    if (--g_stage.pending == 0)
      pthread_cond_signal(&g_stage.cv_done);
  }
  return NULL;
}

/* images [i0, i1) -> dst, shared by the caller and up to STAGE_MAXT - 1 workers; returns when all of it is in place */
void stage_images(uint8_t *dst, const uint8_t *const *images, uint32_t i0, uint32_t i1, size_t img_bytes)
{
  const uint32_t n = i1 - i0;
  StageJob all = {dst, images, i0, i1, img_bytes};
  if ((size_t)n * img_bytes < ((size_t)2 << 20) || n < 2)
  {
    stage_copy(&all);
    return;
  }
  pthread_mutex_lock(&g_stage.user);
  if (!g_stage.started)
  {
    g_stage.started = true;
    for (uint32_t t = 0; t + 1 < STAGE_MAXT; t++)
      if (pthread_create(&g_stage.th[g_stage.nworkers], NULL, stage_worker, (void *)(uintptr_t)g_stage.nworkers) == 0)
      {
        pthread_detach(g_stage.th[g_stage.nworkers]);
        g_stage.nworkers++;
      }
  }
  uint32_t parts = g_stage.nworkers + 1u;
  if (parts > n)
    parts = n;
  pthread_mutex_lock(&g_stage.mu);
  g_stage.cur++;
  g_stage.pending = parts - 1u;
  for (uint32_t t = 1; t < parts; t++)
  {
    StageJob *j = &g_stage.job[t - 1];
    *j = all;
    j->i0 = i0 + (uint32_t)((uint64_t)n * t / parts), j->i1 = i0 + (uint32_t)((uint64_t)n * (t + 1) / parts);
    g_stage.gen[t - 1] = g_stage.cur;
  }
  pthread_cond_broadcast(&g_stage.cv_work);
  pthread_mutex_unlock(&g_stage.mu);
  all.i1 = i0 + (uint32_t)((uint64_t)n / parts);
  stage_copy(&all); /* the caller takes the first share */
  pthread_mutex_lock(&g_stage.mu);
  while (g_stage.pending != 0)
    pthread_cond_wait(&g_stage.cv_done, &g_stage.mu);
  pthread_mutex_unlock(&g_stage.mu);
  pthread_mutex_unlock(&g_stage.user);
}
