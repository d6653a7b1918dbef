/* vksift_runs.c — the walk over a list of SIFT buffers in runs of one section layout (vksift_runs.h): plain host code, no device call. */
#include "vksift_runs.h"

#include <stddef.h>

bool same_layout(const BufferInfo *x, const BufferInfo *y)
{
  if (x->nb_sections != y->nb_sections)
    return false;
  if (x->nb_sections == 0)
    return x->nb_stored == y->nb_stored;
  for (uint32_t o = 0; o < x->nb_sections; o++)
    if (x->sec_off[o] != y->sec_off[o] || x->sec_cap[o] != y->sec_cap[o])
      return false;
  return true;
}

bool next_layout_run(const BufferInfo *bufs, const uint32_t *ids, uint32_t count, const uint32_t *bound, uint32_t *pos, LayoutRun *run)
{
  const uint32_t i0 = *pos;
  if (i0 >= count)
    return false;
  const BufferInfo *b = &bufs[ids[i0]];
  uint32_t i1 = i0 + 1, max_rows = bound ? bound[i0] : 0u;
  for (; i1 < count && same_layout(b, &bufs[ids[i1]]); i1++)
    if (bound && bound[i1] > max_rows)
      max_rows = bound[i1];
  const bool dense = b->nb_sections == 0; /* uploaded: one run of records whose length the host knows */
  run->ids = ids + i0, run->n = i1 - i0, run->max_rows = max_rows, run->dense[0] = 0, run->dense[1] = b->nb_stored;
  run->nsec = dense ? 1u : b->nb_sections, run->found_stride = dense ? 0u : VKSIFT_MAX_OCTAVES;
  run->off = dense ? &run->dense[0] : b->sec_off, run->cap = dense ? &run->dense[1] : b->sec_cap, run->fixed = dense ? &run->dense[1] : NULL;
  *pos = i1;
  return true;
}
