/* layout_runs.c — prints the runs next_layout_run() (csrc/host/vksift_runs.c) yields for hand-built buffer tables; tests/test_layout_runs.py
 * compiles it with that file alone and compares the output with the runs written down there. One line per run:
 *   run first=<ids[0]> n=<ids> nsec=<sections> off=<..> cap=<..> fixed=<..|-> stride=<found_stride> max_rows=<..> */
#include "vksift_runs.h"

#include <stdio.h>
#include <string.h>

#define NBUF 520
static BufferInfo bufs[NBUF];

static BufferInfo dense(uint32_t n)
{
  BufferInfo b;
  memset(&b, 0, sizeof(b));
  b.is_packed = true, b.nb_stored = n;
  return b;
}

/* nsec sections of `cap` records back to back, the last one of last_cap */
static BufferInfo sectioned(uint32_t nsec, uint32_t cap, uint32_t last_cap)
{
  BufferInfo b;
  memset(&b, 0, sizeof(b));
  b.nb_sections = nsec, b.nb_stored = 77; /* (not looked at: the counters are on the device) */
  for (uint32_t o = 0; o < nsec; o++)
    b.sec_off[o] = o * cap, b.sec_cap[o] = o + 1 == nsec ? last_cap : cap;
  return b;
}

static void words(const char *name, const uint32_t *w, uint32_t n)
{
  printf(" %s=", name);
  for (uint32_t i = 0; w && i < n; i++)
    printf("%s%u", i ? "," : "", w[i]);
  if (!w)
    printf("-");
}

static void walk(const char *name, const uint32_t *ids, uint32_t count, const uint32_t *bound)
{
  LayoutRun run;
  uint32_t pos = 0, seen = 0;
  printf("case %s\n", name);
  while (next_layout_run(bufs, ids, count, bound, &pos, &run))
  {
    printf("run first=%u n=%u nsec=%u", run.ids[0], run.n, run.nsec);
    words("off", run.off, run.nsec), words("cap", run.cap, run.nsec), words("fixed", run.fixed, run.nsec);
    printf(" stride=%u max_rows=%u\n", run.found_stride, run.max_rows);
    if (run.ids != ids + seen)
      printf("BAD: the run does not start where the last one ended\n");
    seen += run.n;
  }
  if (seen != count || pos != count || next_layout_run(bufs, ids, count, bound, &pos, &run))
    printf("BAD: %u of %u ids, pos %u\n", seen, count, pos);
}

int main(void)
{
  static uint32_t ids[NBUF], bound[NBUF];
  for (uint32_t i = 0; i < NBUF; i++)
    ids[i] = i, bufs[i] = sectioned(3, 100, 100), bound[i] = 0;

  bufs[0] = dense(40);
  walk("one dense buffer", ids, 1, NULL);
  bufs[1] = dense(40);
  walk("two dense buffers, equal", ids, 2, NULL);
  bufs[1] = dense(41);
  walk("two dense buffers, different", ids, 2, NULL);

  bufs[0] = bufs[1] = sectioned(3, 100, 100);
  for (uint32_t i = 0; i < 512; i++)
    bound[i] = 10 + (i * 37) % 200;
  walk("512 ids, one layout", ids + 4, 512, bound + 4);

  /* layouts A, B, A: runs are consecutive */
  const uint32_t aba[5] = {9, 3, 200, 201, 7};
  const uint32_t aba_bound[5] = {5, 300, 11, 12, 299};
  bufs[200] = bufs[201] = sectioned(4, 50, 50);
  walk("A B A", aba, 5, aba_bound);
  walk("A B A, no bounds", aba, 5, NULL);

  const uint32_t mixed[4] = {10, 300, 11, 12};
  const uint32_t mixed_bound[4] = {1, 1000, 2, 3};
  bufs[300] = dense(1000);
  walk("dense between sectioned", mixed, 4, mixed_bound);

  bufs[400] = bufs[401] = sectioned(16, 8, 8);
  walk("sixteen sections", ids + 400, 2, bound + 400);

  bufs[410] = sectioned(5, 20, 20), bufs[411] = sectioned(5, 20, 19);
  walk("the last capacity differs", ids + 410, 2, NULL);

  walk("a list of one", ids + 17, 1, bound + 17);
  walk("an empty list", ids, 0, NULL);
  return 0;
}
