/* vksift_runs.h — what the host knows of a SIFT buffer's layout, and the walk over a list of buffers in runs that one launch over sectioned
 * buffers can serve (vksift_hip_gather_sections, _keep_strongest, _root_descriptors). No device call and nothing of the instance:
 * vksift_runs.c compiles and is tested alone (tests/test_layout_runs.py). */
#ifndef VKSIFT_RUNS_H
#define VKSIFT_RUNS_H

#include "vksift_hostmath.h" /* VKSIFT_MAX_OCTAVES */

#define VKSIFT_INTERNAL __attribute__((visibility("hidden")))

typedef struct
{
  bool is_packed;       /* true: one section [0, nb_stored) (after upload / after matching) */
  uint32_t nb_stored;   /* valid when is_packed */
  uint32_t nb_sections; /* octaves of the detection that last filled the buffer */
  uint32_t sec_off[VKSIFT_MAX_OCTAVES]; /* in features */
  uint32_t sec_cap[VKSIFT_MAX_OCTAVES];
  uint32_t in_w, in_h;  /* resolution of that detection */
  uint64_t seq;         /* sequence number of the detection that last filled the buffer (0: filled from the host / never). The host
                         * mirror of its per-octave counters is valid once that detection has completed (seq <= det_done) */
} BufferInfo;

/* the same section layout (so one kernel launch can serve both buffers)? */
VKSIFT_INTERNAL bool same_layout(const BufferInfo *x, const BufferInfo *y);

/* A run of consecutive ids whose buffers share a layout (always the whole list after a batched detection), as the launchers take it. An
 * uploaded buffer is one dense section {off 0, cap n} of n = nb_stored fixed records; a detected one has its sections, fixed == NULL, and its
 * counters on the device, found_stride words apart. The dense run's two words live in the struct: off, cap and fixed point into it. */
typedef struct
{
  const uint32_t *ids, *off, *cap, *fixed;
  uint32_t n, nsec, found_stride, dense[2];
  uint32_t max_rows; /* the largest bound[] of the run; 0 without bounds */
} LayoutRun;
/* The run that starts at ids[*pos], *pos moved behind it; false: the list has ended. bound (or NULL): a row bound per id of the list. */
VKSIFT_INTERNAL bool next_layout_run(const BufferInfo *bufs, const uint32_t *ids, uint32_t count, const uint32_t *bound, uint32_t *pos, LayoutRun *run);

#endif
