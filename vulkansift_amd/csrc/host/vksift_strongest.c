/*
 * vksift_strongest.c — the feature budget (vksift_ext_keepStrongestFeatures) and its spatially distributed form (vksift_ext_keepStrongestFeaturesGrid):
 * each SIFT buffer of a range keeps its N strongest features, of the whole image or cell by cell of a grid first, selected and compacted on the
 * device (hip/strongest.hip, hip/spread.hip). No counterpart in the reference, whose only limit is the capacity of a buffer's sections; its
 * callers download, sort and upload. Same contract as a detection: queued on the instance stream, the buffers pending until it has run.
 */
#include "vksift_internal.h"

#include <stdio.h>

/* the grid rule's arguments; NULL: the plain budget */
typedef struct
{
  uint32_t cols, rows;
  float bx[15], by[15]; /* bound j (1 .. n - 1) of n cells over `size` pixels: (float)((double)j * size / n) */
} BudgetGrid;

/* What the two entries are: the selection of buffers [first, first + count), queued like a detection. `valid`: the entry's own arguments are. */
static void keep_range(vksift_Instance inst, uint32_t first_gpu_buffer_id, uint32_t count, uint32_t max_features, const BudgetGrid *grid, bool valid, uint32_t timer,
                       const char *stage, const char *entry)
{
  StageFrame frame = {0};
  char msg[128];
  vksift_hip_set_device(inst->device);
  defer_sync(inst); /* staged plain detections are launched first */
  if (!inplace_range_valid(inst, first_gpu_buffer_id, count) || max_features == 0 || !valid)
  {
    logError(LOG_TAG, "%s() error: invalid input.", entry);
    inst->error_cb(VKSIFT_INVALID_INPUT_ERROR);
    return;
  }
  uint32_t ids[VKSIFT_HIP_GATHER_SLOTS];
  HIP_CHECK(inplace_begin(inst, first_gpu_buffer_id, count, ids), "download stream synchronisation");
  bool known_changed[VKSIFT_HIP_GATHER_SLOTS]; /* the host knows that the buffer holds more than max_features (its cache entry will be rewritten) */
  for (uint32_t i = 0; i < count; i++)
    known_changed[i] = (inst->bufs[ids[i]].nb_sections == 0 || counts_valid(inst, ids[i])) && rows_bound(inst, ids[i]) > max_features;
  HIP_CHECK(stage_begin(inst, &frame, timer, stage), "timer start"); /* (nothing can fail between here and the sequence number) */
  take_sequence(inst, first_gpu_buffer_id, count);
  /* with the matcher's cache in place the launch leaves the selected buffer's entry as the gather pass would */
  const CacheBlocks cache = cache_blocks(inst);
  LayoutRun run;
  for (uint32_t pos = 0; next_layout_run(inst->bufs, ids, count, NULL, &pos, &run);)
  {
    uint32_t *const found = run.fixed ? NULL : inst->d_found, *const post = run.fixed ? NULL : inst->h_found;
    HIP_CHECK(grid ? vksift_hip_keep_grid(inst->d_feats, inst->buf_stride, run.ids, run.n, run.nsec, run.off, run.cap, run.fixed, found, run.found_stride, post,
                                          max_features, grid->cols, grid->rows, grid->bx, grid->by, 2u, cache.desc, inst->desc_slot_stride, cache.norm,
                                          inst->cache_norm_stride, cache.n, 1, inst->stream)
                   : vksift_hip_keep_strongest(inst->d_feats, inst->buf_stride, run.ids, run.n, run.nsec, run.off, run.cap, run.fixed, found, run.found_stride, post,
                                               max_features, 2u, cache.desc, inst->desc_slot_stride, cache.norm, inst->cache_norm_stride, cache.n, 1,
                                               inst->stream),
              "feature selection");
    /* A buffer the launch leaves alone keeps its entry, valid or not. One it selects from has a valid entry afterwards (in stream order in front of
     * every matching queued from here on) if there is a cache; the host can say so only where it knows the count: elsewhere an entry that was not
     * valid stays marked so, and the next matching gathers it. An uploaded buffer's length the host knows, and keeps. */
    const bool *changed = known_changed + (run.ids - ids);
    for (uint32_t k = 0; k < run.n; k++)
    {
      BufferInfo *b = &inst->bufs[run.ids[k]];
      if (run.fixed)
        b->nb_stored = b->nb_stored < max_features ? b->nb_stored : max_features;
      if (changed[k])
        inst->cache_valid[run.ids[k]] = cache.desc != NULL;
      else if (!cache.desc)
        inst->cache_valid[run.ids[k]] = false;
    }
  }
  HIP_CHECK(inplace_end(inst, &frame), "event record");
  return;
gpu_error:
  snprintf(msg, sizeof msg, "%s() error: Failed to start the feature selection.", entry);
  inplace_fail(inst, &frame, msg);
}

void vksift_ext_keepStrongestFeatures(vksift_Instance instance, uint32_t first_gpu_buffer_id, uint32_t count, uint32_t max_features)
{
  keep_range(instance, first_gpu_buffer_id, count, max_features, NULL, true, T_BUDGET, "KeepStrongest", "vksift_ext_keepStrongestFeatures");
}

void vksift_ext_keepStrongestFeaturesGrid(vksift_Instance instance, uint32_t first_gpu_buffer_id, uint32_t count, uint32_t max_features, uint32_t image_width,
                                          uint32_t image_height, uint32_t grid_cols, uint32_t grid_rows)
{
  BudgetGrid grid = {.cols = grid_cols, .rows = grid_rows};
  const bool valid = image_width && image_height && grid_cols >= 1 && grid_cols <= 16 && grid_rows >= 1 && grid_rows <= 16;
  for (uint32_t j = 1; valid && j < grid_cols; j++)
    grid.bx[j - 1] = (float)((double)j * image_width / grid_cols);
  for (uint32_t j = 1; valid && j < grid_rows; j++)
    grid.by[j - 1] = (float)((double)j * image_height / grid_rows);
  keep_range(instance, first_gpu_buffer_id, count, max_features, &grid, valid, T_BUDGET_GRID, "KeepStrongestGrid", "vksift_ext_keepStrongestFeaturesGrid");
}

float vksift_ext_getKeepStrongestTime(vksift_Instance instance) { return timer_read(instance, T_BUDGET); }
float vksift_ext_getKeepStrongestGridTime(vksift_Instance instance) { return timer_read(instance, T_BUDGET_GRID); }
