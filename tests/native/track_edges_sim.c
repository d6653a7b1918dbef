/*
 * track_edges_sim.c — the edge store of tracks across matching calls (vksift_ext_beginTrackAccumulation ... vksift_ext_buildTracksAccumulated) on the
 * simulated device of sim_device.c (tests/test_track_edges_sim.py; no GPU). Built twice. Without WITH_LAUNCHERS the launchers of hip/track_edges.hip do not
 * exist, as on the simulated device: the host file reaches them through weak references, finds none and must fail like any launch failure, after every
 * refusal that comes before. With WITH_LAUNCHERS this program defines them itself (and the observation and triangulation launchers the device lacks), as
 * launches that succeed and compute nothing — the device's posting then reports sim_counts for every count — and walks through what the host keeps: the
 * store across a new matching, the re-sizing by the first begin, the stages behind an accumulated build. A stand-alone program; one line per step for
 * the Python side to read. The device's own log lines (alloc, free, and its VIOLATION lines, if any) come in between.
 */
#include "vksift_ext.h"
#include "vksift_hip.h"
#include "vulkansift/vulkansift.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* sim_device.c */
extern uint32_t sim_counts;
extern uint64_t sim_violations;
void sim_api_return(void);
void sim_report_ledger(void);
void sim_finish(void);

#ifdef WITH_LAUNCHERS
size_t vksift_hip_track_edges_scratch_u32(uint32_t nslots, uint32_t max_n) { return (void)nslots, (void)max_n, 64u; }
int vksift_hip_append_track_edges(const uint8_t *records, uint64_t rec_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, const uint8_t *masks,
                                  uint64_t mask_slot_stride, const uint32_t *valid, uint32_t valid_stride, const uint32_t *slot_tab, uint32_t slot_tab_stride, uint32_t nslots,
                                  const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t max_rows, uint32_t *row_table, uint32_t nb_buffers,
                                  uint8_t *edges, uint32_t max_edges, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  (void)records, (void)rec_slot_stride, (void)n_dev, (void)n_stride, (void)max_n, (void)masks, (void)mask_slot_stride, (void)valid, (void)valid_stride, (void)slot_tab;
  (void)slot_tab_stride, (void)nslots, (void)buf_tab, (void)nbufs, (void)rows_dev, (void)max_rows, (void)row_table, (void)nb_buffers, (void)edges, (void)max_edges;
  (void)stats, (void)scratch, (void)scratch_u32, (void)s;
  return 0;
}
int vksift_hip_build_tracks_from_edges(const uint8_t *edges, const uint32_t *edge_count, uint32_t max_edges, const uint32_t *rank_tab, uint32_t nb_buffers,
                                       const uint32_t *buf_tab, uint32_t nbufs, const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, uint32_t *node_words,
                                       uint8_t *tracks, uint64_t tracks_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  (void)edges, (void)edge_count, (void)max_edges, (void)rank_tab, (void)nb_buffers, (void)buf_tab, (void)rows_dev, (void)node_stride, (void)max_rows, (void)node_words;
  (void)tracks, (void)tracks_cap, (void)stats, (void)scratch, (void)scratch_u32, (void)s;
  printf("build_from_edges nbufs=%u\n", nbufs);
  return 0;
}
size_t vksift_hip_observations_scratch_u32(uint32_t nbufs, uint32_t node_stride, uint32_t max_rows) { return (void)nbufs, (void)node_stride, (void)max_rows, 64u; }
int vksift_hip_track_observations(const uint32_t *node_words, const uint8_t *tracks, const uint32_t *track_stats, const uint32_t *buf_tab, uint32_t nbufs,
                                  const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const uint8_t *feats_base, uint64_t buf_stride,
                                  const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *rank_layouts, const uint32_t *layouts, uint32_t min_length,
                                  uint32_t max_length, uint32_t conflicts, uint32_t *offsets, uint32_t *track_ids, uint64_t tracks_cap, uint8_t *observations,
                                  uint64_t obs_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  (void)node_words, (void)tracks, (void)track_stats, (void)buf_tab, (void)rows_dev, (void)node_stride, (void)max_rows, (void)feats_base, (void)buf_stride;
  (void)found_base, (void)found_buf_stride, (void)layouts, (void)min_length, (void)max_length, (void)conflicts, (void)offsets, (void)track_ids;
  (void)tracks_cap, (void)observations, (void)obs_cap, (void)stats, (void)scratch, (void)scratch_u32, (void)s;
  /* the layout words are the host's, in pinned memory: one per participating buffer */
  uint32_t dense = 0;
  for (uint32_t r = 0; r < nbufs; r++)
    dense += rank_layouts[r] >> 31;
  printf("track_observations nbufs=%u dense=%u\n", nbufs, dense);
  return 0;
}
int vksift_hip_triangulate_tracks(const uint32_t *offsets, const uint8_t *observations, const uint32_t *obs_stats, const float *cameras, uint32_t nb_cameras, float t2,
                                  float cos_min_angle, uint8_t *points, uint64_t points_cap, uint32_t *stats, vksift_hip_stream s)
{
  (void)offsets, (void)observations, (void)obs_stats, (void)cameras, (void)nb_cameras, (void)t2, (void)cos_min_angle, (void)points, (void)points_cap, (void)stats, (void)s;
  return 0;
}
#endif

#define W 160u
#define H 120u
#define NBUF 6u

static uint32_t errors;
static int last_error;

static void on_error(vksift_Result r)
{
  errors++;
  last_error = (int)r;
}

/* closes a step: what the error callback saw during it */
static void step(const char *name, uint32_t errors_before)
{
  sim_api_return();
  printf("step %s errors=%u last=%d\n", name, errors - errors_before, errors != errors_before ? last_error : 0);
}

static vksift_Instance create(uint32_t batch_cap)
{
  vksift_Config cfg = vksift_getDefaultConfig();
  cfg.input_image_max_size = W * H, cfg.max_nb_sift_per_buffer = 600, cfg.sift_buffer_count = NBUF;
  cfg.on_error_callback_function = on_error;
  vksift_Instance inst = NULL;
  if (vksift_ext_createInstanceBatched(&inst, &cfg, batch_cap) != VKSIFT_SUCCESS)
    exit(2);
  for (uint32_t first = 0; first < NBUF; first += batch_cap)
  {
    const uint8_t *imgs[NBUF];
    const uint32_t n = NBUF - first < batch_cap ? NBUF - first : batch_cap;
    for (uint32_t i = 0; i < n; i++)
    {
      uint8_t *p = (uint8_t *)malloc((size_t)W * H);
      for (size_t k = 0; k < (size_t)W * H; k++)
        p[k] = (uint8_t)(k * 31u + first + i);
      imgs[i] = p;
    }
    vksift_ext_detectFeaturesBatch(inst, imgs, n, W, H, first);
    for (uint32_t i = 0; i < n; i++)
      free((void *)imgs[i]);
  }
  return inst;
}

#define STEP(name, call)      \
  do                          \
  {                           \
    const uint32_t e_ = errors; \
    call;                     \
    step(name, e_);           \
  } while (0)

int main(void)
{
  setvbuf(stdout, NULL, _IOFBF, 1 << 16);
  vksift_setLogLevel(VKSIFT_NO_LOG);
  if (vksift_loadVulkan() != VKSIFT_SUCCESS)
    return 2;
  sim_counts = 3; /* what the device reports for every count it is asked */
  vksift_ext_TrackEdgeStats es = {9, 9, 9, 9};
  vksift_ext_TrackEdge edges[4];
  vksift_ext_TrackStats ts = {0};
  memset(edges, 0, sizeof(edges));

  uint32_t e = errors;
  vksift_Instance inst = create(2);
  step("detect", e);
  const uint32_t a0[2] = {0, 2}, b0[2] = {1, 3}, a1[2] = {4, 1}, b1[2] = {5, 4};

  /* before begin: every entry but begin refuses */
  STEP("accumulate_before_begin", vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("build_before_begin", vksift_ext_buildTracksAccumulated(inst));
  STEP("stats_before_begin", vksift_ext_getTrackEdgeStats(inst, &es));
  STEP("edges_before_begin", vksift_ext_downloadTrackEdges(inst, edges));
  STEP("begin_zero", vksift_ext_beginTrackAccumulation(inst, 0));
  STEP("stats_after_begin_zero", vksift_ext_getTrackEdgeStats(inst, &es));
  printf("stats untouched=%d\n", es.nb_edges == 9 && es.nb_calls == 9);
#ifndef WITH_LAUNCHERS
  STEP("begin", vksift_ext_beginTrackAccumulation(inst, 1000));
  STEP("accumulate_without_matching", vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("filtered", vksift_ext_matchFeaturesFiltered(inst, 2, a0, b0, 0.8f, true));
  STEP("stats_null", vksift_ext_getTrackEdgeStats(inst, NULL));
  STEP("edges_null", vksift_ext_downloadTrackEdges(inst, NULL));
  STEP("build_before_accumulate", vksift_ext_buildTracksAccumulated(inst));
  STEP("accumulate_unknown_source", vksift_ext_accumulateTrackEdges(inst, 6));
  STEP("accumulate_stage_not_run", vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_VERIFIED_H));
  STEP("stats_empty", vksift_ext_getTrackEdgeStats(inst, &es));
  printf("stats empty=%u %u %u %u\n", es.nb_edges, es.nb_dropped, es.nb_calls, es.nb_changed_buffers);
  printf("mark before_failure\n");
  STEP("accumulate", vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_FILTERED)); /* no launcher: a launch failure */
  printf("mark after_failure\n");
  /* the store is refused until the next begin */
  STEP("stats_after_failure", vksift_ext_getTrackEdgeStats(inst, &es));
  STEP("edges_after_failure", vksift_ext_downloadTrackEdges(inst, edges));
  STEP("accumulate_after_failure", vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("build_after_failure", vksift_ext_buildTracksAccumulated(inst));
  STEP("begin_again", vksift_ext_beginTrackAccumulation(inst, 1000));
  STEP("stats_after_begin", vksift_ext_getTrackEdgeStats(inst, &es));
  /* the failed call ended its sequence like a complete one: the plain build and a new matching go through */
  STEP("plain_build", vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("plain_stats", vksift_ext_getTrackStats(inst, &ts));
  STEP("filtered_again", vksift_ext_matchFeaturesFiltered(inst, 2, a1, b1, 0.8f, true));
  printf("times %d\n", (int)vksift_ext_getAccumulateTime(inst));
#else
  uint32_t words[600];
  float cameras[NBUF][12];
  for (uint32_t b = 0; b < NBUF; b++)
  {
    const float P[12] = {256.f, 0.f, 0.f, -256.f * (float)b, 0.f, 256.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    memcpy(cameras[b], P, sizeof(P));
  }
  /* the storage of the tracks and what follows exists for 2 batch_cap = 4 buffers */
  STEP("filtered", vksift_ext_matchFeaturesFiltered(inst, 2, a0, b0, 0.8f, true));
  STEP("plain_build", vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("plain_select", vksift_ext_selectTrackObservations(inst, 2, 0, VKSIFT_EXT_OBS_KEEP_CONFLICTING));
  STEP("plain_triangulate", vksift_ext_triangulateTracks(inst, &cameras[0][0], 1.0f, 1.0f));
  printf("mark begin_first\n");
  STEP("begin", vksift_ext_beginTrackAccumulation(inst, 1000));
  printf("mark begin_first_done\n");
  STEP("tracks_after_begin", vksift_ext_getTrackStats(inst, &ts)); /* released with their storage: not served */
  STEP("accumulate_0", vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("filtered_1", vksift_ext_matchFeaturesFiltered(inst, 2, a1, b1, 0.8f, true));
  STEP("accumulate_1", vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("stats", vksift_ext_getTrackEdgeStats(inst, &es));
  printf("stats served=%u %u %u %u\n", es.nb_edges, es.nb_dropped, es.nb_calls, es.nb_changed_buffers);
  STEP("edges", vksift_ext_downloadTrackEdges(inst, edges));
  STEP("build", vksift_ext_buildTracksAccumulated(inst));
  STEP("track_stats", vksift_ext_getTrackStats(inst, &ts));
  STEP("feature_tracks_first_call", vksift_ext_downloadFeatureTracks(inst, 0, words)); /* a buffer of the first call, outside the last pair list */
  STEP("select", vksift_ext_selectTrackObservations(inst, 2, 0, VKSIFT_EXT_OBS_KEEP_CONFLICTING));
  STEP("triangulate", vksift_ext_triangulateTracks(inst, &cameras[0][0], 1.0f, 1.0f));
  /* a new matching: the tracks go, the store stays */
  STEP("filtered_2", vksift_ext_matchFeaturesFiltered(inst, 1, a0, b0, 0.8f, true));
  STEP("track_stats_after_matching", vksift_ext_getTrackStats(inst, &ts));
  STEP("stats_after_matching", vksift_ext_getTrackEdgeStats(inst, &es));
  STEP("build_again", vksift_ext_buildTracksAccumulated(inst));
  STEP("track_stats_again", vksift_ext_getTrackStats(inst, &ts));
  /* a plain build replaces the accumulated tracks and leaves the store */
  STEP("plain_build_again", vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED));
  STEP("feature_tracks_outside_pair_list", vksift_ext_downloadFeatureTracks(inst, 5, words));
  STEP("stats_after_plain_build", vksift_ext_getTrackEdgeStats(inst, &es));
  printf("mark begin_second\n");
  STEP("begin_second", vksift_ext_beginTrackAccumulation(inst, 1000));
  printf("mark begin_second_done\n");
  STEP("build_after_second_begin", vksift_ext_buildTracksAccumulated(inst)); /* emptied: no accumulate yet */
  /* an instance whose pair lists can name every buffer releases nothing */
  vksift_Instance wide = create(3);
  STEP("wide_filtered", vksift_ext_matchFeaturesFiltered(wide, 2, a0, b0, 0.8f, true));
  STEP("wide_plain_build", vksift_ext_buildTracks(wide, VKSIFT_EXT_TRACKS_FILTERED));
  printf("mark begin_wide\n");
  STEP("begin_wide", vksift_ext_beginTrackAccumulation(wide, 1000));
  printf("mark begin_wide_done\n");
  STEP("wide_tracks_after_begin", vksift_ext_getTrackStats(wide, &ts)); /* nothing released: still served */
  vksift_destroyInstance(&wide);
#endif
  vksift_destroyInstance(&inst);
  sim_api_return();
  sim_report_ledger();
  sim_finish();
  fflush(stdout);
  return sim_violations ? 3 : 0;
}
