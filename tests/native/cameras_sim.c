/*
 * cameras_sim.c — vksift_ext_indexObservationsByView and vksift_ext_refineCameras on the simulated device of sim_device.c (tests/test_cameras_sim.py; no
 * GPU), where the launchers of hip/cameras.hip do not exist: the host file reaches them through weak references, finds none and must fail either call like
 * any launch failure. The simulated device has no observation and no triangulation launcher either, and a refinement needs both stages: this program
 * defines their entries itself, as launches that succeed and compute nothing (the device's posting then reports sim_counts for every count, as for every
 * other stage). A stand-alone program: matching, tracks, selection, triangulation, then the two new entries, the accessors around them, destroy and the
 * device's ledger; one line per step for the Python side to read. The device's own log lines (and its VIOLATION lines, if any) come in between.
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

/* the observation launcher the simulated device lacks: accepted, nothing computed */
size_t vksift_hip_observations_scratch_u32(uint32_t nbufs, uint32_t node_stride, uint32_t max_rows) { return (void)nbufs, (void)node_stride, (void)max_rows, 64u; }
int vksift_hip_track_observations(const uint32_t *node_words, const uint8_t *tracks, const uint32_t *track_stats, const uint32_t *buf_tab, uint32_t nbufs,
                                  const uint32_t *rows_dev, uint32_t node_stride, uint32_t max_rows, const uint8_t *feats_base, uint64_t buf_stride,
                                  const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *rank_layouts, const uint32_t *layouts, uint32_t min_length,
                                  uint32_t max_length, uint32_t conflicts, uint32_t *offsets, uint32_t *track_ids, uint64_t tracks_cap, uint8_t *observations,
                                  uint64_t obs_cap, uint32_t *stats, uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  (void)node_words, (void)tracks, (void)track_stats, (void)buf_tab, (void)nbufs, (void)rows_dev, (void)node_stride, (void)max_rows, (void)feats_base, (void)buf_stride;
  (void)found_base, (void)found_buf_stride, (void)rank_layouts, (void)layouts, (void)min_length, (void)max_length, (void)conflicts, (void)offsets, (void)track_ids;
  (void)tracks_cap, (void)observations, (void)obs_cap, (void)stats, (void)scratch, (void)scratch_u32, (void)s;
  return 0;
}

/* and the triangulation launcher: accepted, nothing computed */
int vksift_hip_triangulate_tracks(const uint32_t *offsets, const uint8_t *observations, const uint32_t *obs_stats, const float *cameras, uint32_t nb_cameras, float t2,
                                  float cos_min_angle, uint8_t *points, uint64_t points_cap, uint32_t *stats, vksift_hip_stream s)
{
  (void)offsets, (void)observations, (void)obs_stats, (void)cameras, (void)nb_cameras, (void)t2, (void)cos_min_angle, (void)points, (void)points_cap, (void)stats, (void)s;
  return 0;
}

#define W 160u
#define H 120u
#define NBUF 6u
#define NPAIRS 4u

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

typedef struct
{
  vksift_ext_TrackStats tracks;
  vksift_ext_ObservationStats obs;
  vksift_ext_PointStats points;
  uint32_t offsets[8], ids[8];
  vksift_ext_Observation records[4];
  vksift_ext_Point pts[4];
} Served;

/* what the tracks, the observations and the points serve (sim_counts = 3: three of everything) */
static void read_served(vksift_Instance inst, Served *v)
{
  memset(v, 0, sizeof(*v));
  vksift_ext_getTrackStats(inst, &v->tracks);
  vksift_ext_getObservationStats(inst, &v->obs);
  vksift_ext_getPointStats(inst, &v->points);
  vksift_ext_downloadObservationOffsets(inst, v->offsets);
  vksift_ext_downloadObservationTrackIds(inst, v->ids);
  vksift_ext_downloadObservations(inst, v->records);
  vksift_ext_downloadPoints(inst, v->pts);
}

int main(void)
{
  setvbuf(stdout, NULL, _IOFBF, 1 << 16);
  vksift_setLogLevel(VKSIFT_NO_LOG);
  if (vksift_loadVulkan() != VKSIFT_SUCCESS)
    return 2;
  vksift_Config cfg = vksift_getDefaultConfig();
  cfg.input_image_max_size = W * H, cfg.max_nb_sift_per_buffer = 600, cfg.sift_buffer_count = NBUF;
  cfg.on_error_callback_function = on_error;
  vksift_Instance inst = NULL;
  if (vksift_ext_createInstanceBatched(&inst, &cfg, NPAIRS) != VKSIFT_SUCCESS)
    return 2;
  sim_counts = 3; /* what the device reports for every count it is asked */

  float cameras[NBUF][12];
  for (uint32_t b = 0; b < NBUF; b++)
  {
    const float P[12] = {256.f, 0.f, 0.f, -256.f * (float)b, 0.f, 256.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    memcpy(cameras[b], P, sizeof(P));
  }

  uint32_t e = errors;
  const uint8_t *imgs[NPAIRS];
  for (uint32_t i = 0; i < NPAIRS; i++)
  {
    uint8_t *p = (uint8_t *)malloc((size_t)W * H);
    for (size_t k = 0; k < (size_t)W * H; k++)
      p[k] = (uint8_t)(k * 31u + i);
    imgs[i] = p;
  }
  vksift_ext_detectFeaturesBatch(inst, imgs, NPAIRS, W, H, 0);
  for (uint32_t i = 0; i < NPAIRS; i++)
    free((void *)imgs[i]);
  step("detect", e);

  e = errors;
  const uint32_t ids_a[NPAIRS] = {0, 2, 1, 3}, ids_b[NPAIRS] = {1, 3, 1, 0};
  vksift_ext_matchFeaturesFiltered(inst, NPAIRS, ids_a, ids_b, 0.8f, true);
  step("filtered", e);

  e = errors;
  vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED);
  step("tracks", e);

  e = errors;
  vksift_ext_indexObservationsByView(inst); /* no observations selected: refused */
  step("index_before_selection", e);

  e = errors;
  vksift_ext_selectTrackObservations(inst, 2, 0, VKSIFT_EXT_OBS_KEEP_CONFLICTING);
  step("select", e);

  e = errors;
  vksift_ext_refineCameras(inst, 4); /* no triangulation: refused */
  step("refine_before_triangulation", e);

  e = errors;
  vksift_ext_triangulateTracks(inst, &cameras[0][0], 1.0f, 1.0f);
  step("triangulate", e);

  e = errors;
  Served before, after;
  read_served(inst, &before);
  step("served_before", e);
  printf("served tracks=%u observations=%u points=%u\n", before.obs.nb_tracks, before.obs.nb_observations, before.points.nb_points);

  /* refused before the launcher is looked for */
  e = errors;
  vksift_ext_refineCameras(inst, 0);
  step("refine_zero_steps", e);
  e = errors;
  vksift_ext_refineCameras(inst, 9);
  step("refine_nine_steps", e);

  e = errors;
  vksift_ext_indexObservationsByView(inst);
  step("index", e);
  e = errors;
  vksift_ext_refineCameras(inst, 4);
  step("refine", e);

  e = errors;
  vksift_ext_ViewStats vs = {0};
  vksift_ext_getViewStats(inst, &vs);
  step("vstats", e);
  e = errors;
  uint32_t view_offsets[NBUF + 1u] = {0};
  vksift_ext_downloadViewOffsets(inst, view_offsets);
  step("voffsets", e);
  e = errors;
  vksift_ext_ViewObservation vobs[4];
  memset(vobs, 0, sizeof(vobs));
  vksift_ext_downloadViewObservations(inst, vobs);
  step("vobservations", e);
  e = errors;
  vksift_ext_CameraStats cs = {0};
  vksift_ext_getCameraStats(inst, &cs);
  step("cstats", e);
  e = errors;
  vksift_ext_RefinedCamera refined[NBUF];
  memset(refined, 0, sizeof(refined));
  vksift_ext_downloadRefinedCameras(inst, refined);
  step("ccameras", e);

  e = errors;
  read_served(inst, &after);
  step("served_after", e);
  printf("served same=%d\n", memcmp(&before, &after, sizeof(before)) == 0);
  printf("times %d %d\n", (int)vksift_ext_getIndexViewsTime(inst), (int)vksift_ext_getRefineCamerasTime(inst));

  /* the failed calls ended their sequences like complete ones: the buffers are free again and a new matching goes through */
  e = errors;
  vksift_ext_matchFeaturesFiltered(inst, NPAIRS, ids_a, ids_b, 0.8f, true);
  (void)vksift_ext_getFilteredMatchesNumber(inst, 0);
  step("filtered_again", e);

  vksift_destroyInstance(&inst);
  sim_api_return();
  sim_report_ledger();
  sim_finish();
  fflush(stdout);
  return sim_violations ? 3 : 0;
}
