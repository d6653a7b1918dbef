/*
 * observations_sim.c — vksift_ext_selectTrackObservations on the simulated device of sim_device.c (tests/test_observations_sim.py; no GPU), where the
 * observation launcher does not exist: the host file reaches it through a weak reference, finds none and must fail the call like any launch failure.
 * A stand-alone program: matching, then tracks, then the selection, the accessors around it, destroy and the device's ledger; one line per step for
 * the Python side to read. The device's own log lines (and its VIOLATION lines, if any) come in between.
 */
#include "vksift_ext.h"
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
  vksift_ext_selectTrackObservations(inst, 2, 0, VKSIFT_EXT_OBS_KEEP_CONFLICTING); /* nothing matched, no tracks: refused */
  step("select_before_tracks", e);

  e = errors;
  const uint32_t ids_a[NPAIRS] = {0, 2, 1, 3}, ids_b[NPAIRS] = {1, 3, 1, 0};
  vksift_ext_matchFeaturesFiltered(inst, NPAIRS, ids_a, ids_b, 0.8f, true);
  step("filtered", e);

  e = errors;
  vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED);
  step("tracks", e);

  e = errors;
  vksift_ext_TrackStats before = {0}, after = {0};
  vksift_ext_getTrackStats(inst, &before);
  step("tstats_before", e);

  e = errors;
  vksift_ext_selectTrackObservations(inst, 1, 0, VKSIFT_EXT_OBS_KEEP_CONFLICTING); /* min_length < 2: refused before the launcher is looked for */
  step("select_invalid", e);

  e = errors;
  vksift_ext_selectTrackObservations(inst, 2, 0, VKSIFT_EXT_OBS_KEEP_CONFLICTING);
  step("select", e);

  e = errors;
  vksift_ext_ObservationStats st = {0};
  vksift_ext_getObservationStats(inst, &st);
  step("ostats", e);
  e = errors;
  uint32_t words[8] = {0};
  vksift_ext_downloadObservationOffsets(inst, words);
  step("ooffsets", e);
  e = errors;
  vksift_ext_downloadObservationTrackIds(inst, words);
  step("oids", e);
  e = errors;
  vksift_ext_Observation obs[2];
  memset(obs, 0, sizeof(obs));
  vksift_ext_downloadObservations(inst, obs);
  step("oobs", e);

  e = errors;
  vksift_ext_getTrackStats(inst, &after);
  step("tstats_after", e);
  printf("tracks same=%d\n", memcmp(&before, &after, sizeof(before)) == 0);
  printf("otime %d\n", (int)vksift_ext_getObservationsTime(inst));

  /* the failed call ended its sequence like a complete one: the buffers are free again and a new matching goes through */
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
