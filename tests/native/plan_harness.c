/*
 * plan_harness.c — the public API of the host library, driven over the simulated device of sim_device.c (tests/test_detect_plan.py; no GPU).
 * A small command interpreter: one command per line of stdin (or, given arguments, one per ';'-separated group of argv). Every command is
 * echoed as "> ..." in front of what the device logs for it, and closed by "< ..." with what the call returned; behind every API call the
 * device checks that no capture was left open. The scenarios and every assertion are in Python: this file only drives and reports.
 *
 *   create BC MAX_PX MAX_FEATS NBUF UPSAMPLE FP16   vksift_loadVulkan + vksift_createInstance (BC 1) / vksift_ext_createInstanceBatched
 *   detect W H BUF | batch W H FIRST COUNT | batchdev W H FIRST COUNT WHICH (device input block 0 or 1)
 *   num BUF | download BUF | downloadp BUF (a page-locked destination) | avail BUF | match A B | prof 0|1 | describe W H BUF N [GIVEN] | destroy
 *   busy 0|1 | drain | covered 0|1 | counts V | failin K [J] | ledger
 * and, for the stages behind a matching (tests/test_pair_plan.py):
 *   bmatch N A0 B0 A1 B1 ... | filtered CROSS N A0 B0 ...   vksift_ext_matchFeaturesBatch / vksift_ext_matchFeaturesFiltered (ratio 0.8)
 *   pmatch A B                                               vksift_matchFeatures alone (`match` also reads the result)
 *   mnum PAIR | mdl PAIR | mdlp PAIR | mnum0 | mdl0          the matching's number and download accessors, batch and plain (mdlp: a page-locked destination)
 *   verify M NH SEED | refine M ROUNDS | guided M SUPPLIED CROSS | tracks SOURCE      (M: 0 homography, 1 fundamental matrix; threshold 2.5)
 *   acc K PAIR                                               accessor K of `accnames` (the order of tests/api_model.py: ACCESSORS)
 *   tstats | tdl | tfeat BUF                                 the tracks' accessors
 *   budget FIRST COUNT MAX | grid FIRST COUNT MAX W H COLS ROWS | rootsift FIRST COUNT
 *   upload BUF N | export BUF | times | accnames
 *   roles 0|1 | late 0|1 | countallocs 0|1                   the device's switches
 * An accessor's "<" line carries served (the call reported no error), a hash of everything it returned and poison (1: the device's poison word
 * is among it: the accessor read before it waited). The error callback's code is logged as "error CODE".
 */
#include "vksift_ext.h"
#include "vulkansift/vulkansift.h"

#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* sim_device.c */
extern int sim_busy_mode, sim_covered;
extern uint32_t sim_counts;
extern uint64_t sim_fail_in, sim_fail_then, sim_violations;
extern int sim_roles, sim_late_posts, sim_count_allocs;
#define SIM_POISON 0xD0D0D0D0u
void sim_drain(void);
void sim_api_return(void);
void sim_report_ledger(void);
void sim_finish(void);
uint32_t sim_live_execs(void);
void *vksift_hip_malloc(size_t bytes);
void vksift_hip_free(void *p);
void *vksift_hip_host_malloc(size_t bytes);
void vksift_hip_host_free(void *p);

static vksift_Instance inst;
static vksift_Config cfg;
static uint8_t *d_in[2], *d_out;
static uint32_t errors;

/* what an accessor returned: FNV-1a of the bytes, and whether the device's poison word is among them */
static void report(const char *cmd, const void *p, size_t bytes, uint32_t n, uint32_t errors_before)
{
  uint64_t h = 0xcbf29ce484222325ull;
  bool poison = n == SIM_POISON;
  for (size_t i = 0; i < bytes; i++)
    h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  for (size_t i = 0; i + 4 <= bytes && !poison; i += 4)
  {
    uint32_t w;
    memcpy(&w, (const uint8_t *)p + i, 4);
    poison = w == SIM_POISON;
  }
  printf("< %s served=%d n=%u hash=%llu poison=%d errors=%u\n", cmd, errors == errors_before, n, (unsigned long long)(h >> 1), poison, errors - errors_before);
}

/* the caller's destination of a download: pageable, or page-locked (vksift_hip_is_pinned answers 1 for it). The harness's own block: not a
 * counted call of the entry. Released behind the call, so that the ledger of a script is what the library left */
static void *caller_block(size_t bytes, bool pinned)
{
  if (!pinned)
    return malloc(bytes);
  const int counted = sim_count_allocs;
  sim_count_allocs = 0;
  void *p = vksift_hip_host_malloc(bytes);
  sim_count_allocs = counted;
  return p;
}
static void caller_release(void *p, bool pinned)
{
  if (pinned)
    vksift_hip_host_free(p);
  else
    free(p);
}

static const char *const acc_names[12] = {"filtered n", "filtered", "H", "H mask", "F", "F mask", "refined H", "refined H mask", "refined F", "refined F mask", "guided n", "guided"};

static void on_error(vksift_Result r)
{
  errors++;
  printf("error %d\n", (int)r);
}

static uint8_t *image(uint32_t w, uint32_t h, uint32_t salt)
{
  uint8_t *p = (uint8_t *)malloc((size_t)w * h + 1u);
  for (size_t i = 0; i < (size_t)w * h; i++)
    p[i] = (uint8_t)(i * 31u + salt);
  return p;
}

#define MAX_ARGS 1100
static int run(char *line)
{
  static unsigned long long a[MAX_ARGS];
  char cmd[32] = "";
  int n = sscanf(line, "%31s", cmd), at = 0;
  if (n < 1)
    return 0;
  memset(a, 0, sizeof(a));
  sscanf(line, "%*s%n", &at);
  for (char *q = line + at, *end; n - 1 < MAX_ARGS; q = end, n++)
  {
    a[n - 1] = strtoull(q, &end, 10);
    if (end == q)
      break;
  }
  const uint32_t nargs = (uint32_t)(n - 1);
  (void)nargs;
  printf("> %s\n", line);
  const uint32_t errors_before = errors;
  if (!strcmp(cmd, "create"))
  {
    vksift_setLogLevel(VKSIFT_NO_LOG);
    const vksift_Result l = vksift_loadVulkan();
    cfg = vksift_getDefaultConfig();
    cfg.input_image_max_size = (uint32_t)a[1], cfg.max_nb_sift_per_buffer = (uint32_t)a[2], cfg.sift_buffer_count = (uint32_t)a[3];
    cfg.use_input_upsampling = a[4] != 0;
    cfg.pyramid_precision_mode = a[5] ? VKSIFT_PYRAMID_PRECISION_FLOAT16 : VKSIFT_PYRAMID_PRECISION_FLOAT32;
    cfg.on_error_callback_function = on_error;
    inst = NULL;
    const vksift_Result r = a[0] <= 1 ? vksift_createInstance(&inst, &cfg) : vksift_ext_createInstanceBatched(&inst, &cfg, (uint32_t)a[0]);
    for (int i = 0; i < 2; i++)
      d_in[i] = (uint8_t *)vksift_hip_malloc((size_t)cfg.input_image_max_size * (a[0] ? a[0] : 1));
    printf("< create load=%d result=%d\n", (int)l, (int)r);
  }
  else if (!strcmp(cmd, "detect"))
  {
    uint8_t *img = image((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]);
    vksift_detectFeatures(inst, img, (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]);
    free(img); /* the call has copied it */
    printf("< detect errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "batch"))
  {
    const uint8_t *imgs[64];
    const uint32_t count = a[3] > 64 ? 64u : (uint32_t)a[3];
    for (uint32_t i = 0; i < count; i++)
      imgs[i] = image((uint32_t)a[0], (uint32_t)a[1], i);
    vksift_ext_detectFeaturesBatch(inst, imgs, count, (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]);
    for (uint32_t i = 0; i < count; i++)
      free((void *)imgs[i]);
    printf("< batch errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "batchdev"))
  {
    vksift_ext_detectFeaturesBatchDevice(inst, d_in[a[4] & 1], (uint32_t)a[3], (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]);
    printf("< batchdev errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "num"))
  {
    const uint32_t k = vksift_getFeaturesNumber(inst, (uint32_t)a[0]);
    printf("< num n=%u errors=%u\n", k, errors - errors_before);
  }
  else if (!strcmp(cmd, "download") || !strcmp(cmd, "downloadp"))
  {
    const uint32_t k = vksift_getFeaturesNumber(inst, (uint32_t)a[0]);
    const size_t bytes = sizeof(vksift_Feature) * (k ? k : 1);
    vksift_Feature *f = (vksift_Feature *)caller_block(bytes, cmd[8] != 0);
    for (size_t i = 0; i + 4 <= bytes; i += 4) /* whatever the call leaves unwritten reads as poison */
      memcpy((uint8_t *)f + i, &(uint32_t){SIM_POISON}, 4);
    vksift_downloadFeatures(inst, f, (uint32_t)a[0]);
    bool poison = false;
    for (size_t i = 0; i + 4 <= sizeof(vksift_Feature) * k && !poison; i += 4)
      poison = memcmp((const uint8_t *)f + i, &(uint32_t){SIM_POISON}, 4) == 0;
    caller_release(f, cmd[8] != 0);
    printf("< %s n=%u poison=%d errors=%u\n", cmd, k, poison, errors - errors_before);
  }
  else if (!strcmp(cmd, "avail"))
  {
    const bool ok = vksift_isBufferAvailable(inst, (uint32_t)a[0]);
    printf("< avail ok=%d errors=%u\n", ok, errors - errors_before);
  }
  else if (!strcmp(cmd, "match"))
  {
    vksift_matchFeatures(inst, (uint32_t)a[0], (uint32_t)a[1]);
    const uint32_t k = vksift_getMatchesNumber(inst);
    vksift_Match_2NN *m = (vksift_Match_2NN *)malloc(sizeof(vksift_Match_2NN) * (k ? k : 1));
    vksift_downloadMatches(inst, m);
    free(m);
    printf("< match n=%u errors=%u\n", k, errors - errors_before);
  }
  else if (!strcmp(cmd, "prof"))
  {
    vksift_ext_setProfiling(inst, a[0] != 0);
    printf("< prof errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "describe"))
  {
    const uint32_t w = (uint32_t)a[0], h = (uint32_t)a[1], nk = (uint32_t)a[3];
    uint8_t *img = image(w, h, 7);
    vksift_ext_Keypoint *kp = (vksift_ext_Keypoint *)calloc(nk ? nk : 1, sizeof(*kp));
    for (uint32_t i = 0; i < nk; i++)
      kp[i].x = (float)((i * 7u) % w), kp[i].y = (float)((i * 5u) % h), kp[i].sigma = 2.0f, kp[i].response = 1.0f;
    vksift_ext_describeKeypoints(inst, img, w, h, kp, nk, (uint32_t)a[2], a[4] ? VKSIFT_EXT_DESCRIBE_GIVEN : VKSIFT_EXT_DESCRIBE_ORIENT);
    free(kp);
    free(img);
    printf("< describe errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "destroy"))
  {
    for (int i = 0; i < 2; i++)
      vksift_hip_free(d_in[i]), d_in[i] = NULL;
    vksift_hip_free(d_out), d_out = NULL;
    vksift_destroyInstance(&inst);
    printf("< destroy\n");
  }
  else if (!strcmp(cmd, "bmatch") || !strcmp(cmd, "filtered"))
  {
    const bool filt = cmd[0] == 'f';
    const uint32_t count = (uint32_t)a[filt ? 1 : 0];
    uint32_t *ids = (uint32_t *)malloc(sizeof(uint32_t) * 2u * (count ? count : 1));
    for (uint32_t i = 0; i < count; i++)
      ids[i] = (uint32_t)a[(filt ? 2 : 1) + 2u * i], ids[count + i] = (uint32_t)a[(filt ? 2 : 1) + 2u * i + 1u];
    if (filt)
      vksift_ext_matchFeaturesFiltered(inst, count, ids, ids + count, 0.8f, a[0] != 0);
    else
      vksift_ext_matchFeaturesBatch(inst, count, ids, ids + count);
    free(ids); /* the call has copied them */
    printf("< %s errors=%u\n", cmd, errors - errors_before);
  }
  else if (!strcmp(cmd, "pmatch"))
  {
    vksift_matchFeatures(inst, (uint32_t)a[0], (uint32_t)a[1]);
    printf("< pmatch errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "mnum") || !strcmp(cmd, "mnum0"))
  {
    const uint32_t k = cmd[4] ? vksift_getMatchesNumber(inst) : vksift_ext_getMatchesNumberBatch(inst, (uint32_t)a[0]);
    report(cmd, &k, 4, k, errors_before);
  }
  else if (!strcmp(cmd, "mdl") || !strcmp(cmd, "mdl0") || !strcmp(cmd, "mdlp"))
  {
    const size_t bytes = (size_t)cfg.max_nb_sift_per_buffer * sizeof(vksift_Match_2NN);
    const bool pinned = cmd[3] == 'p';
    vksift_Match_2NN *m = (vksift_Match_2NN *)caller_block(bytes, pinned);
    memset(m, 0, bytes);
    if (cmd[3] == '0')
      vksift_downloadMatches(inst, m);
    else
      vksift_ext_downloadMatchesBatch(inst, (uint32_t)a[0], m);
    report(cmd, m, bytes, 0, errors_before);
    caller_release(m, pinned);
  }
  else if (!strcmp(cmd, "verify"))
  {
    if (a[0])
      vksift_ext_verifyFundamental(inst, (uint32_t)a[1], 2.5f, a[2]);
    else
      vksift_ext_verifyHomography(inst, (uint32_t)a[1], 2.5f, a[2]);
    printf("< verify errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "refine"))
  {
    if (a[0])
      vksift_ext_refineFundamental(inst, (uint32_t)a[1], 2.5f);
    else
      vksift_ext_refineHomography(inst, (uint32_t)a[1], 2.5f);
    printf("< refine errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "guided"))
  {
    const uint32_t cap = cfg.sift_buffer_count * 64u; /* (more pairs than any instance of the tests holds) */
    float *models = (float *)calloc((size_t)9u * cap, sizeof(float));
    for (uint32_t i = 0; i < cap; i++)
      models[9u * i] = models[9u * i + 4u] = models[9u * i + 8u] = 1.f;
    vksift_ext_matchFeaturesGuided(inst, a[0] ? VKSIFT_EXT_GUIDE_FUNDAMENTAL : VKSIFT_EXT_GUIDE_HOMOGRAPHY, a[1] ? models : NULL, 2.5f, 0.8f, 300.f, a[2] != 0);
    free(models); /* the call has copied them */
    printf("< guided errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "tracks"))
  {
    vksift_ext_buildTracks(inst, (uint32_t)a[0]);
    printf("< tracks errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "acc"))
  {
    const size_t bytes = (size_t)cfg.max_nb_sift_per_buffer * 16u + 64u;
    uint8_t *out = (uint8_t *)calloc(1, bytes);
    const uint32_t pair = (uint32_t)a[1];
    uint32_t k = 0;
    switch (a[0])
    {
    case 0: k = vksift_ext_getFilteredMatchesNumber(inst, pair), memcpy(out, &k, 4); break;
    case 1: vksift_ext_downloadFilteredMatches(inst, pair, (vksift_ext_FilteredMatch *)out); break;
    case 2: vksift_ext_getHomography(inst, pair, (vksift_ext_Homography *)out); break;
    case 3: vksift_ext_downloadInlierMask(inst, pair, out); break;
    case 4: vksift_ext_getFundamental(inst, pair, (vksift_ext_Fundamental *)out); break;
    case 5: vksift_ext_downloadFundamentalInlierMask(inst, pair, out); break;
    case 6: vksift_ext_getRefinedHomography(inst, pair, (vksift_ext_RefinedHomography *)out); break;
    case 7: vksift_ext_downloadRefinedInlierMask(inst, pair, out); break;
    case 8: vksift_ext_getRefinedFundamental(inst, pair, (vksift_ext_RefinedFundamental *)out); break;
    case 9: vksift_ext_downloadRefinedFundamentalInlierMask(inst, pair, out); break;
    case 10: k = vksift_ext_getGuidedMatchesNumber(inst, pair), memcpy(out, &k, 4); break;
    case 11: vksift_ext_downloadGuidedMatches(inst, pair, (vksift_ext_FilteredMatch *)out); break;
    default: free(out); return 2;
    }
    report("acc", out, bytes, k, errors_before);
    free(out);
  }
  else if (!strcmp(cmd, "accnames"))
  {
    for (int i = 0; i < 12; i++)
      printf("accname %d %s\n", i, acc_names[i]);
  }
  else if (!strcmp(cmd, "tstats"))
  {
    vksift_ext_TrackStats st = {0};
    vksift_ext_getTrackStats(inst, &st);
    report("tstats", &st, sizeof(st), st.nb_tracks, errors_before);
  }
  else if (!strcmp(cmd, "tdl") || !strcmp(cmd, "tfeat"))
  {
    const size_t bytes = (size_t)cfg.max_nb_sift_per_buffer * 16u + 64u; /* (the device reports `counts` tracks: a handful) */
    uint8_t *out = (uint8_t *)calloc(1, bytes);
    if (cmd[1] == 'd')
      vksift_ext_downloadTracks(inst, (vksift_ext_Track *)out);
    else
      vksift_ext_downloadFeatureTracks(inst, (uint32_t)a[0], (uint32_t *)out);
    report(cmd, out, bytes, 0, errors_before);
    free(out);
  }
  else if (!strcmp(cmd, "budget"))
  {
    vksift_ext_keepStrongestFeatures(inst, (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]);
    printf("< budget errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "grid"))
  {
    vksift_ext_keepStrongestFeaturesGrid(inst, (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5], (uint32_t)a[6]);
    printf("< grid errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "rootsift"))
  {
    vksift_ext_convertToRootSift(inst, (uint32_t)a[0], (uint32_t)a[1]);
    printf("< rootsift errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "upload"))
  {
    vksift_Feature *f = (vksift_Feature *)calloc(a[1] ? a[1] : 1, sizeof(vksift_Feature));
    vksift_uploadFeatures(inst, f, (uint32_t)a[1], (uint32_t)a[0]);
    free(f); /* the call has copied them */
    printf("< upload errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "export"))
  {
    if (!d_out) /* (by the first export: the ledger of a script without one is what it was) */
    {
      const int counted = sim_count_allocs;
      sim_count_allocs = 0; /* (the harness's own block: not a call of the entry) */
      d_out = (uint8_t *)vksift_hip_malloc((size_t)cfg.max_nb_sift_per_buffer * 128u);
      sim_count_allocs = counted;
    }
    const uint32_t k = vksift_ext_exportDescriptorsDevice(inst, (uint32_t)a[0], d_out);
    report("export", &k, 4, k, errors_before);
  }
  else if (!strcmp(cmd, "times"))
  {
    const float t[9] = {vksift_ext_getMatchTime(inst),           vksift_ext_getVerifyTime(inst),      vksift_ext_getRefineTime(inst),
                        vksift_ext_getRefineFundamentalTime(inst), vksift_ext_getGuidedMatchTime(inst), vksift_ext_getTracksTime(inst),
                        vksift_ext_getKeepStrongestTime(inst),   vksift_ext_getKeepStrongestGridTime(inst), vksift_ext_getRootSiftTime(inst)};
    printf("< times");
    for (int i = 0; i < 9; i++)
      printf(" t%d=%d", i, (int)t[i]);
    printf(" errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "roles"))
    sim_roles = (int)a[0];
  else if (!strcmp(cmd, "late"))
    sim_late_posts = (int)a[0];
  else if (!strcmp(cmd, "countallocs"))
    sim_count_allocs = (int)a[0];
  else if (!strcmp(cmd, "busy"))
    sim_busy_mode = (int)a[0];
  else if (!strcmp(cmd, "drain"))
    sim_drain();
  else if (!strcmp(cmd, "covered"))
    sim_covered = (int)a[0];
  else if (!strcmp(cmd, "counts"))
    sim_counts = (uint32_t)a[0];
  else if (!strcmp(cmd, "failin")) /* failin K [J]: the K-th counted call fails, and the J-th behind it */
    sim_fail_in = a[0], sim_fail_then = a[1];
  else if (!strcmp(cmd, "ledger"))
    sim_report_ledger();
  else
  {
    fprintf(stderr, "unknown command %s\n", cmd);
    return 2;
  }
  sim_api_return();
  printf("execs live=%u\n", sim_live_execs());
  return 0;
}

int main(int argc, char **argv)
{
  static char line[1 << 15];
  int rc = 0;
  setvbuf(stdout, NULL, _IOFBF, 1 << 16);
  if (argc > 1)
  {
    line[0] = 0;
    for (int i = 1; i <= argc && rc == 0; i++)
    {
      if (i == argc || !strcmp(argv[i], ";"))
      {
        rc = run(line);
        line[0] = 0;
        continue;
      }
      strncat(line, argv[i], sizeof(line) - strlen(line) - 2);
      strcat(line, " ");
    }
  }
  else
    while (rc == 0 && fgets(line, sizeof(line), stdin))
    {
      line[strcspn(line, "\n")] = 0;
      rc = run(line);
    }
  if (inst)
  {
    char last[] = "destroy";
    (void)run(last);
  }
  sim_finish();
  fflush(stdout);
  return rc ? rc : sim_violations ? 3 : 0;
}
