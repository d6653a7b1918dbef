/*
 * plan_harness.c — the public API of the host library, driven over the simulated device of sim_device.c (tests/test_detect_plan.py; no GPU).
 * A small command interpreter: one command per line of stdin (or, given arguments, one per ';'-separated group of argv). Every command is
 * echoed as "> ..." in front of what the device logs for it, and closed by "< ..." with what the call returned; behind every API call the
 * device checks that no capture was left open. The scenarios and every assertion are in Python: this file only drives and reports.
 *
 *   create BC MAX_PX MAX_FEATS NBUF UPSAMPLE FP16   vksift_loadVulkan + vksift_createInstance (BC 1) / vksift_ext_createInstanceBatched
 *   detect W H BUF | batch W H FIRST COUNT | batchdev W H FIRST COUNT WHICH (device input block 0 or 1)
 *   num BUF | download BUF | avail BUF | match A B | prof 0|1 | describe W H BUF N | destroy
 *   busy 0|1 | drain | covered 0|1 | counts V | failin K | ledger
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
extern uint64_t sim_fail_in, sim_violations;
void sim_drain(void);
void sim_api_return(void);
void sim_report_ledger(void);
void sim_finish(void);
uint32_t sim_live_execs(void);
void *vksift_hip_malloc(size_t bytes);
void vksift_hip_free(void *p);

static vksift_Instance inst;
static vksift_Config cfg;
static uint8_t *d_in[2];
static uint32_t errors;

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

static int run(char *line)
{
  unsigned long long a[8] = {0};
  char cmd[32] = "";
  const int n = sscanf(line, "%31s %llu %llu %llu %llu %llu %llu %llu", cmd, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]);
  if (n < 1)
    return 0;
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
  else if (!strcmp(cmd, "download"))
  {
    const uint32_t k = vksift_getFeaturesNumber(inst, (uint32_t)a[0]);
    vksift_Feature *f = (vksift_Feature *)malloc(sizeof(vksift_Feature) * (k ? k : 1));
    vksift_downloadFeatures(inst, f, (uint32_t)a[0]);
    free(f);
    printf("< download n=%u errors=%u\n", k, errors - errors_before);
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
    vksift_ext_describeKeypoints(inst, img, w, h, kp, nk, (uint32_t)a[2], VKSIFT_EXT_DESCRIBE_ORIENT);
    free(kp);
    free(img);
    printf("< describe errors=%u\n", errors - errors_before);
  }
  else if (!strcmp(cmd, "destroy"))
  {
    for (int i = 0; i < 2; i++)
      vksift_hip_free(d_in[i]), d_in[i] = NULL;
    vksift_destroyInstance(&inst);
    printf("< destroy\n");
  }
  else if (!strcmp(cmd, "busy"))
    sim_busy_mode = (int)a[0];
  else if (!strcmp(cmd, "drain"))
    sim_drain();
  else if (!strcmp(cmd, "covered"))
    sim_covered = (int)a[0];
  else if (!strcmp(cmd, "counts"))
    sim_counts = (uint32_t)a[0];
  else if (!strcmp(cmd, "failin"))
    sim_fail_in = a[0];
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
  char line[256];
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
