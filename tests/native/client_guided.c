/* A plain-C client of the public headers for guided matching: two 640x480 images given as files of raw bytes (the test writes a synthetic
 * image and a warped copy of it), detected into two buffers, matched with the GPU-side filter, verified with both models, then matched again
 * under each verified model and under a model of the caller's own; prints the counts and a digest of the records of each run.
 * tests/test_native_guided.py compares the line with the Python mirror's results for the same inputs. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vulkansift/vulkansift.h>

#include "vksift_ext.h"

static uint8_t *read_image(const char *path, size_t n)
{
  uint8_t *p = malloc(n);
  FILE *f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, n, f) != n)
    return NULL;
  fclose(f);
  return p;
}

static void print_run(vksift_Instance inst, const char *name)
{
  const uint32_t n = vksift_ext_getGuidedMatchesNumber(inst, 0u);
  vksift_ext_FilteredMatch *m = calloc(n + 1u, sizeof(*m));
  vksift_ext_downloadGuidedMatches(inst, 0u, m);
  const uint8_t *bytes = (const uint8_t *)m;
  uint64_t dig = 1469598103934665603ull;
  for (size_t i = 0; i < (size_t)n * sizeof(*m); i++)
    dig = (dig ^ bytes[i]) * 1099511628211ull;
  printf(" %s %u %016llx", name, n, (unsigned long long)dig);
  free(m);
}

int main(int argc, char **argv)
{
  const uint32_t w = 640, h = 480;
  if (argc != 3)
    return 1;
  uint8_t *img1 = read_image(argv[1], (size_t)w * h), *img2 = read_image(argv[2], (size_t)w * h);
  if (!img1 || !img2)
    return 1;
  vksift_setLogLevel(VKSIFT_LOG_ERROR);
  if (vksift_loadVulkan() != VKSIFT_SUCCESS)
    return 2;
  vksift_Config cfg = vksift_getDefaultConfig();
  cfg.input_image_max_size = w * h;
  vksift_Instance inst = NULL;
  if (vksift_createInstance(&inst, &cfg) != VKSIFT_SUCCESS)
    return 3;
  vksift_detectFeatures(inst, img1, w, h, 0u);
  vksift_detectFeatures(inst, img2, w, h, 1u);
  const uint32_t a = 0u, b = 1u;
  vksift_ext_matchFeaturesFiltered(inst, 1u, &a, &b, 0.8f, true);
  vksift_ext_verifyHomography(inst, 1024u, 2.5f, 42ull);
  vksift_ext_verifyFundamental(inst, 1024u, 2.5f, 42ull);
  printf("guided filtered %u", vksift_ext_getFilteredMatchesNumber(inst, 0u));
  vksift_ext_matchFeaturesGuided(inst, VKSIFT_EXT_GUIDE_HOMOGRAPHY, NULL, 2.5f, 0.8f, INFINITY, true);
  print_run(inst, "homography");
  vksift_ext_matchFeaturesGuided(inst, VKSIFT_EXT_GUIDE_FUNDAMENTAL, NULL, 2.5f, 0.8f, 250.0f, false);
  print_run(inst, "fundamental");
  vksift_ext_Homography hom;
  vksift_ext_getHomography(inst, 0u, &hom);
  float own[9];
  for (int i = 0; i < 9; i++)
    own[i] = hom.H[i];
  own[2] += 0.5f; /* the caller's own model: the verified one moved by half a pixel */
  vksift_ext_matchFeaturesGuided(inst, VKSIFT_EXT_GUIDE_HOMOGRAPHY, own, 3.0f, 0.9f, INFINITY, true);
  print_run(inst, "own");
  printf(" valid %u\n", hom.valid);
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  return inst == NULL ? 0 : 4;
}
