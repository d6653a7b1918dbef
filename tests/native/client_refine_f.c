/* A plain-C client of the public headers for the refit of a verified fundamental matrix: two 640x480 images given as files of raw bytes (the test
 * writes a synthetic image and a warped copy of it), detected into two buffers, matched with the GPU-side filter, verified, refined;
 * prints the refined model's bits, the counts and a digest of the refined mask. tests/test_native_refine_f.py compares the line with the
 * Python mirror's results for the same inputs. */
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
  vksift_ext_verifyFundamental(inst, 16u, 2.5f, 42ull);
  vksift_ext_refineFundamental(inst, 3u, 2.5f);
  vksift_ext_Fundamental fun;
  vksift_ext_RefinedFundamental ref;
  vksift_ext_getFundamental(inst, 0u, &fun);
  vksift_ext_getRefinedFundamental(inst, 0u, &ref);
  const uint32_t n = vksift_ext_getFilteredMatchesNumber(inst, 0u);
  uint8_t *mask = calloc(n + 1u, 1);
  vksift_ext_downloadRefinedFundamentalInlierMask(inst, 0u, mask);
  uint64_t dig = 1469598103934665603ull;
  uint32_t ones = 0;
  for (uint32_t i = 0; i < n; i++)
    dig = (dig ^ mask[i]) * 1099511628211ull, ones += mask[i];
  printf("refined");
  for (int i = 0; i < 9; i++)
  {
    union { float f; uint32_t u; } v = {ref.F[i]};
    printf(" %08x", v.u);
  }
  printf(" matches %u %u inliers %u %u ransac %u rounds %u valid %u mask %016llx\n", n, ref.nb_matches, ref.nb_inliers, ones, fun.nb_inliers, ref.rounds, ref.valid,
         (unsigned long long)dig);
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  return inst == NULL ? 0 : 4;
}
