/* A plain-C client of the public headers for the spatially distributed feature budget: a 640x480 image given as a file of raw bytes is detected
 * into buffers 0 and 1, buffer 0 keeps `budget` features spread over a cols x rows grid; prints both counts, the selection's count and a digest of
 * the downloaded records. tests/test_native_spread.py compares the line with the Python mirror's results for the same input. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vulkansift/vulkansift.h>

#include "vksift_ext.h"

int main(int argc, char **argv)
{
  const uint32_t w = 640, h = 480;
  if (argc != 5)
    return 1;
  const uint32_t budget = (uint32_t)strtoul(argv[2], NULL, 10), cols = (uint32_t)strtoul(argv[3], NULL, 10), rows = (uint32_t)strtoul(argv[4], NULL, 10);
  uint8_t *img = malloc((size_t)w * h);
  FILE *f = fopen(argv[1], "rb");
  if (!img || !f || fread(img, 1, (size_t)w * h, f) != (size_t)w * h)
    return 1;
  fclose(f);
  vksift_setLogLevel(VKSIFT_LOG_ERROR);
  if (vksift_loadVulkan() != VKSIFT_SUCCESS)
    return 2;
  vksift_Config cfg = vksift_getDefaultConfig();
  cfg.input_image_max_size = w * h;
  vksift_Instance inst = NULL;
  if (vksift_createInstance(&inst, &cfg) != VKSIFT_SUCCESS)
    return 3;
  vksift_detectFeatures(inst, img, w, h, 0u);
  vksift_detectFeatures(inst, img, w, h, 1u);
  vksift_ext_keepStrongestFeaturesGrid(inst, 0u, 1u, budget, w, h, cols, rows);
  const uint32_t kept = vksift_getFeaturesNumber(inst, 0u), all = vksift_getFeaturesNumber(inst, 1u);
  vksift_Feature *feats = calloc(kept + 1u, sizeof(vksift_Feature));
  vksift_downloadFeatures(inst, feats, 0u);
  uint64_t dig = 1469598103934665603ull;
  const uint8_t *bytes = (const uint8_t *)feats;
  for (size_t i = 0; i < (size_t)kept * sizeof(vksift_Feature); i++)
    dig = (dig ^ bytes[i]) * 1099511628211ull;
  printf("spread detected %u kept %u record %u digest %016llx time %.1f plain %.1f\n", all, kept, (unsigned)sizeof(vksift_Feature), (unsigned long long)dig,
         (double)vksift_ext_getKeepStrongestGridTime(inst), (double)vksift_ext_getKeepStrongestTime(inst));
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  return inst == NULL ? 0 : 4;
}
