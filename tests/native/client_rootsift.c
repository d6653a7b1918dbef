/* A plain-C client of the public headers for the RootSIFT conversion: a 640x480 image given as a file of raw bytes is detected into buffers 0 and 1,
 * buffer 0 is converted; prints both counts and a digest of the downloaded records of each.
 * tests/test_native_rootsift.py compares the line with the Python mirror's results for the same input. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vulkansift/vulkansift.h>

#include "vksift_ext.h"

static uint64_t digest(vksift_Instance inst, uint32_t buf, uint32_t n)
{
  vksift_Feature *feats = calloc(n + 1u, sizeof(vksift_Feature));
  uint64_t dig = 1469598103934665603ull;
  if (!feats)
    return 0;
  vksift_downloadFeatures(inst, feats, buf);
  const uint8_t *bytes = (const uint8_t *)feats;
  for (size_t i = 0; i < (size_t)n * sizeof(vksift_Feature); i++)
    dig = (dig ^ bytes[i]) * 1099511628211ull;
  free(feats);
  return dig;
}

int main(int argc, char **argv)
{
  const uint32_t w = 640, h = 480;
  if (argc != 2)
    return 1;
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
  vksift_ext_convertToRootSift(inst, 0u, 1u);
  const uint32_t converted = vksift_getFeaturesNumber(inst, 0u), all = vksift_getFeaturesNumber(inst, 1u);
  printf("rootsift detected %u converted %u record %u digest %016llx plain %016llx time %.1f\n", all, converted, (unsigned)sizeof(vksift_Feature),
         (unsigned long long)digest(inst, 0u, converted), (unsigned long long)digest(inst, 1u, all), (double)vksift_ext_getRootSiftTime(inst));
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  free(img);
  return inst == NULL ? 0 : 4;
}
