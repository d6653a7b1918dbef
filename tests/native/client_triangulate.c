/* A plain-C client of the public headers for triangulation: the six views of tests/track_scene.py detected into six buffers, all 15 pairs matched with
 * the GPU-side filter, merged into tracks, the tracks of at least two members selected and triangulated under the views' cameras — the crops are exact
 * perspective views of the plane Z = 256, the crop at (x0, y0) under P = [[256, 0, 0, -256 x0], [0, 256, 0, -256 y0], [0, 0, 1, 0]] — once with the angle
 * test off and once with a limit; prints the statistics of each run and a CRC-32 over its point records.
 * tests/test_native_triangulate.py compares the line with the Python mirror's results for the same inputs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vulkansift/vulkansift.h>

#include "vksift_ext.h"

#define NB_VIEWS 6u
#define NB_PAIRS 15u
#define NB_BUFFERS 16u

static const uint32_t views[NB_VIEWS][4] = {{192, 144, 0, 0}, {192, 144, 8, 4}, {192, 144, 16, 10}, {160, 120, 24, 2}, {160, 120, 4, 16}, {160, 120, 12, 12}}; /* w, h, x0, y0 */

/* CRC-32 (IEEE 802.3, zlib's), continued from crc */
static uint32_t crc32_more(uint32_t crc, const void *data, size_t n)
{
  const uint8_t *p = data;
  crc = ~crc;
  for (size_t i = 0; i < n; i++)
  {
    crc ^= p[i];
    for (int k = 0; k < 8; k++)
      crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  }
  return ~crc;
}

static void print_points(vksift_Instance inst, const char *name, const float *cameras, float threshold_px, float cos_min_angle)
{
  vksift_ext_PointStats st;
  vksift_ext_triangulateTracks(inst, cameras, threshold_px, cos_min_angle);
  vksift_ext_getPointStats(inst, &st);
  vksift_ext_Point *pts = calloc(st.nb_points + 1u, sizeof(*pts));
  vksift_ext_downloadPoints(inst, pts);
  printf(" %s %u %u %u %u %08x", name, st.nb_points, st.nb_accepted, st.nb_failed, st.nb_rejected, crc32_more(0u, pts, (size_t)st.nb_points * sizeof(*pts)));
  free(pts);
}

int main(void)
{
  const uint32_t bw = 256, bh = 208;
  uint8_t *base = malloc((size_t)bw * bh), *view = malloc((size_t)192 * 144);
  if (!base || !view)
    return 1;
  vksift_ext_genSyntheticImageFamily(77ull, bw, bh, VKSIFT_EXT_SYNTH_BLOBS, base);
  vksift_setLogLevel(VKSIFT_LOG_ERROR);
  if (vksift_loadVulkan() != VKSIFT_SUCCESS)
    return 2;
  vksift_Config cfg = vksift_getDefaultConfig();
  cfg.input_image_max_size = 192 * 144;
  cfg.sift_buffer_count = NB_BUFFERS;
  vksift_Instance inst = NULL;
  if (vksift_ext_createInstanceBatched(&inst, &cfg, NB_PAIRS) != VKSIFT_SUCCESS)
    return 3;
  float cameras[NB_BUFFERS][12];
  memset(cameras, 0, sizeof(cameras));
  for (uint32_t v = 0; v < NB_VIEWS; v++)
  {
    const uint32_t w = views[v][0], h = views[v][1];
    for (uint32_t y = 0; y < h; y++)
      memcpy(view + (size_t)y * w, base + (size_t)(y + views[v][3]) * bw + views[v][2], w);
    vksift_detectFeatures(inst, view, w, h, v); /* (the image is copied before the call returns) */
    cameras[v][0] = cameras[v][5] = 256.f, cameras[v][10] = 1.f;
    cameras[v][3] = -256.f * (float)views[v][2], cameras[v][7] = -256.f * (float)views[v][3];
  }
  uint32_t ids_a[NB_PAIRS], ids_b[NB_PAIRS], np = 0;
  for (uint32_t a = 0; a < NB_VIEWS; a++)
    for (uint32_t b = a + 1u; b < NB_VIEWS; b++)
      ids_a[np] = a, ids_b[np++] = b;
  vksift_ext_matchFeaturesFiltered(inst, np, ids_a, ids_b, 0.8f, true);
  vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED);
  vksift_ext_selectTrackObservations(inst, 2u, 0u, VKSIFT_EXT_OBS_KEEP_CONFLICTING);
  printf("points");
  print_points(inst, "any_angle", &cameras[0][0], 1.0f, 1.0f);
  print_points(inst, "wide_angle", &cameras[0][0], 1.0f, 0.9992f);
  printf("\n");
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  free(base);
  free(view);
  return inst == NULL ? 0 : 4;
}
