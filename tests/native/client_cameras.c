/* A plain-C client of the public headers for the per-view index and the camera refinement: the six views of tests/track_scene.py detected into six
 * buffers, all 15 pairs matched with the GPU-side filter, merged into tracks, the tracks of at least two members selected and triangulated under the
 * views' cameras — the crops are exact perspective views of the plane Z = 256, the crop at (x0, y0) under P = [[256, 0, 0, -256 x0], [0, 256, 0, -256 y0],
 * [0, 0, 1, 0]], each moved here by a small translation —, the table indexed by view, the cameras refined, and one alternation: the refined cameras
 * triangulate again and are refined again; prints the statistics of each stage and a CRC-32 over its records.
 * tests/test_native_cameras.py compares the line with the Python mirror's results for the same inputs. */
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

static void print_index(vksift_Instance inst)
{
  vksift_ext_ViewStats st;
  uint32_t view_offsets[NB_BUFFERS + 1u];
  vksift_ext_indexObservationsByView(inst);
  vksift_ext_getViewStats(inst, &st);
  vksift_ext_downloadViewOffsets(inst, view_offsets);
  vksift_ext_ViewObservation *obs = calloc(st.nb_observations + 1u, sizeof(*obs));
  vksift_ext_downloadViewObservations(inst, obs);
  uint32_t crc = crc32_more(0u, view_offsets, sizeof(view_offsets));
  printf(" index %u %u %u %08x", st.nb_views, st.nb_observations, st.largest_view, crc32_more(crc, obs, (size_t)st.nb_observations * sizeof(*obs)));
  free(obs);
}

/* refines, prints, and puts the refined cameras of the views back into the table */
static void print_refined(vksift_Instance inst, const char *name, uint32_t nb_steps, float cameras[NB_BUFFERS][12])
{
  vksift_ext_CameraStats st;
  vksift_ext_RefinedCamera rec[NB_BUFFERS];
  vksift_ext_refineCameras(inst, nb_steps);
  vksift_ext_getCameraStats(inst, &st);
  vksift_ext_downloadRefinedCameras(inst, rec);
  printf(" %s %u %u %u %u %08x", name, st.nb_views, st.nb_refined, st.nb_unchanged, st.nb_failed, crc32_more(0u, rec, sizeof(rec)));
  for (uint32_t v = 0; v < NB_VIEWS; v++)
    memcpy(cameras[v], rec[v].P, sizeof(rec[v].P));
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
    /* the true camera, its centre moved by (0.125 v, -0.0625 v, 0): exact in fp32 */
    cameras[v][3] = -256.f * ((float)views[v][2] + 0.125f * (float)v), cameras[v][7] = -256.f * ((float)views[v][3] - 0.0625f * (float)v);
  }
  uint32_t ids_a[NB_PAIRS], ids_b[NB_PAIRS], np = 0;
  for (uint32_t a = 0; a < NB_VIEWS; a++)
    for (uint32_t b = a + 1u; b < NB_VIEWS; b++)
      ids_a[np] = a, ids_b[np++] = b;
  vksift_ext_matchFeaturesFiltered(inst, np, ids_a, ids_b, 0.8f, true);
  vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED);
  vksift_ext_selectTrackObservations(inst, 2u, 0u, VKSIFT_EXT_OBS_KEEP_CONFLICTING);
  printf("cameras");
  vksift_ext_triangulateTracks(inst, &cameras[0][0], 2.0f, 1.0f);
  print_index(inst);
  print_refined(inst, "first", 4u, cameras);
  vksift_ext_triangulateTracks(inst, &cameras[0][0], 2.0f, 1.0f); /* the alternation */
  print_refined(inst, "second", 2u, cameras);
  printf("\n");
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  free(base);
  free(view);
  return inst == NULL ? 0 : 4;
}
