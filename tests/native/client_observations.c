/* A plain-C client of the public headers for track observations: the six views of tests/track_scene.py detected into six buffers, all 15 pairs matched
 * with the GPU-side filter, merged into tracks, then the observation table of the tracks of at least two members and of the consistent tracks of at
 * least three; prints the statistics of each selection and a CRC-32 over its offsets, track ids and observation records.
 * tests/test_native_observations.py compares the line with the Python mirror's results for the same inputs. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vulkansift/vulkansift.h>

#include "vksift_ext.h"

#define NB_VIEWS 6u
#define NB_PAIRS 15u

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

static void print_selection(vksift_Instance inst, const char *name, uint32_t min_length, uint32_t max_length, uint32_t conflicts)
{
  vksift_ext_ObservationStats st;
  vksift_ext_selectTrackObservations(inst, min_length, max_length, conflicts);
  vksift_ext_getObservationStats(inst, &st);
  uint32_t *offsets = calloc(st.nb_tracks + 1u, sizeof(*offsets)), *ids = calloc(st.nb_tracks + 1u, sizeof(*ids));
  vksift_ext_Observation *obs = calloc(st.nb_observations + 1u, sizeof(*obs));
  vksift_ext_downloadObservationOffsets(inst, offsets);
  vksift_ext_downloadObservationTrackIds(inst, ids);
  vksift_ext_downloadObservations(inst, obs);
  uint32_t crc = crc32_more(0u, offsets, ((size_t)st.nb_tracks + 1u) * sizeof(*offsets));
  crc = crc32_more(crc, ids, (size_t)st.nb_tracks * sizeof(*ids));
  crc = crc32_more(crc, obs, (size_t)st.nb_observations * sizeof(*obs));
  printf(" %s %u %u %u %u %08x", name, st.nb_tracks, st.nb_observations, st.nb_rejected_length, st.nb_rejected_conflicting, crc);
  free(offsets);
  free(ids);
  free(obs);
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
  cfg.sift_buffer_count = 16;
  vksift_Instance inst = NULL;
  if (vksift_ext_createInstanceBatched(&inst, &cfg, NB_PAIRS) != VKSIFT_SUCCESS)
    return 3;
  for (uint32_t v = 0; v < NB_VIEWS; v++)
  {
    const uint32_t w = views[v][0], h = views[v][1];
    for (uint32_t y = 0; y < h; y++)
      memcpy(view + (size_t)y * w, base + (size_t)(y + views[v][3]) * bw + views[v][2], w);
    vksift_detectFeatures(inst, view, w, h, v); /* (the image is copied before the call returns) */
  }
  uint32_t ids_a[NB_PAIRS], ids_b[NB_PAIRS], np = 0;
  for (uint32_t a = 0; a < NB_VIEWS; a++)
    for (uint32_t b = a + 1u; b < NB_VIEWS; b++)
      ids_a[np] = a, ids_b[np++] = b;
  vksift_ext_matchFeaturesFiltered(inst, np, ids_a, ids_b, 0.8f, true);
  vksift_ext_buildTracks(inst, VKSIFT_EXT_TRACKS_FILTERED);
  printf("observations");
  print_selection(inst, "all", 2u, 0u, VKSIFT_EXT_OBS_KEEP_CONFLICTING);
  print_selection(inst, "consistent3", 3u, 0u, VKSIFT_EXT_OBS_DROP_CONFLICTING);
  printf("\n");
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  free(base);
  free(view);
  return inst == NULL ? 0 : 4;
}
