/* A plain-C client of the public headers for tracks across matching calls: the six views of tests/native/client_tracks.c in an instance whose batch
 * capacity is 4, all 15 pairs matched in four calls, each accumulated into the edge store, then built into tracks; prints the store's statistics with a
 * CRC-32 over its edges, and the statistics of the build with a CRC-32 over its track records and per-feature words.
 * tests/test_native_track_edges.py compares the line with the Python mirror's results for the same inputs and with the build of all pairs at once. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vulkansift/vulkansift.h>

#include "vksift_ext.h"

#define NB_VIEWS 6u
#define NB_PAIRS 15u
#define CAPACITY 4u /* pairs per matching call */

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

static void print_build(vksift_Instance inst, const char *name)
{
  vksift_ext_TrackStats st;
  vksift_ext_getTrackStats(inst, &st);
  vksift_ext_Track *tracks = calloc(st.nb_tracks + 1u, sizeof(*tracks));
  vksift_ext_downloadTracks(inst, tracks);
  uint32_t crc = crc32_more(0u, tracks, (size_t)st.nb_tracks * sizeof(*tracks));
  for (uint32_t b = 0; b < NB_VIEWS; b++)
  {
    const uint32_t n = vksift_getFeaturesNumber(inst, b);
    uint32_t *words = calloc(n + 1u, sizeof(*words));
    vksift_ext_downloadFeatureTracks(inst, b, words);
    crc = crc32_more(crc, words, (size_t)n * sizeof(*words));
    free(words);
  }
  printf(" %s %u %u %u %u %08x", name, st.nb_tracks, st.nb_conflicting, st.nb_features, st.nb_edges, crc);
  free(tracks);
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
  if (vksift_ext_createInstanceBatched(&inst, &cfg, CAPACITY) != VKSIFT_SUCCESS)
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
  vksift_ext_beginTrackAccumulation(inst, 1u << 16);
  for (uint32_t first = 0; first < np; first += CAPACITY)
  {
    vksift_ext_matchFeaturesFiltered(inst, np - first < CAPACITY ? np - first : CAPACITY, ids_a + first, ids_b + first, 0.8f, true);
    vksift_ext_accumulateTrackEdges(inst, VKSIFT_EXT_TRACKS_FILTERED);
  }
  vksift_ext_TrackEdgeStats es;
  vksift_ext_getTrackEdgeStats(inst, &es);
  vksift_ext_TrackEdge *edges = calloc(es.nb_edges + 1u, sizeof(*edges));
  vksift_ext_downloadTrackEdges(inst, edges);
  printf("edges %u %u %u %u %08x tracks", es.nb_edges, es.nb_dropped, es.nb_calls, es.nb_changed_buffers, crc32_more(0u, edges, (size_t)es.nb_edges * sizeof(*edges)));
  free(edges);
  vksift_ext_buildTracksAccumulated(inst);
  print_build(inst, "accumulated");
  printf("\n");
  vksift_destroyInstance(&inst);
  vksift_unloadVulkan();
  free(base);
  free(view);
  return inst == NULL ? 0 : 4;
}
