/* match_stream.h — the stream decomposition of the single-pair matchers (hip/match.hip: k_match_mfma with `stream` set,
 * k_match_scan32; read back by k_match_merge and k_match_fix). Plain integer arithmetic, shared by the kernels and by the CPU
 * test that checks it over many shapes (tests/test_stream_decomposition.py compiles this header with the host compiler).
 *
 * The list of (row block, B tile) pairs, row block major, is cut into runs of `span` tiles, one per workgroup of a grid of G:
 * all resident workgroups get the same number of tiles whatever N_A is. A run may end one row block and start the next; every
 * (row block, workgroup) piece leaves one partial list, in slot = workgroup - first workgroup of the row block. */
#ifndef VKSIFT_MATCH_STREAM_H
#define VKSIFT_MATCH_STREAM_H

#include <stdint.h>

#include "vksift_hip.h" /* VKSIFT_HIP_MATCH_CHUNKS */

#if defined(__HIPCC__)
#define VKSIFT_HD __host__ __device__
#else
#define VKSIFT_HD
#endif

/* Tiles per workgroup. A row block is covered by at most floor(tiles / span) + 2 runs, which must not exceed
 * VKSIFT_HIP_MATCH_CHUNKS partial lists: that is the second term. */
static inline VKSIFT_HD uint32_t stream_span(uint32_t nblocks, uint32_t tiles, uint32_t G)
{
  const uint32_t even = (nblocks * tiles + G - 1u) / G, floor_ = (tiles + (uint32_t)VKSIFT_HIP_MATCH_CHUNKS - 3u) / ((uint32_t)VKSIFT_HIP_MATCH_CHUNKS - 2u);
  const uint32_t span = even > floor_ ? even : floor_;
  return span > 1u ? span : 1u;
}

typedef struct
{
  uint32_t rb, t_first, t_cnt, slot; /* row block, its first tile and tile count in this piece, partial-list slot */
} stream_piece;

/* The piece at *pos of the run [workgroup * span, pos_end) — pos_end = min((workgroup + 1) * span, nblocks * tiles), *pos < pos_end —
 * and *pos moved behind it. */
static inline VKSIFT_HD stream_piece stream_next(uint32_t *pos, uint32_t pos_end, uint32_t tiles, uint32_t span, uint32_t workgroup)
{
  stream_piece p;
  p.rb = *pos / tiles;
  p.t_first = *pos - p.rb * tiles;
  p.t_cnt = tiles - p.t_first < pos_end - *pos ? tiles - p.t_first : pos_end - *pos;
  p.slot = workgroup - (p.rb * tiles) / span;
  *pos += p.t_cnt;
  return p;
}

/* The inverse: how many pieces (= partial lists, slots 0 .. n-1 in tile order) row block rb has. */
static inline VKSIFT_HD uint32_t stream_pieces(uint32_t rb, uint32_t tiles, uint32_t span)
{
  return ((rb + 1u) * tiles - 1u) / span - (rb * tiles) / span + 1u;
}

#endif
