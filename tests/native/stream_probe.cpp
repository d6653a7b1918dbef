// Prints what csrc/match_stream.h computes, for tests/test_stream_decomposition.py: one shape per input line
// "na nb G block_rows tile_rows". Output per shape: "S span nblocks tiles", one "P workgroup rb t_first t_cnt slot" per piece in
// workgroup order (the walk the kernels do), then "M" followed by stream_pieces of every row block.
#include <cstdio>

#include "match_stream.h"

int main()
{
  unsigned na, nb, G, block_rows, tile_rows;
  while (scanf("%u %u %u %u %u", &na, &nb, &G, &block_rows, &tile_rows) == 5)
  {
    const uint32_t nblocks = (na + block_rows - 1u) / block_rows, tiles = (nb + tile_rows - 1u) / tile_rows;
    const uint32_t span = stream_span(nblocks, tiles, G);
    printf("S %u %u %u\n", span, nblocks, tiles);
    for (uint32_t w = 0; w < G; w++)
    {
      uint32_t pos = w * span;
      const uint32_t pos_end = pos + span < nblocks * tiles ? pos + span : nblocks * tiles;
      while (pos < pos_end)
      {
        const stream_piece p = stream_next(&pos, pos_end, tiles, span, w);
        printf("P %u %u %u %u %u\n", w, p.rb, p.t_first, p.t_cnt, p.slot);
      }
    }
    printf("M");
    for (uint32_t rb = 0; rb < nblocks; rb++)
      printf(" %u", stream_pieces(rb, tiles, span));
    printf("\n");
  }
  return 0;
}
