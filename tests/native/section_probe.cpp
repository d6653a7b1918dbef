// Prints what csrc/hip/records.h computes, for tests/test_section_walk.py: one table per input line
// "nsec off[0..16) cap[0..16) found[0..16)". Output per table: "C total cnt[0..16)" (section_counts), then "R" followed by
// section_row of every download-order row in [0, total).
#include <cstdio>
#include <initializer_list>

#include "hip/records.h"

int main()
{
  unsigned nsec;
  while (scanf("%u", &nsec) == 1)
  {
    uint32_t off[VKSIFT_MAX_SECTIONS], cap[VKSIFT_MAX_SECTIONS], found[VKSIFT_MAX_SECTIONS], cnt[VKSIFT_MAX_SECTIONS];
    for (uint32_t *a : {off, cap, found})
      for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
        if (scanf("%u", &a[o]) != 1)
          return 1;
    const uint32_t total = section_counts(nsec, [&](uint32_t o) { return found[o]; }, cap, cnt);
    printf("C %u", total);
    for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
      printf(" %u", cnt[o]);
    printf("\nR");
    for (uint32_t row = 0; row < total; row++)
      printf(" %u", section_row(cnt, off, row));
    printf("\n");
  }
  printf("K %u %u %u %u %u\n", VKSIFT_RECORD_BYTES, VKSIFT_RECORD_WORDS, VKSIFT_RECORD_DESC_AT, VKSIFT_LAYOUT_WORDS, VKSIFT_LAYOUT_CAP_AT);
  return 0;
}
