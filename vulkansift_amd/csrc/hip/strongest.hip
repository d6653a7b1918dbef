// strongest.hip — the feature budget (vksift_ext_keepStrongestFeatures; OpenCV's nfeatures, SiftGPU's -tc, PopSift's --filter-max-extrema; no
// counterpart in the reference, whose only limit is the capacity of a section): every named SIFT buffer keeps its max_features strongest
// records, in place and in download order, and with cache pointers the same launch leaves the matcher's view of the selected buffer.
// One 1024-thread workgroup per buffer: the compaction is ordered, so it takes no atomics on global memory, and the section walk, the
// ordered append, the per-buffer resolve, the cache row's norm, the pick of a radix pass's bin and the compaction round with what follows it
// (shared with the grid rule of spread.hip) are those of records.h.
//
//   key(row)   the record's intensity word (|DoG response|) with the sign bit cleared, compared as an unsigned integer: a total order on
//              every bit pattern (-0 == +0 < denormals < normals < inf < NaN patterns); no float comparison takes place
//   kept       the first min(total, max_features) rows by (key descending, download row ascending)
//
// 1. section table and counters -> LDS; total <= max_features: the workgroup returns, nothing of the buffer is written
// 2. threshold key: radix select, most significant byte first, four passes over the keys with a 256-bin LDS histogram each (one dword per
//    record and pass; the keys of the first STRONGEST_LDS_KEYS rows are held in LDS after the first pass)
// 3. the select leaves how many rows AT the threshold are kept (the tie quota): max_features less the rows above it
// 4. one ordered pass in rounds of 1024 rows: keep = above, or at the threshold with a tie rank below the quota; a kept row's place is its
//    section's start plus the kept rows of that section in front of it. Every kept record of the round is loaded into registers, a barrier
//    is passed, then it is stored: a destination never lies beyond its source (the kept rows in front of a row are at most the rows in
//    front of it) and never beyond the round (it is the old place of a row at or in front of the source), and rounds run in order — so a
//    store can only land on a record of an earlier round, already consumed, or of this round, already in registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/records.h"
#include "hip/wave.h"

#define STRONGEST_LDS_KEYS 8192u
#define STRONGEST_KEY_WORD 8u /* intensity: word 8 of the record's head */

namespace
{

__global__ void __launch_bounds__(1024) k_keep_strongest(uint32_t *__restrict__ feats_base, uint64_t buf_stride, GatherMap map, SectionTable tab,
                                                         uint32_t *__restrict__ found_base, uint32_t found_buf_stride, uint32_t *__restrict__ found_post,
                                                         uint32_t max_features, CacheEntry cache)
{
  __shared__ uint32_t off_s[VKSIFT_MAX_SECTIONS], cnt_s[VKSIFT_MAX_SECTIONS], kept_s[VKSIFT_MAX_SECTIONS];
  __shared__ uint32_t hist[256], keys_s[STRONGEST_LDS_KEYS];
  __shared__ uint32_t wave_tot[16], tie_carry, keep_carry, sel_s[2];
  const uint32_t tid = threadIdx.x;
  const uint32_t bufi = map.buf[blockIdx.x];
  const auto buf = buffer_ref(feats_base, buf_stride, found_base, found_buf_stride, bufi);
  uint32_t *const feats = buf.recs, *const found = buf.found;

  // ---- 1
  if (tid < VKSIFT_MAX_SECTIONS)
  {
    const uint32_t raw = tid < tab.nsec ? raw_count(tab, found, tid) : 0u;
    off_s[tid] = tab.off[tid];
    cnt_s[tid] = section_stored(raw, tab.cap[tid]); // (cap is zero from nsec on)
    kept_s[tid] = 0;
  }
  if (tid == 0)
    tie_carry = 0, keep_carry = 0;
  __syncthreads();
  uint32_t cnt[VKSIFT_MAX_SECTIONS];
  const uint32_t total = section_counts(VKSIFT_MAX_SECTIONS, [&](uint32_t o) { return cnt_s[o]; }, cnt_s, cnt);
  if (total <= max_features)
    return;

  auto key_at = [&](uint32_t row) { return feats[(size_t)section_row(cnt, off_s, row) * VKSIFT_RECORD_WORDS + STRONGEST_KEY_WORD] & 0x7FFFFFFFu; };

  // ---- 2, 3
  uint32_t prefix = 0, want = max_features; // the want-th largest of the keys that start with `prefix`
  for (uint32_t pass = 0; pass < 4u; pass++)
  {
    const uint32_t shift = 24u - 8u * pass, decided = pass ? 0xFFFFFFFFu << (shift + 8u) : 0u;
    if (tid < 256u)
      hist[tid] = 0;
    __syncthreads();
    for (uint32_t row = tid; row < total; row += 1024u)
    {
      uint32_t key;
      if (pass == 0u)
      {
        key = key_at(row);
        if (row < STRONGEST_LDS_KEYS)
          keys_s[row] = key;
      }
      else
        key = row < STRONGEST_LDS_KEYS ? keys_s[row] : key_at(row);
      if ((key & decided) == prefix)
        atomicAdd(&hist[(key >> shift) & 255u], 1u); // LDS
    }
    __syncthreads();
    if (tid < 64u)
      radix_pick_256(hist, want, sel_s);
    __syncthreads();
    prefix |= sel_s[0] << shift;
    want = sel_s[1];
  }
  const uint32_t threshold = prefix, quota = want; // `quota` of the rows at the threshold are kept, max_features - quota rows lie above it

  // ---- 4
  const CacheEntry entry = cache_entry_of(cache, bufi);
  for (uint32_t base = 0; base < total; base += 1024u)
  {
    const uint32_t row = base + tid;
    uint32_t key = 0, sec = 0, src_row = 0;
    const bool valid = row < total;
    if (valid)
    {
      key = row < STRONGEST_LDS_KEYS ? keys_s[row] : key_at(row);
      src_row = section_row(cnt, off_s, row);
      sec = section_of(cnt, row);
    }
    const bool tie = valid && key == threshold;
    const uint32_t tie_rank = ordered_keep(tie, wave_tot, tie_carry);
    const bool keep = valid && (key > threshold || (tie && tie_rank < quota));
    compact_round(feats, keep, sec, src_row, off_s, kept_s, wave_tot, keep_carry, entry, max_features);
  }
  compact_finish(tab.nsec, found, found_post, bufi, found_buf_stride, kept_s, entry, cache.pad_rows_to, max_features);
}

} // namespace

extern "C" int vksift_hip_keep_strongest(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                                         const uint32_t *sec_cap, const uint32_t *fixed_counts, uint32_t *found_base, uint32_t found_buf_stride,
                                         uint32_t *found_post, uint32_t max_features, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms,
                                         uint64_t norm_stride, uint32_t *n_out_dev, uint32_t n_stride, vksift_hip_stream s)
{
  if (!sectioned_args_ok(ARGS_ONE_COUNTER_SOURCE | ARGS_CACHE_OPTIONAL, nslots, VKSIFT_HIP_GATHER_SLOTS, nsec, feats_base, buf_stride, fixed_counts, found_base,
                         found_buf_stride, found_post, desc, desc_stride, norms, n_out_dev) ||
      max_features < 1 || (found_post && !found_base)) /* (the mirror without device counters has nothing to mirror) */
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_keep_strongest, dim3(nslots), dim3(1024), 0, (hipStream_t)s, (uint32_t *)feats_base, buf_stride / 4u, gather_map(buf_ids, nslots),
                     section_table(nsec, sec_off, sec_cap, fixed_counts), found_base, found_buf_stride, found_post, max_features,
                     cache_entry(desc, desc_stride, norms, norm_stride, n_out_dev, n_stride, pad_rows_to));
  return (int)hipGetLastError();
}
