// rootsift.hip — RootSIFT descriptors (vksift_ext_convertToRootSift; Arandjelovic & Zisserman 2012: COLMAP's L1_ROOT, PopSift's --root-sift, the
// two lines after OpenCV's detectAndCompute; no counterpart in the reference): every stored record of every named SIFT buffer gets its 128 descriptor
// bytes converted in place, and with cache pointers the same launch leaves the matcher's view of the converted buffer. The section walk, the
// launch arguments, the per-buffer resolve and the cache row step are those of records.h, the reductions those of wave.h.
//
//   s        the sum of the row's 128 bytes (0 .. 32640); s == 0: the row stays all zero
//   out[i]   min(255, r), r the integer with (2r - 1)^2 s <= 2^20 d[i] < (2r + 1)^2 s: 512 sqrt(d[i] / s) rounded half up, exactly; 0 for d[i] == 0
//            (tests/np_rootsift.py is the specification)
//
// The shape of k_gather_sections: eight lanes per row, four dwords (sixteen bins) per lane, so a wave has eight rows — 1 KB — in flight, the walk
// from row to record and the reductions are paid once per sixteen bytes of a lane, and a cache row is stored 16 bytes at a time by the lane that
// computed them. (A half-wave per row with one dword per lane was measured first: 0.153 ms for the 512 x 1903 rows of the benchmark, bound by the
// one dword a lane has in flight and by a walk and three five-step butterflies per dword.) The record is 164 bytes and its descriptor starts at
// byte 36: the four loads and the four stores are dword accesses. udot4 sums a lane's bytes, a butterfly over the eight lanes finishes s. Each
// bin takes a float estimate of r (hardware reciprocal and square root, their error some 1e-4 of a unit; leaning up, so that it is r or r + 1)
// and one exact correction in integers against the inequality that tells the two apart — the estimate alone, even with every operation correctly
// rounded, is wrong for 18 of the 8 323 455 (d, s) pairs. The head words of a record are neither read nor written. Rows beyond the stored total up to pad_rows_to are the zero
// rows of quirk Q6 and take the same path with zero dwords. No lane branches on its data; a row is all or nothing for its eight lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/records.h"
#include "hip/wave.h"

namespace
{

// one bin: d of a row whose bytes sum to s >= 1 (inv_s: about 1 / s)
__device__ __forceinline__ uint32_t root_bin(uint32_t d, uint32_t s, float inv_s)
{
  // The estimate leans up by 2^-8, some thirty times the error of the hardware reciprocal, product and square root (about 1e-4 of a unit): it is
  // never below r and at most r + 1, so one of the two inequalities decides: e is r iff (2e - 1)^2 s <= 2^20 d.
  const uint32_t e = (uint32_t)fmaf(__builtin_amdgcn_sqrtf((float)d * inv_s), 512.0f, 0.5f + 0x1p-8f);
  // An arbitrary r against an arbitrary s would need 64 bits (1025^2 * 32640). This product does not: (2r - 1)^2 s <= 2^20 d < 2^28 and r >= 3 for
  // d >= 1 (512 sqrt(1 / 32640) = 2.8), so (2e - 1)^2 s <= (2r + 1)^2 s <= (7 / 5)^2 2^28 < 2^32, and every factor is below 2^24: the full-rate
  // 24-bit multiply serves (a 32-bit one costs four issue slots). tests/test_np_rootsift.py pins the bound over the whole domain. d == 0 is
  // answered at the end, whatever the product was.
  const uint32_t lo = 2u * e - 1u;
  const uint32_t r = e - (uint32_t)(__umul24(__umul24(lo, lo), s) > (d << 20));
  return d ? (r < 255u ? r : 255u) : 0u;
}

// four bins
__device__ __forceinline__ uint32_t root_dword(uint32_t v, uint32_t s, float inv_s)
{
  uint32_t out = 0u;
  VKSIFT_UNROLL
  for (uint32_t k = 0; k < 4u; k++)
    out |= root_bin((v >> (8u * k)) & 255u, s, inv_s) << (8u * k);
  return out;
}

__device__ __forceinline__ uint32_t bytes_sum(uint4 v)
{
  uint32_t s = __builtin_amdgcn_udot4(v.x, 0x01010101u, 0u, false);
  s = __builtin_amdgcn_udot4(v.y, 0x01010101u, s, false);
  s = __builtin_amdgcn_udot4(v.z, 0x01010101u, s, false);
  return __builtin_amdgcn_udot4(v.w, 0x01010101u, s, false);
}

__global__ void __launch_bounds__(256) k_root_descriptors(uint32_t *__restrict__ feats_base, uint64_t buf_stride, GatherMap map, SectionTable tab,
                                                          const uint32_t *__restrict__ found_base, uint32_t found_buf_stride, CacheEntry cache)
{
  const uint32_t bufi = map.buf[blockIdx.y];
  const auto buf = buffer_ref(feats_base, buf_stride, found_base, found_buf_stride, bufi);
  const CacheEntry entry = cache_entry_of(cache, bufi);
  const uint32_t j = threadIdx.x & 7u; // 16 bytes of a row per lane: a wave converts 8 rows at a time, a workgroup 32

  uint32_t cnt[VKSIFT_MAX_SECTIONS];
  const uint32_t total = stored_counts(tab, buf.found, cnt);
  uint32_t nrows = total;
  if (entry.rows)
  {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      *entry.n = total;
    nrows = total > cache.pad_rows_to ? total : cache.pad_rows_to;
  }
  for (uint32_t row = blockIdx.x * GATHER_ROWS_PER_BLOCK + (threadIdx.x >> 3); row < nrows; row += gridDim.x * GATHER_ROWS_PER_BLOCK)
  {
    uint32_t *p = nullptr;
    uint4 v = uint4{0u, 0u, 0u, 0u}; // rows in [total, pad_rows_to): the zero rows of the cache entry only
    if (row < total)
    {
      p = buf.recs + (size_t)section_row(cnt, tab.off, row) * VKSIFT_RECORD_WORDS + VKSIFT_RECORD_HEAD_WORDS + 4u * j;
      v = uint4{p[0], p[1], p[2], p[3]};
    }
    uint32_t s = lanes_sum_u32<8>(bytes_sum(v));
    s = s ? s : 1u; // (an all-zero row: every bin is zero and stays so)
    const float inv_s = __builtin_amdgcn_rcpf((float)s);
    const uint4 out = uint4{root_dword(v.x, s, inv_s), root_dword(v.y, s, inv_s), root_dword(v.z, s, inv_s), root_dword(v.w, s, inv_s)};
    if (p)
      p[0] = out.x, p[1] = out.y, p[2] = out.z, p[3] = out.w;
    if (entry.rows)
      cache_row_store(entry, row, j, out); // the bytes k_gather_sections writes for the converted buffer
  }
}

} // namespace

extern "C" int vksift_hip_root_descriptors(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                                           const uint32_t *sec_cap, const uint32_t *fixed_counts, const uint32_t *found_base, uint32_t found_buf_stride,
                                           uint32_t max_rows, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride,
                                           uint32_t *n_out_dev, uint32_t n_stride, vksift_hip_stream s)
{
  if (!sectioned_args_ok(ARGS_ONE_COUNTER_SOURCE | ARGS_CACHE_OPTIONAL, nslots, VKSIFT_HIP_GATHER_SLOTS, nsec, feats_base, buf_stride, fixed_counts, found_base,
                         found_buf_stride, nullptr, desc, desc_stride, norms, n_out_dev))
    return (int)hipErrorInvalidValue;
  const CacheEntry cache = cache_entry(desc, desc_stride, norms, norm_stride, n_out_dev, n_stride, pad_rows_to);
  hipLaunchKernelGGL(k_root_descriptors, dim3(gather_walk_blocks(max_rows, cache.pad_rows_to, nslots), nslots), dim3(256), 0, (hipStream_t)s, (uint32_t *)feats_base,
                     buf_stride / 4u, gather_map(buf_ids, nslots), section_table(nsec, sec_off, sec_cap, fixed_counts), found_base, found_buf_stride, cache);
  return (int)hipGetLastError();
}
