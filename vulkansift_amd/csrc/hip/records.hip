// records.hip — the record-moving launches around the matcher: SIFT buffer sections -> the matcher's dense rows (pack_BufferMemory,
// sift_memory.c:957-1047: the gather pass that serves uploaded buffers and every buffer an instance matches before its cache exists; freshly
// detected buffers get their rows from the descriptor launch, features.hip), sections -> dense 164-byte records for the batched
// download, and the GPU-side cross-check + ratio filter over 2-NN records (src/examples/test_sift_match.cpp:90-107). Split off match.hip
// in round 6: none of this is matcher arithmetic. The steps these kernels share with each other and with verify.hip / guided.hip — the
// section walk, the ordered append, the record constants — are defined once, in records.h.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/records.h"

namespace
{

__global__ void __launch_bounds__(256) k_gather_desc(const uint8_t *__restrict__ feats, uint32_t n, uint32_t *__restrict__ desc)
{
  uint32_t i = blockIdx.x * 256 + threadIdx.x; // dword index
  if (i >= n * 32u)
    return;
  uint32_t row = i >> 5, j = i & 31u;
  desc[i] = *(const uint32_t *)(feats + (size_t)row * VKSIFT_RECORD_BYTES + VKSIFT_RECORD_DESC_AT + 4 * j);
}

// Gather the descriptors of a (sectioned or packed) SIFT buffer into dense rows in download order AND compute
// their shifted norms, with the per-section feature counts read on the device (no host round trip):
// row -> section by scanning the <= 16 section counts; eight lanes per row, 16 bytes per lane (the cache row step of records.h).
__global__ void __launch_bounds__(256) k_gather_sections(const uint32_t *__restrict__ feats_base, uint64_t buf_stride, GatherMap map, SectionTable tab,
                                                         const uint32_t *__restrict__ found_base, uint32_t found_buf_stride, CacheEntry cache)
{
  const uint32_t bufi = map.buf[blockIdx.y];
  const auto buf = buffer_ref(feats_base, buf_stride, found_base, found_buf_stride, bufi);
  // the dense rows, their norms and the row count land in the per-BUFFER cache entry (reused by every later match of the buffer)
  const CacheEntry entry = cache_entry_of(cache, bufi);

  const uint32_t j = threadIdx.x & 7u; // 16 bytes of a row per lane: a wave moves 8 rows at a time, a workgroup 32
  // stored count of every section (uniform), then a grid-stride walk over the rows that exist
  uint32_t cnt[VKSIFT_MAX_SECTIONS];
  const uint32_t total = stored_counts(tab, buf.found, cnt);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *entry.n = total;
  const uint32_t nrows = total > cache.pad_rows_to ? total : cache.pad_rows_to;
  for (uint32_t row = blockIdx.x * GATHER_ROWS_PER_BLOCK + (threadIdx.x >> 3); row < nrows; row += gridDim.x * GATHER_ROWS_PER_BLOCK)
  {
    uint4 v = uint4{0u, 0u, 0u, 0u}; // rows in [total, pad_rows_to): quirk Q6 padding, all-zero descriptors
    if (row < total)
    {
      // (records are 164 bytes, the descriptor starts at byte 36: dword-aligned 16-byte loads)
      const uint32_t *p = buf.recs + (size_t)section_row(cnt, tab.off, row) * VKSIFT_RECORD_WORDS + VKSIFT_RECORD_HEAD_WORDS + 4u * j;
      v = uint4{p[0], p[1], p[2], p[3]};
    }
    cache_row_store(entry, row, j, v);
  }
}

// Download packing (sift_memory.c:957-1047 pack_BufferMemory, here for a whole batch of buffers at once): the stored features of
// slot blockIdx.y's buffer — its sections in order, min(found, capacity) records each — as dense 164-byte records at
// out + out_row[slot] * 164. One dword per thread step; the host then fetches all buffers of a detection with ONE copy.
// (64 slots, not the 512 of GatherMap: two maps of that size would add 3.5 KB to the launch's kernel arguments)
struct SlotMap
{
  uint32_t buf[64]; // SIFT buffer index handled by slot blockIdx.y
};
struct PackOffsets
{
  uint32_t row[64];
};
__global__ void __launch_bounds__(256) k_pack_features(const uint32_t *__restrict__ feats_base, uint64_t buf_stride, SlotMap map, SectionTable tab,
                                                       const uint32_t *__restrict__ found_base, uint32_t found_buf_stride, uint32_t *__restrict__ out,
                                                       PackOffsets offs, uint32_t *__restrict__ found_post)
{
  const uint32_t slot = blockIdx.y;
  const uint32_t bufi = map.buf[slot];
  const auto buf = buffer_ref(feats_base, buf_stride, found_base, found_buf_stride, bufi);
  // feature posting: the buffer's counters go to the host mirror with the records (same layout as found_base, mapped pinned memory)
  if (found_post && blockIdx.x == 0 && threadIdx.x < found_buf_stride)
    found_post[(size_t)bufi * found_buf_stride + threadIdx.x] = buf.found[threadIdx.x];
  uint32_t cnt[VKSIFT_MAX_SECTIONS];
  const uint32_t total = stored_counts(tab, buf.found, cnt);
  uint32_t *dst = out + (size_t)offs.row[slot] * VKSIFT_RECORD_WORDS;
  const uint32_t ndw = total * VKSIFT_RECORD_WORDS;
  for (uint32_t d = blockIdx.x * 256u + threadIdx.x; d < ndw; d += gridDim.x * 256u)
  {
    const uint32_t row = d / VKSIFT_RECORD_WORDS, w = d - row * VKSIFT_RECORD_WORDS;
    dst[d] = buf.recs[(size_t)section_row(cnt, tab.off, row) * VKSIFT_RECORD_WORDS + w];
  }
}

// Cross-check + Lowe-ratio filter over the 2-NN records of a forward (A -> B) and, optionally, a reverse (B -> A)
// matching — what every caller of the reference runs on the CPU after vksift_downloadMatches
// (src/examples/test_sift_match.cpp:90-107, src/perf/perf_common.cpp:123-169). One 1024-thread workgroup per pair keeps
// the survivors in increasing idx_a order (ordered_keep: ballot + scan compaction, no atomics), 16 B per survivor.
__global__ void __launch_bounds__(1024) k_filter_matches(const uint32_t *__restrict__ fwd, uint64_t fwd_slot_stride, const uint32_t *__restrict__ rev,
                                                         uint64_t rev_slot_stride, const uint32_t *__restrict__ n_fwd, uint32_t n_stride, float ratio,
                                                         uint32_t *__restrict__ out, uint64_t out_slot_stride, uint32_t *__restrict__ out_n)
{
  __shared__ uint32_t wave_tot[16];
  __shared__ uint32_t carry_s;
  const uint32_t slot = blockIdx.x;
  fwd += (size_t)slot * fwd_slot_stride;
  if (rev)
    rev += (size_t)slot * rev_slot_stride;
  out += (size_t)slot * out_slot_stride;
  const uint32_t na = n_fwd[(size_t)slot * n_stride], nb = n_fwd[(size_t)slot * n_stride + 1];
  if (threadIdx.x == 0)
    carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < na; base += 1024)
  {
    const uint32_t i = base + threadIdx.x;
    bool keep = false;
    uint32_t j = 0, d1 = 0, d2 = 0;
    if (i < na)
    {
      const uint32_t *m = fwd + (size_t)i * 5;
      j = m[1], d1 = m[3], d2 = m[4];
      keep = (__uint_as_float(d1) / __uint_as_float(d2)) < ratio;
      if (rev)
      {
        keep = keep && j < nb;
        if (keep)
        {
          const uint32_t *r = rev + (size_t)j * 5;
          keep = r[1] == i && (__uint_as_float(r[3]) / __uint_as_float(r[4])) < ratio;
        }
      }
    }
    uint32_t *o = out + (size_t)ordered_keep(keep, wave_tot, carry_s) * 4;
    if (keep)
      o[0] = fwd[(size_t)i * 5], o[1] = j, o[2] = d1, o[3] = d2;
  }
  if (threadIdx.x == 0)
    out_n[slot] = carry_s;
}

} // namespace

extern "C"
{
  int vksift_hip_gather_descriptors(const uint8_t *feats, uint32_t n, uint8_t *desc, vksift_hip_stream s)
  {
    if (n == 0)
      return 0;
    uint32_t blocks = (n * 32u + 255u) / 256u;
    hipLaunchKernelGGL(k_gather_desc, dim3(blocks), dim3(256), 0, (hipStream_t)s, feats, n, (uint32_t *)desc);
    return (int)hipGetLastError();
  }

  int vksift_hip_gather_sections(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec,
                                 const uint32_t *sec_off, const uint32_t *sec_cap, const uint32_t *fixed_counts, const uint32_t *found_base,
                                 uint32_t found_buf_stride, uint32_t max_rows, uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_slot_stride,
                                 uint32_t *norms, uint64_t norm_slot_stride, uint32_t *n_out_dev, uint32_t n_slot_stride, vksift_hip_stream s)
  {
    /* (this entry predates the others: it takes either counter source as it comes, and its cache block is not optional) */
    if (!sectioned_args_ok(0u, nslots, VKSIFT_HIP_GATHER_SLOTS, nsec, feats_base, buf_stride, fixed_counts, found_base, found_buf_stride, nullptr, desc,
                           desc_slot_stride, norms, n_out_dev))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_sections, dim3(gather_walk_blocks(max_rows, pad_rows_to, nslots), nslots), dim3(256), 0, (hipStream_t)s, (const uint32_t *)feats_base,
                       buf_stride / 4u, gather_map(buf_ids, nslots), section_table(nsec, sec_off, sec_cap, fixed_counts), found_base, found_buf_stride,
                       cache_entry(desc, desc_slot_stride, norms, norm_slot_stride, n_out_dev, n_slot_stride, pad_rows_to));
    return (int)hipGetLastError();
  }

  int vksift_hip_pack_features(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, const uint32_t *out_rows, uint32_t nslots, uint32_t nsec,
                               const uint32_t *sec_off, const uint32_t *sec_cap, const uint32_t *found_base, uint32_t found_buf_stride, uint8_t *out,
                               uint32_t max_rows, uint32_t *found_post, vksift_hip_stream s)
  {
    if (!sectioned_args_ok(0u, nslots, 64u, nsec, feats_base, buf_stride, nullptr, found_base, found_buf_stride, found_post, nullptr, 0, nullptr, nullptr) ||
        ((uintptr_t)out & 3u)) /* records are copied dword by dword */
      return (int)hipErrorInvalidValue;
    const SectionTable t = section_table(nsec, sec_off, sec_cap, nullptr);
    SlotMap m;
    PackOffsets po;
    for (uint32_t i = 0; i < 64; i++)
      m.buf[i] = i < nslots ? buf_ids[i] : 0u, po.row[i] = i < nslots ? out_rows[i] : 0u;
    uint32_t blocks = (uint32_t)(((uint64_t)max_rows * VKSIFT_RECORD_WORDS + 1023u) / 1024u); /* four dwords per thread */
    blocks = blocks < 1u ? 1u : (blocks > 128u ? 128u : blocks);
    hipLaunchKernelGGL(k_pack_features, dim3(blocks, nslots), dim3(256), 0, (hipStream_t)s, (const uint32_t *)feats_base, buf_stride / 4u, m, t, found_base,
                       found_buf_stride, (uint32_t *)out, po, found_post);
    return (int)hipGetLastError();
  }

  int vksift_hip_filter_matches(const uint8_t *fwd, uint64_t fwd_slot_stride, const uint8_t *rev, uint64_t rev_slot_stride, const uint32_t *n_fwd,
                                uint32_t n_stride, float ratio, uint32_t nslots, uint8_t *out, uint64_t out_slot_stride, uint32_t *out_n, vksift_hip_stream s)
  {
    if (nslots < 1)
      return (int)hipErrorInvalidValue;
    /* records are read and written dword by dword; the byte strides are handed to the kernel in dwords */
    if (((uintptr_t)fwd & 3u) || (fwd_slot_stride & 3u) || ((uintptr_t)out & 3u) || (out_slot_stride & 3u) ||
        (rev && (((uintptr_t)rev & 3u) || (rev_slot_stride & 3u))))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_filter_matches, dim3(nslots), dim3(1024), 0, (hipStream_t)s, (const uint32_t *)fwd, fwd_slot_stride / 4, (const uint32_t *)rev,
                       rev_slot_stride / 4, n_fwd, n_stride, ratio, (uint32_t *)out, out_slot_stride / 4, out_n);
    return (int)hipGetLastError();
  }
}
