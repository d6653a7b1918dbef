// spread.hip — the spatially distributed feature budget (vksift_ext_keepStrongestFeaturesGrid; PopSift's --filter-grid, AliceVision's gridFiltering,
// OpenCV's GridAdaptedFeatureDetector; no counterpart in the reference): every named SIFT buffer keeps max_features records, each cell of a
// grid_cols x grid_rows grid its own strongest first, in place and in download order, and with cache pointers the same launch leaves the matcher's
// view of the selected buffer. One 1024-thread workgroup per buffer; the section walk, the pick of a 256-bin pass, the ordered compaction and what
// follows it are those of records.h, shared with strongest.hip.
//
//   key(row)    the key of strongest.hip: the intensity word with the sign bit cleared, as an unsigned integer
//   cell(row)   cy * grid_cols + cx; cx = how many of the grid_cols - 1 column bounds x (word 0, fp32) is at or above, cy likewise from y (word 1)
//               and the row bounds. Comparisons only: a NaN or a negative coordinate counts none, -0.0 compares as 0.0, no bit pattern is refused
//   comp(row)   key << B | (total - 1 - row), B the bits of total - 1 rounded up to whole 4-bit digits: (key descending, row ascending) is comp
//               descending, and no two rows share a comp — there are no ties, so no ordered tie ranks per cell
//   phase 1     q = max_features / cells; every cell keeps its min(n_cell, q) largest comps
//   phase 2     the rows phase 1 left keep their max_features - (phase 1's rows) largest comps, wherever they lie
//
// 1. section table and counters -> LDS; total <= max_features: the workgroup returns, nothing of the buffer is written
// 2. key and cell of the first GRID_LDS_ROWS rows -> LDS (the rows beyond are read from the records again in every pass)
// 3. phase 1: radix select in ALL cells at once, most significant digit first, 4 bits per pass — a 16-bin histogram per cell in LDS (256 cells x
//    256 bins would not fit), one thread per cell picks its cell's bin. 8 passes over the key's digits and one per digit of the row: 11 for up
//    to 4096 rows. The first pass also counts the cells' rows. Leaves thr_s[cell]: the smallest comp the cell keeps (none: all ones)
// 4. phase 2: radix select of one threshold over the rows below their cell's, 8 bits per pass, the 256-bin pass of strongest.hip
// 5. the ordered compaction of records.h in rounds of 1024 rows: keep = comp >= thr_s[cell] or comp >= phase 2's threshold; exactly max_features rows
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/records.h"
#include "hip/wave.h"

#define GRID_LDS_ROWS 8192u
#define GRID_MAX_SIDE 16u
#define GRID_MAX_CELLS (GRID_MAX_SIDE * GRID_MAX_SIDE)
#define GRID_HIST_STRIDE 17u /* 16 bins per cell and a word that keeps the cells' threads on different LDS banks */
#define GRID_KEY_WORD 8u     /* intensity: word 8 of the record's head */

namespace
{

struct GridBounds
{
  uint32_t cols, rows;
  float bx[GRID_MAX_SIDE - 1u], by[GRID_MAX_SIDE - 1u]; // cols - 1 and rows - 1 of them are looked at
};

__device__ __forceinline__ uint32_t grid_cell(const GridBounds &g, float x, float y)
{
  uint32_t cx = 0, cy = 0;
  VKSIFT_UNROLL
  for (uint32_t j = 0; j + 1u < GRID_MAX_SIDE; j++)
  {
    cx += (j + 1u < g.cols && x >= g.bx[j]) ? 1u : 0u;
    cy += (j + 1u < g.rows && y >= g.by[j]) ? 1u : 0u;
  }
  return cy * g.cols + cx;
}

__global__ void __launch_bounds__(1024) k_keep_grid(uint32_t *__restrict__ feats_base, uint64_t buf_stride, GatherMap map, SectionTable tab,
                                                    uint32_t *__restrict__ found_base, uint32_t found_buf_stride, uint32_t *__restrict__ found_post,
                                                    uint32_t max_features, GridBounds grid, CacheEntry cache)
{
  __shared__ uint32_t off_s[VKSIFT_MAX_SECTIONS], cnt_s[VKSIFT_MAX_SECTIONS], kept_s[VKSIFT_MAX_SECTIONS];
  __shared__ uint32_t keys_s[GRID_LDS_ROWS], hist[GRID_MAX_CELLS * GRID_HIST_STRIDE], want_s[GRID_MAX_CELLS];
  __shared__ uint64_t thr_s[GRID_MAX_CELLS];
  __shared__ uint8_t cell_s[GRID_LDS_ROWS];
  __shared__ uint32_t wave_tot[16], keep_carry, phase1_kept, sel_s[2];
  const uint32_t tid = threadIdx.x;
  const uint32_t bufi = map.buf[blockIdx.x];
  const auto buf = buffer_ref(feats_base, buf_stride, found_base, found_buf_stride, bufi);
  uint32_t *const feats = buf.recs, *const found = buf.found;
  const uint32_t ncell = grid.cols * grid.rows, per_cell = max_features / ncell;

  // ---- 1
  if (tid < VKSIFT_MAX_SECTIONS)
  {
    const uint32_t raw = tid < tab.nsec ? raw_count(tab, found, tid) : 0u;
    off_s[tid] = tab.off[tid];
    cnt_s[tid] = section_stored(raw, tab.cap[tid]); // (cap is zero from nsec on)
    kept_s[tid] = 0;
  }
  if (tid == 0)
    keep_carry = 0, phase1_kept = 0;
  if (tid < GRID_MAX_CELLS)
    thr_s[tid] = ~0ull, want_s[tid] = (per_cell && tid < ncell) ? 1u : 0u; // (pass 0 takes every row of a cell that wants any)
  for (uint32_t i = tid; i < GRID_MAX_CELLS * GRID_HIST_STRIDE; i += 1024u)
    hist[i] = 0;
  __syncthreads();
  uint32_t cnt[VKSIFT_MAX_SECTIONS];
  const uint32_t total = section_counts(VKSIFT_MAX_SECTIONS, [&](uint32_t o) { return cnt_s[o]; }, cnt_s, cnt);
  if (total <= max_features)
    return;

  // key and cell of a row beyond the LDS copy: from its record
  auto read_row = [&](uint32_t row, uint32_t &key, uint32_t &cell) {
    const uint32_t *r = feats + (size_t)section_row(cnt, off_s, row) * VKSIFT_RECORD_WORDS;
    key = r[GRID_KEY_WORD] & 0x7FFFFFFFu;
    cell = grid_cell(grid, __uint_as_float(r[0]), __uint_as_float(r[1]));
  };
  // comp(row), and the row's cell
  uint32_t row_digits = 1;
  while (row_digits < 8u && ((total - 1u) >> (4u * row_digits)))
    row_digits++;
  const uint32_t row_bits = 4u * row_digits, digits = 8u + row_digits;
  auto comp_of = [&](uint32_t row, uint32_t &cell) {
    uint32_t key;
    if (row < GRID_LDS_ROWS)
      key = keys_s[row], cell = cell_s[row];
    else
      read_row(row, key, cell);
    return ((uint64_t)key << row_bits) | (uint64_t)(total - 1u - row);
  };

  // ---- 2
  for (uint32_t row = tid; row < total && row < GRID_LDS_ROWS; row += 1024u)
  {
    uint32_t key, cell;
    read_row(row, key, cell);
    keys_s[row] = key, cell_s[row] = (uint8_t)cell;
  }
  __syncthreads();

  // ---- 3
  for (uint32_t pass = 0; pass < (per_cell ? digits : 0u); pass++)
  {
    const uint32_t shift = 4u * (digits - 1u - pass);
    for (uint32_t row = tid; row < total; row += 1024u)
    {
      uint32_t cell;
      const uint64_t c = comp_of(row, cell);
      if (want_s[cell] && (pass == 0u || (c >> (shift + 4u)) == (thr_s[cell] >> (shift + 4u))))
        atomicAdd(&hist[cell * GRID_HIST_STRIDE + ((uint32_t)(c >> shift) & 15u)], 1u); // LDS
    }
    __syncthreads();
    if (tid < ncell)
    {
      // one thread per cell: its bins from the top down, cleared for the next pass; the cell's rows that start with its prefix are at least `want`
      uint32_t *h = hist + tid * GRID_HIST_STRIDE;
      uint32_t want = want_s[tid];
      if (pass == 0u)
      {
        uint32_t n = 0;
        VKSIFT_UNROLL
        for (uint32_t b = 0; b < 16u; b++)
          n += h[b];
        want = n < per_cell ? n : per_cell;
        thr_s[tid] = want ? 0ull : ~0ull;
        if (want)
          atomicAdd(&phase1_kept, want); // LDS
      }
      if (want)
      {
        uint32_t above = 0, bin = 0, rest = 0;
        bool found_bin = false;
        VKSIFT_UNROLL
        for (uint32_t i = 0; i < 16u; i++)
        {
          const uint32_t b = 15u - i, n = h[b];
          h[b] = 0;
          if (!found_bin && above + n >= want)
            bin = b, rest = want - above, found_bin = true;
          above += n;
        }
        thr_s[tid] |= (uint64_t)bin << shift;
        want = rest;
      }
      want_s[tid] = want;
    }
    __syncthreads();
  }

  // ---- 4
  const uint32_t left = max_features - phase1_kept;
  uint64_t threshold = ~0ull; // of the rows phase 1 left: none
  if (left)
  {
    const uint32_t passes = (32u + row_bits + 7u) / 8u;
    uint64_t prefix = 0;
    uint32_t want = left;
    for (uint32_t pass = 0; pass < passes; pass++)
    {
      const uint32_t shift = 8u * (passes - 1u - pass);
      if (tid < 256u)
        hist[tid] = 0;
      __syncthreads();
      for (uint32_t row = tid; row < total; row += 1024u)
      {
        uint32_t cell;
        const uint64_t c = comp_of(row, cell);
        if (c < thr_s[cell] && (pass == 0u || (c >> (shift + 8u)) == (prefix >> (shift + 8u))))
          atomicAdd(&hist[(uint32_t)(c >> shift) & 255u], 1u); // LDS
      }
      __syncthreads();
      if (tid < 64u)
        radix_pick_256(*(const uint32_t(*)[256])hist, want, sel_s);
      __syncthreads();
      prefix |= (uint64_t)sel_s[0] << shift;
      want = sel_s[1];
    }
    threshold = prefix;
  }

  // ---- 5
  const CacheEntry entry = cache_entry_of(cache, bufi);
  for (uint32_t base = 0; base < total; base += 1024u)
  {
    const uint32_t row = base + tid;
    uint32_t sec = 0, src_row = 0;
    bool keep = false;
    if (row < total)
    {
      uint32_t cell;
      const uint64_t c = comp_of(row, cell);
      keep = c >= thr_s[cell] || c >= threshold;
      src_row = section_row(cnt, off_s, row);
      sec = section_of(cnt, row);
    }
    compact_round(feats, keep, sec, src_row, off_s, kept_s, wave_tot, keep_carry, entry, max_features);
  }
  compact_finish(tab.nsec, found, found_post, bufi, found_buf_stride, kept_s, entry, cache.pad_rows_to, max_features);
}

} // namespace

extern "C" int vksift_hip_keep_grid(uint8_t *feats_base, uint64_t buf_stride, const uint32_t *buf_ids, uint32_t nslots, uint32_t nsec, const uint32_t *sec_off,
                                    const uint32_t *sec_cap, const uint32_t *fixed_counts, uint32_t *found_base, uint32_t found_buf_stride, uint32_t *found_post,
                                    uint32_t max_features, uint32_t grid_cols, uint32_t grid_rows, const float *col_bounds, const float *row_bounds,
                                    uint32_t pad_rows_to, uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride, uint32_t *n_out_dev,
                                    uint32_t n_stride, vksift_hip_stream s)
{
  if (!sectioned_args_ok(ARGS_ONE_COUNTER_SOURCE | ARGS_CACHE_OPTIONAL, nslots, VKSIFT_HIP_GATHER_SLOTS, nsec, feats_base, buf_stride, fixed_counts, found_base,
                         found_buf_stride, found_post, desc, desc_stride, norms, n_out_dev) ||
      max_features < 1 || (found_post && !found_base) || grid_cols < 1 || grid_cols > GRID_MAX_SIDE || grid_rows < 1 || grid_rows > GRID_MAX_SIDE ||
      (grid_cols > 1 && !col_bounds) || (grid_rows > 1 && !row_bounds))
    return (int)hipErrorInvalidValue;
  GridBounds g = {};
  g.cols = grid_cols, g.rows = grid_rows;
  for (uint32_t j = 0; j + 1u < grid_cols; j++)
    g.bx[j] = col_bounds[j];
  for (uint32_t j = 0; j + 1u < grid_rows; j++)
    g.by[j] = row_bounds[j];
  hipLaunchKernelGGL(k_keep_grid, dim3(nslots), dim3(1024), 0, (hipStream_t)s, (uint32_t *)feats_base, buf_stride / 4u, gather_map(buf_ids, nslots),
                     section_table(nsec, sec_off, sec_cap, fixed_counts), found_base, found_buf_stride, found_post, max_features, g,
                     cache_entry(desc, desc_stride, norms, norm_stride, n_out_dev, n_stride, pad_rows_to));
  return (int)hipGetLastError();
}
