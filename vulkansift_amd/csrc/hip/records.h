/* records.h — the steps every launch that moves or addresses SIFT records shares (hip/records.hip, hip/strongest.hip, hip/spread.hip,
 * hip/rootsift.hip, hip/verify.hip, hip/guided.hip), each defined once: the record and section-table constants, the walk from a download-order
 * row to a stored row, the decode of a pair table's layout word, the ordered append of a 1024-thread workgroup, what the launches over
 * sectioned buffers (vksift_hip_gather_sections, _pack_features, _keep_strongest, _keep_grid, _root_descriptors) have in common — the by-value
 * launch arguments, the prologue check of their entries, the grid of the gather walk, the per-buffer resolve, the stored counts and the cache
 * row step — and the in-place ordered compaction of the two budgets (vksift_hip_keep_strongest, _keep_grid) with what follows it. The
 * constants compile as C (host/vksift_internal.h takes them from here), the walk as host C++ too: plain integer arithmetic, checked row by
 * row by tests/test_section_walk.py, which compiles this header with the host compiler. The rest is device code and its launchers' host side. */
#ifndef VKSIFT_RECORDS_H
#define VKSIFT_RECORDS_H

#include <stdint.h>

#define VKSIFT_RECORD_BYTES 164u /* a stored feature: {x, y, ...} from byte 0, the 128 descriptor bytes from VKSIFT_RECORD_DESC_AT */
#define VKSIFT_RECORD_WORDS 41u
#define VKSIFT_RECORD_HEAD_WORDS 9u /* {x, y, scale_x, scale_y, scale_idx, octave_idx, sigma, orientation, intensity} */
#define VKSIFT_RECORD_DESC_AT 36u
#define VKSIFT_MAX_SECTIONS 16u /* one section per octave */
/* A pair table names each buffer's layout by one word: VKSIFT_LAYOUT_DENSE | n for n dense records (uploaded features), else the index
 * of a section table of VKSIFT_LAYOUT_WORDS words {nsec, off[16], cap[16]}. */
#define VKSIFT_LAYOUT_DENSE 0x80000000u
#define VKSIFT_LAYOUT_OFF_AT 1u
#define VKSIFT_LAYOUT_CAP_AT (1u + VKSIFT_MAX_SECTIONS)
#define VKSIFT_LAYOUT_WORDS (1u + 2u * VKSIFT_MAX_SECTIONS)

#ifdef __cplusplus

#if defined(__HIPCC__)
#define VKSIFT_HD __host__ __device__
#define VKSIFT_UNROLL _Pragma("unroll")
#else
#define VKSIFT_HD
#define VKSIFT_UNROLL
#endif

/* ---- the walk -------------------------------------------------------------------------------------------------------------------------
 * A buffer stores section o's features from record off[o] on, min(raw count, cap[o]) of them; download order is the sections in turn. */
static inline VKSIFT_HD uint32_t section_stored(uint32_t raw, uint32_t cap) { return raw < cap ? raw : cap; }

/* cnt[o] = stored count of section o (raw(o): the detector's counter, or a fixed count), zero from nsec on; returns their total */
template <class Raw, class Cap, class Cnt> static inline VKSIFT_HD uint32_t section_counts(uint32_t nsec, Raw raw, const Cap &cap, Cnt &cnt)
{
  uint32_t total = 0;
  VKSIFT_UNROLL
  for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
  {
    const uint32_t n = o < nsec ? section_stored(raw(o), cap[o]) : 0u;
    cnt[o] = n;
    total += n;
  }
  return total;
}

/* the stored row of download-order row `row` < total: every section is tried, unrolled, so that cnt and off stay where they are
 * (registers, kernel arguments or LDS) and no lane branches */
template <class Cnt, class Off> static inline VKSIFT_HD uint32_t section_row(const Cnt &cnt, const Off &off, uint32_t row)
{
  uint32_t base = 0, src_row = 0;
  VKSIFT_UNROLL
  for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
  {
    const uint32_t c = cnt[o];
    if (row >= base && row < base + c)
      src_row = off[o] + (row - base);
    base += c;
  }
  return src_row;
}

#if defined(__HIPCC__)

#include "vksift_hip.h" /* VKSIFT_HIP_GATHER_SLOTS */
#include "wave.h"

/* ---- launch arguments -----------------------------------------------------------------------------------------------------------------
 * What the launches over sectioned buffers take by value (vksift_hip_gather_sections, vksift_hip_pack_features, vksift_hip_keep_strongest,
 * vksift_hip_root_descriptors): the
 * section table every buffer of the launch shares, and the buffer each slot serves. */
struct SectionTable
{
  uint32_t nsec;
  uint32_t off[VKSIFT_MAX_SECTIONS];   // first feature of each section inside the buffer
  uint32_t cap[VKSIFT_MAX_SECTIONS];   // capacity (stored = min(found, cap))
  uint32_t fixed[VKSIFT_MAX_SECTIONS]; // used instead of found[] when found == nullptr (uploaded / packed buffers)
};

/* entries at and beyond nsec are zero; fixed_counts may be NULL (all zero) */
static inline SectionTable section_table(uint32_t nsec, const uint32_t *sec_off, const uint32_t *sec_cap, const uint32_t *fixed_counts)
{
  SectionTable t;
  t.nsec = nsec;
  for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
  {
    t.off[o] = o < nsec ? sec_off[o] : 0u;
    t.cap[o] = o < nsec ? sec_cap[o] : 0u;
    t.fixed[o] = (o < nsec && fixed_counts) ? fixed_counts[o] : 0u;
  }
  return t;
}

// (all buffers of a batched detection in ONE launch: 512 buffers = 8 launches of 64 slots x 256 blocks until round 5 — 25 us each alone,
// 330 us each queued behind the next detection's blur launches, 16 384 mostly idle workgroups per launch)
struct GatherMap
{
  uint32_t buf[VKSIFT_HIP_GATHER_SLOTS]; // SIFT buffer index handled by the slot's workgroup(s)
};

static inline GatherMap gather_map(const uint32_t *buf_ids, uint32_t nslots)
{
  GatherMap m;
  for (uint32_t i = 0; i < VKSIFT_HIP_GATHER_SLOTS; i++)
    m.buf[i] = i < nslots ? buf_ids[i] : 0u;
  return m;
}

/* The matcher's cache block as the launches of the family take it: vksift_hip_gather_sections fills the entry of a buffer, and the launches that
 * rewrite records in place (vksift_hip_keep_strongest, vksift_hip_root_descriptors) leave it as the gather pass would write it for the buffer
 * afterwards. rows == nullptr: none. */
struct CacheEntry
{
  uint32_t *rows, *norms, *n;
  uint64_t row_stride, norm_stride; // dwords per buffer
  uint32_t n_stride, pad_rows_to;
};

/* from the entry arguments: the byte stride of the rows in dwords; without desc there is no entry, whatever the other arguments say */
static inline CacheEntry cache_entry(uint8_t *desc, uint64_t desc_stride, uint32_t *norms, uint64_t norm_stride, uint32_t *n_out, uint32_t n_stride, uint32_t pad_rows_to)
{
  return CacheEntry{(uint32_t *)desc, desc ? norms : nullptr, desc ? n_out : nullptr, desc_stride / 4u, norm_stride, n_stride, desc ? pad_rows_to : 0u};
}
/* the entry of buffer bufi (strides no longer apply) */
__device__ __forceinline__ CacheEntry cache_entry_of(CacheEntry c, uint32_t bufi)
{
  if (c.rows)
    c.rows += (size_t)bufi * c.row_stride, c.norms += (size_t)bufi * c.norm_stride, c.n += (size_t)bufi * c.n_stride;
  return c;
}

/* ---- the launch prologue ---------------------------------------------------------------------------------------------------------------
 * What the entries of the family refuse before they launch, once. Always: 1 <= nslots <= max_slots, nsec <= 16, records that move dword by
 * dword, at most 256 posted counters per buffer (one thread each), cache rows that are stored 16 bytes at a time. An entry without one of the
 * arguments passes nullptr / 0. The parts an entry asks for: */
#define ARGS_ONE_COUNTER_SOURCE 1u /* exactly one of fixed_counts / found_base */
#define ARGS_CACHE_OPTIONAL 2u     /* the cache block is looked at only with desc, and then norms and n_out are there too */
static inline bool sectioned_args_ok(uint32_t parts, uint32_t nslots, uint32_t max_slots, uint32_t nsec, const uint8_t *feats_base, uint64_t buf_stride,
                                     const uint32_t *fixed_counts, const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *found_post,
                                     const uint8_t *desc, uint64_t desc_stride, const uint32_t *norms, const uint32_t *n_out)
{
  const bool one_source = !(parts & ARGS_ONE_COUNTER_SOURCE) || (fixed_counts != nullptr) != (found_base != nullptr);
  const bool cache = desc || !(parts & ARGS_CACHE_OPTIONAL), complete = !(parts & ARGS_CACHE_OPTIONAL) || !desc || (norms && n_out);
  return nslots >= 1 && nslots <= max_slots && nsec <= VKSIFT_MAX_SECTIONS && !((uintptr_t)feats_base & 3u) && !(buf_stride & 3u) && one_source &&
         !(found_post && found_buf_stride > 256u) && !(cache && (((uintptr_t)desc & 15u) || (desc_stride & 15u))) && complete;
}

/* The grid of the gather walk (vksift_hip_gather_sections, vksift_hip_root_descriptors): a grid-stride walk over the rows that exist (the count
 * is read on the device), some 4096 workgroups of 32 rows (256 threads, eight lanes per row) per launch whatever the batch — a buffer alone
 * gets up to 256, 512 buffers 8 each (8 rounds over 1900 rows) */
#define GATHER_ROWS_PER_BLOCK 32u
static inline uint32_t gather_walk_blocks(uint32_t max_rows, uint32_t pad_rows_to, uint32_t nslots)
{
  max_rows = max_rows < pad_rows_to ? pad_rows_to : max_rows;
  uint32_t blocks = (max_rows + GATHER_ROWS_PER_BLOCK - 1u) / GATHER_ROWS_PER_BLOCK, cap_blocks = 4096u / nslots;
  cap_blocks = cap_blocks < 8u ? 8u : (cap_blocks > 256u ? 256u : cap_blocks);
  return blocks < 1u ? 1u : (blocks > cap_blocks ? cap_blocks : blocks);
}

/* ---- per buffer ------------------------------------------------------------------------------------------------------------------------
 * The records and the counters of buffer bufi (buf_stride in dwords; found == nullptr: no counters on the device, the table's fixed counts) */
template <class Word, class Count> struct BufferRef
{
  Word *recs;
  Count *found;
};
template <class Word, class Count> __device__ __forceinline__ BufferRef<Word, Count> buffer_ref(Word *feats_base, uint64_t buf_stride, Count *found_base, uint32_t found_buf_stride, uint32_t bufi)
{
  return {feats_base + (size_t)bufi * buf_stride, found_base ? found_base + (size_t)bufi * found_buf_stride : nullptr};
}

/* raw count of section o, and the stored counts of all sections (section_counts) from it */
template <class Count> __device__ __forceinline__ uint32_t raw_count(const SectionTable &tab, Count *found, uint32_t o) { return found ? found[o] : tab.fixed[o]; }
template <class Count> __device__ __forceinline__ uint32_t stored_counts(const SectionTable &tab, Count *found, uint32_t (&cnt)[VKSIFT_MAX_SECTIONS])
{
  return section_counts(tab.nsec, [&](uint32_t o) { return raw_count(tab, found, o); }, tab.cap, cnt);
}

/* ---- the cache row step ----------------------------------------------------------------------------------------------------------------
 * A cache row is the 128 descriptor bytes and their shifted norm, the sum of (byte - 128)^2 = s2 - 256 s1 + 128 * 128^2. Sixteen bytes contribute
 * their own s2 - 256 s1 + 16 * 128^2: modulo 2^32 on the way, exact in the end, whatever the grouping. */
#define VKSIFT_ZERO_ROW_NORM (128u * 128u * 128u) /* of the all-zero rows of quirk Q6 */
__device__ __forceinline__ uint32_t shifted_norm_part(uint4 v)
{
  uint32_t s2 = __builtin_amdgcn_udot4(v.x, v.x, 0u, false), s1 = __builtin_amdgcn_udot4(v.x, 0x01010101u, 0u, false);
  s2 = __builtin_amdgcn_udot4(v.y, v.y, s2, false), s1 = __builtin_amdgcn_udot4(v.y, 0x01010101u, s1, false);
  s2 = __builtin_amdgcn_udot4(v.z, v.z, s2, false), s1 = __builtin_amdgcn_udot4(v.z, 0x01010101u, s1, false);
  s2 = __builtin_amdgcn_udot4(v.w, v.w, s2, false), s1 = __builtin_amdgcn_udot4(v.w, 0x01010101u, s1, false);
  return s2 - 256u * s1 + VKSIFT_ZERO_ROW_NORM / 8u;
}

/* eight lanes per row, lane j of them holds bytes 16 j .. 16 j + 15: called by all eight */
__device__ __forceinline__ void cache_row_store(const CacheEntry &e, uint32_t row, uint32_t j, uint4 v)
{
  *(uint4 *)(e.rows + (size_t)row * 32u + 4u * j) = v;
  const uint32_t norm = lanes_sum_u32<8>(shifted_norm_part(v));
  if (j == 0u)
    e.norms[row] = norm;
}

/* ---- layout decode --------------------------------------------------------------------------------------------------------------------
 * One side of a pair-table slot, resolved into LDS: what section_row needs, the total and the buffer. */
struct SideLayout
{
  uint32_t off[VKSIFT_MAX_SECTIONS], cnt[VKSIFT_MAX_SECTIONS], total, buf;
};

/* Called by every thread of a workgroup of at least 16 * NSIDES threads. slot: the slot's {buffer A, buffer B, layout A, layout B}; L[s]
 * becomes side first_side + s, its stored counts min(found, cap) read on the device (sixteen lanes per side, one section each; the table
 * may live in mapped host memory and is read once). Complete when this returns. */
template <uint32_t NSIDES>
__device__ __forceinline__ void layout_decode(SideLayout (&L)[NSIDES], const uint32_t *__restrict__ slot, uint32_t first_side, const uint32_t *__restrict__ layouts,
                                              const uint32_t *__restrict__ found_base, uint32_t found_buf_stride)
{
  const uint32_t tid = threadIdx.x;
  if (tid < VKSIFT_MAX_SECTIONS * NSIDES)
  {
    const uint32_t s = tid / VKSIFT_MAX_SECTIONS, o = tid % VKSIFT_MAX_SECTIONS;
    const uint32_t bufi = slot[first_side + s], lay = slot[2u + first_side + s];
    uint32_t off = 0, cnt = 0;
    if (lay & VKSIFT_LAYOUT_DENSE)
      cnt = o == 0u ? (lay & ~VKSIFT_LAYOUT_DENSE) : 0u;
    else
    {
      const uint32_t *t = layouts + (size_t)lay * VKSIFT_LAYOUT_WORDS;
      if (o < t[0] && o < found_buf_stride)
      {
        off = t[VKSIFT_LAYOUT_OFF_AT + o];
        cnt = section_stored(found_base[(size_t)bufi * found_buf_stride + o], t[VKSIFT_LAYOUT_CAP_AT + o]);
      }
    }
    L[s].off[o] = off, L[s].cnt[o] = cnt;
    if (o == 0u)
      L[s].buf = bufi;
  }
  __syncthreads();
  if (tid < NSIDES)
  {
    uint32_t t = 0;
    for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
      t += L[tid].cnt[o];
    L[tid].total = t;
  }
  __syncthreads();
}

/* ---- ordered keep ---------------------------------------------------------------------------------------------------------------------
 * One round of a 1024-thread workgroup that appends the items its threads keep in thread order, without atomics: ballot and rank inside
 * the wave, the sixteen wave totals through LDS, the rounds so far in carry_s (zeroed, and a barrier passed, before the first round).
 * Called by every thread; returns where in the output a thread that keeps its item writes it. */
__device__ __forceinline__ uint32_t ordered_keep(bool keep, uint32_t (&wave_tot)[16], uint32_t &carry_s)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  const uint32_t rank = ballot_rank(bal, lane);
  if (lane == 0)
    wave_tot[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t wave_base = 0, total = 0;
  for (int wv = 0; wv < 16; wv++)
  {
    if (wv < wave)
      wave_base += wave_tot[wv];
    total += wave_tot[wv];
  }
  const uint32_t carry = carry_s;
  __syncthreads();
  if (threadIdx.x == 0)
    carry_s = carry + total;
  __syncthreads();
  return carry + wave_base + rank;
}

/* ---- select and compact in place ---------------------------------------------------------------------------------------------------------
 * What the launches that keep some rows of a buffer where they are share (strongest.hip, spread.hip; one 1024-thread workgroup per buffer): the
 * bin of a 256-bin radix pass, and the ordered compaction with everything that follows it. */

/* Called by the 64 lanes of the first wave after a 256-bin histogram pass: sel_s = {the bin that holds the want-th largest key, how many keys of
 * that bin are still wanted}. Lane l owns bins 255 - 4l .. 252 - 4l: an inclusive scan over the lanes counts the keys from the top bin down. The
 * histogram holds at least `want` keys, want >= 1. */
__device__ __forceinline__ void radix_pick_256(const uint32_t (&hist)[256], uint32_t want, uint32_t (&sel_s)[2])
{
  const uint32_t tid = threadIdx.x;
  uint32_t h[4], sum = 0;
  for (uint32_t i = 0; i < 4u; i++)
    h[i] = hist[255u - 4u * tid - i], sum += h[i];
  const uint32_t incl = wave_scan_incl_u32(sum, (int)tid);
  uint32_t above = incl - sum;
  if (above < want && want <= incl) // one lane
  {
    uint32_t bin = 255u - 4u * tid;
    for (uint32_t i = 0; i < 3u && want > above + h[i]; i++)
      above += h[i], bin--;
    sel_s[0] = bin, sel_s[1] = want - above;
  }
}

/* the section of download-order row `row` < total (section_row's walk) */
template <class Cnt> __device__ __forceinline__ uint32_t section_of(const Cnt &cnt, uint32_t row)
{
  uint32_t first = 0, sec = 0;
  VKSIFT_UNROLL
  for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
  {
    if (row >= first && row < first + cnt[o])
      sec = o;
    first += cnt[o];
  }
  return sec;
}

/* One round of 1024 download-order rows of the ordered compaction, rounds in order; called by every thread. keep: the thread's row — stored row
 * src_row, of section sec — is kept. A kept row's place is its section's start plus the kept rows of that section in front of it. Every kept
 * record of the round is loaded into registers, a barrier is passed, then it is stored: a destination never lies beyond its source (the kept rows
 * in front of a row are at most the rows in front of it) and never beyond the round (it is the old place of a row at or in front of the source),
 * so a store can only land on a record of an earlier round, already consumed, or of this round, already in registers. With an entry the kept
 * row is written to the matcher's cache from the same registers. kept_s (the kept rows per section) and keep_carry are zero, and a barrier
 * passed, before the first round; max_rows: the entry's rows (the launch keeps no more). */
__device__ __forceinline__ void compact_round(uint32_t *feats, bool keep, uint32_t sec, uint32_t src_row, const uint32_t (&off_s)[VKSIFT_MAX_SECTIONS],
                                              uint32_t (&kept_s)[VKSIFT_MAX_SECTIONS], uint32_t (&wave_tot)[16], uint32_t &keep_carry, const CacheEntry &entry,
                                              uint32_t max_rows)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t out_row = ordered_keep(keep, wave_tot, keep_carry); // its download-order row afterwards
  // kept rows of every section, this round's included: those of the sections in front of a row's own are complete when it is placed
  VKSIFT_UNROLL
  for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
  {
    const unsigned long long bal = __ballot(keep && sec == o);
    if (lane == 0u && bal)
      atomicAdd(&kept_s[o], (uint32_t)__popcll(bal)); // LDS
  }
  __syncthreads();
  uint32_t rec[VKSIFT_RECORD_WORDS], dst_row = 0;
  if (keep)
  {
    uint32_t in_front = 0;
    VKSIFT_UNROLL
    for (uint32_t o = 0; o < VKSIFT_MAX_SECTIONS; o++)
      in_front += o < sec ? kept_s[o] : 0u;
    dst_row = off_s[sec] + (out_row - in_front);
    const uint32_t *src = feats + (size_t)src_row * VKSIFT_RECORD_WORDS;
    VKSIFT_UNROLL
    for (uint32_t w = 0; w < VKSIFT_RECORD_WORDS; w++)
      rec[w] = src[w];
  }
  __builtin_amdgcn_s_waitcnt(0); // every record of the round is in registers ...
  __syncthreads();               // ... in every wave, before any is overwritten
  if (keep)
  {
    if (dst_row != src_row)
    {
      uint32_t *dst = feats + (size_t)dst_row * VKSIFT_RECORD_WORDS;
      VKSIFT_UNROLL
      for (uint32_t w = 0; w < VKSIFT_RECORD_WORDS; w++)
        dst[w] = rec[w];
    }
    if (entry.rows && out_row < max_rows) // (always: max_rows rows are kept; the entry holds no more)
    {
      // the bytes k_gather_sections writes for the selected buffer: one thread stores the eight pieces of the row and sums their norm parts
      uint32_t norm = 0;
      VKSIFT_UNROLL
      for (uint32_t q = 0; q < 8u; q++)
      {
        const uint32_t *d = rec + VKSIFT_RECORD_HEAD_WORDS + 4u * q;
        const uint4 v = uint4{d[0], d[1], d[2], d[3]};
        *(uint4 *)(entry.rows + (size_t)out_row * 32u + 4u * q) = v;
        norm += shifted_norm_part(v);
      }
      entry.norms[out_row] = norm;
    }
  }
}

/* After the last round, called by every thread: the counters become the kept counts, on the device and posted to the host mirror by this launch
 * (mapped pinned memory; no dependent copy), and the cache entry gets its row count (rows_kept) and the all-zero rows of quirk Q6 from there up
 * to pad_rows_to. */
__device__ __forceinline__ void compact_finish(uint32_t nsec, uint32_t *found, uint32_t *found_post, uint32_t bufi, uint32_t found_buf_stride,
                                               const uint32_t (&kept_s)[VKSIFT_MAX_SECTIONS], const CacheEntry &entry, uint32_t pad_rows_to, uint32_t rows_kept)
{
  const uint32_t tid = threadIdx.x;
  if (tid < nsec)
  {
    if (found)
      found[tid] = kept_s[tid];
    if (found_post)
      found_post[(size_t)bufi * found_buf_stride + tid] = kept_s[tid];
  }
  if (entry.rows)
  {
    if (tid == 0)
      *entry.n = rows_kept;
    for (uint32_t i = rows_kept * 32u + tid; i < pad_rows_to * 32u && rows_kept < pad_rows_to; i += 1024u)
    {
      entry.rows[i] = 0u;
      if ((i & 31u) == 0u)
        entry.norms[i >> 5] = VKSIFT_ZERO_ROW_NORM;
    }
  }
}

#endif /* __HIPCC__ */
#endif /* __cplusplus */
#endif
