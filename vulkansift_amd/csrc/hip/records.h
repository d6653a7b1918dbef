/* records.h — the steps every launch that moves or addresses SIFT records shares (hip/records.hip, hip/verify.hip, hip/guided.hip), each
 * defined once: the record and section-table constants, the walk from a download-order row to a stored row, the decode of a pair table's
 * layout word, the by-value launch arguments, and the ordered append of a 1024-thread workgroup. The constants compile as C (host/vksift_internal.h takes them from
 * here), the walk as host C++ too: plain integer arithmetic, checked row by row by tests/test_section_walk.py, which compiles this header
 * with the host compiler. The rest is device code. */
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

/* The matcher's cache block as the launches that rewrite records in place take it (vksift_hip_keep_strongest, vksift_hip_root_descriptors): they
 * leave the entry of a buffer as vksift_hip_gather_sections would write it for the buffer afterwards. rows == nullptr: none. */
struct CacheEntry
{
  uint32_t *rows, *norms, *n;
  uint64_t row_stride, norm_stride; // dwords per buffer
  uint32_t n_stride, pad_rows_to;
};

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

#endif /* __HIPCC__ */
#endif /* __cplusplus */
#endif
