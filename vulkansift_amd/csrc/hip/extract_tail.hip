// extract_tail.hip — the tail of the keypoint extraction of a BATCH as one launch (gfx950).
//
// Behind the streaming scan (extrema.hip: k_extrema_lean leaves one u64 candidate ballot per 64-pixel row segment) the four-launch tail turns
// the ballots into records through HBM: segment offsets, a candidate list, accept flags and two levels of chunk totals are written and read
// back, the ballots are read twice, and every accepted candidate is refined twice because its first refinement ran before its rank was known.
// With one WORKGROUP per (image, octave) none of that is needed:
//   * the workgroup walks its image's ballots in segment order — (scale * h + y) * nseg + segx, the order k_cand_list produces — a tile at a time:
//     popcount, workgroup exclusive scan, expansion of the set bits into a candidate list in LDS (x | y << 14 | scale << 28, as k_cand_list packs)
//   * whenever the list holds a full round (one candidate per thread) the round is refined: refine_candidate() ONCE per candidate, a ballot and
//     the waves' accept counts in LDS give every accepted candidate its rank, and the thread that holds the record stores it at base + rank
//   * base, the candidate count and the list's fill level are workgroup-uniform registers; what is left of the list after the last tile is the
//     last (partial) round
// Candidates wait in the list across tiles, so rounds are full whatever the density of a tile, and a tile with more candidates than the list has
// room for (up to 64 per segment) is expanded in several windows with the rounds in between. Same results as the four launches, bit for bit:
// raster order, candidates at list positions >= cand_cap dropped, cand_n and found un-clamped, records only for ranks < cap.
// seg_off, cand_xy and cand_flag are not touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "extrema_refine.h"
#include "multi.h"
#include "records.h"
#include "vksift_hip.h"
#include "wave.h"

namespace
{

constexpr uint32_t TAIL_SPT = 2;     // segments per thread and tile: a tile is 2 * blockDim.x segments (1024 or 2048)
constexpr uint32_t TAIL_LIST = 4096; // candidates the LDS list holds: a multiple of both workgroup sizes, so a full list is whole rounds

// 6 waves per SIMD (80 VGPRs): a CU then holds three 512-thread workgroups instead of two, and the refinement, a chain of dependent loads, is
// bound by the waves in flight — 512 frames: 432 -> 380 us. (The tile's ballots are loaded where they are used: keeping the next tile's in
// registers across the rounds cost the registers this needs and gained nothing, 432 against 431 us.)
template <bool F16, bool BUF>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(6, 8))) k_extract_tail(Multi<ExtremaArgs> m)
{
  __shared__ uint32_t s_list[TAIL_LIST];
  __shared__ uint32_t s_wtot[2][16]; // candidates of a tile per wave (double-buffered over tiles: one barrier per tile)
  __shared__ uint32_t s_cnt[2][16];  // accepted candidates of a round per wave (double-buffered over rounds: one barrier per round)
  const VBlock vb = vblock(m); // virtual grid (images)
  const ExtremaArgs &a = m.oct[vb.o];
  const int b = (int)vb.x;
  const uint32_t tid = threadIdx.x, NT = blockDim.x, nw = NT >> 6, lane = tid & 63u, wave = tid >> 6;
  constexpr unsigned EB = F16 ? 2u : 4u;
  const DogView d{(const float *)((const uint8_t *)a.gauss + (size_t)b * a.img_stride * EB), a.w, a.h, a.pitch, (size_t)a.plane_stride, a.S};
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)d.base, 0, (int)((unsigned)(a.S + 3) * (unsigned)a.plane_stride * EB), 0x00020000);
  const RefineCtx c{a, 0u, 0u, d, rsrc, nullptr, nullptr, nullptr}; // no list in HBM: the candidates come from s_list
  const uint64_t *__restrict__ mask = a.seg_mask + (size_t)b * a.seg_img_stride;
  uint8_t *const feats = a.feats + (size_t)b * a.feat_img_stride;
  const uint32_t nsegs = a.nsegs, tile = NT * TAIL_SPT;

  uint32_t base = 0;   // accepted candidates so far = rank of the next round's first accepted one
  uint32_t ncand = 0;  // candidates so far (un-clamped)
  uint32_t fill = 0;   // candidates waiting in s_list[0 .. fill)
  uint32_t rpar = 0;   // s_cnt buffer of the next round

  // one round: thread t refines s_list[c0 + t], t < cnt <= NT; every wave reaches the barrier
  auto round = [&](uint32_t c0, uint32_t cnt) {
    KpRecord kp;
    bool ok = false;
    if (tid < cnt)
      ok = refine_candidate<F16, BUF>(c, s_list[c0 + tid], &kp);
    const unsigned long long bal = __ballot(ok);
    if (lane == 0)
      s_cnt[rpar][wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t rank = ballot_rank(bal, (int)lane), total = 0;
    for (uint32_t wv = 0; wv < nw; wv++)
    {
      const uint32_t n = s_cnt[rpar][wv];
      rank += wv < wave ? n : 0u;
      total += n;
    }
    const uint32_t idx = base + rank;
    if (ok && idx < a.cap)
      store_record((uint32_t *)(feats + (size_t)idx * VKSIFT_RECORD_BYTES), kp);
    base += total;
    rpar ^= 1u;
  };

  auto load_tile = [&](uint32_t t0, unsigned long long(&mk)[TAIL_SPT]) {
    const uint32_t i0 = t0 + TAIL_SPT * tid;
#pragma unroll
    for (uint32_t k = 0; k < TAIL_SPT; k++)
      mk[k] = i0 + k < nsegs ? mask[i0 + k] : 0ull;
  };

  unsigned long long cur[TAIL_SPT];
  uint32_t tpar = 0;
  for (uint32_t t0 = 0; t0 < nsegs; t0 += tile, tpar ^= 1u)
  {
    load_tile(t0, cur);
    // exclusive scan of the candidates per thread over the workgroup
    uint32_t tsum = 0;
#pragma unroll
    for (uint32_t k = 0; k < TAIL_SPT; k++)
      tsum += (uint32_t)__popcll(cur[k]);
    const uint32_t incl = wave_scan_incl_u32(tsum, (int)lane);
    if (lane == 63u)
      s_wtot[tpar][wave] = incl;
    __syncthreads();
    uint32_t off = incl - tsum, T = 0; // this thread's first candidate inside the tile, candidates of the tile
    for (uint32_t wv = 0; wv < nw; wv++)
    {
      const uint32_t n = s_wtot[tpar][wv];
      off += wv < wave ? n : 0u;
      T += n;
    }
    // the list of an image ends at cand_cap: what lies beyond it is counted and dropped
    const uint32_t valid = ncand >= a.cand_cap ? 0u : (T < a.cand_cap - ncand ? T : a.cand_cap - ncand);
    ncand += T;
    for (uint32_t w0 = 0; w0 < valid;)
    {
      // window [w0, hi) of the tile's candidates goes to s_list[fill ..): all that is left of them, or as many as the list has room for
      const uint32_t room = TAIL_LIST - fill, hi = valid - w0 < room ? valid : w0 + room;
      if (off < hi && off + tsum > w0)
      {
        uint32_t pos = off;
#pragma unroll
        for (uint32_t k = 0; k < TAIL_SPT; k++)
        {
          unsigned long long mk = cur[k];
          if (mk == 0ull)
            continue;
          const uint32_t seg = t0 + TAIL_SPT * tid + k;
          const uint32_t row = seg / (uint32_t)a.nseg, segx = seg - row * (uint32_t)a.nseg;
          const uint32_t sz = row / (uint32_t)a.h, yy = row - sz * (uint32_t)a.h;
          const uint32_t head = (segx * 64u) | (yy << 14) | ((sz + 1u) << 28);
          while (mk)
          {
            const uint32_t bit = (uint32_t)__ffsll((long long)mk) - 1u;
            mk &= mk - 1ull;
            if (pos >= w0 && pos < hi)
              s_list[fill + (pos - w0)] = head + bit;
            pos++;
          }
        }
      }
      fill += hi - w0;
      w0 = hi;
      __syncthreads();
      // the full rounds of the list (a window that was cut leaves the list full: whole rounds, nothing left over)
      const uint32_t nfull = fill - fill % NT, left = fill - nfull;
      for (uint32_t c0 = 0; c0 < nfull; c0 += NT)
        round(c0, NT);
      if (nfull != 0u && left != 0u)
      {
        // what is left moves to the front (left < NT <= nfull: source and destination do not overlap; every thread has read its entry of
        // the rounds before it passed their barriers)
        if (tid < left)
          s_list[tid] = s_list[nfull + tid];
        __syncthreads();
      }
      fill = left;
    }
  }
  if (fill != 0u)
    round(0u, fill);
  if (tid == 0u)
  {
    a.cand_n[b] = ncand;
    a.found[(size_t)b * a.found_img_stride] = base; // un-clamped, like nb_elem; 0 for an image without candidates
  }
}

} // namespace

int extract_tail_launch(const ExtremaArgs *args, uint32_t n, uint32_t batch, bool f16, bool buf, bool small_wg, hipStream_t hs)
{
  Multi<ExtremaArgs> mt;
  mt.n = 0;
  for (uint32_t i = 0; i < n; i++)
    if (!multi_add(mt, args[i], batch, 1u, 1u))
      return (int)hipErrorInvalidValue;
  /* 1024 threads while the launch has fewer than 512 workgroups (under two per CU: threads are what fills the chip); from there on 512, so
   * that a CU holds more images at once and the long ones (an image's candidate count decides its workgroup's time) overlap the short */
  const dim3 grid(mt.start[mt.n]), block(mt.start[mt.n] < 512u && !small_wg ? 1024u : 512u);
  with_bool(f16, [&](auto F16) {
    with_bool(buf, [&](auto BUF) { hipLaunchKernelGGL((k_extract_tail<decltype(F16)::value, decltype(BUF)::value>), grid, block, 0, hs, mt); });
  });
  return (int)hipGetLastError();
}
