// extrema.hip — DoG extrema detection, sub-pixel refinement and deterministic compaction (gfx950).
//
// The DoG planes of the reference (DifferenceOfGaussian.comp: D[z] = G[z+1] - G[z]) are not stored by this build: every
// DoG value below is formed where it is consumed as ONE fp32 subtraction of two stored Gaussian texels, which is the
// shader's own expression — bit-identical, and 20 B per octave pixel of HBM writes + 20 B of reads become 24 B of reads.
//
// Replaces ExtractKeypoints.comp (dispatch: sift_detector.c:1106-1189). The reference appends
// keypoints with a global atomicAdd (ExtractKeypoints.comp:208), which makes their order
// non-deterministic. Here the append is an atomic-free pipeline whose output order is raster (scale, y, x):
//   k_extrema_lean   : streaming 26-neighbour test; one u64 candidate ballot per 64-pixel row segment
//   k_segment_scan   : exclusive prefix sum of popcount(mask) over segments in (scale, y, x) order
//   k_cand_list      : one thread per segment writes its candidates' packed (x, y, s) at offset + rank
//   k_refine_flags   : one thread per CANDIDATE (dense waves: no lane idles while a neighbour refines) -> accept flag
//   k_cand_emit      : second level of the scan of the accept counts, accepted candidates recompute their record and store it
//                      at their rank (clamped to the section capacity); the un-clamped count goes to found[]
// The refinement is a LOADER, which fetches the 19 DoG values around a position (PtrLoader: 64-bit pointers, any octave size;
// BufLoader: one buffer resource per image's octave), and refine_core(), everything else, written once. The arithmetic of
// refine_core() is kept operation-for-operation identical to oracle/sift_oracle.c:extract_one (fp32, no contraction) so
// results are bit-exact.
// Both live in extrema_refine.h, which extract_tail.hip shares: batches of 64 images and more take everything behind k_extrema_lean as ONE launch
// there (k_extract_tail, one workgroup per image and octave), with the same results bit for bit; extract_run() chooses.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <vector>
#include <stdint.h>
#include <stdlib.h>

#include "../detmath.h"
#include "extrema_refine.h"
#include "multi.h"
#include "records.h"
#include "vksift_hip.h"
#include "wave.h"

namespace
{

// Streaming detection pass: one wave owns a 64-column segment and marches down a band of
// rows. For every DoG layer it keeps, for the last three rows, the horizontal 3-max / 3-min of its column
// (neighbours come from lane shuffles, the two halo columns from one extra 2-lane load), so the 26-neighbour test of
// a texel of scale s is  c > max over {layers s-1,s,s+1} x {rows y-1,y,y+1} of the 3-max  with the centre's own
// entry replaced by max(left, right) — identical to 26 strict comparisons for finite values. Each DoG plane is read
// exactly once (20 B per octave pixel at S = 3, coalesced) instead of 27 scattered loads per candidate. The
// per-segment candidate ballots feed k_segment_scan / k_cand_list; refinement happens later on dense waves.
// lane i <- lane i-1 (lane 0 keeps `edge`), lane i <- lane i+1 (lane 63 keeps `edge`): gfx9 DPP wave shifts, one VALU op
__device__ __forceinline__ float wave_shr1(float v, float edge)
{
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v, float edge)
{
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

// v_max_f32 / v_min_f32 / v_max3_f32 / v_min3_f32 on values known to be finite. fmaxf()/fminf() in IEEE mode first
// canonicalise both operands (one extra v_max_f32 x, x each) to quieten signalling NaNs; DoG planes never hold NaNs.
__device__ __forceinline__ float fmax2(float a, float b)
{
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float fmin2(float a, float b)
{
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float fmax3(float a, float b, float c)
{
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float fmin3(float a, float b, float c)
{
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// spread the low 32 bits of x to the even bit positions of a 64-bit word
__device__ __forceinline__ unsigned long long spread32(unsigned long long x)
{
  x &= 0xFFFFFFFFull;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// ---------------------------------------------------------------------------------------------
// k_extrema_lean — the streaming 26-neighbour test, built around what bounds it. The pass is a pure stream (20 B per octave pixel
// at S = 3, no reuse beyond a 3-row window), so its speed is the number of bytes a CU keeps in flight:
//   * the window holds the RAW texels (3 rows x (2 columns + 1 halo) per layer — they serve max and min alike); the
//     vertical 3-max / 3-min of a column is formed first, its left / right neighbours then come from ONE lane shift per
//     side, layer and sign. 60-75 registers of state: 4 waves per SIMD with two rows of loads in flight each.
//   * raw buffer loads straight into the window slots: lane-constant byte offset (out-of-range for lanes that must not
//     load: the hardware returns 0), the row offset is one SGPR, one resource per layer — no VALU address arithmetic,
//     no branches. The row loop is unrolled over the NSLOT window slots, so the window rotates by renaming.
//   * rows are clamped and columns are not masked: values outside the image only ever reach the test of non-interior
//     texels, which the (lane-constant) column masks and the scalar row range remove
//   * the comparisons are ballots combined on the scalar unit; the (rare) store of a non-empty ballot interleaves the
//     two column masks with two more ballots instead of 100 scalar bit operations
// 26 strict comparisons == centre above the max / below the min of: the own layer's 8 neighbours
// (max3(left column's vertical max, right column's vertical max, max(up, down))) and the full 3x3 of both adjacent layers.
// ---------------------------------------------------------------------------------------------
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
constexpr unsigned EXT_OOB = 0x80000000u;

template <int S, int NSLOT, bool F16>
__global__ void __launch_bounds__(256, 4) k_extrema_lean(Multi<ExtremaArgs> m, int strip_major)
{
  const VBlock vb = vblock(m);
  const ExtremaArgs &a = m.oct[vb.o];
  const int band = a.band;
  constexpr int NL = S + 2;
  constexpr int EB = F16 ? 2 : 4; // bytes per texel
  constexpr int AHEAD = NSLOT - 3; // rows of loads in flight behind the 3-row window
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // 4 independent waves per block, one row band each
  int b = vb.z;
  int bx = vb.x, by = vb.y * 4 + wv;
  if (strip_major)
  {
    // the 4 waves of a block take 4 adjacent strips of one band (strips fastest over the flattened wave index)
    unsigned blk = vb.y * vb.gx + vb.x;
    if (strip_major & 2)
    {
      // XCD-contiguous order (workgroup n runs on XCD n % 8, each with its own L2): every XCD takes a contiguous range of the
      // (image, band, strip) space, so the bands that share halo rows are read through the same L2
      const unsigned per_img = vb.gx * vb.gy, total = per_img * vb.gz;
      if ((total & 7u) == 0)
      {
        const unsigned n = blk + per_img * vb.z, per = total >> 3, k = n >> 3;
        const unsigned wi = (n & 7u) * per + (a.scan_rev ? per - 1u - k : k);
        b = (int)(wi / per_img);
        blk = wi - (unsigned)b * per_img;
      }
    }
    const unsigned id = blk * 4u + (unsigned)wv, ns = (unsigned)(a.nseg + 1) / 2u;
    by = (int)(id / ns), bx = (int)(id - (unsigned)by * ns);
  }
  const int y0 = by * band;
  if (y0 >= a.h)
    return;
  const int y1 = min(y0 + band, a.h);
  const int x0 = bx * 128, x = x0 + 2 * lane;
  const uint8_t *img = (const uint8_t *)a.gauss + (size_t)b * a.img_stride * EB;
  const int pitch4 = a.pitch * EB; // row pitch in bytes
  __amdgpu_buffer_rsrc_t rs[NL + 1]; // one resource per GAUSSIAN layer
#pragma unroll
  for (int l = 0; l <= NL; l++)
    rs[l] = __builtin_amdgcn_make_buffer_rsrc((void *)(img + (size_t)l * a.plane_stride * EB), 0, a.pitch * a.h * EB, 0x00020000);
  // x is even: the pair (x, x+1) starts inside the row or is left out. With an odd pitch (fp32 only) the pair at x = pitch - 1 takes its second
  // texel from the next row (zero behind the last one): columns at and beyond w only ever reach the tests of columns >= w - 1, which colA / colB
  // remove. A binary16 pair is one dword: make_extrema_args admits even pitches and strides on a 4-byte-aligned base only
  const unsigned off2 = x < a.pitch ? (unsigned)x * (unsigned)EB : EXT_OOB;
  const int hx = lane == 0 ? x0 - 1 : x0 + 128;
  const unsigned offh = ((lane == 0 || lane == 63) && hx >= 0 && hx < a.pitch) ? (unsigned)hx * (unsigned)EB : EXT_OOB;
  const unsigned long long colA = __ballot(x >= 1 && x < a.w - 1), colB = __ballot(x + 1 < a.w - 1);
  const float pre = a.dog_threshold * 0.8f;
  const int seg0 = bx * 2;
  const bool has_seg1 = seg0 + 1 < a.nseg;
  const int ylo = max(y0, 1), yhi = min(y1, a.h - 1); // rows tested by this wave
  const bool odd = lane & 1;
  const unsigned half = (unsigned)lane >> 1;

  // a slot receives the NL+1 Gaussian texels of a row; when the row becomes the newest row of the window they are turned
  // into the NL DoG texels in place (entry NL is dead from then on)
  u32x2_t wv2[NSLOT][NL + 1]; // columns x, x+1
  unsigned wh[NSLOT][NL + 1]; // halo column (lanes 0 and 63)
  auto fetch_row = [&](int r, auto SLOT) {
    constexpr int slot = decltype(SLOT)::value;
    const int rr = min(max(r, 0), a.h - 1);
    const int so = rr * pitch4;
#pragma unroll
    for (int l = 0; l <= NL; l++)
    {
      if (F16)
      {
        // two binary16 texels in one dword, the halo texel in the low half of another: half the registers of the fp32 form in flight
        wv2[slot][l].x = __builtin_amdgcn_raw_buffer_load_b32(rs[l], off2, so, 0);
        wh[slot][l] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs[l], offh, so, 0);
      }
      else
      {
        wv2[slot][l] = __builtin_amdgcn_raw_buffer_load_b64(rs[l], off2, so, 0);
        wh[slot][l] = __builtin_amdgcn_raw_buffer_load_b32(rs[l], offh, so, 0);
      }
    }
  };
  typedef _Float16 h2x __attribute__((ext_vector_type(2)));
  auto to_dog = [&](auto SLOT) {
    constexpr int slot = decltype(SLOT)::value;
    if (F16)
    {
      float lo0, lo1, loh;
      {
        const h2x t = __builtin_bit_cast(h2x, wv2[slot][0].x);
        lo0 = (float)t.x, lo1 = (float)t.y;
        loh = (float)__builtin_bit_cast(h2x, wh[slot][0]).x;
      }
#pragma unroll
      for (int l = 0; l < NL; l++)
      {
        const h2x t = __builtin_bit_cast(h2x, wv2[slot][l + 1].x);
        const float hi0 = (float)t.x, hi1 = (float)t.y, hih = (float)__builtin_bit_cast(h2x, wh[slot][l + 1]).x;
        // the DoG image of a binary16 pyramid is a binary16 image: round the difference, keep it widened
        wv2[slot][l].x = __float_as_uint((float)(_Float16)(hi0 - lo0));
        wv2[slot][l].y = __float_as_uint((float)(_Float16)(hi1 - lo1));
        wh[slot][l] = __float_as_uint((float)(_Float16)(hih - loh));
        lo0 = hi0, lo1 = hi1, loh = hih;
      }
      return;
    }
#pragma unroll
    for (int l = 0; l < NL; l++)
    {
      wv2[slot][l].x = __float_as_uint(__uint_as_float(wv2[slot][l + 1].x) - __uint_as_float(wv2[slot][l].x));
      wv2[slot][l].y = __float_as_uint(__uint_as_float(wv2[slot][l + 1].y) - __uint_as_float(wv2[slot][l].y));
      wh[slot][l] = __float_as_uint(__uint_as_float(wh[slot][l + 1]) - __uint_as_float(wh[slot][l]));
    }
  };

  // Row r has just become the newest row of the window (slot P); the centre row is y = r - 1. Slot (P + 1 + AHEAD - 1) ...
  // receives row r + AHEAD: it held row r - 3, which no later test reads.
  auto phase = [&](auto PC, int r) {
    constexpr int P = decltype(PC)::value;
    constexpr int sn = P, sm = (P + NSLOT - 1) % NSLOT, so_ = (P + NSLOT - 2) % NSLOT, sf = (P + AHEAD) % NSLOT;
    if (r + AHEAD <= y1)
      fetch_row(r + AHEAD, std::integral_constant<int, sf>{});
    to_dog(std::integral_constant<int, sn>{}); // row r: Gaussian texels -> DoG texels (every row passes here exactly once)
    const int y = r - 1;
    if (y < ylo || y >= yhi)
      return;
    float ownxA[S], ownnA[S], ownxB[S], ownnB[S], fullxA[NL], fullnA[NL], fullxB[NL], fullnB[NL];
#pragma unroll
    for (int l = 0; l < NL; l++)
    {
      const float ao = __uint_as_float(wv2[so_][l].x), am = __uint_as_float(wv2[sm][l].x), an = __uint_as_float(wv2[sn][l].x);
      const float bo = __uint_as_float(wv2[so_][l].y), bm = __uint_as_float(wv2[sm][l].y), bn = __uint_as_float(wv2[sn][l].y);
      const float ho = __uint_as_float(wh[so_][l]), hm = __uint_as_float(wh[sm][l]), hn = __uint_as_float(wh[sn][l]);
      const float vxa = fmax3(ao, am, an), vna = fmin3(ao, am, an);
      const float vxb = fmax3(bo, bm, bn), vnb = fmin3(bo, bm, bn);
      const float vxh = fmax3(ho, hm, hn), vnh = fmin3(ho, hm, hn);
      const float Lx = wave_shr1(vxb, vxh), Ln = wave_shr1(vnb, vnh); // column x-1 = previous lane's column x+1
      const float Rx = wave_shl1(vxa, vxh), Rn = wave_shl1(vna, vnh); // column x+2 = next lane's column x
      if (l >= 1 && l <= S)
      {
        ownxA[l - 1] = fmax3(Lx, vxb, fmax2(ao, an)), ownnA[l - 1] = fmin3(Ln, vnb, fmin2(ao, an));
        ownxB[l - 1] = fmax3(vxa, Rx, fmax2(bo, bn)), ownnB[l - 1] = fmin3(vna, Rn, fmin2(bo, bn));
      }
      fullxA[l] = fmax3(Lx, vxa, vxb), fullnA[l] = fmin3(Ln, vna, vnb);
      fullxB[l] = fmax3(vxa, vxb, Rx), fullnB[l] = fmin3(vna, vnb, Rn);
    }
#pragma unroll
    for (int sz = 0; sz < S; sz++)
    {
      const int l = sz + 1;
      const float ca = __uint_as_float(wv2[sm][l].x), cb = __uint_as_float(wv2[sm][l].y);
      const float nxa = fmax3(ownxA[sz], fullxA[l - 1], fullxA[l + 1]), nna = fmin3(ownnA[sz], fullnA[l - 1], fullnA[l + 1]);
      const float nxb = fmax3(ownxB[sz], fullxB[l - 1], fullxB[l + 1]), nnb = fmin3(ownnB[sz], fullnB[l - 1], fullnB[l + 1]);
      const unsigned long long ma = (__ballot(ca > nxa) | __ballot(ca < nna)) & __ballot(fabsf(ca) > pre) & colA;
      const unsigned long long mb = (__ballot(cb > nxb) | __ballot(cb < nnb)) & __ballot(fabsf(cb) > pre) & colB;
      if ((ma | mb) != 0ull) // the mask array was zeroed by a memset: only non-empty ballots are written
      {
        // pixel 2i of the wave comes from ma bit i, pixel 2i+1 from mb bit i: lane j of a segment looks up its own bit
        const unsigned lo = odd ? (unsigned)mb : (unsigned)ma, hi = odd ? (unsigned)(mb >> 32) : (unsigned)(ma >> 32);
        const unsigned long long m0 = __ballot((lo >> half) & 1u), m1 = __ballot((hi >> half) & 1u);
        if (lane == 0)
        {
          const size_t base = ((size_t)sz * a.h + y) * a.nseg + (size_t)b * a.seg_img_stride;
          a.seg_mask[base + seg0] = m0;
          if (has_seg1)
            a.seg_mask[base + seg0 + 1] = m1;
        }
      }
    }
  };

  // rows y0-1 .. y0-2+AHEAD are in flight before the loop; phase k handles row r = y0 - 1 + k
  if (AHEAD >= 1)
    fetch_row(y0 - 1, std::integral_constant<int, 0>{});
  if (AHEAD >= 2)
    fetch_row(y0, std::integral_constant<int, 1 % NSLOT>{});
  int r = y0 - 1;
  for (;;)
  {
    phase(std::integral_constant<int, 0>{}, r);
    if (++r > y1)
      break;
    phase(std::integral_constant<int, 1>{}, r);
    if (++r > y1)
      break;
    phase(std::integral_constant<int, 2>{}, r);
    if (++r > y1)
      break;
    phase(std::integral_constant<int, 3>{}, r);
    if (++r > y1)
      break;
    if (NSLOT > 4)
    {
      phase(std::integral_constant<int, 4 % NSLOT>{}, r);
      if (++r > y1)
        break;
    }
  }
}

// Exclusive scan of popcount(mask) over the n segments of an image, in two parallel levels (a single workgroup per image
// made this the longest kernel of a 1080p detection): every 1024-thread workgroup scans one chunk of SEG_CHUNK segments
// locally and publishes the chunk total; the consumer (k_cand_list) adds up the totals in front of its chunk (in place)
// and adds base + local offset.
constexpr uint32_t SEG_CHUNK = 4096;

__global__ void __launch_bounds__(1024) k_segment_scan(Multi<ExtremaArgs> m)
{
  __shared__ uint32_t wave_tot[16];
  const VBlock vb = vblock(m); // virtual grid (chunks, images)
  const ExtremaArgs &a = m.oct[vb.o];
  const int b = (int)vb.y;
  const uint64_t *__restrict__ mask = a.seg_mask + (size_t)b * a.seg_img_stride;
  uint32_t *__restrict__ off = a.seg_off + (size_t)b * a.seg_img_stride;
  uint32_t *__restrict__ chunk_tot = a.cand_flag; // the chunk totals / bases live at the start of the flag array until the refinement overwrites it
  const uint64_t chunk_img_stride = a.cand_img_stride;
  const uint32_t n = a.nsegs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i0 = vb.x * SEG_CHUNK + 4u * threadIdx.x;
  uint32_t p[4];
#pragma unroll
  for (int k = 0; k < 4; k++)
    p[k] = i0 + k < n ? (uint32_t)__popcll(mask[i0 + k]) : 0u;
  const uint32_t tsum = p[0] + p[1] + p[2] + p[3];
  const uint32_t incl = wave_scan_incl_u32(tsum, lane);
  if (lane == 63)
    wave_tot[wave] = incl;
  __syncthreads();
  uint32_t wave_base = 0, total = 0;
  for (int wv = 0; wv < 16; wv++)
  {
    if (wv < wave)
      wave_base += wave_tot[wv];
    total += wave_tot[wv];
  }
  uint32_t run = wave_base + incl - tsum;
#pragma unroll
  for (int k = 0; k < 4; k++)
  {
    if (i0 + k < n)
      off[i0 + k] = run;
    run += p[k];
  }
  if (threadIdx.x == 0)
    chunk_tot[(size_t)b * chunk_img_stride + vb.x] = total;
}

// The second level of the two-level scans lives in the consumers since round 6: the lists are short (an image has nsegs / 4096 segment
// chunks and candidates / 256 refinement chunks), and adding up the entries in front of one's own chunk costs less than the launch of a
// scan kernel did (k_chunk_offsets: two launches of ~5 us each on the critical path of a single-image detection).

// One thread per 64-pixel segment: expand its candidate ballot into packed coordinates at offset + rank.
__global__ void __launch_bounds__(256) k_cand_list(Multi<ExtremaArgs> mu)
{
  const VBlock vb = vblock(mu); // virtual grid (segment blocks, images)
  const ExtremaArgs &a = mu.oct[vb.o];
  const uint32_t seg = vb.x * 256 + threadIdx.x;
  const int b = (int)vb.y;
  // (k_segment_scan left the chunk totals at the start of the still unused flag array)
  const uint32_t *chunk_tot = a.cand_flag + (size_t)b * a.cand_img_stride;
  if (vb.x == 0 && threadIdx.x == 0)
  {
    // the first workgroup of an image posts the candidate count: the totals of all its chunks (15 for a 1280x960 octave)
    uint32_t total = 0;
    for (uint32_t c = 0; c < a.nchunks; c++)
      total += chunk_tot[c];
    a.cand_n[b] = total;
    if (total == 0)
      a.found[(size_t)b * a.found_img_stride] = 0; // no candidate: k_cand_emit visits no chunk of this image
  }
  unsigned long long m = seg < a.nsegs ? a.seg_mask[seg + (size_t)b * a.seg_img_stride] : 0ull;
  if (__ballot(m != 0ull) == 0ull)
    return; // (wave-uniform) no candidate in these 64 segments: most waves of the launch
  // offset inside the chunk (k_segment_scan) + base of the chunk = the totals of the chunks in front of it: a wave's 64 segments lie in one
  // chunk, so the wave adds the totals up together — lane c loads chunk c (one load for up to 64 chunks), a butterfly sums them. No barrier,
  // no dependent chain of loads (a per-lane loop over the 15 totals of a 1280x960 octave was one).
  uint32_t base = 0;
  for (uint32_t c = threadIdx.x & 63u, nc = (vb.x * 256u) / SEG_CHUNK; c < nc; c += 64u)
    base += chunk_tot[c];
  base = wave_sum_u32(base);
  if (m == 0ull)
    return;
  uint32_t pos = a.seg_off[seg + (size_t)b * a.seg_img_stride] + base;
  const uint32_t segx = seg % (uint32_t)a.nseg;
  const uint32_t yy = (seg / (uint32_t)a.nseg) % (uint32_t)a.h;
  const uint32_t sz = seg / ((uint32_t)a.nseg * (uint32_t)a.h);
  uint32_t *out = a.cand_xy + (size_t)b * a.cand_img_stride;
  while (m)
  {
    const int bit = __ffsll((long long)m) - 1;
    m &= m - 1;
    if (pos < a.cand_cap)
      out[pos] = (segx * 64u + (uint32_t)bit) | (yy << 14) | ((sz + 1u) << 28);
    pos++;
  }
}

// Dense refinement: thread t of a 256-candidate chunk refines candidate chunk*256 + t (count read from HBM, workgroups
// stride over the chunks). Besides the accept flags every chunk publishes its number of accepted candidates for the second
// scan level inside k_cand_emit.
template <bool F16, bool BUF>
__global__ void __launch_bounds__(256) k_refine_flags(Multi<ExtremaArgs> m)
{
  __shared__ uint32_t s_cnt[4];
  const VBlock vb = vblock(m); // virtual grid (images, chunks)
  const RefineCtx c = refine_ctx<F16>(m.oct[vb.o], (int)vb.x); // image index fastest: see the launch
  for (uint32_t chunk = vb.y; chunk < c.nch; chunk += vb.gy)
  {
    const uint32_t i = chunk * 256u + threadIdx.x;
    bool ok = false;
    if (i < c.n)
    {
      KpRecord kp;
      ok = refine_candidate<F16, BUF>(c, c.xy[i], &kp);
      c.flag[i] = ok ? 1u : 0u;
    }
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0)
      s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0)
      c.chunk_sum[chunk] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
  }
}

// Accepted candidates recompute their record (bit-identical) and store it at chunk base + rank inside the chunk (raster
// order is preserved) if it fits the section. About one candidate in six is accepted: the accepted ones of a chunk are
// first compacted through LDS, so the recomputation runs on dense lanes (one wave per chunk instead of four sparse ones).
template <bool F16, bool BUF>
__global__ void __launch_bounds__(256) k_cand_emit(Multi<ExtremaArgs> m)
{
  __shared__ uint32_t s_cnt[4];
  __shared__ uint32_t s_red[4];
  __shared__ uint32_t s_list[256];
  const VBlock vb = vblock(m); // virtual grid (images, chunks)
  const ExtremaArgs &a = m.oct[vb.o];
  const int b = (int)vb.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RefineCtx c = refine_ctx<F16>(a, b);
  for (uint32_t chunk = vb.y; chunk < c.nch; chunk += vb.gy)
  {
    // records of the chunks in front of this one (raster order is preserved): partial sums of their accept counts ride on the barrier
    // the rank computation needs anyway; the image's last chunk posts the keypoint count
    uint32_t part = 0;
    for (uint32_t k = threadIdx.x; k < chunk; k += 256u)
      part += c.chunk_sum[k];
    part = wave_sum_u32(part);
    const uint32_t i = chunk * 256u + threadIdx.x;
    const bool v = i < c.n && c.flag[i] != 0u;
    const unsigned long long bal = __ballot(v);
    if (lane == 0)
      s_cnt[wave] = (uint32_t)__popcll(bal), s_red[wave] = part;
    __syncthreads();
    const uint32_t cbase = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    uint32_t rank = ballot_rank(bal, lane);
    for (int wv = 0; wv < wave; wv++)
      rank += s_cnt[wv];
    const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (v)
      s_list[rank] = c.xy[i];
    __syncthreads();
    const uint32_t idx = cbase + threadIdx.x;
    if (chunk + 1u == c.nch && threadIdx.x == 0)
      a.found[(size_t)b * a.found_img_stride] = cbase + total; // un-clamped, like nb_elem (0 candidates: the counter reset's 0 stays)
    if (threadIdx.x < total && idx < a.cap)
    {
      KpRecord kp;
      refine_candidate<F16, BUF>(c, s_list[threadIdx.x], &kp);
      store_record((uint32_t *)(a.feats + (size_t)b * a.feat_img_stride + (size_t)idx * VKSIFT_RECORD_BYTES), kp);
    }
    __syncthreads();
  }
}

} // namespace

/* Everything the contract of vksift_hip_extract_keypoints (include/vksift_hip.h) excludes is refused here, before anything is launched. */
static int make_extrema_args(const vksift_hip_OctaveJob *job, ExtremaArgs *out)
{
  if (job->w == 0u || job->h == 0u || job->w > VKSIFT_HIP_MAX_OCTAVE_SIDE || job->h > VKSIFT_HIP_MAX_OCTAVE_SIDE || job->S == 0u || job->S > 13u)
    return (int)hipErrorInvalidValue; /* candidate coordinates are packed 14 + 14 + 4 bits; k_extrema_lean is instantiated for S = 1 .. 13 */
  const uint64_t eb = job->fp16 ? 2u : 4u;
  /* rows inside their pitch, layers that do not overlap (the buffer form of the refinement sees an image's octave as (S + 3) * plane_stride
   * texels), planes below 2 GiB (the scan addresses a plane with 32-bit byte offsets) */
  if (job->pitch < job->w || job->plane_stride < (uint64_t)job->pitch * job->h || (uint64_t)job->pitch * job->h * eb >= 0x80000000ull)
    return (int)hipErrorInvalidValue;
  /* texels at their natural alignment; the scan loads the binary16 pair (x, x + 1), x even, as ONE dword: every row of every layer of every
   * image has to start on a 4-byte boundary */
  if (((uintptr_t)job->gauss & 3u) != 0u || (job->fp16 && ((job->pitch | job->plane_stride | job->img_stride) & 1u) != 0u))
    return (int)hipErrorInvalidValue;
  ExtremaArgs a;
  a.gauss = job->gauss;
  a.fp16 = (int)job->fp16;
  a.w = (int)job->w, a.h = (int)job->h, a.pitch = (int)job->pitch;
  a.plane_stride = job->plane_stride, a.img_stride = job->img_stride;
  a.S = (int)job->S, a.octave_idx = job->octave_idx;
  a.seed_sigma = job->seed_sigma, a.dog_threshold = job->dog_threshold, a.edge_limit = job->edge_limit;
  a.seg_mask = job->seg_mask, a.seg_off = job->seg_off, a.seg_img_stride = job->seg_img_stride;
  a.nseg = (int)((job->w + 63) / 64);
  a.feats = job->feats, a.feat_img_stride = job->feat_img_stride, a.cap = job->cap;
  a.found = job->found, a.found_img_stride = job->found_img_stride;
  a.cand_xy = job->cand_xy, a.cand_flag = job->cand_flag, a.cand_n = job->cand_n;
  a.cand_img_stride = job->cand_img_stride, a.cand_cap = job->cand_cap;
  a.scan_rev = (int)job->scan_reverse;
  /* 48 rows per wave on the large octaves (2 halo rows per band: 4 %; swept in the pipeline, 512 frames: 32 rows 3.91 ms, 40 3.85, 48 3.83,
   * 56 3.84, 64 3.89); 16 on the small ones, whose share of a launch is latency bound and gains more from twice the waves */
  a.band = job->h > 256u ? 48 : 16;
  if (vksift_hip_tune_get(VKSIFT_TUNE_SCAN_BAND) > 0 && job->h > 256u)
    a.band = vksift_hip_tune_get(VKSIFT_TUNE_SCAN_BAND);
  a.nsegs = job->S * job->h * (uint32_t)a.nseg;
  a.nchunks = (a.nsegs + SEG_CHUNK - 1u) / SEG_CHUNK;
  /* the per-image mask regions are contiguous (the clear below is one fill per octave), the chunk bases fit the flag array, the candidate
   * lists of consecutive images do not overlap */
  if (job->seg_img_stride != a.nsegs || a.nchunks > a.cand_cap || job->cand_img_stride < job->cand_cap)
    return (int)hipErrorInvalidValue;
  *out = a;
  return 0;
}

/* one fill per run of octaves whose mask regions follow each other (the instance's layout) */
static int clear_masks(const ExtremaArgs *args, uint32_t n, uint32_t batch, hipStream_t hs)
{
  for (uint32_t i = 0; i < n;)
  {
    uint32_t j = i + 1;
    size_t bytes = sizeof(uint64_t) * (size_t)args[i].nsegs * batch;
    while (j < n && (const uint8_t *)args[j].seg_mask == (const uint8_t *)args[i].seg_mask + bytes)
      bytes += sizeof(uint64_t) * (size_t)args[j].nsegs * batch, j++;
    const hipError_t me = hipMemsetAsync(args[i].seg_mask, 0, bytes, hs);
    if (me != hipSuccess)
      return (int)me;
    i = j;
  }
  return 0;
}

/* the launches of one run of at most MULTI_MAX octaves (same S, same texel type); args: the jobs' validated arguments (make_extrema_args) */
static int extract_run(const vksift_hip_OctaveJob *jobs, ExtremaArgs *args, uint32_t n, uint32_t batch, hipStream_t hs, hipEvent_t scan_done)
{
  const bool f16 = args[0].fp16 != 0;
  const int S = args[0].S;
  {
    /* A launch that cannot fill the chip (one image, a handful) is bound by the length of a wave's march, not by bandwidth: 16-row bands
     * everywhere give it twice the waves at half the length (one 640x480 image: the scan 35 -> ~20 us, detection 0.367 -> 0.347 ms) */
    uint64_t waves = 0;
    for (uint32_t i = 0; i < n; i++)
      waves += (uint64_t)batch * ((args[i].w + 127) / 128) * ((args[i].h + args[i].band - 1) / args[i].band);
    if (waves < 2048u && vksift_hip_tune_get(VKSIFT_TUNE_SCAN_BAND) <= 0)
      for (uint32_t i = 0; i < n; i++)
        args[i].band = 16;
  }

  /* 1. candidate ballots: only non-empty 64-pixel segments are stored (scattered 8-byte stores were the bottleneck of this
   * pass), so the mask arrays are cleared first: one fill when the octaves' regions follow each other (the instance's layout) */
  bool cleared = true;
  for (uint32_t i = 0; i < n; i++)
    cleared = cleared && jobs[i].masks_cleared != 0;
  if (!cleared)
  {
    const int me = clear_masks(args, n, batch, hs);
    if (me)
      return me;
  }
  /* bit 0: the 4 waves of a block take adjacent strips (-5 % against adjacent bands), bit 1: XCD-contiguous block order (-3 %) */
  const int sm = 3;

#define VKSIFT_MULTI(M, GX, GY, GZ)                              \
  Multi<ExtremaArgs> M;                                           \
  M.n = 0;                                                        \
  for (uint32_t i = 0; i < n; i++)                                \
  {                                                               \
    const ExtremaArgs &a = args[i];                               \
    (void)a;                                                      \
    if (!multi_add(M, args[i], (GX), (GY), (GZ)))                 \
      return (int)hipErrorInvalidValue;                           \
  }
  {
    VKSIFT_MULTI(ms, (uint32_t)(a.nseg + 1) / 2u, ((a.h + a.band - 1) / a.band + 3u) / 4u, batch)
    const dim3 sgrid(ms.start[ms.n]);
    /* window slots: fp32 texels 4 (one row of loads in flight; two rows spill registers since the slots receive S+3 Gaussian
     * texels), binary16 texels 5 (a row in flight costs half the registers) */
    const bool known = with_scales(S, [&](auto NS) {
      with_bool(f16, [&](auto F16) {
        constexpr bool h = decltype(F16)::value;
        hipLaunchKernelGGL((k_extrema_lean<decltype(NS)::value, h ? 5 : 4, h>), sgrid, dim3(256), 0, hs, ms, sm);
      });
    });
    if (!known)
      return (int)hipErrorInvalidValue;
  }
  if (scan_done)
    (void)hipEventRecord(scan_done, hs);
  /* the refinement addresses an image's octave through one buffer resource with 32-bit offsets where it fits (always, short of
   * 4096 x 4096 octaves with many scales); the pointer form serves the rest */
  bool buf = vksift_hip_tune_get(VKSIFT_TUNE_REFINE_PTR) == 0;
  for (uint32_t i = 0; i < n; i++)
    buf = buf && (uint64_t)(args[i].S + 3) * args[i].plane_stride * (f16 ? 2u : 4u) < 0x7FFF0000ull;
  /* A batch of 64 images and more (64 x octaves workgroups: about one per CU) takes the tail as ONE launch, one workgroup per image and octave
   * (extract_tail.hip): ballots read once, every candidate refined once, no list, flags or offsets through HBM. Smaller calls — single
   * images, captured detections — cannot fill the chip that way and keep the four launches below. VKSIFT_TUNE_TAIL_FUSED: 1 never, 2 always, 3 always and with the
   * workgroup size of large launches */
  const int fused = vksift_hip_tune_get(VKSIFT_TUNE_TAIL_FUSED);
  if (fused == 2 || fused == 3 || (fused != 1 && batch >= 64u))
    return extract_tail_launch(args, n, batch, f16, buf, fused == 3, hs);
  /* 2. offsets + candidate count: chunk-local scan (the scan of the chunk totals happens in the consumer); the totals live at
   * the start of the flag array until the refinement overwrites it */
  {
    VKSIFT_MULTI(m2, a.nchunks, batch, 1u)
    hipLaunchKernelGGL(k_segment_scan, dim3(m2.start[m2.n]), dim3(1024), 0, hs, m2);
  }
  /* 3. compact list */
  {
    VKSIFT_MULTI(m3, (a.nsegs + 255u) / 256u, batch, 1u)
    hipLaunchKernelGGL(k_cand_list, dim3(m3.start[m3.n]), dim3(256), 0, hs, m3);
  }
  /* 4. dense refinement (+ per-chunk accept counts), 5. accepted -> records.
   * virtual grid = (image, chunk): the busy workgroups (chunk < candidates / 256, a small and unknown part of the grid) are then
   * contiguous in dispatch order. With the chunk index fastest they formed a short run at the start of every image's row of
   * 512 workgroups, which the dispatcher's round-robin maps onto the same half of the shader engines of every XCD:
   * measured 221 us instead of 70 us for this launch (and 137 instead of 51 us for k_cand_emit). */
  /* at most 512 chunk workgroups per image, and ~64 k per octave whatever the batch (they stride over the chunks; idle ones only
   * cost dispatch: 512 frames with 512 per image 1.25 ms for the stage without the scan, with 128 per image 0.86 ms) */
  const uint32_t rcap = 65536u / batch < 16u ? 16u : (65536u / batch > 512u ? 512u : 65536u / batch);
  /* (and no more than a quarter of the list's capacity, S*w*h/4 texels, asks for: the capacity holds the densest image there can be, a
   * 2x2-periodic texture — natural images stay far below a quarter of it, and the workgroups of a denser octave stride over its chunks) */
#define VKSIFT_REFINE_CHUNKS(a) (((uint64_t)(a).S * (uint32_t)(a).w * (uint32_t)(a).h / 4u + 64u + 255u) / 256u)
  VKSIFT_MULTI(mr, batch, VKSIFT_REFINE_CHUNKS(a) > rcap ? rcap : (uint32_t)VKSIFT_REFINE_CHUNKS(a), 1u)
#undef VKSIFT_REFINE_CHUNKS
#undef VKSIFT_MULTI
  const dim3 rgrid(mr.start[mr.n]);
  with_bool(f16, [&](auto F16) {
    with_bool(buf, [&](auto BUF) {
      hipLaunchKernelGGL((k_refine_flags<decltype(F16)::value, decltype(BUF)::value>), rgrid, dim3(256), 0, hs, mr);
      hipLaunchKernelGGL((k_cand_emit<decltype(F16)::value, decltype(BUF)::value>), rgrid, dim3(256), 0, hs, mr);
    });
  });
  return (int)hipGetLastError();
}

/* the validated arguments of every job, or the error of the first one the contract excludes */
static int make_all_extrema_args(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, std::vector<ExtremaArgs> &args)
{
  args.resize(n_jobs);
  for (uint32_t i = 0; i < n_jobs; i++)
  {
    const int e = make_extrema_args(&jobs[i], &args[i]);
    if (e)
      return e;
  }
  return 0;
}

extern "C" int vksift_hip_extract_keypoints_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s,
                                                  vksift_hip_event scan_done)
{
  if (n_jobs == 0 || batch == 0)
    return 0;
  /* a job the contract excludes refuses the whole call before the first run is launched */
  std::vector<ExtremaArgs> args;
  const int bad = make_all_extrema_args(jobs, n_jobs, args);
  if (bad)
    return bad;
  /* runs of octaves that one launch can serve: same S and texel type (always the case inside one detection), at most MULTI_MAX */
  for (uint32_t i0 = 0; i0 < n_jobs;)
  {
    uint32_t i1 = i0 + 1;
    while (i1 < n_jobs && i1 - i0 < multi_run_max() && jobs[i1].S == jobs[i0].S && jobs[i1].fp16 == jobs[i0].fp16)
      i1++;
    const int e = extract_run(jobs + i0, args.data() + i0, i1 - i0, batch, (hipStream_t)s, i1 == n_jobs ? (hipEvent_t)scan_done : nullptr);
    if (e)
      return e;
    i0 = i1;
  }
  return 0;
}

extern "C" int vksift_hip_clear_segment_masks(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s)
{
  if (n_jobs == 0 || batch == 0)
    return 0;
  if (n_jobs > 16)
    return (int)hipErrorInvalidValue;
  std::vector<ExtremaArgs> args;
  const int bad = make_all_extrema_args(jobs, n_jobs, args);
  return bad ? bad : clear_masks(args.data(), n_jobs, batch, (hipStream_t)s);
}

extern "C" int vksift_hip_extract_keypoints(const vksift_hip_OctaveJob *job, uint32_t batch, vksift_hip_stream s, vksift_hip_event scan_done)
{
  return vksift_hip_extract_keypoints_multi(job, 1, batch, s, scan_done);
}
