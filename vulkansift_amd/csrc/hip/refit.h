// refit.h — what the refits on the inliers share whatever the model (refine.hip: homography, refine_f.hip: fundamental matrix): the fixed-order
// reductions over a workgroup of 256 threads, the conditioning of the two sides, and the elimination of an 8x9 system in registers.
// Everything is integer arithmetic or correctly rounded fp32 add / sub / mul / div in a fixed order (the tree is built with -ffp-contract=off and no
// fmaf is used here). Every sum over correspondences has one order whatever the scheduling: thread t adds its elements k = t, t + 256, ... in
// increasing k, the 64 lanes of a wave are added by a butterfly (p + p[lane ^ off], off = 32 .. 1: addition commutes, so every lane holds the same
// bits), the four waves as ((w0 + w1) + w2) + w3. No float atomics. tests/np_refine.py restates these pieces bit for bit.
#ifndef VKSIFT_REFIT_H
#define VKSIFT_REFIT_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hip/two_view.h"

namespace refit
{

constexpr uint32_t kThreads = 256u;
constexpr uint32_t kMaxRounds = 8u;
constexpr uint32_t kResultWords = 13u; // {model[9], nb_matches, nb_inliers, rounds, valid}

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// 2^(127 - e) for the exponent e of the largest magnitude `mbits`; ok: that magnitude is normal and below 2^127 (verify.hip's idiom)
__device__ __forceinline__ float unit_scale(uint32_t mbits, bool &ok)
{
  const uint32_t e = mbits >> 23;
  ok = e >= 1u && e <= 253u;
  return __uint_as_float((254u - (ok ? e : 127u)) << 23);
}

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// zero, subnormal or not finite
__device__ __forceinline__ bool unusable_bits(float x)
{
  const uint32_t e = abs_bits(x) >> 23;
  return e == 0u || e == 255u;
}

// ---- fixed-order reductions over the workgroup; the result in every thread. `part`: LDS, one row per wave ------------------------------
template <int N> __device__ __forceinline__ void block_sum(float (&v)[N], float (*part)[N])
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int i = 0; i < N; i++)
      v[i] = v[i] + __shfl_xor(v[i], off, 64);
  __syncthreads(); // the previous reduction's readers are through with `part`
  if ((threadIdx.x & 63u) == 0u)
  {
#pragma unroll
    for (int i = 0; i < N; i++)
      part[threadIdx.x >> 6][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; i++)
    v[i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i]; // every lane reads the same words: broadcast LDS accesses
}

template <bool MAX> __device__ __forceinline__ uint32_t block_u32(uint32_t v, uint32_t (&part)[4])
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
  {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
    v = MAX ? max(v, o) : v + o;
  }
  __syncthreads();
  if ((threadIdx.x & 63u) == 0u)
    part[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? max(max(part[0], part[1]), max(part[2], part[3])) : ((part[0] + part[1]) + part[2]) + part[3];
}

// The LDS of a refit kernel with N sums per accumulation
template <int N> struct Shared
{
  float part[4][N];
  float part4[4][4];
  uint32_t upart[4];
};

// One side of the inliers: x, y become s (x - cx), s (y - cy)
struct Side
{
  float cx, cy, s;
};

// The number of correspondences the mask marks
template <int N> __device__ __forceinline__ uint32_t count_marked(uint32_t n, const uint8_t *mask, Shared<N> &sh)
{
  uint32_t m = 0u;
  for (uint32_t k = threadIdx.x; k < n; k += kThreads)
    m += mask[k] == 1u ? 1u : 0u;
  return block_u32<false>(m, sh.upart);
}

// Both sides, each on its own: the centroid (fixed-order sums divided by the count m of inliers) and the power of two s that brings the
// largest |deviation| over the inliers into [1, 2); false when a side has no such power (all inliers in one point, a coordinate that is
// not finite).
template <int N>
__device__ __forceinline__ bool condition_sides(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, uint32_t m, Side &A, Side &B, Shared<N> &sh)
{
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t k = threadIdx.x; k < n; k += kThreads)
  {
    const bool in = mask[k] == 1u;
    const float4 q = c[k];
    s4[0] = s4[0] + (in ? q.x : 0.f), s4[1] = s4[1] + (in ? q.y : 0.f), s4[2] = s4[2] + (in ? q.z : 0.f), s4[3] = s4[3] + (in ? q.w : 0.f);
  }
  block_sum<4>(s4, sh.part4);
  const float fm = (float)m;
  A.cx = s4[0] / fm, A.cy = s4[1] / fm, B.cx = s4[2] / fm, B.cy = s4[3] / fm;
  uint32_t ma = 0u, mb = 0u;
  for (uint32_t k = threadIdx.x; k < n; k += kThreads)
  {
    if (mask[k] != 1u)
      continue;
    const float4 q = c[k];
    ma = max(ma, max(abs_bits(q.x - A.cx), abs_bits(q.y - A.cy)));
    mb = max(mb, max(abs_bits(q.z - B.cx), abs_bits(q.w - B.cy)));
  }
  ma = block_u32<true>(ma, sh.upart);
  mb = block_u32<true>(mb, sh.upart);
  bool oka, okb;
  A.s = unit_scale(ma, oka), B.s = unit_scale(mb, okb);
  return oka && okb;
}

// An 8x9 system solved like solve_f7 eliminates (verify.hip): Gauss-Jordan, for column k the rows k+1..7 compared with row k in turn and
// exchanged when their |entry| (bit pattern) is strictly larger; row k times 1 / pivot; every other row r minus a[r][k] times row k. Fully
// unrolled: every index is a compile-time constant, the system lives in registers. false: a pivot that is zero, subnormal or not finite, or a
// solution entry that is not finite.
__device__ __forceinline__ bool solve8(float (&a)[8][9], float (&x)[8])
{
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; k++)
  {
#pragma unroll
    for (int r = k + 1; r < 8; r++)
    {
      const bool sw = abs_bits(a[r][k]) > abs_bits(a[k][k]);
#pragma unroll
      for (int j = k; j < 9; j++)
      {
        const float top = a[k][j], low = a[r][j];
        a[k][j] = sw ? low : top, a[r][j] = sw ? top : low;
      }
    }
    const uint32_t e = abs_bits(a[k][k]) >> 23;
    ok = ok && e != 0u && e != 255u;
    const float inv = 1.0f / a[k][k];
#pragma unroll
    for (int j = k + 1; j < 9; j++)
      a[k][j] = a[k][j] * inv;
#pragma unroll
    for (int r = 0; r < 8; r++)
      if (r != k)
      {
        const float f = a[r][k];
#pragma unroll
        for (int j = k + 1; j < 9; j++)
          a[r][j] = a[r][j] - f * a[k][j];
      }
  }
#pragma unroll
  for (int r = 0; r < 8; r++)
    x[r] = a[r][8], ok = ok && finite_bits(x[r]);
  return ok;
}

template <int KIND> __device__ __forceinline__ bool admits(const float (&M)[9], float4 q, float t2)
{
  return admissible<KIND>(side_a<KIND>(M, float2{q.x, q.y}, t2), side_b<KIND>(M, float2{q.z, q.w}), t2);
}

// The chain of rounds of one slot (blockIdx.x), the whole body of a refit kernel. KIND: the model of two_view.h's test; START_WORDS: the words
// of the verification's record {model[9], nb_matches, nb_inliers, ..., valid}; round(c, n, mask, kept, o, sh): one refit on the
// correspondences `mask` marks, starting from the model `kept`, the published model in o, uniform over the workgroup, false when the round failed.
// Round r starts from the mask and the model round r - 1 left; a round is accepted iff it did not fail and counts at least as many inliers under
// two_view.h's test on the published model (exactly what guided matching would admit) as the result kept so far (the RANSAC result at first); the
// first round that is not accepted ends the loop. start_masks and masks_out are not __restrict__: from the second round on the mask read is the
// one the round before wrote, in this workgroup (a barrier lies between the stores and the loads).
template <int KIND, uint32_t START_WORDS, class Lds, class Round>
__device__ __forceinline__ void refit_chain(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev, uint32_t n_stride,
                                            uint32_t max_n, const uint32_t *__restrict__ start_results, const uint8_t *start_masks, uint64_t mask_slot_stride,
                                            uint32_t nb_rounds, float t2, uint32_t *__restrict__ results, uint8_t *masks_out, Lds &sh, Round round)
{
  const uint32_t slot = blockIdx.x, tid = threadIdx.x;
  uint32_t n = n_dev[(size_t)slot * n_stride];
  n = n < max_n ? n : max_n;
  const float4 *c = corr + (size_t)slot * corr_slot_stride;
  const uint8_t *start = start_masks + (size_t)slot * mask_slot_stride;
  uint8_t *out = masks_out + (size_t)slot * mask_slot_stride;
  const uint32_t *sr = start_results + (size_t)slot * START_WORDS;
  uint32_t *res = results + (size_t)slot * kResultWords;
  if (sr[START_WORDS - 1u] == 0u) // uniform: nothing was verified for this slot
  {
    for (uint32_t k = tid; k < n; k += kThreads)
      out[k] = 0u;
    if (tid < kResultWords)
      res[tid] = 0u;
    return;
  }
  float kept[9];
#pragma unroll
  for (int i = 0; i < 9; i++)
    kept[i] = __uint_as_float(sr[i]);
  uint32_t kept_cnt = sr[10], rounds = 0u;
  const uint8_t *cur = start;
  for (uint32_t r = 1u; r <= nb_rounds; r++)
  {
    float o[9];
    if (!round(c, n, cur, kept, o, sh)) // uniform
      break;
    uint32_t cnt = 0u;
    for (uint32_t k = tid; k < n; k += kThreads)
      cnt += admits<KIND>(o, c[k], t2) ? 1u : 0u;
    cnt = block_u32<false>(cnt, sh.upart);
    if (cnt < kept_cnt)
      break;
    // accepted: every thread is past its last read of `cur` (the barriers of the reductions); the new mask replaces it in place
    for (uint32_t k = tid; k < n; k += kThreads)
      out[k] = admits<KIND>(o, c[k], t2) ? 1u : 0u;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 9; i++)
      kept[i] = o[i];
    kept_cnt = cnt, rounds = r, cur = out;
  }
  if (rounds == 0u)
    for (uint32_t k = tid; k < n; k += kThreads)
      out[k] = start[k];
  if (tid == 0u)
  {
#pragma unroll
    for (int i = 0; i < 9; i++)
      res[i] = __float_as_uint(kept[i]);
    res[9] = n, res[10] = kept_cnt, res[11] = rounds, res[12] = 1u;
  }
}

// The launcher's refusals, the same for every model: false = hipErrorInvalidValue, nothing launched. t2 receives the squared threshold in
// pixels, formed like guided matching forms it: the verification's (threshold_px 2^-13)^2 brought back by 2^26.
inline bool launch_admitted(const float *corr, uint64_t corr_slot_stride, uint32_t max_n, uint32_t nslots, const uint8_t *start_results, const uint8_t *start_masks,
                            uint64_t mask_slot_stride, uint32_t nb_rounds, float threshold_px, const uint8_t *results, const uint8_t *masks_out, float &t2)
{
  const float ts = threshold_px * (1.0f / 8192.0f);
  t2 = (ts * ts) * 67108864.0f;
  if (nslots < 1 || nb_rounds == 0 || nb_rounds > kMaxRounds || !(threshold_px > 0.f) || !isfinite(threshold_px) || !(t2 > 0.f) || !isfinite(t2) ||
      (corr_slot_stride & 15u) || ((uintptr_t)corr & 15u) || ((uintptr_t)results & 3u) || ((uintptr_t)start_results & 3u) ||
      (nslots > 1 && (corr_slot_stride < 16u * (uint64_t)max_n || mask_slot_stride < max_n)))
    return false;
  // the output masks may not overlap the start masks: a slot whose first round is not accepted reports its start mask
  const uint64_t extent = (uint64_t)(nslots - 1u) * mask_slot_stride + max_n;
  const uintptr_t a = (uintptr_t)start_masks, b = (uintptr_t)masks_out;
  return !(a == b || (a < b ? b - a < extent : a - b < extent));
}

} // namespace refit

#endif
