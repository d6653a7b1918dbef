// refine.hip — locally optimised refit of the verified homographies on their inliers (no counterpart in the reference, whose callers refit
// on the CPU after downloading matches, features and masks). One launch serves every pair (slot) of a call, one workgroup of 256 threads
// per slot, all rounds inside it:
//   round   a least-squares homography on the correspondences the current mask marks (conditioning, a linear start with h8 = 1, two
//           Gauss-Newton steps on the forward transfer error), published in pixel coordinates, and all n correspondences re-scored
//           under it with two_view.h's test on the published model (exactly what guided matching would admit)
//   chain   round r starts from the mask round r - 1 left; a round is accepted iff it did not fail and counts at least as many inliers as
//           the result kept so far (the RANSAC result at first); the first round that is not accepted ends the loop
// Everything is integer arithmetic or correctly rounded fp32 add / sub / mul / div in a fixed order (the tree is built with
// -ffp-contract=off and no fmaf is used here). Every sum over correspondences has one order whatever the scheduling: thread t adds its
// elements k = t, t + 256, ... in increasing k, the 64 lanes of a wave are added by a butterfly (p + p[lane ^ off], off = 32 .. 1: addition
// commutes, so every lane holds the same bits), the four waves as ((w0 + w1) + w2) + w3. No float atomics. tests/np_refine.py is the
// specification of the operation order and restates every output bit for bit.
// Model-free: the reductions (block_sum, block_u32) and the conditioning (condition_sides); a refit of the fundamental
// matrix would reuse them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/two_view.h"

namespace
{

constexpr uint32_t kThreads = 256u;
constexpr int kGaussNewtonSteps = 2; // one step after the linear start reaches 4 digits of the cost; not a knob
constexpr int kSums = 27;            // distinct sums of the 8x8 normal equations and their right-hand side
constexpr uint32_t kMaxRounds = 8u;
constexpr uint32_t kResultWords = 13u; // {H[9], nb_matches, nb_inliers, rounds, valid}; the RANSAC record has best_hypothesis in place of rounds
constexpr int kKind = (int)VKSIFT_HIP_GUIDE_HOMOGRAPHY;

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// 2^(127 - e) for the exponent e of the largest magnitude `mbits`; ok: that magnitude is normal and below 2^127 (verify.hip's idiom)
__device__ __forceinline__ float unit_scale(uint32_t mbits, bool &ok)
{
  const uint32_t e = mbits >> 23;
  ok = e >= 1u && e <= 253u;
  return __uint_as_float((254u - (ok ? e : 127u)) << 23);
}

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

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

struct Shared
{
  float part[4][kSums];
  float part4[4][4];
  uint32_t upart[4];
};

// One side of the inliers: x, y become s (x - cx), s (y - cy)
struct Side
{
  float cx, cy, s;
};

// Both sides, each on its own: the centroid (fixed-order sums divided by the count m of inliers) and the power of two s that brings the
// largest |deviation| over the inliers into [1, 2); false when a side has no such power (all inliers in one point, a coordinate that is
// not finite).
__device__ __forceinline__ bool condition_sides(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, uint32_t m, Side &A, Side &B, Shared &sh)
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

// The 27 sums of the rows [a b i 0 0 0 -pu a -pu b | -ru], [0 0 0 a b i -pv a -pv b | -rv] over the inliers. LINEAR: the linear start
// (a, b, i, pu, pv, ru, rv) = (x, y, 1, X, Y, -X, -Y) in conditioned coordinates; otherwise the Gauss-Newton step at h, the Jacobian
// rows of the forward transfer error (u / d - X, v / d - Y).
template <bool LINEAR>
__device__ __forceinline__ void accumulate(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, const Side &A, const Side &B, const float (&h)[8],
                                           float (&S)[kSums], Shared &sh)
{
#pragma unroll
  for (int i = 0; i < kSums; i++)
    S[i] = 0.f;
  for (uint32_t k = threadIdx.x; k < n; k += kThreads)
  {
    const bool in = mask[k] == 1u;
    const float4 q = c[k];
    const float x = (q.x - A.cx) * A.s, y = (q.y - A.cy) * A.s, X = (q.z - B.cx) * B.s, Y = (q.w - B.cy) * B.s;
    float a, b, i, pu, pv, ru, rv;
    if (LINEAR)
      a = x, b = y, i = 1.0f, pu = X, pv = Y, ru = -X, rv = -Y;
    else
    {
      const float u = (h[0] * x + h[1] * y) + h[2];
      const float v = (h[3] * x + h[4] * y) + h[5];
      const float d = (h[6] * x + h[7] * y) + 1.0f;
      i = 1.0f / d;
      a = x * i, b = y * i, pu = u * i, pv = v * i, ru = pu - X, rv = pv - Y;
    }
    const float aa = a * a, ab = a * b, ai = a * i, bb = b * b, bi = b * i, ii = i * i;
    const float w = pu * pu + pv * pv;
    const float g = pu * ru + pv * rv;
    const float t[kSums] = {aa,      ab,      ai,      bb,      bi,      ii,     pu * aa, pu * ab, pu * bb, pu * ai, pu * bi, pv * aa, pv * ab, pv * bb,
                            pv * ai, pv * bi, w * aa,  w * ab,  w * bb,  a * ru, b * ru,  i * ru,  a * rv,  b * rv,  i * rv,  g * a,   g * b};
#pragma unroll
    for (int j = 0; j < kSums; j++)
      S[j] = S[j] + (in ? t[j] : 0.f); // an element outside the mask adds +0: no bit changes (a partial sum that starts at +0 is never -0)
  }
  block_sum<kSums>(S, sh.part);
}

// The 8x9 normal equations of the sums, solved like solve_f7 eliminates (verify.hip): Gauss-Jordan, for column k the rows k+1..7 compared
// with row k in turn and exchanged when their |entry| (bit pattern) is strictly larger; row k times 1 / pivot; every other row r minus
// a[r][k] times row k. Fully unrolled: every index is a compile-time constant, the system lives in registers. false: a pivot that is zero,
// subnormal or not finite, or a solution entry that is not finite.
__device__ __forceinline__ bool solve8(const float (&S)[kSums], float (&x)[8])
{
  const float z = 0.f;
  float a[8][9] = {{S[0], S[1], S[2], z, z, z, -S[6], -S[7], -S[19]},          {S[1], S[3], S[4], z, z, z, -S[7], -S[8], -S[20]},
                   {S[2], S[4], S[5], z, z, z, -S[9], -S[10], -S[21]},         {z, z, z, S[0], S[1], S[2], -S[11], -S[12], -S[22]},
                   {z, z, z, S[1], S[3], S[4], -S[12], -S[13], -S[23]},        {z, z, z, S[2], S[4], S[5], -S[14], -S[15], -S[24]},
                   {-S[6], -S[7], -S[9], -S[11], -S[12], -S[14], S[16], S[17], S[25]}, {-S[7], -S[8], -S[10], -S[12], -S[13], -S[15], S[17], S[18], S[26]}};
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

// One refit on the correspondences `mask` marks: conditioning, linear start, Gauss-Newton steps, back to pixels, divided by h22. Uniform
// over the workgroup (every thread holds the same sums and solves the same systems). false: the round failed.
// h8 = 1 can be fixed in conditioned coordinates: the test that made the mask requires d > 0 on every inlier, d is affine in (xa, ya), so
// it is positive on the inliers' convex hull, which holds their centroid — the origin of the conditioned frame, where d = h8. A model
// that explains the inliers therefore has h8 > 0 there and can be scaled to h8 = 1.
__device__ __forceinline__ bool refit_round(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, float (&o)[9], Shared &sh)
{
  uint32_t m = 0u;
  for (uint32_t k = threadIdx.x; k < n; k += kThreads)
    m += mask[k] == 1u ? 1u : 0u;
  m = block_u32<false>(m, sh.upart);
  if (m < 4u)
    return false;
  Side A, B;
  if (!condition_sides(c, n, mask, m, A, B, sh))
    return false;
  float S[kSums], h[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dlt[8];
  accumulate<true>(c, n, mask, A, B, h, S, sh);
  if (!solve8(S, h))
    return false;
  for (int step = 0; step < kGaussNewtonSteps; step++)
  {
    accumulate<false>(c, n, mask, A, B, h, S, sh);
    if (!solve8(S, dlt))
      return false;
#pragma unroll
    for (int i = 0; i < 8; i++)
      h[i] = h[i] + dlt[i];
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 8; i++)
    ok = ok && finite_bits(h[i]);
  if (!ok)
    return false;
  // H = Tb^-1 Hc Ta, Ta = [s 0 -s cx; 0 s -s cy; 0 0 1] of side A, Tb^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1] of side B
  const float hc[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0f};
  const float ua = A.s * A.cx, va = A.s * A.cy, isb = 1.0f / B.s;
  float g[9], H[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    g[3 * r] = hc[3 * r] * A.s, g[3 * r + 1] = hc[3 * r + 1] * A.s;
    g[3 * r + 2] = (hc[3 * r + 2] - hc[3 * r] * ua) - hc[3 * r + 1] * va;
  }
#pragma unroll
  for (int col = 0; col < 3; col++)
  {
    H[col] = g[col] * isb + B.cx * g[6 + col];
    H[3 + col] = g[3 + col] * isb + B.cy * g[6 + col];
    H[6 + col] = g[6 + col];
  }
  ok = H[8] != 0.f;
#pragma unroll
  for (int i = 0; i < 9; i++)
    o[i] = H[i] / H[8], ok = ok && finite_bits(o[i]);
  return ok;
}

__device__ __forceinline__ bool admits(const float (&M)[9], float4 q, float t2)
{
  return admissible<kKind>(side_a<kKind>(M, float2{q.x, q.y}, t2), side_b<kKind>(M, float2{q.z, q.w}), t2);
}

// start_masks and masks_out are not __restrict__: from the second round on the mask read is the one the round before wrote, in this
// workgroup (a barrier lies between the stores and the loads).
__global__ void __launch_bounds__(256) k_refit_h(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev, uint32_t n_stride,
                                                 uint32_t max_n, const uint32_t *__restrict__ start_results, const uint8_t *start_masks,
                                                 uint64_t mask_slot_stride, uint32_t nb_rounds, float t2, uint32_t *__restrict__ results, uint8_t *masks_out)
{
  __shared__ Shared sh;
  const uint32_t slot = blockIdx.x, tid = threadIdx.x;
  uint32_t n = n_dev[(size_t)slot * n_stride];
  n = n < max_n ? n : max_n;
  const float4 *c = corr + (size_t)slot * corr_slot_stride;
  const uint8_t *start = start_masks + (size_t)slot * mask_slot_stride;
  uint8_t *out = masks_out + (size_t)slot * mask_slot_stride;
  const uint32_t *sr = start_results + (size_t)slot * kResultWords;
  uint32_t *res = results + (size_t)slot * kResultWords;
  if (sr[kResultWords - 1u] == 0u) // uniform: nothing was verified for this slot
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
    if (!refit_round(c, n, cur, o, sh)) // uniform
      break;
    uint32_t cnt = 0u;
    for (uint32_t k = tid; k < n; k += kThreads)
      cnt += admits(o, c[k], t2) ? 1u : 0u;
    cnt = block_u32<false>(cnt, sh.upart);
    if (cnt < kept_cnt)
      break;
    // accepted: every thread is past its last read of `cur` (the barriers of the reductions); the new mask replaces it in place
    for (uint32_t k = tid; k < n; k += kThreads)
      out[k] = admits(o, c[k], t2) ? 1u : 0u;
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

} // namespace

extern "C"
{
  int vksift_hip_refit_homography(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                  const uint8_t *start_results, const uint8_t *start_masks, uint64_t mask_slot_stride, uint32_t nb_rounds, float threshold_px,
                                  uint8_t *results, uint8_t *masks_out, vksift_hip_stream s)
  {
    // the squared threshold in pixels, formed like guided matching forms it: the verification's (threshold_px 2^-13)^2 brought back by 2^26
    const float ts = threshold_px * (1.0f / 8192.0f), t2 = (ts * ts) * 67108864.0f;
    if (nslots < 1 || nb_rounds == 0 || nb_rounds > kMaxRounds || !(threshold_px > 0.f) || !isfinite(threshold_px) || !(t2 > 0.f) || !isfinite(t2) ||
        (corr_slot_stride & 15u) || ((uintptr_t)corr & 15u) || ((uintptr_t)results & 3u) || ((uintptr_t)start_results & 3u) ||
        (nslots > 1 && (corr_slot_stride < 16u * (uint64_t)max_n || mask_slot_stride < max_n)))
      return (int)hipErrorInvalidValue;
    // the output masks may not overlap the start masks: a slot whose first round is not accepted reports its start mask
    const uint64_t extent = (uint64_t)(nslots - 1u) * mask_slot_stride + max_n;
    const uintptr_t a = (uintptr_t)start_masks, b = (uintptr_t)masks_out;
    if (a == b || (a < b ? b - a < extent : a - b < extent))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refit_h, dim3(nslots), dim3(kThreads), 0, (hipStream_t)s, (const float4 *)corr, corr_slot_stride / 16u, n_dev, n_stride, max_n,
                       (const uint32_t *)start_results, start_masks, mask_slot_stride, nb_rounds, t2, (uint32_t *)results, masks_out);
    return (int)hipGetLastError();
  }
}
