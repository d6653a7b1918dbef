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
// Model-free and shared with the refit of the fundamental matrix (refine_f.hip): the reductions, the conditioning, the elimination of the
// 8x9 system, the chain of rounds and the launcher's refusals (hip/refit.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/refit.h"
#include "hip/two_view.h"

namespace
{

using namespace refit;

constexpr int kGaussNewtonSteps = 2; // one step after the linear start reaches 4 digits of the cost; not a knob
constexpr int kSums = 27;            // distinct sums of the 8x8 normal equations and their right-hand side
constexpr uint32_t kStartWords = 13u; // the RANSAC record {H[9], nb_matches, nb_inliers, best_hypothesis, valid}
constexpr int kKind = (int)VKSIFT_HIP_GUIDE_HOMOGRAPHY;

using SharedH = refit::Shared<kSums>;

// The 27 sums of the rows [a b i 0 0 0 -pu a -pu b | -ru], [0 0 0 a b i -pv a -pv b | -rv] over the inliers. LINEAR: the linear start
// (a, b, i, pu, pv, ru, rv) = (x, y, 1, X, Y, -X, -Y) in conditioned coordinates; otherwise the Gauss-Newton step at h, the Jacobian
// rows of the forward transfer error (u / d - X, v / d - Y).
template <bool LINEAR>
__device__ __forceinline__ void accumulate(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, const Side &A, const Side &B, const float (&h)[8],
                                           float (&S)[kSums], SharedH &sh)
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

// The 8x9 normal equations of the sums, eliminated by refit::solve8
__device__ __forceinline__ bool solve_sums(const float (&S)[kSums], float (&x)[8])
{
  const float z = 0.f;
  float a[8][9] = {{S[0], S[1], S[2], z, z, z, -S[6], -S[7], -S[19]},          {S[1], S[3], S[4], z, z, z, -S[7], -S[8], -S[20]},
                   {S[2], S[4], S[5], z, z, z, -S[9], -S[10], -S[21]},         {z, z, z, S[0], S[1], S[2], -S[11], -S[12], -S[22]},
                   {z, z, z, S[1], S[3], S[4], -S[12], -S[13], -S[23]},        {z, z, z, S[2], S[4], S[5], -S[14], -S[15], -S[24]},
                   {-S[6], -S[7], -S[9], -S[11], -S[12], -S[14], S[16], S[17], S[25]}, {-S[7], -S[8], -S[10], -S[12], -S[13], -S[15], S[17], S[18], S[26]}};
  return solve8(a, x);
}

// One refit on the correspondences `mask` marks: conditioning, linear start, Gauss-Newton steps, back to pixels, divided by h22. Uniform
// over the workgroup (every thread holds the same sums and solves the same systems). false: the round failed.
// h8 = 1 can be fixed in conditioned coordinates: the test that made the mask requires d > 0 on every inlier, d is affine in (xa, ya), so
// it is positive on the inliers' convex hull, which holds their centroid — the origin of the conditioned frame, where d = h8. A model
// that explains the inliers therefore has h8 > 0 there and can be scaled to h8 = 1.
__device__ __forceinline__ bool refit_round(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, float (&o)[9], SharedH &sh)
{
  const uint32_t m = count_marked(n, mask, sh);
  if (m < 4u)
    return false;
  Side A, B;
  if (!condition_sides(c, n, mask, m, A, B, sh))
    return false;
  float S[kSums], h[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dlt[8];
  accumulate<true>(c, n, mask, A, B, h, S, sh);
  if (!solve_sums(S, h))
    return false;
  for (int step = 0; step < kGaussNewtonSteps; step++)
  {
    accumulate<false>(c, n, mask, A, B, h, S, sh);
    if (!solve_sums(S, dlt))
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

__global__ void __launch_bounds__(256) k_refit_h(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev, uint32_t n_stride,
                                                 uint32_t max_n, const uint32_t *__restrict__ start_results, const uint8_t *start_masks,
                                                 uint64_t mask_slot_stride, uint32_t nb_rounds, float t2, uint32_t *__restrict__ results, uint8_t *masks_out)
{
  __shared__ SharedH sh;
  refit_chain<kKind, kStartWords>(corr, corr_slot_stride, n_dev, n_stride, max_n, start_results, start_masks, mask_slot_stride, nb_rounds, t2, results, masks_out, sh,
                                  [](const float4 *c, uint32_t n, const uint8_t *mask, const float (&)[9], float (&o)[9], SharedH &s) { return refit_round(c, n, mask, o, s); });
}

} // namespace

extern "C"
{
  int vksift_hip_refit_homography(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                  const uint8_t *start_results, const uint8_t *start_masks, uint64_t mask_slot_stride, uint32_t nb_rounds, float threshold_px,
                                  uint8_t *results, uint8_t *masks_out, vksift_hip_stream s)
  {
    float t2;
    if (!launch_admitted(corr, corr_slot_stride, max_n, nslots, start_results, start_masks, mask_slot_stride, nb_rounds, threshold_px, results, masks_out, t2))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refit_h, dim3(nslots), dim3(kThreads), 0, (hipStream_t)s, (const float4 *)corr, corr_slot_stride / 16u, n_dev, n_stride, max_n,
                       (const uint32_t *)start_results, start_masks, mask_slot_stride, nb_rounds, t2, (uint32_t *)results, masks_out);
    return (int)hipGetLastError();
  }
}
