// refine_f.hip — locally optimised refit of the verified fundamental matrices on their inliers, the counterpart of refine.hip (no counterpart
// in the reference, whose callers refit on the CPU after downloading matches, features and masks). One launch serves every pair (slot) of a call,
// one workgroup of 256 threads per slot, all rounds inside it (refit::refit_chain, hip/refit.h):
//   round   a least-squares fundamental matrix on the correspondences the current mask marks: conditioning, the gauge f_j = 1 at the largest
//           entry of the model the round starts from, a linear start, two steps reweighted by the Sampson denominator of the step before, two
//           Newton steps on the determinant (rank 2 without an SVD), published in pixel coordinates with the largest |entry| in [1, 2), and all n
//           correspondences re-scored under it with two_view.h's test on the published model (exactly what guided matching would admit)
// Everything is integer arithmetic or correctly rounded fp32 add / sub / mul / div in a fixed order, every sum over correspondences in the one
// order of hip/refit.h. tests/np_refine_f.py is the specification of the operation order and restates every output bit for bit.
// Not attempted: no chirality test, no handling of the planar degeneracy (coplanar inliers give a near-singular system; whatever model comes
// out is subject to the acceptance rule like any other).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/refit.h"

namespace
{

using namespace refit;

constexpr int kReweightedSteps = 2; // a constant like refine.hip's kGaussNewtonSteps; not a knob
constexpr int kProjectionSteps = 2; // Newton steps on det F
constexpr int kSums = 44;           // the 36 distinct sums of the 8x8 normal equations and the 8 of their right-hand side
constexpr uint32_t kMinMatches = 8u;
constexpr uint32_t kStartWords = 14u; // the RANSAC record {F[9], nb_matches, nb_inliers, best_hypothesis, best_root, valid}
constexpr int kKind = (int)VKSIFT_HIP_GUIDE_FUNDAMENTAL;

using SharedF = refit::Shared<kSums>;

// where the sum of b_i b_p, i <= p < 8, stands among the first 36: row by row of the upper triangle
constexpr int tri(int i, int p) { return i * 8 - i * (i - 1) / 2 + (p - i); }
static_assert(tri(0, 0) == 0 && tri(1, 1) == 8 && tri(7, 7) == 35, "the upper triangle of 8x8, row-major");

// The kept model (pixels) in the conditioned frame, Fc = Tb^-T F Ta^-1 with Ta^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1], and the index of its largest
// |entry| by bit pattern, ties to the lowest
__device__ __forceinline__ int gauge_index(const float (&F)[9], const Side &A, const Side &B)
{
  const float isa = 1.0f / A.s, isb = 1.0f / B.s;
  float g[9], fc[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    g[3 * r] = F[3 * r] * isa, g[3 * r + 1] = F[3 * r + 1] * isa;
    g[3 * r + 2] = (F[3 * r] * A.cx + F[3 * r + 1] * A.cy) + F[3 * r + 2];
  }
#pragma unroll
  for (int col = 0; col < 3; col++)
  {
    fc[col] = g[col] * isb, fc[3 + col] = g[3 + col] * isb;
    fc[6 + col] = (B.cx * g[col] + B.cy * g[3 + col]) + g[6 + col];
  }
  int j = 0;
  uint32_t best = abs_bits(fc[0]);
#pragma unroll
  for (int i = 1; i < 9; i++)
  {
    const bool up = abs_bits(fc[i]) > best;
    j = up ? i : j, best = up ? abs_bits(fc[i]) : best;
  }
  return j;
}

// The eight free entries f with 1 put back at j: selects between compile-time indices, no run-time register index
__device__ __forceinline__ void with_one(const float (&f)[8], int j, float (&fc)[9])
{
#pragma unroll
  for (int i = 0; i < 9; i++)
  {
    const float below = f[i < 8 ? i : 7], above = f[i > 0 ? i - 1 : 0];
    fc[i] = i < j ? below : i == j ? 1.0f : above;
  }
}

// The 44 sums of w b_i b_k over the inliers: b the nine monomials (X x, X y, X, Y x, Y y, Y, x, y, 1) of the conditioned coordinates with
// monomial j moved to the last place. WEIGHTED: w = 1 / g with the Sampson denominator g of the model fc (the factor rho = (sb / sa)^2 brings
// the two normals to one unit); otherwise w = 1. false (WEIGHTED only): g is zero, subnormal or not finite on an inlier.
template <bool WEIGHTED>
__device__ __forceinline__ bool accumulate(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, const Side &A, const Side &B, int j, const float (&fc)[9],
                                           float rho, float (&S)[kSums], SharedF &sh)
{
#pragma unroll
  for (int i = 0; i < kSums; i++)
    S[i] = 0.f;
  uint32_t bad = 0u;
  for (uint32_t k = threadIdx.x; k < n; k += kThreads)
  {
    const bool in = mask[k] == 1u;
    const float4 q = c[k];
    const float x = (q.x - A.cx) * A.s, y = (q.y - A.cy) * A.s, X = (q.z - B.cx) * B.s, Y = (q.w - B.cy) * B.s;
    const float a[9] = {X * x, X * y, X, Y * x, Y * y, Y, x, y, 1.0f};
    float b[9];
#pragma unroll
    for (int i = 0; i < 8; i++)
      b[i] = i < j ? a[i] : a[i + 1];
    b[8] = a[0];
#pragma unroll
    for (int i = 1; i < 9; i++)
      b[8] = j == i ? a[i] : b[8];
    float w = 1.0f;
    if (WEIGHTED)
    {
      const float l0 = (fc[0] * x + fc[1] * y) + fc[2];
      const float l1 = (fc[3] * x + fc[4] * y) + fc[5];
      const float m0 = (fc[0] * X + fc[3] * Y) + fc[6];
      const float m1 = (fc[1] * X + fc[4] * Y) + fc[7];
      const float g = rho * (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1);
      bad |= in && unusable_bits(g) ? 1u : 0u;
      w = 1.0f / g;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
    {
      const float wb = w * b[i];
#pragma unroll
      for (int p = i; p < 8; p++)
      {
        const float t = wb * b[p];
        S[tri(i, p)] = S[tri(i, p)] + (in ? t : 0.f); // an element outside the mask adds +0: no bit changes (a partial sum that starts at +0 is never -0)
      }
      const float t = wb * b[8];
      S[36 + i] = S[36 + i] + (in ? t : 0.f);
    }
  }
  block_sum<kSums>(S, sh.part);
  if (WEIGHTED)
    bad = block_u32<true>(bad, sh.upart);
  return bad == 0u;
}

// The 8x9 normal equations of the sums (the matrix is symmetric, the right-hand side minus the last eight sums), eliminated by refit::solve8
__device__ __forceinline__ bool solve_sums(const float (&S)[kSums], float (&x)[8])
{
  float a[8][9];
#pragma unroll
  for (int i = 0; i < 8; i++)
  {
#pragma unroll
    for (int p = i; p < 8; p++)
      a[i][p] = S[tri(i, p)], a[p][i] = S[tri(i, p)];
    a[i][8] = -S[36 + i];
  }
  return solve8(a, x);
}

// Newton steps on det F along its gradient, the cofactor matrix C: F <- F - (det F / |C|^2) C, the minimal-norm first-order correction onto
// det = 0. No square root, no branch. false: |C|^2 is zero, subnormal or not finite.
__device__ __forceinline__ bool project_rank2(float (&F)[9])
{
  bool ok = true;
#pragma unroll
  for (int step = 0; step < kProjectionSteps; step++)
  {
    const float C[9] = {F[4] * F[8] - F[5] * F[7], F[5] * F[6] - F[3] * F[8], F[3] * F[7] - F[4] * F[6],
                        F[2] * F[7] - F[1] * F[8], F[0] * F[8] - F[2] * F[6], F[1] * F[6] - F[0] * F[7],
                        F[1] * F[5] - F[2] * F[4], F[2] * F[3] - F[0] * F[5], F[0] * F[4] - F[1] * F[3]};
    const float det = (F[0] * C[0] + F[1] * C[1]) + F[2] * C[2];
    float nrm = C[0] * C[0];
#pragma unroll
    for (int i = 1; i < 9; i++)
      nrm = nrm + C[i] * C[i];
    ok = ok && !unusable_bits(nrm);
    const float t = det / nrm;
#pragma unroll
    for (int i = 0; i < 9; i++)
      F[i] = F[i] - t * C[i];
  }
  return ok;
}

// One refit on the correspondences `mask` marks, from the model `kept`. Uniform over the workgroup (every thread holds the same sums and solves
// the same systems). false: the round failed.
__device__ __forceinline__ bool refit_round(const float4 *__restrict__ c, uint32_t n, const uint8_t *mask, const float (&kept)[9], float (&o)[9], SharedF &sh)
{
  const uint32_t m = count_marked(n, mask, sh);
  if (m < kMinMatches)
    return false;
  Side A, B;
  if (!condition_sides(c, n, mask, m, A, B, sh))
    return false;
  const int j = gauge_index(kept, A, B);
  const float q = B.s / A.s, rho = q * q; // an exact power of two
  float S[kSums], f[8], fc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  accumulate<false>(c, n, mask, A, B, j, fc, rho, S, sh);
  if (!solve_sums(S, f))
    return false;
  for (int step = 0; step < kReweightedSteps; step++)
  {
    with_one(f, j, fc);
    if (!accumulate<true>(c, n, mask, A, B, j, fc, rho, S, sh))
      return false;
    if (!solve_sums(S, f))
      return false;
  }
  with_one(f, j, fc);
  if (!project_rank2(fc))
    return false;
  // F = Tb^T Fc Ta, Ta = [s 0 -s cx; 0 s -s cy; 0 0 1] (verify.hip's solve_f7 goes back the same way)
  const float ua = A.s * A.cx, va = A.s * A.cy, ub = B.s * B.cx, vb = B.s * B.cy;
  float g[9], F[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    g[3 * r] = fc[3 * r] * A.s, g[3 * r + 1] = fc[3 * r + 1] * A.s;
    g[3 * r + 2] = (fc[3 * r + 2] - fc[3 * r] * ua) - fc[3 * r + 1] * va;
  }
  uint32_t mbits = 0u;
#pragma unroll
  for (int col = 0; col < 3; col++)
  {
    F[col] = B.s * g[col], F[3 + col] = B.s * g[3 + col];
    F[6 + col] = (g[6 + col] - ub * g[col]) - vb * g[3 + col];
  }
#pragma unroll
  for (int i = 0; i < 9; i++)
    mbits = max(mbits, abs_bits(F[i]));
  bool ok;
  const float unit = unit_scale(mbits, ok); // not ok: all zero, subnormal, or an entry that is not finite (a NaN's bits are above every number's)
#pragma unroll
  for (int i = 0; i < 9; i++)
    o[i] = F[i] * unit;
  return ok;
}

__global__ void __launch_bounds__(256) k_refit_f(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev, uint32_t n_stride,
                                                 uint32_t max_n, const uint32_t *__restrict__ start_results, const uint8_t *start_masks,
                                                 uint64_t mask_slot_stride, uint32_t nb_rounds, float t2, uint32_t *__restrict__ results, uint8_t *masks_out)
{
  __shared__ SharedF sh;
  refit_chain<kKind, kStartWords>(corr, corr_slot_stride, n_dev, n_stride, max_n, start_results, start_masks, mask_slot_stride, nb_rounds, t2, results, masks_out, sh,
                                  [](const float4 *c, uint32_t n, const uint8_t *mask, const float (&kept)[9], float (&o)[9], SharedF &s)
                                  { return refit_round(c, n, mask, kept, o, s); });
}

} // namespace

extern "C"
{
  int vksift_hip_refit_fundamental(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                   const uint8_t *start_results, const uint8_t *start_masks, uint64_t mask_slot_stride, uint32_t nb_rounds, float threshold_px,
                                   uint8_t *results, uint8_t *masks_out, vksift_hip_stream s)
  {
    float t2;
    if (!launch_admitted(corr, corr_slot_stride, max_n, nslots, start_results, start_masks, mask_slot_stride, nb_rounds, threshold_px, results, masks_out, t2))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refit_f, dim3(nslots), dim3(kThreads), 0, (hipStream_t)s, (const float4 *)corr, corr_slot_stride / 16u, n_dev, n_stride, max_n,
                       (const uint32_t *)start_results, start_masks, mask_slot_stride, nb_rounds, t2, (uint32_t *)results, masks_out);
    return (int)hipGetLastError();
  }
}
