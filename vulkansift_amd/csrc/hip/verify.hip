// verify.hip — geometric verification of filtered matches: batched, deterministic RANSAC estimators of a homography and of a fundamental
// matrix (no counterpart in the reference, whose callers run a CPU RANSAC after downloading matches and features; the reference's own
// evaluation judges matches by a homography, src/perf/perf_matching.cpp:30-79). Three launches serve every pair (slot) of a call:
//   k_gather_corr      filtered matches {idx_a, idx_b} (download-order rows) -> {xa, ya, xb, yb} read from the SIFT buffers' sections
//                      (layout decode and walk: records.h)
//   k_ransac_score_*   one lane per hypothesis: counter-based sample, closed-form models, inlier counts over the slot's correspondences
//                      staged through LDS (broadcast 16-byte reads), best (count, lowest model id) per workgroup
//   k_ransac_final_*   best model per slot, recomputed and brought to pixel coordinates, the inlier mask (same test: popcount == count)
// _h is the homography (four-point samples, one model per lane), _f the fundamental matrix (seven-point samples, up to three). Both are one
// body, ransac_score<Model> / ransac_final<Model>: a model (ModelH, ModelF) is its sizes, its solver and how its winner is published; the
// inlier test is two_view.h's, the gather, the sampler, the key reduction and the launch wrapper are model-free.
// Everything is integer arithmetic or correctly rounded fp32 add / sub / mul / div / sqrt in a fixed order (the tree is built with
// -ffp-contract=off and no fmaf is used here), so tests/np_verify.py and tests/np_verify_f.py restate it bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/records.h"
#include "hip/two_view.h"

namespace
{

constexpr uint32_t kHypPerBlock = 256u; // lanes (= hypotheses) per workgroup of the scoring kernel, and correspondences per LDS tile
// Coordinates enter the solve scaled by 2^-13 (exact): the entries of the un-normalised homography are polynomials of degree 9 in the
// coordinates, 16383^9 would not fit fp32. Powers of two change no rounding, so the result is that of the unscaled computation.
constexpr float kCoordScale = 1.0f / 8192.0f;
constexpr float kCoordUnscale = 8192.0f;

// a model of either kind, row-major (wrapped in a struct: as a bare float[9] it costs k_ransac_final_h 12 VGPRs, NOTEBOOK.md section 15)
struct Mat9
{
  float f[9];
};

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// 2^(127 - e) for the exponent e of the largest magnitude `mbits`; ok: that magnitude is normal and below 2^127
__device__ __forceinline__ float unit_scale(uint32_t mbits, bool &ok)
{
  const uint32_t e = mbits >> 23;
  ok = e >= 1u && e <= 253u;
  return __uint_as_float((254u - (ok ? e : 127u)) << 23);
}

__device__ __forceinline__ uint64_t splitmix64_next(uint64_t &state)
{
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t draw_below(uint64_t &state, uint32_t m) { return (uint32_t)(((splitmix64_next(state) >> 32) * (uint64_t)m) >> 32); }

// K distinct indices below n (n >= K), in draw order: draw j is uniform over the n - j indices left and stepped over the ones already
// drawn in increasing order (kept sorted in `sorted`, compile-time indices only). seed_key = the first splitmix64 output of the state `seed`.
template <int K> __device__ __forceinline__ void draw_sample(uint64_t seed_key, uint32_t slot, uint32_t hyp, uint32_t n, uint32_t (&idx)[K])
{
  uint64_t st = seed_key ^ (((uint64_t)slot << 32) | (uint64_t)hyp);
  uint32_t sorted[K];
#pragma unroll
  for (int j = 0; j < K; j++)
  {
    uint32_t r = draw_below(st, n - (uint32_t)j);
#pragma unroll
    for (int q = 0; q < j; q++)
      r += r >= sorted[q] ? 1u : 0u;
    idx[j] = r;
    uint32_t v = r;
#pragma unroll
    for (int q = 0; q < j; q++)
    {
      const uint32_t lo = sorted[q] < v ? sorted[q] : v, hi = sorted[q] < v ? v : sorted[q];
      sorted[q] = lo, v = hi;
    }
    sorted[j] = v;
  }
}

__device__ __forceinline__ float4 scaled(float4 c) { return float4{c.x * kCoordScale, c.y * kCoordScale, c.z * kCoordScale, c.w * kCoordScale}; }

// Homography through four correspondences c_i = {xa, ya, xb, yb} (scaled), projective-basis form: with p_i = (xa_i, ya_i, 1),
// lambda = adj([p0 p1 p2]) p3 and A = [lambda_i p_i] (likewise mu, B for the q_i = (xb_i, yb_i, 1)), H = B adj(A); the rows of
// adj(A) are lambda_j lambda_k (p_j x p_k), so the cross products are formed once. The result is scaled by the power of two that
// brings its largest entry into [1, 2) (exact), negated if it maps the first sample point behind the plane; a sample whose largest entry is zero, subnormal, at or above 2^127, infinite or NaN
// is degenerate and becomes all-NaN (no correspondence is an inlier of it).
__device__ __forceinline__ void solve_h4(float4 c0, float4 c1, float4 c2, float4 c3, float (&H)[9])
{
  // source side: rows of adj([p0 p1 p2]) and lambda
  const float ax = c1.y - c2.y, ay = c2.x - c1.x, az = c1.x * c2.y - c2.x * c1.y; // p1 x p2
  const float bx = c2.y - c0.y, by = c0.x - c2.x, bz = c2.x * c0.y - c0.x * c2.y; // p2 x p0
  const float gx = c0.y - c1.y, gy = c1.x - c0.x, gz = c0.x * c1.y - c1.x * c0.y; // p0 x p1
  const float l0 = (ax * c3.x + ay * c3.y) + az;
  const float l1 = (bx * c3.x + by * c3.y) + bz;
  const float l2 = (gx * c3.x + gy * c3.y) + gz;
  // destination side: mu only
  const float m0 = ((c1.w - c2.w) * c3.z + (c2.z - c1.z) * c3.w) + (c1.z * c2.w - c2.z * c1.w);
  const float m1 = ((c2.w - c0.w) * c3.z + (c0.z - c2.z) * c3.w) + (c2.z * c0.w - c0.z * c2.w);
  const float m2 = ((c0.w - c1.w) * c3.z + (c1.z - c0.z) * c3.w) + (c0.z * c1.w - c1.z * c0.w);
  const float w0 = m0 * (l1 * l2), w1 = m1 * (l2 * l0), w2 = m2 * (l0 * l1);
  const float u0 = w0 * c0.z, u1 = w1 * c1.z, u2 = w2 * c2.z; // row 0 of B, times the weights of adj(A)'s rows
  const float v0 = w0 * c0.w, v1 = w1 * c1.w, v2 = w2 * c2.w; // row 1
  H[0] = (u0 * ax + u1 * bx) + u2 * gx;
  H[1] = (u0 * ay + u1 * by) + u2 * gy;
  H[2] = (u0 * az + u1 * bz) + u2 * gz;
  H[3] = (v0 * ax + v1 * bx) + v2 * gx;
  H[4] = (v0 * ay + v1 * by) + v2 * gy;
  H[5] = (v0 * az + v1 * bz) + v2 * gz;
  H[6] = (w0 * ax + w1 * bx) + w2 * gx;
  H[7] = (w0 * ay + w1 * by) + w2 * gy;
  H[8] = (w0 * az + w1 * bz) + w2 * gz;
  uint32_t m = 0u; // largest magnitude by its bit pattern (NaN and infinity sort above every finite value)
#pragma unroll
  for (int i = 0; i < 9; i++)
    m = max(m, abs_bits(H[i]));
  bool ok;
  const float fa = unit_scale(m, ok);
  // the sign of B adj(A) follows the orientation of the sample: chosen so that the first sample point lies in front of the plane (d > 0)
  const float d0 = (H[6] * c0.x + H[7] * c0.y) + H[8];
  const float f = d0 < 0.f ? -fa : fa;
#pragma unroll
  for (int i = 0; i < 9; i++)
    H[i] = ok ? H[i] * f : __uint_as_float(0x7fc00000u);
}

// What ransac_score / ransac_final need of a model: sample size, models per lane (a model's id is hypothesis << kRootBits | root; ids order
// the ties), fewest inliers of a valid result, words of the result record ({M[9], nb_matches, nb_inliers, best_hypothesis, [best_root,]
// valid}), the unroll factor of the scoring loop, solve (the models of hypothesis hyp's sample, absent ones all-NaN; returns how many
// there are) and publish (the winner in pixel coordinates, and whether it can be given out).
struct ModelH
{
  static constexpr int kKind = (int)VKSIFT_HIP_GUIDE_HOMOGRAPHY;
  static constexpr uint32_t kSample = 4u, kModels = 1u, kRootBits = 0u, kMinInliers = 4u, kResultWords = 13u, kUnroll = 4u;

  static __device__ __forceinline__ uint32_t solve(const float4 *__restrict__ c, uint64_t seed_key, uint32_t slot, uint32_t hyp, uint32_t n, Mat9 (&M)[1])
  {
    uint32_t i4[4];
    draw_sample<4>(seed_key, slot, hyp, n, i4);
    solve_h4(scaled(c[i4[0]]), scaled(c[i4[1]]), scaled(c[i4[2]]), scaled(c[i4[3]]), M[0].f);
    return 1u;
  }

  // back to pixel coordinates (powers of two) and divided by h22
  static __device__ __forceinline__ void publish(const float (&H)[9], float (&o)[9], bool &valid)
  {
    const float p2 = H[2] * kCoordUnscale, p5 = H[5] * kCoordUnscale, p6 = H[6] * kCoordScale, p7 = H[7] * kCoordScale;
    o[0] = H[0] / H[8], o[1] = H[1] / H[8], o[2] = p2 / H[8];
    o[3] = H[3] / H[8], o[4] = H[4] / H[8], o[5] = p5 / H[8];
    o[6] = p6 / H[8], o[7] = p7 / H[8], o[8] = H[8] / H[8];
    valid = H[8] != 0.f;
#pragma unroll
    for (int i = 0; i < 9; i++)
      valid = valid && ((__float_as_uint(o[i]) & 0x7f800000u) != 0x7f800000u);
  }
};

template <class Model> __device__ __forceinline__ bool is_inlier(const float (&M)[9], float4 c, float t2)
{
  return admissible<Model::kKind>(side_a<Model::kKind>(M, float2{c.x, c.y}, t2), side_b<Model::kKind>(M, float2{c.z, c.w}), t2);
}

// the largest key of a 256-thread workgroup, in every thread
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long k, unsigned long long (&wave_best)[4])
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
  {
    const unsigned long long o = __shfl_xor(k, off, 64);
    k = o > k ? o : k;
  }
  if ((threadIdx.x & 63u) == 0u)
    wave_best[threadIdx.x >> 6] = k;
  __syncthreads();
  k = wave_best[0];
  for (int w = 1; w < 4; w++)
    k = wave_best[w] > k ? wave_best[w] : k;
  return k;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per slot. slot_tab: {buffer A, buffer B, layout A, layout B} per slot, layouts: the section tables (records.h). A match
// that names a row the buffer does not hold yields a NaN correspondence (never an inlier); nothing is read out of bounds.
__global__ void __launch_bounds__(256) k_gather_corr(const uint8_t *__restrict__ feats_base, uint64_t buf_stride, const uint32_t *__restrict__ found_base,
                                                     uint32_t found_buf_stride, const uint32_t *__restrict__ slot_tab, const uint32_t *__restrict__ layouts,
                                                     const uint32_t *__restrict__ filtered, uint64_t filtered_slot_stride, const uint32_t *__restrict__ filtered_n,
                                                     uint32_t max_n, float4 *__restrict__ corr, uint64_t corr_slot_stride)
{
  __shared__ SideLayout L[2];
  const uint32_t slot = blockIdx.x;
  layout_decode(L, slot_tab + (size_t)slot * 4u, 0u, layouts, found_base, found_buf_stride);
  uint32_t n = filtered_n[slot];
  n = n < max_n ? n : max_n;
  const uint32_t *fm = filtered + (size_t)slot * filtered_slot_stride;
  float4 *out = corr + (size_t)slot * corr_slot_stride;
  const float bad = __uint_as_float(0x7fc00000u);
  for (uint32_t k = threadIdx.x; k < n; k += 256u)
  {
    float xy[4] = {bad, bad, bad, bad};
#pragma unroll
    for (uint32_t side = 0; side < 2u; side++)
    {
      const uint32_t row = fm[(size_t)k * 4u + side];
      if (row < L[side].total)
      {
        const float *f = (const float *)(feats_base + (size_t)L[side].buf * buf_stride + (size_t)section_row(L[side].cnt, L[side].off, row) * VKSIFT_RECORD_BYTES);
        xy[2u * side] = f[0], xy[2u * side + 1u] = f[1];
      }
    }
    out[k] = float4{xy[0], xy[1], xy[2], xy[3]};
  }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
// Workgroup (slot, blk) scores hypotheses blk*256 .. blk*256+255 of its slot against all n correspondences and stores the largest
// key (count << 32 | ~model id) — most inliers, ties to the lowest id — as two words at keys[2 * (slot * nblk + blk)]. With several
// models per lane, roots 1 and 2 are scored only when some lane of the wave has them (a wave-uniform branch; an absent root is all-NaN
// and counts nothing).
template <class Model>
__device__ __forceinline__ void ransac_score(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev, uint32_t n_stride,
                                             uint32_t max_n, uint32_t nb_hyp, uint32_t nblk, float t2, uint64_t seed_key, uint32_t *__restrict__ keys)
{
  __shared__ float4 tile[kHypPerBlock];
  __shared__ unsigned long long wave_best[4];
  const uint32_t slot = blockIdx.x / nblk, blk = blockIdx.x - slot * nblk;
  const uint32_t tid = threadIdx.x;
  uint32_t n = n_dev[(size_t)slot * n_stride];
  n = n < max_n ? n : max_n;
  uint32_t *kout = keys + 2u * (size_t)blockIdx.x;
  if (n < Model::kSample)
  {
    if (tid == 0)
      kout[0] = 0u, kout[1] = 0u;
    return;
  }
  const float4 *c = corr + (size_t)slot * corr_slot_stride;
  const uint32_t hyp = blk * kHypPerBlock + tid;
  const bool active = hyp < nb_hyp;
  Mat9 M[Model::kModels];
  const uint32_t nroots = Model::solve(c, seed_key, slot, active ? hyp : 0u, n, M);
  bool any[Model::kModels];
  uint32_t cnt[Model::kModels];
#pragma unroll
  for (uint32_t r = 0; r < Model::kModels; r++)
    any[r] = r == 0u || __ballot(nroots > r) != 0ull, cnt[r] = 0u;
  for (uint32_t base = 0; base < n; base += kHypPerBlock)
  {
    __syncthreads();
    if (base + tid < n)
      tile[tid] = scaled(c[base + tid]);
    __syncthreads();
    const uint32_t m = n - base < kHypPerBlock ? n - base : kHypPerBlock;
#pragma unroll Model::kUnroll
    for (uint32_t j = 0; j < m; j++)
    {
      const float4 q = tile[j]; // every lane reads the same 16 bytes: one broadcast LDS access
#pragma unroll
      for (uint32_t r = 0; r < Model::kModels; r++)
        if (any[r])
          cnt[r] += is_inlier<Model>(M[r].f, q, t2) ? 1u : 0u;
    }
  }
  unsigned long long key = 0ull;
#pragma unroll
  for (uint32_t r = 0; r < Model::kModels; r++)
  {
    const unsigned long long k = ((unsigned long long)cnt[r] << 32) | (unsigned long long)(~((hyp << Model::kRootBits) + r));
    key = k > key ? k : key;
  }
  key = block_max_u64(active ? key : 0ull, wave_best);
  if (tid == 0)
    kout[0] = (uint32_t)key, kout[1] = (uint32_t)(key >> 32);
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per slot: the best key over the slot's nblk workgroups, the winner's model recomputed from its sample and root and
// published; the result record and one mask byte per correspondence.
template <class Model>
__device__ __forceinline__ void ransac_final(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev, uint32_t n_stride,
                                             uint32_t max_n, uint32_t nblk, float t2, uint64_t seed_key, const uint32_t *__restrict__ keys,
                                             uint32_t *__restrict__ results, uint8_t *__restrict__ masks, uint64_t mask_slot_stride)
{
  __shared__ unsigned long long wave_best[4];
  const uint32_t slot = blockIdx.x, tid = threadIdx.x;
  uint32_t n = n_dev[(size_t)slot * n_stride];
  n = n < max_n ? n : max_n;
  unsigned long long key = 0ull;
  for (uint32_t b = tid; b < nblk; b += 256u)
  {
    const uint32_t *k = keys + 2u * ((size_t)slot * nblk + b);
    const unsigned long long v = ((unsigned long long)k[1] << 32) | (unsigned long long)k[0];
    key = v > key ? v : key;
  }
  key = block_max_u64(key, wave_best);
  const uint32_t cnt = (uint32_t)(key >> 32), id = ~(uint32_t)key, hyp = id >> Model::kRootBits, rt = id & ((1u << Model::kRootBits) - 1u);
  const float4 *c = corr + (size_t)slot * corr_slot_stride;
  uint8_t *mask = masks + (size_t)slot * mask_slot_stride;
  uint32_t *res = results + (size_t)slot * Model::kResultWords;
  bool valid = n >= Model::kSample && cnt >= Model::kMinInliers;
  Mat9 W = {};
  float o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (valid) // uniform over the workgroup
  {
    Mat9 M[Model::kModels];
    Model::solve(c, seed_key, slot, hyp, n, M);
#pragma unroll
    for (uint32_t r = 0; r < Model::kModels; r++)
#pragma unroll
      for (int i = 0; i < 9; i++)
        W.f[i] = (r == 0u || rt == r) ? M[r].f[i] : W.f[i];
    Model::publish(W.f, o, valid);
  }
  for (uint32_t k = tid; k < n; k += 256u)
    mask[k] = (valid && is_inlier<Model>(W.f, scaled(c[k]), t2)) ? 1u : 0u;
  if (tid == 0)
  {
#pragma unroll
    for (int i = 0; i < 9; i++)
      res[i] = valid ? __float_as_uint(o[i]) : 0u;
    res[9] = n;
    res[10] = valid ? cnt : 0u;
    res[11] = valid ? hyp : 0u;
    if (Model::kRootBits)
      res[12] = valid ? rt : 0u;
    res[Model::kResultWords - 1u] = valid ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(256) k_ransac_score_h(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev,
                                                        uint32_t n_stride, uint32_t max_n, uint32_t nb_hyp, uint32_t nblk, float t2, uint64_t seed_key,
                                                        uint32_t *__restrict__ keys)
{
  ransac_score<ModelH>(corr, corr_slot_stride, n_dev, n_stride, max_n, nb_hyp, nblk, t2, seed_key, keys);
}

__global__ void __launch_bounds__(256) k_ransac_final_h(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev,
                                                        uint32_t n_stride, uint32_t max_n, uint32_t nblk, float t2, uint64_t seed_key,
                                                        const uint32_t *__restrict__ keys, uint32_t *__restrict__ results, uint8_t *__restrict__ masks,
                                                        uint64_t mask_slot_stride)
{
  ransac_final<ModelH>(corr, corr_slot_stride, n_dev, n_stride, max_n, nblk, t2, seed_key, keys, results, masks, mask_slot_stride);
}

// ---- the second model: fundamental matrix ----------------------------------------------------------------------------------------------
// Seven-point algorithm in fp32, one operation order (tests/np_verify_f.py restates it bit for bit). Per hypothesis up to three models
// (the real roots of a cubic), model id = 4 * hypothesis + root. Not done here: no rank or orientation (chirality) test beyond what the
// seven-point construction gives; no handling of the planar degeneracy (a caller runs both models on the same filtered matching and
// compares the counts); no refit on the inliers.
constexpr int kBisectSteps = 48; // halvings of a bracket no wider than 2 R: to the last bit of a root down to 2^-24 R

// One side of the sample: x, y become s (x - cx), s (y - cy) with the centroid (cx, cy) (fixed-order sum times 1.0f / 7.0f) and the power
// of two s that brings the largest |deviation| into [1, 2); u = s cx, v = s cy. s is NaN (and with it the whole solve) when there is no such power.
__device__ __forceinline__ void condition7(float (&x)[7], float (&y)[7], float &s, float &u, float &v)
{
  const float seventh = 1.0f / 7.0f;
  const float cx = ((((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]) + x[6]) * seventh;
  const float cy = ((((((y[0] + y[1]) + y[2]) + y[3]) + y[4]) + y[5]) + y[6]) * seventh;
  uint32_t m = 0u;
#pragma unroll
  for (int i = 0; i < 7; i++)
  {
    x[i] = x[i] - cx, y[i] = y[i] - cy;
    m = max(m, max(abs_bits(x[i]), abs_bits(y[i])));
  }
  bool ok;
  const float f = unit_scale(m, ok);
  s = ok ? f : __uint_as_float(0x7fc00000u);
#pragma unroll
  for (int i = 0; i < 7; i++)
    x[i] = x[i] * s, y[i] = y[i] * s;
  u = s * cx, v = s * cy;
}

// Real roots of c0 + c1 a + c2 a^2 + c3 a^3 in increasing order into root[0..count), NaN beyond; a fixed number of steps. Degenerate
// (no root): c3 zero or subnormal, a coefficient or the root bound not finite. Else monic b_i = c_i / c3, all roots inside (-R, R) with
// R = 1 + max |b_i| (Cauchy); the critical points lo <= hi of the cubic (equal when it is monotone) split that into three intervals on
// each of which it is monotone; an interval whose end points differ in `p(x) < 0` is bisected kBisectSteps times.
__device__ __forceinline__ uint32_t cubic_roots(float c0, float c1, float c2, float c3, float (&root)[3])
{
  const uint32_t mc = max(max(abs_bits(c0), abs_bits(c1)), max(abs_bits(c2), abs_bits(c3)));
  const float b2 = c2 / c3, b1 = c1 / c3, b0 = c0 / c3;
  const float R = 1.0f + __uint_as_float(max(max(abs_bits(b2), abs_bits(b1)), abs_bits(b0)));
  const bool deg = (abs_bits(c3) >> 23) == 0u || (mc >> 23) == 255u || (abs_bits(R) >> 23) == 255u;
  const float disc = b2 * b2 - 3.0f * b1;
  const float sq = sqrtf(disc > 0.f ? disc : 0.f);
  const float ends[4] = {-R, (-b2 - sq) / 3.0f, (-b2 + sq) / 3.0f, R};
  bool ng[4];
#pragma unroll
  for (int i = 0; i < 4; i++)
    ng[i] = (((ends[i] + b2) * ends[i] + b1) * ends[i] + b0) < 0.f;
  float l[3], r[3];
#pragma unroll
  for (int i = 0; i < 3; i++)
    l[i] = ends[i], r[i] = ends[i + 1];
  for (int step = 0; step < kBisectSteps; step++)
  {
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
      const float m = (l[i] + r[i]) * 0.5f;
      const bool same = ((((m + b2) * m + b1) * m + b0) < 0.f) == ng[i];
      l[i] = same ? m : l[i], r[i] = same ? r[i] : m;
    }
  }
  const float bad = __uint_as_float(0x7fc00000u);
  root[0] = bad, root[1] = bad, root[2] = bad;
  uint32_t cnt = 0u;
#pragma unroll
  for (int i = 0; i < 3; i++)
  {
    const bool has = ng[i] != ng[i + 1] && !deg;
    const float x = (l[i] + r[i]) * 0.5f;
#pragma unroll
    for (int k = 0; k < 3; k++)
      root[k] = (has && cnt == (uint32_t)k) ? x : root[k];
    cnt += has ? 1u : 0u;
  }
  return cnt;
}

// The models through seven correspondences c_i = {xa, ya, xb, yb} (scaled): (xb, yb, 1) F (xa, ya, 1)^T = 0. Both sides conditioned
// (condition7), the 7x9 system with rows (xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1) reduced by Gauss-Jordan on its first seven
// columns — for column k the rows k+1..6 are compared with row k in turn and exchanged when their |entry| (bit pattern) is strictly
// larger; row k times 1 / pivot; every other row r minus a[r][k] times row k —, everything unrolled so that the system lives in
// registers. The free columns give F1 = (-a[.][7], 1, 0) and F2 = (-a[.][8], 0, 1); det(F1 + a F2) is expanded along the last row;
// each real root gives F^ = F1 + a F2, taken back as T_b^T F^ T_a and scaled by the power of two that brings its largest entry into
// [1, 2). A model that is absent or not finite is all-NaN (no correspondence is an inlier of it). Returns the number of roots.
__device__ __forceinline__ uint32_t solve_f7(const float4 (&c)[7], Mat9 (&M)[3])
{
  float xa[7], ya[7], xb[7], yb[7];
#pragma unroll
  for (int i = 0; i < 7; i++)
    xa[i] = c[i].x, ya[i] = c[i].y, xb[i] = c[i].z, yb[i] = c[i].w;
  float sa, ua, va, sb, ub, vb;
  condition7(xa, ya, sa, ua, va);
  condition7(xb, yb, sb, ub, vb);
  float a[7][9];
#pragma unroll
  for (int i = 0; i < 7; i++)
  {
    a[i][0] = xb[i] * xa[i], a[i][1] = xb[i] * ya[i], a[i][2] = xb[i];
    a[i][3] = yb[i] * xa[i], a[i][4] = yb[i] * ya[i], a[i][5] = yb[i];
    a[i][6] = xa[i], a[i][7] = ya[i], a[i][8] = 1.0f;
  }
#pragma unroll
  for (int k = 0; k < 7; k++)
  {
#pragma unroll
    for (int r = k + 1; r < 7; r++)
    {
      const bool sw = abs_bits(a[r][k]) > abs_bits(a[k][k]);
#pragma unroll
      for (int j = k; j < 9; j++)
      {
        const float top = a[k][j], low = a[r][j];
        a[k][j] = sw ? low : top, a[r][j] = sw ? top : low;
      }
    }
    const float inv = 1.0f / a[k][k];
#pragma unroll
    for (int j = k + 1; j < 9; j++)
      a[k][j] = a[k][j] * inv;
#pragma unroll
    for (int r = 0; r < 7; r++)
      if (r != k)
      {
        const float f = a[r][k];
#pragma unroll
        for (int j = k + 1; j < 9; j++)
          a[r][j] = a[r][j] - f * a[k][j];
      }
  }
  float p[7], q[7];
#pragma unroll
  for (int i = 0; i < 7; i++)
    p[i] = -a[i][7], q[i] = -a[i][8];
  // det(P + a Q), P = (p0..p6, 1, 0), Q = (q0..q6, 0, 1), with m_i = p_i + a q_i: m0 (m4 a - m5) - m1 (m3 a - m5 m6) + m2 (m3 - m4 m6)
  const float t1[3] = {-p[5], p[4] - q[5], q[4]};
  const float t2[3] = {-(p[5] * p[6]), p[3] - (p[5] * q[6] + q[5] * p[6]), q[3] - q[5] * q[6]};
  const float t3[3] = {p[3] - p[4] * p[6], q[3] - (p[4] * q[6] + q[4] * p[6]), -(q[4] * q[6])};
  const float A[4] = {p[0] * t1[0], p[0] * t1[1] + q[0] * t1[0], p[0] * t1[2] + q[0] * t1[1], q[0] * t1[2]};
  const float B[4] = {p[1] * t2[0], p[1] * t2[1] + q[1] * t2[0], p[1] * t2[2] + q[1] * t2[1], q[1] * t2[2]};
  const float C[4] = {p[2] * t3[0], p[2] * t3[1] + q[2] * t3[0], p[2] * t3[2] + q[2] * t3[1], q[2] * t3[2]};
  float root[3];
  const uint32_t cnt = cubic_roots((A[0] - B[0]) + C[0], (A[1] - B[1]) + C[1], (A[2] - B[2]) + C[2], (A[3] - B[3]) + C[3], root);
  const float bad = __uint_as_float(0x7fc00000u);
#pragma unroll
  for (int k = 0; k < 3; k++)
  {
    const float al = root[k];
    float fh[9], g[9], F[9];
#pragma unroll
    for (int i = 0; i < 7; i++)
      fh[i] = p[i] + al * q[i];
    fh[7] = 1.0f, fh[8] = al;
#pragma unroll
    for (int r = 0; r < 3; r++) // F^ T_a
    {
      g[3 * r] = fh[3 * r] * sa, g[3 * r + 1] = fh[3 * r + 1] * sa;
      g[3 * r + 2] = (fh[3 * r + 2] - fh[3 * r] * ua) - fh[3 * r + 1] * va;
    }
    uint32_t m = 0u;
#pragma unroll
    for (int col = 0; col < 3; col++) // T_b^T (F^ T_a)
    {
      F[col] = sb * g[col], F[3 + col] = sb * g[3 + col];
      F[6 + col] = (g[6 + col] - ub * g[col]) - vb * g[3 + col];
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
      m = max(m, abs_bits(F[i]));
    bool ok;
    const float f = unit_scale(m, ok);
#pragma unroll
    for (int i = 0; i < 9; i++)
      M[k].f[i] = ok ? F[i] * f : bad;
  }
  return cnt;
}

struct ModelF
{
  static constexpr int kKind = (int)VKSIFT_HIP_GUIDE_FUNDAMENTAL;
  static constexpr uint32_t kSample = 7u, kModels = 3u, kRootBits = 2u, kMinInliers = 8u, kResultWords = 14u, kUnroll = 1u;

  static __device__ __forceinline__ uint32_t solve(const float4 *__restrict__ c, uint64_t seed_key, uint32_t slot, uint32_t hyp, uint32_t n, Mat9 (&M)[3])
  {
    uint32_t idx[7];
    draw_sample<7>(seed_key, slot, hyp, n, idx);
    float4 sc[7];
#pragma unroll
    for (int i = 0; i < 7; i++)
      sc[i] = scaled(c[idx[i]]);
    return solve_f7(sc, M);
  }

  // pixel coordinates by powers of two (F_px = K F K with K = diag(2^-13, 2^-13, 1), times 2^26), scaled again so that the largest entry
  // lies in [1, 2)
  static __device__ __forceinline__ void publish(const float (&F)[9], float (&o)[9], bool &valid)
  {
    const float k1 = kCoordUnscale, k2 = kCoordUnscale * kCoordUnscale;
    o[0] = F[0], o[1] = F[1], o[2] = F[2] * k1;
    o[3] = F[3], o[4] = F[4], o[5] = F[5] * k1;
    o[6] = F[6] * k1, o[7] = F[7] * k1, o[8] = F[8] * k2;
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < 9; i++)
      m = max(m, abs_bits(o[i]));
    const float f = unit_scale(m, valid);
#pragma unroll
    for (int i = 0; i < 9; i++)
      o[i] = o[i] * f;
  }
};

__global__ void __launch_bounds__(256) k_ransac_score_f(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev,
                                                        uint32_t n_stride, uint32_t max_n, uint32_t nb_hyp, uint32_t nblk, float t2, uint64_t seed_key,
                                                        uint32_t *__restrict__ keys)
{
  ransac_score<ModelF>(corr, corr_slot_stride, n_dev, n_stride, max_n, nb_hyp, nblk, t2, seed_key, keys);
}

__global__ void __launch_bounds__(256) k_ransac_final_f(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev,
                                                        uint32_t n_stride, uint32_t max_n, uint32_t nblk, float t2, uint64_t seed_key,
                                                        const uint32_t *__restrict__ keys, uint32_t *__restrict__ results, uint8_t *__restrict__ masks,
                                                        uint64_t mask_slot_stride)
{
  ransac_final<ModelF>(corr, corr_slot_stride, n_dev, n_stride, max_n, nblk, t2, seed_key, keys, results, masks, mask_slot_stride);
}

uint64_t seed_key_of(uint64_t seed)
{
  uint64_t z = seed + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

using ScoreKernel = void (*)(const float4 *, uint64_t, const uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, float, uint64_t, uint32_t *);
using FinalKernel = void (*)(const float4 *, uint64_t, const uint32_t *, uint32_t, uint32_t, uint32_t, float, uint64_t, const uint32_t *, uint32_t *, uint8_t *,
                             uint64_t);

// the refusals and the two launches of either model
int ransac_launch(ScoreKernel score, FinalKernel final, const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n,
                  uint32_t nslots, uint32_t nb_hypotheses, float threshold_px, uint64_t seed, uint8_t *results, uint8_t *masks, uint64_t mask_slot_stride,
                  uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
{
  if (nslots < 1 || nb_hypotheses == 0 || nb_hypotheses > 65536u || !(threshold_px > 0.f) || !isfinite(threshold_px) ||
      scratch_u32 < vksift_hip_ransac_scratch_u32(nslots, nb_hypotheses) || (corr_slot_stride & 15u) || ((uintptr_t)corr & 15u) || ((uintptr_t)results & 3u) ||
      (nslots > 1 && (corr_slot_stride < 16u * (uint64_t)max_n || mask_slot_stride < max_n)))
    return (int)hipErrorInvalidValue;
  const uint32_t nblk = (nb_hypotheses + kHypPerBlock - 1u) / kHypPerBlock;
  if ((uint64_t)nslots * nblk > 0x7fffffffull)
    return (int)hipErrorInvalidValue;
  const float ts = threshold_px * kCoordScale, t2 = ts * ts;
  const uint64_t key = seed_key_of(seed);
  hipLaunchKernelGGL(score, dim3(nslots * nblk), dim3(kHypPerBlock), 0, (hipStream_t)s, (const float4 *)corr, corr_slot_stride / 16u, n_dev, n_stride, max_n,
                     nb_hypotheses, nblk, t2, key, scratch);
  int e = (int)hipGetLastError();
  if (e)
    return e;
  hipLaunchKernelGGL(final, dim3(nslots), dim3(256), 0, (hipStream_t)s, (const float4 *)corr, corr_slot_stride / 16u, n_dev, n_stride, max_n, nblk, t2, key,
                     (const uint32_t *)scratch, (uint32_t *)results, masks, mask_slot_stride);
  return (int)hipGetLastError();
}

} // namespace

extern "C"
{
  size_t vksift_hip_ransac_scratch_u32(uint32_t nslots, uint32_t nb_hypotheses)
  {
    return 2u * (size_t)nslots * (((size_t)nb_hypotheses + kHypPerBlock - 1u) / kHypPerBlock);
  }

  int vksift_hip_gather_correspondences(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *found_base, uint32_t found_buf_stride,
                                        const uint32_t *slot_tab, const uint32_t *layouts, const uint8_t *filtered, uint64_t filtered_slot_stride,
                                        const uint32_t *filtered_n, uint32_t max_n, uint32_t nslots, float *corr, uint64_t corr_slot_stride, vksift_hip_stream s)
  {
    if (nslots < 1 || (filtered_slot_stride & 3u) || (corr_slot_stride & 15u) || ((uintptr_t)corr & 15u))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_corr, dim3(nslots), dim3(256), 0, (hipStream_t)s, feats_base, buf_stride, found_base, found_buf_stride, slot_tab, layouts,
                       (const uint32_t *)filtered, filtered_slot_stride / 4u, filtered_n, max_n, (float4 *)corr, corr_slot_stride / 16u);
    return (int)hipGetLastError();
  }

  int vksift_hip_ransac_homography(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                   uint32_t nb_hypotheses, float threshold_px, uint64_t seed, uint8_t *results, uint8_t *masks, uint64_t mask_slot_stride,
                                   uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
  {
    return ransac_launch(k_ransac_score_h, k_ransac_final_h, corr, corr_slot_stride, n_dev, n_stride, max_n, nslots, nb_hypotheses, threshold_px, seed, results,
                         masks, mask_slot_stride, scratch, scratch_u32, s);
  }

  int vksift_hip_ransac_fundamental(const float *corr, uint64_t corr_slot_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n, uint32_t nslots,
                                    uint32_t nb_hypotheses, float threshold_px, uint64_t seed, uint8_t *results, uint8_t *masks, uint64_t mask_slot_stride,
                                    uint32_t *scratch, size_t scratch_u32, vksift_hip_stream s)
  {
    return ransac_launch(k_ransac_score_f, k_ransac_final_f, corr, corr_slot_stride, n_dev, n_stride, max_n, nslots, nb_hypotheses, threshold_px, seed, results,
                         masks, mask_slot_stride, scratch, scratch_u32, s);
  }
}
