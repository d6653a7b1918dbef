// verify.hip — geometric verification of filtered matches: a batched, deterministic RANSAC homography estimator (no counterpart in the
// reference, whose callers run a CPU RANSAC after downloading matches and features; the reference's own evaluation judges matches by
// a homography, src/perf/perf_matching.cpp:30-79). Three launches serve every pair (slot) of a call:
//   k_gather_corr      filtered matches {idx_a, idx_b} (download-order rows) -> {xa, ya, xb, yb} read from the SIFT buffers' sections
//   k_ransac_score_h   one lane per hypothesis: counter-based sample, closed-form four-point homography, inlier count over the slot's
//                      correspondences staged through LDS (broadcast 16-byte reads), best (count, lowest index) per workgroup
//   k_ransac_final_h   best hypothesis per slot, its model in pixel coordinates, the inlier mask (same test: popcount == count)
// Everything is integer arithmetic or correctly rounded fp32 add / sub / mul / div in a fixed order (the tree is built with
// -ffp-contract=off and no fmaf is used here), so tests/np_verify.py restates it bit for bit. A second model (fundamental matrix) is a
// second pair of score / final kernels beside these; the gather and the sampler are model-free.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vksift_hip.h"

namespace
{

constexpr uint32_t kHypPerBlock = 256u; // lanes (= hypotheses) per workgroup of the scoring kernel, and correspondences per LDS tile
// Coordinates enter the solve scaled by 2^-13 (exact): the entries of the un-normalised homography are polynomials of degree 9 in the
// coordinates, 16383^9 would not fit fp32. Powers of two change no rounding, so the result is that of the unscaled computation.
constexpr float kCoordScale = 1.0f / 8192.0f;
constexpr float kCoordUnscale = 8192.0f;

struct Hom
{
  float h0, h1, h2, h3, h4, h5, h6, h7, h8;
};

__device__ __forceinline__ uint64_t splitmix64_next(uint64_t &state)
{
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t draw_below(uint64_t &state, uint32_t m) { return (uint32_t)(((splitmix64_next(state) >> 32) * (uint64_t)m) >> 32); }

// Four distinct indices below n (n >= 4), in draw order: draw k is uniform over the n - k indices left and stepped over the ones
// already drawn (kept sorted in a <= b <= c). seed_key = the first splitmix64 output of the state `seed`.
__device__ __forceinline__ void draw_sample(uint64_t seed_key, uint32_t slot, uint32_t hyp, uint32_t n, uint32_t &i0, uint32_t &i1, uint32_t &i2, uint32_t &i3)
{
  uint64_t st = seed_key ^ (((uint64_t)slot << 32) | (uint64_t)hyp);
  i0 = draw_below(st, n);
  uint32_t r = draw_below(st, n - 1u);
  r += r >= i0 ? 1u : 0u;
  i1 = r;
  uint32_t a = i0 < i1 ? i0 : i1, b = i0 < i1 ? i1 : i0;
  r = draw_below(st, n - 2u);
  r += r >= a ? 1u : 0u;
  r += r >= b ? 1u : 0u;
  i2 = r;
  const uint32_t lo = b < i2 ? b : i2, c = b < i2 ? i2 : b;
  b = a < lo ? lo : a;
  a = a < lo ? a : lo;
  r = draw_below(st, n - 3u);
  r += r >= a ? 1u : 0u;
  r += r >= b ? 1u : 0u;
  r += r >= c ? 1u : 0u;
  i3 = r;
}

__device__ __forceinline__ float4 scaled(float4 c) { return float4{c.x * kCoordScale, c.y * kCoordScale, c.z * kCoordScale, c.w * kCoordScale}; }

// Homography through four correspondences c_i = {xa, ya, xb, yb} (scaled), projective-basis form: with p_i = (xa_i, ya_i, 1),
// lambda = adj([p0 p1 p2]) p3 and A = [lambda_i p_i] (likewise mu, B for the q_i = (xb_i, yb_i, 1)), H = B adj(A); the rows of
// adj(A) are lambda_j lambda_k (p_j x p_k), so the cross products are formed once. The result is scaled by the power of two that
// brings its largest entry into [1, 2) (exact), negated if it maps the first sample point behind the plane; a sample whose largest entry is zero, subnormal, at or above 2^127, infinite or NaN
// is degenerate and becomes all-NaN (no correspondence is an inlier of it).
__device__ __forceinline__ Hom solve_h4(float4 c0, float4 c1, float4 c2, float4 c3)
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
  Hom H;
  H.h0 = (u0 * ax + u1 * bx) + u2 * gx;
  H.h1 = (u0 * ay + u1 * by) + u2 * gy;
  H.h2 = (u0 * az + u1 * bz) + u2 * gz;
  H.h3 = (v0 * ax + v1 * bx) + v2 * gx;
  H.h4 = (v0 * ay + v1 * by) + v2 * gy;
  H.h5 = (v0 * az + v1 * bz) + v2 * gz;
  H.h6 = (w0 * ax + w1 * bx) + w2 * gx;
  H.h7 = (w0 * ay + w1 * by) + w2 * gy;
  H.h8 = (w0 * az + w1 * bz) + w2 * gz;
  // largest magnitude by its bit pattern (NaN and infinity sort above every finite value)
  uint32_t m = __float_as_uint(H.h0) & 0x7fffffffu;
  m = max(m, __float_as_uint(H.h1) & 0x7fffffffu);
  m = max(m, __float_as_uint(H.h2) & 0x7fffffffu);
  m = max(m, __float_as_uint(H.h3) & 0x7fffffffu);
  m = max(m, __float_as_uint(H.h4) & 0x7fffffffu);
  m = max(m, __float_as_uint(H.h5) & 0x7fffffffu);
  m = max(m, __float_as_uint(H.h6) & 0x7fffffffu);
  m = max(m, __float_as_uint(H.h7) & 0x7fffffffu);
  m = max(m, __float_as_uint(H.h8) & 0x7fffffffu);
  const uint32_t e = m >> 23;
  const bool ok = e >= 1u && e <= 253u;
  // the sign of B adj(A) follows the orientation of the sample: chosen so that the first sample point lies in front of the plane (d > 0)
  const float d0 = (H.h6 * c0.x + H.h7 * c0.y) + H.h8;
  const float fa = __uint_as_float((254u - (ok ? e : 127u)) << 23); // 2^(127 - e)
  const float f = d0 < 0.f ? -fa : fa;
  const float bad = __uint_as_float(0x7fc00000u);
  H.h0 = ok ? H.h0 * f : bad, H.h1 = ok ? H.h1 * f : bad, H.h2 = ok ? H.h2 * f : bad;
  H.h3 = ok ? H.h3 * f : bad, H.h4 = ok ? H.h4 * f : bad, H.h5 = ok ? H.h5 * f : bad;
  H.h6 = ok ? H.h6 * f : bad, H.h7 = ok ? H.h7 * f : bad, H.h8 = ok ? H.h8 * f : bad;
  return H;
}

// Forward transfer error below the threshold, without a division: with (u, v, d) = H (xa, ya, 1), the correspondence is an inlier iff
// d > 0 and (u - xb d)^2 + (v - yb d)^2 < t^2 d^2. A NaN anywhere fails both comparisons.
__device__ __forceinline__ bool is_inlier(const Hom &H, float4 c, float t2)
{
  const float u = (H.h0 * c.x + H.h1 * c.y) + H.h2;
  const float v = (H.h3 * c.x + H.h4 * c.y) + H.h5;
  const float d = (H.h6 * c.x + H.h7 * c.y) + H.h8;
  const float ru = u - c.z * d, rv = v - c.w * d;
  const float e2 = ru * ru + rv * rv;
  const float lim = (d * d) * t2;
  return d > 0.f && e2 < lim;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
  {
    const unsigned long long o = __shfl_xor(k, off, 64);
    k = o > k ? o : k;
  }
  return k;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per slot. slot_tab: {buffer A, buffer B, layout A, layout B} per slot; a layout word with bit 31 set names a buffer
// of that many dense rows (uploaded features), any other value a section table in `layouts` ({nsec, off[16], cap[16]}: the walk of
// k_gather_sections / k_pack_features, records.hip, with the stored counts min(found, cap) read on the device). A match that names a
// row the buffer does not hold yields a NaN correspondence (never an inlier); nothing is read out of bounds.
__global__ void __launch_bounds__(256) k_gather_corr(const uint8_t *__restrict__ feats_base, uint64_t buf_stride, const uint32_t *__restrict__ found_base,
                                                     uint32_t found_buf_stride, const uint32_t *__restrict__ slot_tab, const uint32_t *__restrict__ layouts,
                                                     const uint32_t *__restrict__ filtered, uint64_t filtered_slot_stride, const uint32_t *__restrict__ filtered_n,
                                                     uint32_t max_n, float4 *__restrict__ corr, uint64_t corr_slot_stride)
{
  __shared__ uint32_t s_off[2][16], s_cnt[2][16], s_total[2], s_buf[2];
  const uint32_t slot = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t *tab = slot_tab + (size_t)slot * 4u;
  if (tid < 32u)
  {
    const uint32_t side = tid >> 4, o = tid & 15u;
    const uint32_t bufi = tab[side], lay = tab[2u + side];
    uint32_t off = 0, cnt = 0;
    if (lay & 0x80000000u)
      cnt = o == 0u ? (lay & 0x7fffffffu) : 0u;
    else
    {
      const uint32_t *L = layouts + (size_t)lay * 33u;
      if (o < L[0] && o < found_buf_stride)
      {
        const uint32_t f = found_base[(size_t)bufi * found_buf_stride + o], cap = L[17u + o];
        off = L[1u + o];
        cnt = f < cap ? f : cap;
      }
    }
    s_off[side][o] = off, s_cnt[side][o] = cnt;
    if (o == 0u)
      s_buf[side] = bufi; // (the table may live in mapped host memory: read once)
  }
  __syncthreads();
  if (tid < 2u)
  {
    uint32_t t = 0;
    for (uint32_t o = 0; o < 16u; o++)
      t += s_cnt[tid][o];
    s_total[tid] = t;
  }
  __syncthreads();
  uint32_t n = filtered_n[slot];
  n = n < max_n ? n : max_n;
  const uint32_t *fm = filtered + (size_t)slot * filtered_slot_stride;
  float4 *out = corr + (size_t)slot * corr_slot_stride;
  const float bad = __uint_as_float(0x7fc00000u);
  for (uint32_t k = tid; k < n; k += 256u)
  {
    float xy[4] = {bad, bad, bad, bad};
#pragma unroll
    for (uint32_t side = 0; side < 2u; side++)
    {
      const uint32_t row = fm[(size_t)k * 4u + side];
      if (row < s_total[side])
      {
        uint32_t base = 0, src_row = 0;
#pragma unroll
        for (uint32_t o = 0; o < 16u; o++)
        {
          const uint32_t c = s_cnt[side][o];
          if (row >= base && row < base + c)
            src_row = s_off[side][o] + (row - base);
          base += c;
        }
        const float *f = (const float *)(feats_base + (size_t)s_buf[side] * buf_stride + (size_t)src_row * 164u);
        xy[2u * side] = f[0], xy[2u * side + 1u] = f[1];
      }
    }
    out[k] = float4{xy[0], xy[1], xy[2], xy[3]};
  }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
// Workgroup (slot, blk) scores hypotheses blk*256 .. blk*256+255 of its slot against all n correspondences and stores the largest
// key (count << 32 | ~hypothesis) — most inliers, ties to the lowest hypothesis — as two words at keys[2 * (slot * nblk + blk)].
__global__ void __launch_bounds__(256) k_ransac_score_h(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev,
                                                        uint32_t n_stride, uint32_t max_n, uint32_t nb_hyp, uint32_t nblk, float t2, uint64_t seed_key,
                                                        uint32_t *__restrict__ keys)
{
  __shared__ float4 tile[kHypPerBlock];
  __shared__ unsigned long long wave_best[4];
  const uint32_t slot = blockIdx.x / nblk, blk = blockIdx.x - slot * nblk;
  const uint32_t tid = threadIdx.x;
  uint32_t n = n_dev[(size_t)slot * n_stride];
  n = n < max_n ? n : max_n;
  uint32_t *kout = keys + 2u * (size_t)blockIdx.x;
  if (n < 4u)
  {
    if (tid == 0)
      kout[0] = 0u, kout[1] = 0u;
    return;
  }
  const float4 *c = corr + (size_t)slot * corr_slot_stride;
  const uint32_t hyp = blk * kHypPerBlock + tid;
  const bool active = hyp < nb_hyp;
  uint32_t i0, i1, i2, i3;
  draw_sample(seed_key, slot, active ? hyp : 0u, n, i0, i1, i2, i3);
  const Hom H = solve_h4(scaled(c[i0]), scaled(c[i1]), scaled(c[i2]), scaled(c[i3]));
  uint32_t cnt = 0;
  for (uint32_t base = 0; base < n; base += kHypPerBlock)
  {
    __syncthreads();
    if (base + tid < n)
      tile[tid] = scaled(c[base + tid]);
    __syncthreads();
    const uint32_t m = n - base < kHypPerBlock ? n - base : kHypPerBlock;
#pragma unroll 4
    for (uint32_t j = 0; j < m; j++)
      cnt += is_inlier(H, tile[j], t2) ? 1u : 0u; // every lane reads the same 16 bytes: one broadcast LDS access
  }
  unsigned long long key = active ? (((unsigned long long)cnt << 32) | (unsigned long long)(~hyp)) : 0ull;
  key = wave_max_u64(key);
  if ((tid & 63u) == 0u)
    wave_best[tid >> 6] = key;
  __syncthreads();
  if (tid == 0)
  {
    for (int w = 1; w < 4; w++)
      key = wave_best[w] > key ? wave_best[w] : key;
    kout[0] = (uint32_t)key, kout[1] = (uint32_t)(key >> 32);
  }
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per slot: the best key over the slot's nblk workgroups, the winner's model recomputed from its sample, brought back to
// pixel coordinates (powers of two) and divided by h22; result record (13 words: H[9], nb_matches, nb_inliers, best_hypothesis, valid)
// and one mask byte per correspondence.
__global__ void __launch_bounds__(256) k_ransac_final_h(const float4 *__restrict__ corr, uint64_t corr_slot_stride, const uint32_t *__restrict__ n_dev,
                                                        uint32_t n_stride, uint32_t max_n, uint32_t nblk, float t2, uint64_t seed_key,
                                                        const uint32_t *__restrict__ keys, uint32_t *__restrict__ results, uint8_t *__restrict__ masks,
                                                        uint64_t mask_slot_stride)
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
  key = wave_max_u64(key);
  if ((tid & 63u) == 0u)
    wave_best[tid >> 6] = key;
  __syncthreads();
  key = wave_best[0];
  for (int w = 1; w < 4; w++)
    key = wave_best[w] > key ? wave_best[w] : key;
  const uint32_t cnt = (uint32_t)(key >> 32), hyp = ~(uint32_t)key;
  const float4 *c = corr + (size_t)slot * corr_slot_stride;
  uint8_t *mask = masks + (size_t)slot * mask_slot_stride;
  uint32_t *res = results + (size_t)slot * 13u;
  bool valid = n >= 4u && cnt >= 4u;
  Hom H = {};
  float o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (valid) // uniform over the workgroup
  {
    uint32_t i0, i1, i2, i3;
    draw_sample(seed_key, slot, hyp, n, i0, i1, i2, i3);
    H = solve_h4(scaled(c[i0]), scaled(c[i1]), scaled(c[i2]), scaled(c[i3]));
    const float p2 = H.h2 * kCoordUnscale, p5 = H.h5 * kCoordUnscale, p6 = H.h6 * kCoordScale, p7 = H.h7 * kCoordScale;
    o[0] = H.h0 / H.h8, o[1] = H.h1 / H.h8, o[2] = p2 / H.h8;
    o[3] = H.h3 / H.h8, o[4] = H.h4 / H.h8, o[5] = p5 / H.h8;
    o[6] = p6 / H.h8, o[7] = p7 / H.h8, o[8] = H.h8 / H.h8;
    valid = H.h8 != 0.f;
#pragma unroll
    for (int i = 0; i < 9; i++)
      valid = valid && ((__float_as_uint(o[i]) & 0x7f800000u) != 0x7f800000u);
  }
  for (uint32_t k = tid; k < n; k += 256u)
    mask[k] = (valid && is_inlier(H, scaled(c[k]), t2)) ? 1u : 0u;
  if (tid == 0)
  {
#pragma unroll
    for (int i = 0; i < 9; i++)
      res[i] = valid ? __float_as_uint(o[i]) : 0u;
    res[9] = n;
    res[10] = valid ? cnt : 0u;
    res[11] = valid ? hyp : 0u;
    res[12] = valid ? 1u : 0u;
  }
}

uint64_t seed_key_of(uint64_t seed)
{
  uint64_t z = seed + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
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
    if (nslots < 1 || nb_hypotheses == 0 || nb_hypotheses > 65536u || !(threshold_px > 0.f) || !isfinite(threshold_px) ||
        scratch_u32 < vksift_hip_ransac_scratch_u32(nslots, nb_hypotheses) || (corr_slot_stride & 15u) || ((uintptr_t)corr & 15u) || ((uintptr_t)results & 3u) ||
        (nslots > 1 && (corr_slot_stride < 16u * (uint64_t)max_n || mask_slot_stride < max_n)))
      return (int)hipErrorInvalidValue;
    const uint32_t nblk = (nb_hypotheses + kHypPerBlock - 1u) / kHypPerBlock;
    if ((uint64_t)nslots * nblk > 0x7fffffffull)
      return (int)hipErrorInvalidValue;
    const float ts = threshold_px * kCoordScale, t2 = ts * ts;
    const uint64_t key = seed_key_of(seed);
    hipLaunchKernelGGL(k_ransac_score_h, dim3(nslots * nblk), dim3(kHypPerBlock), 0, (hipStream_t)s, (const float4 *)corr, corr_slot_stride / 16u, n_dev, n_stride,
                       max_n, nb_hypotheses, nblk, t2, key, scratch);
    int e = (int)hipGetLastError();
    if (e)
      return e;
    hipLaunchKernelGGL(k_ransac_final_h, dim3(nslots), dim3(256), 0, (hipStream_t)s, (const float4 *)corr, corr_slot_stride / 16u, n_dev, n_stride, max_n, nblk, t2,
                       key, (const uint32_t *)scratch, (uint32_t *)results, masks, mask_slot_stride);
    return (int)hipGetLastError();
  }
}
