// guided.hip — guided matching: every feature of a verified pair matched again against only those features of the other image that agree
// with the pair's model (a homography or a fundamental matrix), so that the ratio test compares the best candidate with the second best
// among the geometrically possible ones (no counterpart in the reference, whose callers loop over downloaded features on the CPU).
//   k_gather_xy        {x, y} of every stored row of both buffers of every slot, download order, dense float2 (layout decode and walk:
//                      records.h)
//   k_guided_2nn<M, R> one workgroup per tile of 256 owner rows of a slot, a lane owns one row. The sweep over the other side is the
//                      geometric test alone (about 8 VALU operations per pair: what depends on one side only is computed once, in the
//                      owner's registers or while the other side is staged in LDS, read back as broadcasts). Admissible pairs are rare;
//                      they are queued per wave in LDS as (owner lane, candidate) and drained one lane per entry whenever 64 wait: exact
//                      integer distance from the matcher's cached rows and shifted norms, folded as a 64-bit key (d2 << 32 | candidate)
//                      into the owner's two LDS slots (atomic min on the first; what loses there goes by atomic min into the second).
//   k_guided_keep      per slot: max_distance, ratio test, cross-check; survivors in increasing idx_a (ordered_keep, records.h)
// The test is two_view.h's, the one the verification counted inliers with, here on unscaled pixel coordinates with the published model:
// correctly rounded fp32 add / sub / mul in the order written, so tests/np_guided.py restates every record bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vksift_hip.h"
#include "hip/records.h"
#include "hip/two_view.h"

namespace
{

constexpr uint32_t kTile = 256u;                      // owner rows per workgroup, and candidates per LDS tile
constexpr uint32_t kChunk = 16u;                      // candidates a lane tests between two looks at its wave's queue
constexpr uint32_t kWaveQueue = kChunk * 64u + 64u;   // fewer than 64 entries wait when a chunk starts, a chunk adds at most 16 per lane
constexpr unsigned long long kNoKey = ~0ull;

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
// Workgroup 2 * slot + side. slot_tab: {buffer A, buffer B, layout A, layout B} per slot, layouts: the section tables (records.h). Rows
// [0, min(total, max_n)) are written, nothing else.
__global__ void __launch_bounds__(256) k_gather_xy(const uint8_t *__restrict__ feats_base, uint64_t buf_stride, const uint32_t *__restrict__ found_base,
                                                   uint32_t found_buf_stride, const uint32_t *__restrict__ slot_tab, const uint32_t *__restrict__ layouts,
                                                   uint32_t max_n, float2 *__restrict__ xy, uint64_t xy_side_stride)
{
  __shared__ SideLayout L[1];
  layout_decode(L, slot_tab + (size_t)(blockIdx.x >> 1) * 4u, blockIdx.x & 1u, layouts, found_base, found_buf_stride);
  const uint32_t n = L[0].total < max_n ? L[0].total : max_n;
  float2 *out = xy + (size_t)blockIdx.x * xy_side_stride;
  const uint8_t *feats = feats_base + (size_t)L[0].buf * buf_stride;
  for (uint32_t row = threadIdx.x; row < n; row += 256u)
  {
    const float *f = (const float *)(feats + (size_t)section_row(L[0].cnt, L[0].off, row) * VKSIFT_RECORD_BYTES);
    out[row] = float2{f[0], f[1]};
  }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
// lanes of one wave exchange data through LDS without a workgroup barrier: the wave's LDS operations complete in program order, the
// fence keeps the compiler from moving them
__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Owner rows tile * 256 .. of slot blockIdx.y: rows of A against the features of B (REVERSE: rows of B against the features of A; the
// relation is the same one on the ordered pair (a, b), the model is not inverted). keys: per (slot, direction) max_n pairs {k1, k2} of
// 64-bit keys d2 << 32 | candidate, the smallest and the second smallest over the admissible candidates, ~0 where there is none. Slots whose
// model is not valid are left alone (k_guided_keep does not read their keys).
template <int MODEL, bool REVERSE>
__global__ void __launch_bounds__(256)
    k_guided_2nn(const uint8_t *__restrict__ cache_desc, uint64_t desc_stride, const uint32_t *__restrict__ cache_norm, uint64_t norm_stride,
                 const uint32_t *__restrict__ slot_tab, uint32_t tab_stride, const float2 *__restrict__ xy, uint64_t xy_side_stride,
                 const uint32_t *__restrict__ n_dev, uint32_t n_stride, uint32_t max_n, const float *__restrict__ models, uint32_t model_stride,
                 const uint32_t *__restrict__ valid, uint32_t valid_stride, float t2, unsigned long long *__restrict__ keys)
{
  __shared__ float4 tile[kTile];
  __shared__ unsigned long long s_k1[kTile], s_k2[kTile];
  __shared__ uint32_t s_q[4][kWaveQueue];
  __shared__ uint32_t s_qn[4];
  const uint32_t slot = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (valid[(size_t)slot * valid_stride] == 0u)
    return;
  uint32_t na = n_dev[(size_t)slot * n_stride], nb = n_dev[(size_t)slot * n_stride + 1u];
  na = na < max_n ? na : max_n, nb = nb < max_n ? nb : max_n;
  const uint32_t n_own = REVERSE ? nb : na, n_oth = REVERSE ? na : nb;
  const uint32_t row0 = blockIdx.x * kTile;
  if (row0 >= n_own)
    return;
  float M[9];
#pragma unroll
  for (int i = 0; i < 9; i++)
    M[i] = models[(size_t)slot * model_stride + i];
  const uint32_t buf_own = slot_tab[(size_t)slot * tab_stride + (REVERSE ? 1u : 0u)], buf_oth = slot_tab[(size_t)slot * tab_stride + (REVERSE ? 0u : 1u)];
  const float2 *xy_own = xy + ((size_t)2u * slot + (REVERSE ? 1u : 0u)) * xy_side_stride;
  const float2 *xy_oth = xy + ((size_t)2u * slot + (REVERSE ? 0u : 1u)) * xy_side_stride;
  const uint4 *desc_own = (const uint4 *)(cache_desc + (size_t)buf_own * desc_stride), *desc_oth = (const uint4 *)(cache_desc + (size_t)buf_oth * desc_stride);
  const uint32_t *norm_own = cache_norm + (size_t)buf_own * norm_stride, *norm_oth = cache_norm + (size_t)buf_oth * norm_stride;
  const float bad = __uint_as_float(0x7fc00000u);

  const uint32_t own = row0 + tid;
  const float2 p_own = own < n_own ? xy_own[own] : float2{bad, bad};
  const float4 q_own = REVERSE ? side_b<MODEL>(M, p_own) : side_a<MODEL>(M, p_own, t2);
  s_k1[tid] = kNoKey, s_k2[tid] = kNoKey; // touched by the lanes of this wave only
  if (lane == 0u)
    s_qn[wave] = 0u;
  uint32_t *q = s_q[wave];
  wave_sync();

  // one queue entry: the exact squared distance of (owner row, candidate) from the shifted bytes and norms, then the fold
  auto drain_entry = [&](uint32_t e) {
    const uint32_t o = e >> 24, c = e & 0xffffffu;
    const uint4 *ra = desc_own + (size_t)(row0 + o) * 8u, *rb = desc_oth + (size_t)c * 8u;
    int dot = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
      const uint4 va = ra[k], vb = rb[k];
      dot = __builtin_amdgcn_sdot4((int)(va.x ^ 0x80808080u), (int)(vb.x ^ 0x80808080u), dot, false);
      dot = __builtin_amdgcn_sdot4((int)(va.y ^ 0x80808080u), (int)(vb.y ^ 0x80808080u), dot, false);
      dot = __builtin_amdgcn_sdot4((int)(va.z ^ 0x80808080u), (int)(vb.z ^ 0x80808080u), dot, false);
      dot = __builtin_amdgcn_sdot4((int)(va.w ^ 0x80808080u), (int)(vb.w ^ 0x80808080u), dot, false);
    }
    const uint32_t d2 = (uint32_t)((int)norm_own[row0 + o] + (int)norm_oth[c] - 2 * dot);
    const unsigned long long key = ((unsigned long long)d2 << 32) | (unsigned long long)c;
    const unsigned long long old = atomicMin(&s_k1[o], key);
    atomicMin(&s_k2[o], old > key ? old : key);
  };

  for (uint32_t base = 0; base < n_oth; base += kTile)
  {
    __syncthreads(); // every wave is through with the previous tile
    {
      const uint32_t r = base + tid;
      const float2 p = r < n_oth ? xy_oth[r] : float2{bad, bad};
      tile[tid] = REVERSE ? side_a<MODEL>(M, p, t2) : side_b<MODEL>(M, p);
    }
    __syncthreads();
    const uint32_t m = n_oth - base < kTile ? n_oth - base : kTile; // (the tile is NaN beyond m: chunks need no tail)
    for (uint32_t j0 = 0; j0 < m; j0 += kChunk)
    {
      uint32_t mask = 0;
#pragma unroll
      for (uint32_t k = 0; k < kChunk; k++)
      {
        const float4 t = tile[j0 + k]; // every lane reads the same 16 bytes: one broadcast LDS access
        const bool ok = REVERSE ? admissible<MODEL>(t, q_own, t2) : admissible<MODEL>(q_own, t, t2);
        mask |= ok ? (1u << k) : 0u;
      }
      if (mask)
      {
        uint32_t pos = atomicAdd(&s_qn[wave], (uint32_t)__popc(mask));
        while (mask)
        {
          const uint32_t k = (uint32_t)__ffs((int)mask) - 1u;
          mask &= mask - 1u;
          q[pos++] = (tid << 24) | (base + j0 + k);
        }
      }
      wave_sync();
      const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&s_qn[wave], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (n >= 64u) // uniform over the wave
      {
        uint32_t head = 0;
        for (; n - head >= 64u; head += 64u)
          drain_entry(q[head + lane]);
        const uint32_t rem = n - head;
        const uint32_t left = lane < rem ? q[head + lane] : 0u;
        wave_sync();
        if (lane < rem)
          q[lane] = left;
        if (lane == 0u)
          s_qn[wave] = rem;
        wave_sync();
      }
    }
  }
  wave_sync();
  {
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&s_qn[wave], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (lane < n) // fewer than 64 are left
      drain_entry(q[lane]);
  }
  wave_sync();
  if (own < n_own)
  {
    unsigned long long *k = keys + (((size_t)2u * slot + (REVERSE ? 1u : 0u)) * max_n + own) * 2u;
    k[0] = s_k1[tid], k[1] = s_k2[tid];
  }
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float key_dist(unsigned long long k) { return k == kNoKey ? __uint_as_float(0x7f800000u) : sqrtf((float)(uint32_t)(k >> 32)); }

// One 1024-thread workgroup per slot: the match (a, idx(k1(a))) is kept iff dist1 <= max_distance, dist1 / dist2 < ratio (true without a
// second candidate, false for 0 / 0) and, with cross_check, idx(k1_rev(b)) == a and the reverse record passes its own ratio test. 16-byte records {idx_a, idx_b, dist1, dist2} in increasing idx_a, their number in out_n[slot].
__global__ void __launch_bounds__(1024)
    k_guided_keep(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ n_dev, uint32_t n_stride, uint32_t max_n,
                  const uint32_t *__restrict__ valid, uint32_t valid_stride, float ratio, float max_distance, uint32_t cross_check, uint32_t *__restrict__ out,
                  uint64_t out_slot_stride, uint32_t *__restrict__ out_n)
{
  __shared__ uint32_t wave_tot[16];
  __shared__ uint32_t carry_s;
  const uint32_t slot = blockIdx.x;
  const unsigned long long *fwd = keys + (size_t)2u * slot * max_n * 2u, *rev = fwd + (size_t)max_n * 2u;
  out += (size_t)slot * out_slot_stride;
  uint32_t na = n_dev[(size_t)slot * n_stride], nb = n_dev[(size_t)slot * n_stride + 1u];
  na = na < max_n ? na : max_n, nb = nb < max_n ? nb : max_n;
  if (valid[(size_t)slot * valid_stride] == 0u)
    na = 0u;
  if (threadIdx.x == 0)
    carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < na; base += 1024u)
  {
    const uint32_t i = base + threadIdx.x;
    bool keep = false;
    uint32_t j = 0;
    float d1 = 0.f, d2 = 0.f;
    if (i < na)
    {
      const unsigned long long k1 = fwd[(size_t)i * 2u], k2 = fwd[(size_t)i * 2u + 1u];
      if (k1 != kNoKey)
      {
        j = (uint32_t)k1;
        d1 = key_dist(k1), d2 = key_dist(k2);
        keep = d1 <= max_distance && (d1 / d2) < ratio;
        if (cross_check)
        {
          keep = keep && j < nb;
          if (keep)
          {
            const unsigned long long r1 = rev[(size_t)j * 2u], r2 = rev[(size_t)j * 2u + 1u];
            keep = r1 != kNoKey && (uint32_t)r1 == i && (key_dist(r1) / key_dist(r2)) < ratio;
          }
        }
      }
    }
    uint32_t *o = out + (size_t)ordered_keep(keep, wave_tot, carry_s) * 4u;
    if (keep)
      o[0] = i, o[1] = j, o[2] = __float_as_uint(d1), o[3] = __float_as_uint(d2);
  }
  if (threadIdx.x == 0)
    out_n[slot] = carry_s;
}

using SweepKernel = void (*)(const uint8_t *, uint64_t, const uint32_t *, uint64_t, const uint32_t *, uint32_t, const float2 *, uint64_t, const uint32_t *, uint32_t,
                             uint32_t, const float *, uint32_t, const uint32_t *, uint32_t, float, unsigned long long *);

} // namespace

extern "C"
{
  size_t vksift_hip_guided_scratch_u32(uint32_t nslots, uint32_t max_n) { return (size_t)nslots * max_n * 8u; }

  int vksift_hip_gather_xy(const uint8_t *feats_base, uint64_t buf_stride, const uint32_t *found_base, uint32_t found_buf_stride, const uint32_t *slot_tab,
                           const uint32_t *layouts, uint32_t max_n, uint32_t nslots, float *xy, uint64_t xy_side_stride, vksift_hip_stream s)
  {
    if (nslots < 1 || nslots > 0x3fffffffu || xy_side_stride < max_n || ((uintptr_t)xy & 7u))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_xy, dim3(2u * nslots), dim3(256), 0, (hipStream_t)s, feats_base, buf_stride, found_base, found_buf_stride, slot_tab, layouts, max_n,
                       (float2 *)xy, xy_side_stride);
    return (int)hipGetLastError();
  }

  int vksift_hip_match_guided(const uint8_t *cache_desc, uint64_t cache_desc_stride, const uint32_t *cache_norm, uint64_t cache_norm_stride, const uint32_t *slot_tab,
                              uint32_t slot_tab_stride, const float *xy, uint64_t xy_side_stride, const uint32_t *n_dev, uint32_t n_stride, uint32_t max_n,
                              const float *models, uint32_t model_stride, const uint32_t *valid, uint32_t valid_stride, uint32_t model_kind, float t2, float ratio,
                              float max_distance, uint32_t cross_check, uint32_t nslots, uint8_t *out, uint64_t out_slot_stride, uint32_t *out_n, uint32_t *scratch,
                              size_t scratch_u32, vksift_hip_stream s)
  {
    if (model_kind > VKSIFT_HIP_GUIDE_FUNDAMENTAL || !(t2 > 0.f) || !isfinite(t2) || !(ratio > 0.f) || !(max_distance > 0.f) || nslots < 1 || nslots > 65535u ||
        max_n > (1u << 24) || scratch_u32 < vksift_hip_guided_scratch_u32(nslots, max_n) || ((uintptr_t)scratch & 7u) || ((uintptr_t)cache_desc & 15u) ||
        (cache_desc_stride & 15u) || ((uintptr_t)xy & 7u) || ((uintptr_t)out & 3u) || (out_slot_stride & 3u) || cache_desc_stride < 128u * (uint64_t)max_n ||
        cache_norm_stride < max_n || xy_side_stride < max_n || out_slot_stride < 16u * (uint64_t)max_n || slot_tab_stride < 2u || n_stride < 2u ||
        model_stride < 9u || valid_stride < 1u)
      return (int)hipErrorInvalidValue;
    const uint32_t tiles = (max_n + kTile - 1u) / kTile;
    const bool f = model_kind == VKSIFT_HIP_GUIDE_FUNDAMENTAL;
    unsigned long long *keys = (unsigned long long *)scratch;
    if (tiles > 0u)
    {
      const SweepKernel fwd = f ? k_guided_2nn<(int)VKSIFT_HIP_GUIDE_FUNDAMENTAL, false> : k_guided_2nn<(int)VKSIFT_HIP_GUIDE_HOMOGRAPHY, false>;
      const SweepKernel rev = f ? k_guided_2nn<(int)VKSIFT_HIP_GUIDE_FUNDAMENTAL, true> : k_guided_2nn<(int)VKSIFT_HIP_GUIDE_HOMOGRAPHY, true>;
      hipLaunchKernelGGL(fwd, dim3(tiles, nslots), dim3(kTile), 0, (hipStream_t)s, cache_desc, cache_desc_stride, cache_norm, cache_norm_stride, slot_tab,
                         slot_tab_stride, (const float2 *)xy, xy_side_stride, n_dev, n_stride, max_n, models, model_stride, valid, valid_stride, t2, keys);
      int e = (int)hipGetLastError();
      if (e)
        return e;
      if (cross_check)
      {
        hipLaunchKernelGGL(rev, dim3(tiles, nslots), dim3(kTile), 0, (hipStream_t)s, cache_desc, cache_desc_stride, cache_norm, cache_norm_stride, slot_tab,
                           slot_tab_stride, (const float2 *)xy, xy_side_stride, n_dev, n_stride, max_n, models, model_stride, valid, valid_stride, t2, keys);
        e = (int)hipGetLastError();
        if (e)
          return e;
      }
    }
    hipLaunchKernelGGL(k_guided_keep, dim3(nslots), dim3(1024), 0, (hipStream_t)s, (const unsigned long long *)keys, n_dev, n_stride, max_n, valid, valid_stride, ratio,
                       max_distance, cross_check ? 1u : 0u, (uint32_t *)out, out_slot_stride / 4u, out_n);
    return (int)hipGetLastError();
  }
}
