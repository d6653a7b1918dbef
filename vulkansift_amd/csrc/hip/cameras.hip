// cameras.hip — the motion half of resection-intersection on the observation table: the table's per-view index (vksift_hip_index_views) and the
// refinement of every camera on the triangulated points, the points held fixed (vksift_hip_refine_cameras). No counterpart in the reference, whose
// callers download the table and the points, invert the table by view on the host and run a Gauss-Newton per view there. DESIGN.md, "Camera
// refinement", holds the argument; the header (include/vksift_hip.h) the contract and the rule, tests/np_cameras.py restates both bit for bit.
//
// The index is a stable LSD radix sort of the observation numbers by gpu_buffer_id with the pass structure of observations.hip (its own passes: the
// tile and the element type are the same, the keys and what is carried are not). A launch sequence on one stream; every phase that reads another
// phase's plain stores is a launch of its own:
//   k_view_keys     observation i -> {key, i} and its point (a binary search in offsets); key VW_NONE for what is left out and for the padding
//   per 8-bit digit, low to high: k_view_hist, k_view_scan, k_view_scatter (per-block LDS histograms into a digit-major table, one scan workgroup,
//                   ballot match groups per wave)
//   k_view_offsets  view_offsets[b] = the first sorted position whose key is not below b (one workgroup), and the statistics
//   k_view_expand   sorted position p -> {point, row, x, y}
// The refinement: one workgroup of 256 lanes per view (CAM_THREADS is part of the rule: the order of every sum), refit.h's fixed-order block sums, a 6x7
// Gauss-Jordan in registers, everything correctly rounded fp32 add / sub / mul / div in a written order (the tree is built with -ffp-contract=off and
// nothing is fused here):
//   k_refine_cameras  the evaluation at P, up to nb_steps steps P' = P [[C, tau], [0, 1]], the record
//   k_cam_stats       the four statistics, counted from the records by one workgroup
// No scratch memory, no atomics on global memory, no lane waits for another workgroup, every grid and loop is bounded by the launcher's arguments
// (counts read on the device are clamped to them), and every output depends on the inputs alone.
#include "vksift_hip.h"
#include "hip/refit.h"
#include "wave.h"

#include <hip/hip_runtime.h>

#define VW_THREADS 256u
#define VW_ITEMS 8u
#define VW_TILE (VW_THREADS * VW_ITEMS) /* elements per sort block */
#define VW_NONE 0xFFFFFFFFu             /* the key of an observation that is left out, and of the last sort block's padding */

#define CAM_THREADS 256u
#define CAM_SUMS 28                     /* cost, the 21 upper entries of N row by row, the 6 entries of g */
#define CAM_WORDS 18u                   /* vksift_ext_RefinedCamera */
#define CAM_MIN_OBS 6u                  /* VKSIFT_EXT_CAMERA_MIN_OBSERVATIONS */
#define CAM_MAX_STEPS 8u
#define CAM_ABSENT 1u
#define CAM_TOO_FEW 2u
#define CAM_DEGENERATE 4u
#define CAM_BEHIND 8u

namespace
{

using refit::abs_bits;
using refit::finite_bits;
using refit::unusable_bits;

// ============================================================================================================ the per-view index
__device__ __forceinline__ uint32_t clamped(uint32_t v, uint32_t bound) { return v < bound ? v : bound; }

// The selected track whose extent holds observation i: the last m of [0, M) the search below reaches with offsets[m] <= i (M >= 1), VW_NONE when the
// extent found does not hold i or ends beyond the table's nobs observations (the triangulation's test of an extent)
__device__ __forceinline__ uint32_t point_of(const uint32_t *__restrict__ offsets, uint32_t M, uint32_t nobs, uint32_t i)
{
  uint32_t lo = 0u, hi = M;
  while (hi - lo > 1u)
  {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (offsets[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t begin = offsets[lo], end = offsets[lo + 1u];
  return (begin <= i && i < end && end <= nobs) ? lo : VW_NONE;
}

// element e of the padded list: pts[e] is written for every e, so that every word the later launches read is written
__global__ __launch_bounds__(VW_THREADS) void k_view_keys(const uint32_t *__restrict__ offsets, const uint4 *__restrict__ obs, const uint32_t *__restrict__ obs_stats,
                                                          uint32_t tracks_cap, uint32_t obs_cap, uint32_t nb_cameras, uint32_t *__restrict__ keys,
                                                          uint32_t *__restrict__ vals, uint32_t *__restrict__ pts)
{
  const uint32_t e = blockIdx.x * VW_THREADS + threadIdx.x;
  const uint32_t M = clamped(obs_stats[0], tracks_cap), nobs = clamped(obs_stats[1], obs_cap);
  uint32_t key = VW_NONE, m = VW_NONE;
  if (e < nobs && M != 0u)
  {
    const uint32_t buf = obs[e].x;
    m = point_of(offsets, M, nobs, e);
    if (buf < nb_cameras && m != VW_NONE)
      key = buf;
  }
  keys[e] = key, vals[e] = e, pts[e] = m;
}

// a[0 .. n) becomes its exclusive prefix sum. One workgroup of 1024; wsum: 17 words of LDS.
__device__ __forceinline__ void view_scan_1024(uint32_t *a, uint32_t n, uint32_t (&wsum)[17])
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 1024u)
  {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n ? a[i] : 0u;
    const uint32_t incl = wave_scan_incl_u32(v, lane);
    if (lane == 63)
      wsum[wave] = incl;
    __syncthreads();
    if (wave == 0)
    {
      const uint32_t t = lane < 16 ? wsum[lane] : 0u;
      const uint32_t ti = wave_scan_incl_u32(t, lane);
      if (lane < 16)
        wsum[lane] = ti - t;
      if (lane == 15)
        wsum[16] = ti;
    }
    __syncthreads();
    if (i < n)
      a[i] = carry + wsum[wave] + incl - v;
    carry += wsum[16];
    __syncthreads();
  }
}

// table[d * gridDim.x + block] = the elements of the block whose digit is d
__global__ __launch_bounds__(VW_THREADS) void k_view_hist(const uint32_t *__restrict__ keys, uint32_t shift, uint32_t *__restrict__ table)
{
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t *k = keys + (size_t)blockIdx.x * VW_TILE;
  for (uint32_t r = 0; r < VW_ITEMS; r++)
    atomicAdd(&hist[(k[r * VW_THREADS + threadIdx.x] >> shift) & 255u], 1u); // LDS
  __syncthreads();
  table[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(1024) void k_view_scan(uint32_t *table, uint32_t n)
{
  __shared__ uint32_t wsum[17];
  view_scan_1024(table, n, wsum);
}

// The block's elements go, in element order, behind the elements of the blocks in front of it that share their digit: rounds of 256 in order, inside a
// round the waves in order, inside a wave the lanes in order. A position is below the padded length: the table's counts add up to it.
__global__ __launch_bounds__(VW_THREADS) void k_view_scatter(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t shift,
                                                             const uint32_t *__restrict__ table, uint32_t padded, uint32_t *__restrict__ keys_out,
                                                             uint32_t *__restrict__ vals_out)
{
  __shared__ uint32_t base[256], wcnt[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  base[threadIdx.x] = table[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
  for (int w = 0; w < 4; w++)
    wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  const size_t first = (size_t)blockIdx.x * VW_TILE;
  for (uint32_t r = 0; r < VW_ITEMS; r++)
  {
    const uint32_t key = keys[first + r * VW_THREADS + threadIdx.x], val = vals[first + r * VW_THREADS + threadIdx.x];
    const uint32_t d = (key >> shift) & 255u;
    unsigned long long same = ~0ull; // the lanes of the wave with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++)
    {
      const unsigned long long bal = __ballot((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t rank = ballot_rank(same, lane);
    if (rank == 0u)
      wcnt[wave][d] = (uint32_t)__popcll(same); // (one lane per digit and wave)
    __syncthreads();
    uint32_t pos = base[d] + rank;
    for (int w = 0; w < wave; w++)
      pos += wcnt[w][d];
    if (pos < padded) // (always)
      keys_out[pos] = key, vals_out[pos] = val;
    __syncthreads();
    base[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
    for (int w = 0; w < 4; w++)
      wcnt[w][threadIdx.x] = 0;
    __syncthreads();
  }
}

// the first position of the sorted keys[0 .. n) whose key is not below b
__device__ __forceinline__ uint32_t first_not_below(const uint32_t *__restrict__ keys, uint32_t n, uint32_t b)
{
  uint32_t lo = 0u, hi = n;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (keys[mid] < b)
      lo = mid + 1u;
    else
      hi = mid;
  }
  return lo;
}

// one workgroup of 1024: view_offsets[0 .. nb_cameras], stats = {views with an observation, observations indexed, the largest view, 0}
__global__ __launch_bounds__(1024) void k_view_offsets(const uint32_t *__restrict__ keys, uint32_t padded, uint32_t nb_cameras, uint32_t *__restrict__ view_offsets,
                                                       uint32_t *__restrict__ stats)
{
  __shared__ uint32_t part[16][2];
  uint32_t views = 0u, largest = 0u;
  for (uint32_t b = threadIdx.x; b < nb_cameras; b += 1024u)
  {
    const uint32_t lo = first_not_below(keys, padded, b), hi = first_not_below(keys, padded, b + 1u);
    view_offsets[b] = lo;
    if (b + 1u == nb_cameras)
      view_offsets[nb_cameras] = hi, stats[1] = hi;
    views += hi > lo ? 1u : 0u;
    largest = max(largest, hi - lo);
  }
  views = wave_sum_u32(views), largest = wave_max_u32(largest);
  if ((threadIdx.x & 63u) == 0u)
    part[threadIdx.x >> 6][0] = views, part[threadIdx.x >> 6][1] = largest;
  __syncthreads();
  if (threadIdx.x == 0u)
  {
    uint32_t v = 0u, l = 0u;
    for (int w = 0; w < 16; w++)
      v += part[w][0], l = max(l, part[w][1]);
    stats[0] = v, stats[2] = l, stats[3] = 0u;
  }
}

// the indexed observations are the sorted positions in front of the first VW_NONE key
__global__ __launch_bounds__(VW_THREADS) void k_view_expand(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ pts,
                                                            const uint4 *__restrict__ obs, uint32_t obs_cap, uint4 *__restrict__ view_obs)
{
  const uint32_t p = blockIdx.x * VW_THREADS + threadIdx.x;
  if (p >= obs_cap || keys[p] == VW_NONE)
    return;
  const uint32_t i = vals[p];
  if (i >= obs_cap) // (never: a key other than VW_NONE belongs to an observation below the clamped count)
    return;
  const uint4 o = obs[i];
  view_obs[p] = uint4{pts[i], o.y, o.z, o.w};
}

inline uint64_t view_sort_blocks(uint64_t obs_cap) { return (obs_cap + VW_TILE - 1u) / VW_TILE; }

// ============================================================================================================ camera refinement
struct CamLds
{
  float part[4][CAM_SUMS]; // the waves' partial sums
  float total[CAM_SUMS];   // ((w0 + w1) + w2) + w3
  uint32_t upart[4];
};

// refit.h's block sum — the 64 lanes of a wave by the xor butterfly, offsets 32 .. 1, the four waves as ((w0 + w1) + w2) + w3 —, the result in every
// lane. The four-term sum of entry i is formed once, by lane i, and read back by all: a lane that read the 4 x 28 partials itself would hold them in
// registers until the solve uses them.
__device__ __forceinline__ void cam_block_sum(float (&v)[CAM_SUMS], CamLds &sh)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int i = 0; i < CAM_SUMS; i++)
      v[i] = v[i] + __shfl_xor(v[i], off, 64);
  __syncthreads(); // the previous reduction's readers are through with the LDS
  if ((threadIdx.x & 63u) == 0u)
  {
#pragma unroll
    for (int i = 0; i < CAM_SUMS; i++)
      sh.part[threadIdx.x >> 6][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < CAM_SUMS)
    sh.total[threadIdx.x] = ((sh.part[0][threadIdx.x] + sh.part[1][threadIdx.x]) + sh.part[2][threadIdx.x]) + sh.part[3][threadIdx.x];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CAM_SUMS; i++)
    v[i] = sh.total[i];
}

// a x b, each component (a1 b2) - (a2 b1): the triangulation's
__device__ __forceinline__ void cross3(const float *a, const float *b, float (&c)[3])
{
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// What a step and the record need at a camera P, uniform over the workgroup
struct CamEval
{
  float s[CAM_SUMS];
  uint32_t used;   // the used members
  uint32_t flags;  // 1: some w is zero, subnormal or not finite; 2: some w <= 0
  uint32_t max_e2; // the largest squared error by |bit pattern|
};

// lane j visits positions j, j + 256, ... of the view's n records in increasing order
__device__ __forceinline__ CamEval cam_evaluate(const float (&P)[12], const uint4 *__restrict__ members, uint32_t n, const uint4 *__restrict__ points,
                                                uint32_t points_cap, CamLds &sh)
{
  CamEval E;
#pragma unroll
  for (int i = 0; i < CAM_SUMS; i++)
    E.s[i] = 0.f;
  E.used = 0u, E.flags = 0u, E.max_e2 = 0u;
  for (uint32_t k = threadIdx.x; k < n; k += CAM_THREADS)
  {
    const uint4 o = members[k];
    if (o.x >= points_cap) // no such point: not used, nothing read
      continue;
    const uint4 tail = points[2u * (size_t)o.x + 1u];
    if (tail.y != 0u) // USED iff the status word of the point is 0
      continue;
    const uint4 head = points[2u * (size_t)o.x];
    const float X[3] = {__uint_as_float(head.x), __uint_as_float(head.y), __uint_as_float(head.z)};
    const float x = __uint_as_float(o.z), y = __uint_as_float(o.w);
    const float u = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const float v = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    const float w = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    const float pu = u / w, pv = v / w;
    const float ru = pu - x, rv = pv - y;
    const float e2 = ru * ru + rv * rv;
    const float iw = 1.0f / w;
    float ju[3], jv[3], p[6], q[6];
#pragma unroll
    for (int i = 0; i < 3; i++)
      ju[i] = (P[i] - pu * P[8 + i]) * iw, jv[i] = (P[4 + i] - pv * P[8 + i]) * iw;
    float au[3], av[3];
    cross3(X, ju, au);
    cross3(X, jv, av);
#pragma unroll
    for (int i = 0; i < 3; i++)
      p[i] = au[i], p[3 + i] = ju[i], q[i] = av[i], q[3 + i] = jv[i];
    E.s[0] = E.s[0] + e2;
    int at = 1;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = a; b < 6; b++, at++)
        E.s[at] = E.s[at] + (p[a] * p[b] + q[a] * q[b]);
#pragma unroll
    for (int a = 0; a < 6; a++)
      E.s[22 + a] = E.s[22 + a] + (p[a] * ru + q[a] * rv);
    E.used++;
    E.flags |= (unusable_bits(w) ? 1u : 0u) | (w <= 0.f ? 2u : 0u);
    E.max_e2 = max(E.max_e2, abs_bits(e2));
  }
  cam_block_sum(E.s, sh);
  E.used = refit::block_u32<false>(E.used, sh.upart);
  E.flags = refit::block_u32<true>(E.flags & 1u, sh.upart) | (refit::block_u32<true>(E.flags & 2u, sh.upart));
  E.max_e2 = refit::block_u32<true>(E.max_e2, sh.upart);
  return E;
}

// N d = -g from the 28 sums: refit.h's elimination for a 6x7 system — Gauss-Jordan, for column k the rows below compared with row k in turn and exchanged
// when their |entry| (bit pattern) is strictly larger; row k times 1 / pivot; every other row r minus a[r][k] times row k. false: an unusable pivot or a
// solution entry that is not finite. The system is spread over the lanes of each wave, which all hold the same sums: lane c < 6 keeps column c, every
// other lane the right-hand side, so a lane holds six entries and not forty-two. Column k is broadcast from lane k before it is used; each entry sees
// exactly the operations the elimination in one lane's registers would apply to it (columns at and in front of k go on being updated; nothing reads them).
__device__ __forceinline__ bool cam_solve(const float *s, float (&d)[6])
{
  const uint32_t lane = threadIdx.x & 63u;
  float col[6];
#pragma unroll
  for (int r = 0; r < 6; r++)
  {
    float v = -s[22 + r];
#pragma unroll
    for (int c = 0; c < 6; c++)
    {
      const int lo = r < c ? r : c, hi = r < c ? c : r; // N[lo][hi] is sum 1 + (6 lo - lo (lo - 1) / 2) + (hi - lo)
      v = lane == (uint32_t)c ? s[1 + 6 * lo - (lo * (lo - 1)) / 2 + (hi - lo)] : v;
    }
    col[r] = v;
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++)
  {
    float piv[6]; // column k, the same in every lane
#pragma unroll
    for (int r = k; r < 6; r++)
      piv[r] = __shfl(col[r], k, 64);
#pragma unroll
    for (int r = k + 1; r < 6; r++)
    {
      const bool sw = abs_bits(piv[r]) > abs_bits(piv[k]);
      const float top = col[k], low = col[r], ptop = piv[k], plow = piv[r];
      col[k] = sw ? low : top, col[r] = sw ? top : low;
      piv[k] = sw ? plow : ptop, piv[r] = sw ? ptop : plow;
    }
    ok = ok && !unusable_bits(piv[k]);
    const float inv = 1.0f / piv[k];
    col[k] = col[k] * inv;
#pragma unroll
    for (int r = 0; r < 6; r++)
      if (r != k)
        col[r] = col[r] - __shfl(col[r], k, 64) * col[k];
  }
#pragma unroll
  for (int r = 0; r < 6; r++)
    d[r] = __shfl(col[r], 6, 64), ok = ok && finite_bits(d[r]);
  return ok;
}

// P becomes P [[C, tau], [0, 1]] with the Cayley rotation C of omega = d[0..2] and tau = d[3..5]; false when an entry of it is not finite
__device__ __forceinline__ bool cam_step(float (&P)[12], const float (&d)[6])
{
  const float a[3] = {0.5f * d[0], 0.5f * d[1], 0.5f * d[2]};
  const float a2[3] = {2.0f * a[0], 2.0f * a[1], 2.0f * a[2]};
  const float q = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
  const float s = 1.0f / (1.0f + q), t = 1.0f - q;
  float C[3][3];
  C[0][0] = (t + a2[0] * a[0]) * s, C[0][1] = (a2[0] * a[1] - a2[2]) * s, C[0][2] = (a2[0] * a[2] + a2[1]) * s;
  C[1][0] = (a2[1] * a[0] + a2[2]) * s, C[1][1] = (t + a2[1] * a[1]) * s, C[1][2] = (a2[1] * a[2] - a2[0]) * s;
  C[2][0] = (a2[2] * a[0] - a2[1]) * s, C[2][1] = (a2[2] * a[1] + a2[0]) * s, C[2][2] = (t + a2[2] * a[2]) * s;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    const float p0 = P[4 * r], p1 = P[4 * r + 1], p2 = P[4 * r + 2];
#pragma unroll
    for (int c = 0; c < 3; c++)
      P[4 * r + c] = (p0 * C[0][c] + p1 * C[1][c]) + p2 * C[2][c];
    P[4 * r + 3] = ((p0 * d[3] + p1 * d[4]) + p2 * d[5]) + P[4 * r + 3];
  }
#pragma unroll
  for (int i = 0; i < 12; i++)
    ok = ok && finite_bits(P[i]);
  return ok;
}

// workgroup b refines the camera of gpu_buffer_id b
__global__ __launch_bounds__(CAM_THREADS) void k_refine_cameras(const uint32_t *__restrict__ view_offsets, const uint4 *__restrict__ view_obs,
                                                                const uint32_t *__restrict__ view_stats, uint32_t obs_cap, const uint4 *__restrict__ points,
                                                                uint32_t points_cap, const float4 *__restrict__ cameras, const uint32_t *__restrict__ buf_tab,
                                                                uint32_t nbufs, uint32_t nb_steps, uint32_t *__restrict__ out)
{
  __shared__ CamLds sh;
  const uint32_t b = blockIdx.x;
  uint32_t *rec = out + (size_t)CAM_WORDS * b;
  // took the buffer part in the build? its id is one of the nbufs entries of the table (uniform after the reduction)
  uint32_t present = 0u;
  for (uint32_t r = threadIdx.x; r < nbufs; r += CAM_THREADS)
    present |= buf_tab[2u * (size_t)r] == b ? 1u : 0u;
  present = refit::block_u32<true>(present, sh.upart);
  if (present == 0u)
  {
    if (threadIdx.x < CAM_WORDS)
      rec[threadIdx.x] = threadIdx.x == CAM_WORDS - 1u ? CAM_ABSENT : 0u;
    return;
  }
  // the view's extent, clamped to the index's own count
  const uint32_t total = clamped(view_stats[1], obs_cap);
  const uint32_t end = clamped(view_offsets[b + 1u], total), begin = clamped(view_offsets[b], end);
  const uint32_t n = end - begin;
  const uint4 *members = view_obs + begin;
  // One call site of the evaluation: round 0 evaluates the input camera, round `it` the candidate of step `it`. What is kept of an evaluation is the
  // cost, the flags and the largest error (its sums are consumed by the solve of the next step); the camera kept so far is in the record, the next
  // candidate is formed from it in place.
  float Q[12];
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    const float4 q = cameras[3u * (size_t)b + r];
    Q[4 * r] = q.x, Q[4 * r + 1] = q.y, Q[4 * r + 2] = q.z, Q[4 * r + 3] = q.w;
  }
  uint32_t status = 0u, steps = 0u, used = 0u, flags = 0u, max_e2 = 0u;
  float cost_start = 0.f, cost = 0.f;
  for (uint32_t it = 0;; it++)
  {
    const CamEval F = cam_evaluate(Q, members, n, points, points_cap, sh);
    if (it == 0u)
    {
      used = F.used;
      if (used < CAM_MIN_OBS)
        status = CAM_TOO_FEW;
      else if ((F.flags & 1u) || !finite_bits(F.s[0]))
        status = CAM_DEGENERATE;
      else
        cost_start = F.s[0];
    }
    else if (!(F.s[0] <= cost))
      break;
    if (threadIdx.x < 12u) // the camera kept so far (every lane holds the same Q; the selects keep the indices constant)
    {
      float v = Q[0];
#pragma unroll
      for (int i = 1; i < 12; i++)
        v = threadIdx.x == (uint32_t)i ? Q[i] : v;
      rec[threadIdx.x] = __float_as_uint(v);
    }
    if (status != 0u)
      break;
    cost = F.s[0], flags = F.flags, max_e2 = F.max_e2, steps = it;
    float d[6];
    if (it == nb_steps || (flags & 1u) || !cam_solve(F.s, d) || !cam_step(Q, d))
      break;
  }
  float max_sq_error = 0.f;
  if (status == 0u)
  {
    max_sq_error = __uint_as_float(max_e2 > 0x7f800000u ? 0x7fc00000u : max_e2);
    status = (flags & 2u) ? CAM_BEHIND : 0u;
  }
  if (threadIdx.x == 0u)
  {
    rec[12] = __float_as_uint(cost_start), rec[13] = __float_as_uint(cost), rec[14] = __float_as_uint(max_sq_error);
    rec[15] = used, rec[16] = steps, rec[17] = status;
  }
}

// stats = {views (not ABSENT), refined (steps > 0), unchanged (status 0 or BEHIND only, no step), failed (TOO_FEW or DEGENERATE)}
__global__ __launch_bounds__(1024) void k_cam_stats(const uint32_t *__restrict__ recs, uint32_t nb_cameras, uint32_t *__restrict__ stats)
{
  __shared__ uint32_t part[16][4];
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  for (uint32_t b = threadIdx.x; b < nb_cameras; b += 1024u)
  {
    const uint32_t steps = recs[(size_t)CAM_WORDS * b + 16u], st = recs[(size_t)CAM_WORDS * b + 17u];
    if (st & CAM_ABSENT)
      continue;
    c[0]++;
    c[(st & (CAM_TOO_FEW | CAM_DEGENERATE)) ? 3 : steps > 0u ? 1 : 2]++;
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
    c[i] = wave_sum_u32(c[i]);
  if ((threadIdx.x & 63u) == 0u)
  {
#pragma unroll
    for (int i = 0; i < 4; i++)
      part[threadIdx.x >> 6][i] = c[i];
  }
  __syncthreads();
  if (threadIdx.x < 4u)
  {
    uint32_t t = 0u;
    for (int w = 0; w < 16; w++)
      t += part[w][threadIdx.x];
    stats[threadIdx.x] = t;
  }
}

} // namespace

extern "C" size_t vksift_hip_views_scratch_u32(uint64_t obs_cap)
{
  const uint64_t blocks = view_sort_blocks(obs_cap);
  // two {key, observation} lists of whole sort blocks, the points of the observations, the digit table
  return (size_t)(5u * blocks * VW_TILE + 256u * blocks);
}

extern "C" int vksift_hip_index_views(const uint32_t *offsets, const uint8_t *observations, const uint32_t *obs_stats, uint64_t tracks_cap, uint64_t obs_cap,
                                      uint32_t nb_cameras, uint32_t *view_offsets, uint8_t *view_observations, uint32_t *stats, uint32_t *scratch,
                                      size_t scratch_u32, vksift_hip_stream s)
{
  const uint64_t blocks = view_sort_blocks(obs_cap);
  if (!offsets || !observations || !obs_stats || !view_offsets || !view_observations || !stats || !scratch || nb_cameras == 0u || nb_cameras == VW_NONE ||
      tracks_cap == 0u || tracks_cap > 0x7FFFFFFFull || obs_cap == 0u || blocks * VW_TILE > 0x7FFFFFFFull || ((uintptr_t)offsets & 3u) ||
      ((uintptr_t)obs_stats & 3u) || ((uintptr_t)view_offsets & 3u) || ((uintptr_t)stats & 3u) || ((uintptr_t)scratch & 3u) || ((uintptr_t)observations & 15u) ||
      ((uintptr_t)view_observations & 15u) || scratch_u32 < vksift_hip_views_scratch_u32(obs_cap))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s;
  const uint32_t sort_blocks = (uint32_t)blocks, padded = sort_blocks * VW_TILE, cap = (uint32_t)obs_cap;
  uint32_t *keys[2], *vals[2];
  keys[0] = scratch, vals[0] = keys[0] + padded, keys[1] = vals[0] + padded, vals[1] = keys[1] + padded;
  uint32_t *pts = vals[1] + padded, *table = pts + padded;
  k_view_keys<<<sort_blocks * VW_ITEMS, VW_THREADS, 0, st>>>(offsets, (const uint4 *)observations, obs_stats, (uint32_t)tracks_cap, cap, nb_cameras, keys[0], vals[0],
                                                             pts);
  // a key is below nb_cameras or VW_NONE, whose digits are all 255: `passes` digits order them as long as nb_cameras < 256^passes
  uint32_t passes = 1;
  while (passes < 4u && (nb_cameras >> (8u * passes)) != 0u)
    passes++;
  uint32_t cur = 0;
  for (uint32_t p = 0; p < passes; p++, cur ^= 1u)
  {
    k_view_hist<<<sort_blocks, VW_THREADS, 0, st>>>(keys[cur], 8u * p, table);
    k_view_scan<<<1, 1024, 0, st>>>(table, 256u * sort_blocks);
    k_view_scatter<<<sort_blocks, VW_THREADS, 0, st>>>(keys[cur], vals[cur], 8u * p, table, padded, keys[cur ^ 1u], vals[cur ^ 1u]);
  }
  k_view_offsets<<<1, 1024, 0, st>>>(keys[cur], padded, nb_cameras, view_offsets, stats);
  k_view_expand<<<(cap + VW_THREADS - 1u) / VW_THREADS, VW_THREADS, 0, st>>>(keys[cur], vals[cur], pts, (const uint4 *)observations, cap, (uint4 *)view_observations);
  return (int)hipGetLastError();
}

extern "C" int vksift_hip_refine_cameras(const uint32_t *view_offsets, const uint8_t *view_observations, const uint32_t *view_stats, uint64_t obs_cap,
                                         const uint8_t *points, uint64_t points_cap, const float *cameras, uint32_t nb_cameras, const uint32_t *buf_tab,
                                         uint32_t nbufs, uint32_t nb_steps, uint8_t *refined, uint32_t *stats, vksift_hip_stream s)
{
  if (!view_offsets || !view_observations || !view_stats || !points || !cameras || !buf_tab || !refined || !stats || nb_cameras == 0u ||
      nb_cameras > 0x7FFFFFFFu || nbufs == 0u || obs_cap == 0u || obs_cap > 0x7FFFFFFFull || points_cap == 0u || points_cap > 0x7FFFFFFFull || nb_steps == 0u ||
      nb_steps > CAM_MAX_STEPS || ((uintptr_t)view_offsets & 3u) || ((uintptr_t)view_stats & 3u) || ((uintptr_t)buf_tab & 3u) || ((uintptr_t)refined & 3u) ||
      ((uintptr_t)stats & 3u) || ((uintptr_t)view_observations & 15u) || ((uintptr_t)points & 15u) || ((uintptr_t)cameras & 15u))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s;
  k_refine_cameras<<<nb_cameras, CAM_THREADS, 0, st>>>(view_offsets, (const uint4 *)view_observations, view_stats, (uint32_t)obs_cap, (const uint4 *)points,
                                                       (uint32_t)points_cap, (const float4 *)cameras, buf_tab, nbufs, nb_steps, (uint32_t *)refined);
  k_cam_stats<<<1, 1024, 0, st>>>((const uint32_t *)refined, nb_cameras, stats);
  return (int)hipGetLastError();
}
