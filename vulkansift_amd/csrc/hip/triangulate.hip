// triangulate.hip — the selected tracks of the observation table (observations.hip) triangulated under caller-supplied 3x4 cameras
// (vksift_hip_triangulate_tracks; no counterpart in the reference, whose callers download the table and triangulate track by track on the host).
// DESIGN.md, "Triangulation", holds the argument; the header (include/vksift_hip.h) the contract and the rule, tests/np_triangulate.py restates it bit
// for bit.
//
// A group of TRI_G = 16 lanes owns a track, four tracks per wave, sixteen per workgroup. Everything is integer arithmetic or correctly rounded fp32
// add / sub / mul / div / sqrtf in a written order (the tree is built with -ffp-contract=off and no fmaf is used here). Every sum over the members of a
// track has one order whatever the scheduling: lane j adds members j, j + 16, ... in increasing order, the sixteen lanes are added by refit.h's xor
// butterfly (p + p[lane ^ off], off = 8 .. 1: addition commutes, so every lane of the group holds the same bits and solves the same 3x3 system).
// Minima and maxima are taken over integer keys. A launch sequence on one stream:
//   k_triangulate   one group per selected track: bearings and their smallest cosine, the linear start, up to two Gauss-Newton steps, the scoring
//   k_tri_stats     the four statistics, counted from the status words by one workgroup
// No scratch, no atomics on global memory, no lane waits for another workgroup, every grid and loop is bounded by the launcher's arguments (counts read
// on the device are clamped to them, a track's extent to the table's own observation count).
#include "vksift_hip.h"
#include "hip/refit.h"
#include "wave.h"

#include <hip/hip_runtime.h>

#define TRI_THREADS 256u
#define TRI_G 16u                                  /* lanes per track: part of the rule (the order of every sum) */
#define TRI_TRACKS (TRI_THREADS / TRI_G)           /* tracks per workgroup */
#define TRI_MAX_OBS 1024u                          /* VKSIFT_EXT_TRIANGULATE_MAX_OBSERVATIONS */
#define TRI_GN_STEPS 2u
#define TRI_DEGENERATE 1u
#define TRI_TOO_LONG 2u
#define TRI_BEHIND 4u
#define TRI_ERROR 8u
#define TRI_ANGLE 16u
#define TRI_POINT_WORDS 8u

namespace
{

using refit::abs_bits;
using refit::finite_bits;
using refit::unusable_bits;

// ---- over the sixteen lanes of a group, the result in every lane --------------------------------------------------------------------------
template <int N> __device__ __forceinline__ void group_sum(float (&v)[N])
{
#pragma unroll
  for (int off = TRI_G / 2; off >= 1; off >>= 1)
#pragma unroll
    for (int i = 0; i < N; i++)
      v[i] = v[i] + __shfl_xor(v[i], off, 64);
}

__device__ __forceinline__ uint32_t group_or(uint32_t v)
{
#pragma unroll
  for (int off = TRI_G / 2; off >= 1; off >>= 1)
    v |= (uint32_t)__shfl_xor((int)v, off, 64);
  return v;
}

__device__ __forceinline__ uint32_t group_max(uint32_t v)
{
#pragma unroll
  for (int off = TRI_G / 2; off >= 1; off >>= 1)
    v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}

__device__ __forceinline__ int group_min(int v)
{
#pragma unroll
  for (int off = TRI_G / 2; off >= 1; off >>= 1)
    v = min(v, __shfl_xor(v, off, 64));
  return v;
}

// a float as an integer that orders like it (-0 below +0); its own inverse
__device__ __forceinline__ int order_key(int bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }

// ---- one member: its camera and its pixel ---------------------------------------------------------------------------------------------------
struct Member
{
  float P[12];
  float x, y;
  bool cam_ok; // gpu_buffer_id < nb_cameras (camera 0 stands in otherwise: the track is DEGENERATE, nothing of it is published)
};

__device__ __forceinline__ Member load_member(const uint4 *__restrict__ obs, const float4 *__restrict__ cameras, uint32_t nb_cameras, size_t idx)
{
  const uint4 o = obs[idx];
  Member m;
  m.x = __uint_as_float(o.z), m.y = __uint_as_float(o.w), m.cam_ok = o.x < nb_cameras;
  const float4 *c = cameras + 3u * (size_t)(m.cam_ok ? o.x : 0u);
#pragma unroll
  for (int r = 0; r < 3; r++)
  {
    const float4 q = c[r];
    m.P[4 * r] = q.x, m.P[4 * r + 1] = q.y, m.P[4 * r + 2] = q.z, m.P[4 * r + 3] = q.w;
  }
  return m;
}

// member k of the track: lane j keeps its first one (k == j) in registers
#define TRI_MEMBER(k) ((k) == j ? m0 : load_member(obs, cameras, nb_cameras, first + (k)))

// a x b, each component (a1 b2) - (a2 b1)
__device__ __forceinline__ void cross3(const float *a, const float *b, float (&c)[3])
{
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// step 1: the unit bearing of a member; false when its squared length or the scale is zero, subnormal or not finite
__device__ __forceinline__ bool bearing(const Member &m, float (&b)[3])
{
  float c23[3], c31[3], c12[3];
  cross3(m.P + 4, m.P + 8, c23);
  cross3(m.P + 8, m.P, c31);
  cross3(m.P, m.P + 4, c12);
#pragma unroll
  for (int i = 0; i < 3; i++)
    b[i] = (m.x * c23[i] + m.y * c31[i]) + c12[i];
  const float q = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
  const float s = 1.0f / sqrtf(q);
#pragma unroll
  for (int i = 0; i < 3; i++)
    b[i] = b[i] * s;
  return !unusable_bits(q) && !unusable_bits(s);
}

// refit.h's elimination for a 3x4 system: Gauss-Jordan, for column k the rows below compared with row k in turn and exchanged when their |entry| (bit
// pattern) is strictly larger; row k times 1 / pivot; every other row r minus a[r][k] times row k. false: a pivot that is zero, subnormal or not
// finite, or a solution entry that is not finite.
__device__ __forceinline__ bool solve3(float (&a)[3][4], float (&x)[3])
{
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++)
  {
#pragma unroll
    for (int r = k + 1; r < 3; r++)
    {
      const bool sw = abs_bits(a[r][k]) > abs_bits(a[k][k]);
#pragma unroll
      for (int c = k; c < 4; c++)
      {
        const float top = a[k][c], low = a[r][c];
        a[k][c] = sw ? low : top, a[r][c] = sw ? top : low;
      }
    }
    ok = ok && !unusable_bits(a[k][k]);
    const float inv = 1.0f / a[k][k];
#pragma unroll
    for (int c = k + 1; c < 4; c++)
      a[k][c] = a[k][c] * inv;
#pragma unroll
    for (int r = 0; r < 3; r++)
      if (r != k)
      {
        const float f = a[r][k];
#pragma unroll
        for (int c = k + 1; c < 4; c++)
          a[r][c] = a[r][c] - f * a[k][c];
      }
  }
#pragma unroll
  for (int r = 0; r < 3; r++)
    x[r] = a[r][3], ok = ok && finite_bits(x[r]);
  return ok;
}

// the nine sums {S00, S01, S02, S11, S12, S22, r0, r1, r2} of two rows p, q of three entries with right-hand values pr, qr: S += p p^T + q q^T, r += p pr + q qr
__device__ __forceinline__ void add_rows(float *s, const float (&p)[3], float pr, const float (&q)[3], float qr)
{
  s[0] = s[0] + (p[0] * p[0] + q[0] * q[0]);
  s[1] = s[1] + (p[0] * p[1] + q[0] * q[1]);
  s[2] = s[2] + (p[0] * p[2] + q[0] * q[2]);
  s[3] = s[3] + (p[1] * p[1] + q[1] * q[1]);
  s[4] = s[4] + (p[1] * p[2] + q[1] * q[2]);
  s[5] = s[5] + (p[2] * p[2] + q[2] * q[2]);
  s[6] = s[6] + (p[0] * pr + q[0] * qr);
  s[7] = s[7] + (p[1] * pr + q[1] * qr);
  s[8] = s[8] + (p[2] * pr + q[2] * qr);
}

// S d = -r
__device__ __forceinline__ bool solve_normal(const float *s, float (&d)[3])
{
  float a[3][4] = {{s[0], s[1], s[2], -s[6]}, {s[1], s[3], s[4], -s[7]}, {s[2], s[4], s[5], -s[8]}};
  return solve3(a, d);
}

// step 2, per member: the rows x P3 - P1 and y P3 - P2, each times 1 / sqrtf of the squared length of its first three entries
__device__ __forceinline__ bool scaled_row(const Member &m, float t, int row, float (&p)[3], float &pr)
{
  float e[4];
#pragma unroll
  for (int i = 0; i < 4; i++)
    e[i] = t * m.P[8 + i] - m.P[4 * row + i];
  const float q = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
  const float s = 1.0f / sqrtf(q);
#pragma unroll
  for (int i = 0; i < 3; i++)
    p[i] = e[i] * s;
  pr = e[3] * s;
  return !unusable_bits(q) && !unusable_bits(s);
}

// What step 3 and step 4 need at a point X: the cost, the normal equations of a Gauss-Newton step, and the scoring
struct Eval
{
  float s[10];     // {cost, N00, N01, N02, N11, N12, N22, g0, g1, g2}
  uint32_t flags;  // 1: some w is zero, subnormal or not finite; 2: some w <= 0
  uint32_t max_e2; // the largest squared error by |bit pattern| (NaN above infinity above everything finite)
};

__device__ __forceinline__ Eval evaluate(const float (&X)[3], const Member &m0, const uint4 *__restrict__ obs, const float4 *__restrict__ cameras,
                                         uint32_t nb_cameras, size_t first, uint32_t n, uint32_t j)
{
  Eval E;
#pragma unroll
  for (int i = 0; i < 10; i++)
    E.s[i] = 0.f;
  E.flags = 0u, E.max_e2 = 0u;
  for (uint32_t k = j; k < n; k += TRI_G)
  {
    const Member m = TRI_MEMBER(k);
    const float *P = m.P;
    const float u = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const float v = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    const float w = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    const float pu = u / w, pv = v / w;
    const float ru = pu - m.x, rv = pv - m.y;
    const float e2 = ru * ru + rv * rv;
    const float iw = 1.0f / w;
    float ju[3], jv[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
      ju[i] = (P[i] - pu * P[8 + i]) * iw, jv[i] = (P[4 + i] - pv * P[8 + i]) * iw;
    E.s[0] = E.s[0] + e2;
    add_rows(E.s + 1, ju, ru, jv, rv);
    E.flags |= (unusable_bits(w) ? 1u : 0u) | (w <= 0.f ? 2u : 0u);
    E.max_e2 = max(E.max_e2, abs_bits(e2));
  }
  group_sum<10>(E.s);
  E.flags = group_or(E.flags);
  E.max_e2 = group_max(E.max_e2);
  return E;
}

__global__ __launch_bounds__(TRI_THREADS) void k_triangulate(const uint32_t *__restrict__ offsets, const uint4 *__restrict__ obs,
                                                             const uint32_t *__restrict__ obs_stats, const float4 *__restrict__ cameras, uint32_t nb_cameras,
                                                             float t2, float cos_min_angle, uint4 *__restrict__ points, uint32_t points_cap)
{
  const uint32_t j = threadIdx.x & (TRI_G - 1u);
  const uint32_t track = blockIdx.x * TRI_TRACKS + threadIdx.x / TRI_G;
  const uint32_t M = obs_stats[0] < points_cap ? obs_stats[0] : points_cap;
  if (track >= M) // (the whole group)
    return;
  const uint32_t begin = offsets[track], end = offsets[track + 1u];
  const size_t first = begin;
  uint32_t n = 0u, status = 0u, steps = 0u;
  if (end < begin || end > obs_stats[1]) // not an extent of the table: nothing is read
    status = TRI_DEGENERATE;
  else
  {
    n = end - begin;
    status = n > TRI_MAX_OBS ? TRI_TOO_LONG : n < 2u ? TRI_DEGENERATE : 0u;
  }
  float X[3] = {0.f, 0.f, 0.f}, max_sq_error = 0.f, min_cos = 0.f;
  if (status == 0u) // uniform over the group from here on
  {
    Member m0 = {};
    m0.cam_ok = true;
    if (j < n)
      m0 = load_member(obs, cameras, nb_cameras, first + j);
    // ---- step 1: bearings, and the smallest cosine over all pairs: chunk a against chunks b >= a, sixteen rotations of chunk b past chunk a
    uint32_t bad = 0u;
    int key = 0x7fffffff;
    for (uint32_t a = 0; a < n; a += TRI_G)
    {
      float A[3] = {0.f, 0.f, 0.f};
      const bool have_a = a + j < n;
      if (have_a)
      {
        const Member m = TRI_MEMBER(a + j);
        bad |= (m.cam_ok && bearing(m, A)) ? 0u : 1u;
      }
      for (uint32_t b = a; b < n; b += TRI_G)
      {
        float B[3] = {A[0], A[1], A[2]};
        if (b != a && b + j < n)
        {
          const Member m = TRI_MEMBER(b + j);
          (void)bearing(m, B);
        }
#pragma unroll
        for (uint32_t r = 0; r < TRI_G; r++)
        {
          const uint32_t src = (j + r) & (TRI_G - 1u);
          const float o0 = __shfl(B[0], (int)src, TRI_G), o1 = __shfl(B[1], (int)src, TRI_G), o2 = __shfl(B[2], (int)src, TRI_G);
          const float c = (A[0] * o0 + A[1] * o1) + A[2] * o2;
          if (have_a && b + src < n && (b != a || r != 0u))
            key = min(key, order_key(__float_as_int(c)));
        }
      }
    }
    bad = group_or(bad);
    key = group_min(key);
    // ---- step 2: the linear start
    float L[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint32_t k = j; k < n; k += TRI_G)
    {
      const Member m = TRI_MEMBER(k);
      float p[3], q[3], pr, qr;
      const bool okp = scaled_row(m, m.x, 0, p, pr), okq = scaled_row(m, m.y, 1, q, qr);
      bad |= (okp && okq) ? 0u : 1u;
      add_rows(L, p, pr, q, qr);
    }
    group_sum<9>(L);
    bad = group_or(bad);
    const bool started = solve_normal(L, X);
    if (bad != 0u || !started)
      status = TRI_DEGENERATE;
    else
    {
      // ---- step 3: Gauss-Newton steps, each kept iff it can be computed and does not raise the cost
      Eval E = evaluate(X, m0, obs, cameras, nb_cameras, first, n, j);
      for (uint32_t it = 0; it < TRI_GN_STEPS; it++)
      {
        float d[3];
        if ((E.flags & 1u) || !solve_normal(E.s + 1, d))
          break;
        const float Y[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
        if (!(finite_bits(Y[0]) && finite_bits(Y[1]) && finite_bits(Y[2])))
          break;
        const Eval F = evaluate(Y, m0, obs, cameras, nb_cameras, first, n, j);
        if (!(F.s[0] <= E.s[0]))
          break;
        X[0] = Y[0], X[1] = Y[1], X[2] = Y[2], E = F, steps = it + 1u;
      }
      // ---- step 4: scoring at the final X
      max_sq_error = __uint_as_float(E.max_e2 > 0x7f800000u ? 0x7fc00000u : E.max_e2); // (one NaN pattern)
      min_cos = __int_as_float(order_key(key));
      status = ((E.flags & 2u) ? TRI_BEHIND : 0u) | (max_sq_error < t2 ? 0u : TRI_ERROR) |
               ((cos_min_angle < 1.0f && !(min_cos < cos_min_angle)) ? TRI_ANGLE : 0u);
    }
  }
  if (status & (TRI_DEGENERATE | TRI_TOO_LONG))
    X[0] = X[1] = X[2] = max_sq_error = min_cos = 0.f, steps = 0u;
  if (j == 0u)
  {
    points[2u * (size_t)track] = uint4{__float_as_uint(X[0]), __float_as_uint(X[1]), __float_as_uint(X[2]), __float_as_uint(max_sq_error)};
    points[2u * (size_t)track + 1u] = uint4{__float_as_uint(min_cos), status, steps, n};
  }
}

// stats = {points, accepted, failed (DEGENERATE or TOO_LONG), rejected (computed, some of BEHIND / ERROR / ANGLE)}: integer counts, one workgroup
__global__ __launch_bounds__(1024) void k_tri_stats(const uint32_t *__restrict__ obs_stats, uint32_t points_cap, const uint32_t *__restrict__ points,
                                                    uint32_t *__restrict__ stats)
{
  __shared__ uint32_t part[16][3];
  const uint32_t M = obs_stats[0] < points_cap ? obs_stats[0] : points_cap;
  uint32_t c[3] = {0u, 0u, 0u};
  for (uint32_t i = threadIdx.x; i < M; i += 1024u)
  {
    const uint32_t st = points[TRI_POINT_WORDS * (size_t)i + 5u];
    c[st == 0u ? 0 : (st & (TRI_DEGENERATE | TRI_TOO_LONG)) ? 1 : 2]++;
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
    c[i] = wave_sum_u32(c[i]);
  if ((threadIdx.x & 63u) == 0u)
    part[threadIdx.x >> 6][0] = c[0], part[threadIdx.x >> 6][1] = c[1], part[threadIdx.x >> 6][2] = c[2];
  __syncthreads();
  if (threadIdx.x == 0u)
  {
    uint32_t t[3] = {0u, 0u, 0u};
    for (int w = 0; w < 16; w++)
      t[0] += part[w][0], t[1] += part[w][1], t[2] += part[w][2];
    stats[0] = M, stats[1] = t[0], stats[2] = t[1], stats[3] = t[2];
  }
}

} // namespace

extern "C" int vksift_hip_triangulate_tracks(const uint32_t *offsets, const uint8_t *observations, const uint32_t *obs_stats, const float *cameras,
                                             uint32_t nb_cameras, float t2, float cos_min_angle, uint8_t *points, uint64_t points_cap, uint32_t *stats,
                                             vksift_hip_stream s)
{
  if (!offsets || !observations || !obs_stats || !cameras || !points || !stats || nb_cameras == 0u || points_cap == 0u || points_cap > 0x7FFFFFFFull ||
      !(t2 > 0.f) || !isfinite(t2) || isnan(cos_min_angle) || ((uintptr_t)offsets & 3u) || ((uintptr_t)obs_stats & 3u) || ((uintptr_t)stats & 3u) ||
      ((uintptr_t)observations & 15u) || ((uintptr_t)cameras & 15u) || ((uintptr_t)points & 15u))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)s;
  const uint32_t cap = (uint32_t)points_cap;
  k_triangulate<<<(cap + TRI_TRACKS - 1u) / TRI_TRACKS, TRI_THREADS, 0, st>>>(offsets, (const uint4 *)observations, obs_stats, (const float4 *)cameras, nb_cameras, t2,
                                                                             cos_min_angle, (uint4 *)points, cap);
  k_tri_stats<<<1, 1024, 0, st>>>(obs_stats, cap, (const uint32_t *)points, stats);
  return (int)hipGetLastError();
}
