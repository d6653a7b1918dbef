// features_selftest.hip — test only (vksift_hip_selftest_inrange): the short forms of features_math.h against the compiler's general ones on
// pseudo-random operands inside their ranges. Built with the flags of features.hip, so that it checks the code the feature kernels get.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "features_math.h"
#include "vksift_hip.h"

namespace
{
__device__ __forceinline__ uint32_t st_hash(uint32_t x)
{
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x;
}
// 2^e * (1 + m / 2^23) with e uniform in [elo, ehi]
__device__ __forceinline__ float st_float(uint32_t h, int elo, int ehi)
{
  const int e = elo + (int)((h >> 23) % (uint32_t)(ehi - elo + 1));
  return __uint_as_float(((uint32_t)(e + 127) << 23) | (h & 0x7FFFFFu));
}
__global__ void __launch_bounds__(256) k_inrange_selftest(uint32_t n, uint32_t seed, uint32_t *bad)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n)
    return;
  const uint32_t h0 = st_hash(i * 3u + seed), h1 = st_hash(i * 3u + 1u + seed), h2 = st_hash(i * 3u + 2u + seed);
  uint32_t miss = 0;
  // sqrt: 0 and [2^-96, 2^8), the ends of the range in the first lanes
  float x = i == 0 ? 0.f : (i == 1 ? 0x1p-96f : (i == 2 ? __uint_as_float(0x0F800001u) : st_float(h0, -96, 7)));
  asm volatile("" : "+v"(x));
  miss += __float_as_uint(sqrt_inrange(x)) != __float_as_uint(sqrtf(x));
  // a / b: b in [2^-49, 4), a = 0 or in [2^-64, b]
  float b = st_float(h1, -49, 1), a = st_float(h2, -64, 1);
  a = (i & 15u) == 3u ? 0.f : (a > b ? b * __uint_as_float(0x3F000000u | (h2 & 0x7FFFFFu)) : a); // b * [0.5, 1) where the draw exceeds b
  a = a < 0x1p-64f && a != 0.f ? 0x1p-64f : a;
  asm volatile("" : "+v"(a), "+v"(b));
  miss += __float_as_uint(div_inrange(a, b)) != __float_as_uint(a / b);
  // x / 2 pi: +-[2^-96, 2^8)
  float y = st_float(h0 ^ h1, -96, 7);
  y = (h2 & 1u) ? -y : y;
  asm volatile("" : "+v"(y));
  miss += __float_as_uint(div_2pi_inrange(y)) != __float_as_uint(y / (2.f * PI_F));
  // grad_polar's own guard: wherever it does not ask for the general forms, the short forms must give their bits — components from
  // denormals to 4 and exact zeros, incl. (0, denormal), whose squares underflow to 0
  {
    auto comp = [](uint32_t h, uint32_t i) {
      const uint32_t kind = (h >> 27) & 7u;
      float v = kind == 0u ? 0.f : (kind == 1u ? __uint_as_float(h & 0x7FFFFFu) /* denormal */ : __uint_as_float((((h >> 23) & 0xFFu) % 129u) << 23 | (h & 0x7FFFFFu)));
      if (i == 4u)
        v = __uint_as_float(1u);
      return (h & 0x80000000u) ? -v : v;
    };
    float gx = comp(st_hash(h0 ^ 0x9E3779B9u), 0u), gy = comp(st_hash(h1 ^ 0x85EBCA6Bu), i);
    if (i == 4u || i == 5u)
      gx = 0.f;
    asm volatile("" : "+v"(gx), "+v"(gy));
    float o1, l1, o2, l2;
    bool odd;
    grad_polar<true>(gx, gy, &o1, &l1, &odd);
    grad_polar<false>(gx, gy, &o2, &l2, nullptr);
    miss += !odd && (__float_as_uint(o1) != __float_as_uint(o2) || __float_as_uint(l1) != __float_as_uint(l2));
  }
  if (miss)
    atomicAdd(bad, miss);
}
} // namespace

extern "C" int vksift_hip_selftest_inrange(uint32_t n, uint32_t seed, uint32_t *d_mismatches, vksift_hip_stream s)
{
  hipError_t e = hipMemsetAsync(d_mismatches, 0, sizeof(uint32_t), (hipStream_t)s);
  if (e != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL(k_inrange_selftest, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)s, n, seed, d_mismatches);
  return (int)hipGetLastError();
}
