// wave.h — the wave-level primitives of the kernels (wave64), each written once. `lane` is threadIdx.x & 63.
//
// Not here: match.hip's partial butterflies (top-2 merges over 16 / 32 lanes) and the block reductions of refit.h / verify.hip, which
// have their own LDS protocol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// sum over every aligned group of LANES lanes (a power of two, at most 64), in every lane of the group (xor butterfly)
template <int LANES> __device__ __forceinline__ uint32_t lanes_sum_u32(uint32_t v)
{
#pragma unroll
  for (int dlt = LANES / 2; dlt >= 1; dlt >>= 1)
    v += __shfl_xor(v, dlt, 64);
  return v;
}

// sum over the lanes of a wave, in every lane
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return lanes_sum_u32<64>(v); }

// maximum over the lanes of a wave, in every lane
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1)
  {
    const uint32_t t = __shfl_xor(v, dlt, 64);
    v = t > v ? t : v;
  }
  return v;
}

// inclusive prefix sum over the lanes of a wave: lane l gets v(0) + ... + v(l), lane 63 the wave's total
__device__ __forceinline__ uint32_t wave_scan_incl_u32(uint32_t v, int lane)
{
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1)
  {
    const uint32_t t = __shfl_up(v, dlt, 64);
    if (lane >= dlt)
      v += t;
  }
  return v;
}

// rank of a lane within a ballot: the set bits below its own
__device__ __forceinline__ uint32_t ballot_rank(unsigned long long bal, int lane) { return (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)); }
