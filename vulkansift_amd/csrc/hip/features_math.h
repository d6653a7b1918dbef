// features_math.h — the arithmetic both per-keypoint kernels of features.hip rest on: the texel load through a layer's buffer resource,
// the angle wrap, and the short forms of sqrt, division and x / (2 pi) with their range flags. features_selftest.hip runs the short
// forms against the compiler's general ones (tests/test_gpu_descriptor_ranges.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../detmath.h"

#define PI_F 3.14159265358979323846f

// One texel of the keypoint's Gaussian layer through its buffer resource. voff / soff are the byte offsets of the fp32 layout;
// a binary16 pyramid (VKSIFT_PYRAMID_PRECISION_FLOAT16) halves them and widens the texel exactly.
// (F16 is a template parameter of the kernels: as a run-time flag it cost the VALU-bound descriptor kernel 60 %)
template <bool F16>
__device__ __forceinline__ float tap_ld(const __amdgpu_buffer_rsrc_t rs, unsigned voff, int soff)
{
  if (F16)
    return (float)__builtin_bit_cast(_Float16, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rs, voff >> 1, soff >> 1, 0));
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0));
}
// layer `layer` of image `img` (strides in texels)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t layer_rsrc(const float *gauss, size_t texel_off, int pitch, int h, bool f16)
{
  const void *p = f16 ? (const void *)((const _Float16 *)gauss + texel_off) : (const void *)(gauss + texel_off);
  return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, pitch * h * (f16 ? 2 : 4), 0x00020000);
}

// ComputeDescriptors.comp:160-171 / ComputeOrientation.comp:100-104 wrap an angle with "if (t < 0) t += 2 pi; else if
// (t > 2 pi) t -= 2 pi". Both places only ever see t <= 2 pi — atan2 returns (-pi, pi], and the relative orientation is the
// difference of two angles of [0, 2 pi] (the keypoint orientations are (k/2 + 0.5) * 2 pi / 36 with k/2 <= 35.5) — so the
// second branch is dead and the wrap is one add, one compare, one select.
__device__ __forceinline__ float wrap_2pi(float t)
{
  const float up = t + 2.f * PI_F;
  return t < 0 ? up : t;
}

// sqrtf(x) and a / b as hipcc expands them, minus the parts that only matter outside the range the caller has checked:
// * sqrt_inrange: v_sqrt_f32 (<= 1 ulp), then one step down / up by the signs of two exact residuals — the compiler's own correctly rounded
//   expansion without the 2^32 input scaling for x < 2^-96 and without the class test for 0 / inf behind it (x = 0: both residual tests fail
//   on NaN / zero, the result is the 0 v_sqrt_f32 returned);
// * div_inrange: v_rcp_f32, one Newton step, quotient, two remainder corrections — the compiler's expansion without v_div_scale (operands
//   with exponents far apart or near the ends of the range), v_div_fmas' rescaling and v_div_fixup (zeros, infinities, NaN). With
//   2^-64 <= a <= b <= 2^2 (or a = 0) no intermediate leaves the normal range, so every step computes what the scaled sequence computes.
// Both return the bits of the IEEE operation (the descriptor parity tests run both paths against the oracle's sqrtf and '/').
// 14 instead of 26 and 8 instead of 11 instructions; k_descriptor is bound by VALU issue (profiles/r05_descriptor_floor.md).
__device__ __forceinline__ float sqrt_inrange(float x)
{
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
  const float rd = fmaf(-sd, s, x), ru = fmaf(-su, s, x);
  float r = rd <= 0.f ? sd : s;
  r = ru > 0.f ? su : r;
  return r;
}
__device__ __forceinline__ float div_inrange(float a, float b)
{
  float r = __builtin_amdgcn_rcpf(b);
  const float e = fmaf(-b, r, 1.f);
  r = fmaf(e, r, r);
  float q = a * r;
  float m = fmaf(-b, q, a);
  q = fmaf(m, r, q);
  m = fmaf(-b, q, a);
  return fmaf(m, r, q);
}
// v is 0 or at least 2^(E - 127) (v >= 0): one subtract, one unsigned compare
template <uint32_t E>
__device__ __forceinline__ bool below_range(float v) { return __float_as_uint(v) - 1u < (E << 23) - 1u; }

// x / (2*pi): the 3-operation form of dm_div_2pi (detmath.h) without its tests. The caller checks the range (non-zero magnitudes below 2^-96
// take the general form); a zero comes out as +0 whatever its sign, and floor and remainder of a zero bin coordinate are the same for both.
__device__ __forceinline__ float div_2pi_inrange(float x)
{
  const float c2 = 2.f * PI_F, rc = 0x1.45f306p-3f;
  const float q = x * rc;
  return fmaf(fmaf(-q, c2, x), rc, q);
}

// Angle and length of a gradient for both per-keypoint kernels (ComputeOrientation.comp:102-106, ComputeDescriptors.comp:146-162): atan2 and
// sqrt. INRANGE: the short forms; *odd is set where their range conditions do not hold (the caller then repeats the step with the general
// forms: a wave-uniform branch that real images take in regions darker than ~2^-30, if at all; black synthetic backgrounds do, in the
// tails of the blurs: tests/test_gpu_descriptor_ranges.py)
template <bool INRANGE>
__device__ __forceinline__ void grad_polar(float gradX, float gradY, float *ori, float *len, bool *odd)
{
  const float g2 = (gradX * gradX) + (gradY * gradY);
  if (INRANGE)
  {
    const float ax = fabsf(gradX), ay = fabsf(gradY);
    const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
    *ori = dm_atan2f_ratio(div_inrange(mn, mx == 0.f ? 1.f : mx), ax, ay, gradX, gradY);
    *len = sqrt_inrange(g2);
    // mx >= 2^-48 (then g2 >= 2^-96 and no square underflowed) or 0; mn >= 2^-64 or 0. (Tested on mx, not on g2: a denormal mx beside
    // mn = 0 squares to an exact 0, which a test of g2 lets through to rcp(denormal) = inf.)
    *odd = below_range<127 - 48>(mx) || below_range<127 - 64>(mn);
  }
  else
  {
    *ori = dm_atan2f(gradY, gradX);
    *len = sqrtf(g2);
  }
}

// Bin coordinate of an angle: x = angle * bins -> x / (2 pi), the step behind grad_polar in both kernels. INRANGE: the short form, which does
// not hold for a non-zero |x| below 2^-96: angle_bin_odd() is its range flag (the caller ORs it into grad_polar's and repeats the step with
// the general forms if any lane has it set). The flag is a function of its own, OR-ed in by the caller as one expression: written through a
// pointer here, or kept in a variable of its own there, it cost the descriptor kernel two instructions in its sample loop or a pair of SGPRs,
// which it does not have (the record pointer was spilled and the record head loaded in two trips: descriptor stage +0.8 %).
template <bool INRANGE>
__device__ __forceinline__ float angle_bin(float x) { return INRANGE ? div_2pi_inrange(x) : dm_div_2pi(x); }
__device__ __forceinline__ bool angle_bin_odd(float x) { return below_range<127 - 96>(fabsf(x)); }
