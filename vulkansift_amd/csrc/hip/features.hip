// features.hip — keypoint orientation assignment and 4x4x8 descriptor extraction (gfx950, wave64).
//
// Replaces ComputeOrientation.comp (dispatch sift_detector.c:1191-1241) and ComputeDescriptors.comp
// (sift_detector.c:1243-1259). The reference launches them with vkCmdDispatchIndirect, one small
// workgroup per keypoint; HIP has no indirect dispatch, so both kernels are persistent grid-stride
// loops that read the keypoint count from HBM. One 64-lane wave owns one keypoint; histograms are
// accumulated with integer LDS atomics (ds_add_u32) on the reference's fixed-point scale, so the
// result does not depend on the order in which lanes arrive (bit-reproducible run to run).
//
// Extra orientations are appended through a prefix scan (k_orientation_finalize) instead of the
// reference's global atomicAdd (ComputeOrientation.comp:170-183): order = (keypoint, histogram bin).
//
// All per-pixel arithmetic mirrors oracle/sift_oracle.c (orc_orientations / orc_descriptor) in its
// "det" math mode operation for operation; exp/atan2/sin/cos come from detmath.h.
//
// Shared steps are stated once: image_view() and keypoint_head() below, the short arithmetic forms in features_math.h, the wave primitives in
// wave.h. k_descriptor is a sequence of named steps (desc_*) with explicit inputs and outputs, all inlined.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "../detmath.h"
#include "features_math.h"
#include "multi.h"
#include "records.h"
#include "vksift_hip.h"
#include "wave.h"

namespace
{

struct FeatArgs
{
  const float *gauss;
  uint32_t fp16; // binary16 texels
  int w, h, pitch;
  uint64_t plane_stride, img_stride;
  uint8_t *feats;
  uint64_t feat_img_stride;
  uint32_t cap;
  uint32_t *found;
  uint32_t found_img_stride;
  float *ori_ang;
  uint32_t *ori_cnt;
  uint64_t ori_img_stride;
  uint32_t max_keep; // orientations kept per keypoint (1..18)
  uint32_t use_vlfeat;
  const float *desc_fp_tab;
  uint32_t desc_fp_tab_len;
  uint32_t sec; // section of the SIFT buffer this octave fills (k_descriptor's dense rows)
};

// What all three kernels derive from their octave and image b (w, h, pitch, plane: copies the window loops read from registers — read
// through FeatArgs they are loaded again behind every atomic, +28 instructions in k_orientation's border loop)
struct ImageView
{
  uint32_t found, n; // the section's device-side feature count; min(found, cap): the records that exist
  uint8_t *feats;    // the image's section records
  int w, h, pitch;
  size_t plane;
};
__device__ __forceinline__ ImageView image_view(const FeatArgs &a, int b)
{
  ImageView v;
  v.found = a.found[(size_t)b * a.found_img_stride];
  v.n = v.found < a.cap ? v.found : a.cap;
  v.feats = a.feats + (size_t)b * a.feat_img_stride;
  v.w = a.w, v.h = a.h, v.pitch = a.pitch;
  v.plane = (size_t)a.plane_stride;
  return v;
}

// The head of keypoint k's record and the buffer resource of its Gaussian layer (both per-keypoint kernels open a keypoint with it)
struct KeyHead
{
  const float *rec;
  float scale_x, scale_y, sigma, theta;
  int octave_idx;
  __amdgpu_buffer_rsrc_t rs;
};
template <bool F16>
__device__ __forceinline__ KeyHead keypoint_head(const FeatArgs &a, const ImageView &v, int b, uint32_t k)
{
  KeyHead kh;
  kh.rec = (const float *)(v.feats + (size_t)k * VKSIFT_RECORD_BYTES);
  // wave-uniform (every wave of a keypoint reads the same record): keeps the resource in SGPRs
  const uint32_t scale_idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)((const uint32_t *)kh.rec)[4]);
  kh.octave_idx = ((const int *)kh.rec)[5];
  kh.sigma = kh.rec[6];
  kh.scale_x = kh.rec[2], kh.scale_y = kh.rec[3], kh.theta = kh.rec[7];
  // planes stay below 2 GiB (vksift_hip_extract_keypoints refuses sides of 16384 and more): 32-bit byte offsets
  kh.rs = layer_rsrc(a.gauss, (size_t)b * a.img_stride + (size_t)scale_idx * v.plane, v.pitch, v.h, F16);
  return kh;
}

// -------------------------------------------------------------------------------------------------
// Orientation histogram (ComputeOrientation.comp:52-186). grid = (blocks, batch); 4 keypoints/block.
// -------------------------------------------------------------------------------------------------
template <bool IMG_FAST, bool F16>
__global__ void __launch_bounds__(256) k_orientation(Multi<FeatArgs> m)
{
  const VBlock vb = vblock(m); // virtual grid (images, blocks) when IMG_FAST, (blocks, images) otherwise
  const FeatArgs &a = m.oct[vb.o];
  // One wave per keypoint, four independent waves per block: every wave owns its histogram and LDS executes the DS
  // operations of a wave in program order, so no workgroup barrier is needed (a wave with a 15x15 window does not wait
  // for a neighbour with a 29x29 one).
  __shared__ uint32_t s_hist[4][36];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = (int)(IMG_FAST ? vb.x : vb.y);
  const ImageView g = image_view(a, b);
  uint32_t *hist = s_hist[wave];

  const uint32_t bk = IMG_FAST ? vb.y : vb.x, nbk = IMG_FAST ? vb.gy : vb.gx;
  for (uint32_t k = bk * 4 + wave; k < g.n; k += nbk * 4)
  {
    if (lane < 36)
      hist[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    float fp = 0.f;
    {
      const KeyHead kh = keypoint_head<F16>(a, g, b, k);
      // sigma / 2^octave_idx as a product with 2^-octave_idx: the same real number, rounded once either way
      float lambda = 1.5f * (kh.sigma * dm_pow2i(-kh.octave_idx));
      int r = (int)floorf(3 * lambda);
      float es = -1.f / (2.f * lambda * lambda);
      // the window's largest squared distance is 2 (r + 1)^2 (offsets of at most r + 0.5 + 0.5 per axis): can es * d2 pass the clamp of dm_expf?
      const bool may_clamp = (2.f * (float)(r + 1) * (float)(r + 1)) * es < -87.f;

      // fixed-point scale: M = (sum_i e^{es i^2})^2 * sqrt(2)  (separable form of :75-79, same order as the oracle's det mode)
      float gsum = 1.f;
      for (int cb = 0; cb <= r; cb += 64)
      {
        int i = cb + lane;
        float e = (i >= 1 && i <= r) ? dm_expf(es * (float)(i * i)) : 0.f;
        int lim = r - cb < 63 ? r - cb : 63;
        for (int j = 0; j <= lim; j++)
        {
          float ej = __shfl(e, j, 64);
          if (cb + j >= 1)
            gsum += 2.f * ej;
        }
      }
      float M = (gsum * gsum) * sqrtf(2.f);
      fp = (float)(1u << (uint32_t)(30 - dm_ceil_log2f(M)));

      float rsx = roundf(kh.scale_x), rsy = roundf(kh.scale_y);
      int box = 2 * r + 1;
      int npix = box * box;
      // lane l visits window pixels l, l + 64, ...: (row, column) advance by (64 / box, 64 % box) with at most one carry
      // a / box for 0 <= a <= 64 as (int)((a + 0.5) * rcp(box)): (a + 0.5) / box stays 0.5 / box away from every integer — for box < 32768
      // far more than the error of v_rcp_f32 and one product — 4 instructions instead of the ~25 of a 32-bit integer division
      const float rbox = __builtin_amdgcn_rcpf((float)box);
      const bool small_box = box < 32768;
      const int step_q = small_box ? (int)(64.5f * rbox) : 64 / box, step_r = 64 - step_q * box;
      int py = small_box ? (int)(((float)lane + 0.5f) * rbox) : lane / box, px = lane - py * box;
      // the contribution of one window texel given its gradient taps (ComputeOrientation.comp:102-121)
      auto accumulate = [&](float sdx2, float tr, float tl, float td, float tu) {
        const float gradX = 0.5f * (tr - tl);
        const float gradY = 0.5f * (td - tu);
        // dm_expf_nb_nonpos(sdx2 * es): its clamp as one v_max, its zero result only for keypoints whose window can reach the clamp at all
        // (exponents below -87.3: never with lambda >= 0.08, i.e. for any sigma a SIFT configuration produces)
        const float xe = sdx2 * es; /* d2 >= 0 > es */
        float e = dm_expf_core_nonpos(fmaxf(xe, -87.3f));
        if (may_clamp)
          e = xe < -87.3f ? 0.f : e;
        float ori, len;
        bool odd;
        grad_polar<true>(gradX, gradY, &ori, &len, &odd);
        float x36 = wrap_2pi(ori) * 36.f;
        float fbin = angle_bin<true>(x36); // == ori * 36 / (2 pi)
        odd |= angle_bin_odd(x36);
        if (__builtin_expect(__ballot(odd) != 0ull, 0))
        {
          grad_polar<false>(gradX, gradY, &ori, &len, nullptr);
          fbin = angle_bin<false>(wrap_2pi(ori) * 36.f);
        }
        const float mag = e * len;
        // ComputeOrientation.comp:107-112 wraps bin < 0 and bin >= 36; the angle is in [0, 2 pi] here (wrap_2pi), its quotient by 2 pi is
        // the correctly rounded one of a non-negative number: only 36 itself can occur
        int bin = (int)fbin;
        bin = bin >= 36 ? bin - 36 : bin;
        atomicAdd(&hist[bin], (uint32_t)(mag * fp));
      };
      const int cxi = (int)rsx, cyi = (int)rsy;
      const int pitch4 = g.pitch * 4;
      // The window loop: the lane walk and the window offsets once, the tap addressing in two forms.
      auto window = [&](auto INTERIOR) {
        for (int pix = lane; pix < npix; pix += 64)
        {
          const int dy = py - r, dx = px - r;
          px += step_r, py += step_q;
          if (px >= box)
            px -= box, py++;
          const float sdx = (rsx + (float)dx) - kh.scale_x;
          const float sdy = (rsy + (float)dy) - kh.scale_y;
          const float d2 = (sdx * sdx) + (sdy * sdy);
          if constexpr (decltype(INTERIOR)::value)
          {
            // byte offset of texel (x - 1, y - 1): the four taps are immediate / scalar offsets from it (scalar offsets are unsigned)
            const unsigned v0 = (__umul24((unsigned)(cyi + dy - 1), (unsigned)g.pitch) + (unsigned)(cxi + dx - 1)) * 4u;
            accumulate(d2, tap_ld<F16>(kh.rs, v0 + 8u, pitch4), tap_ld<F16>(kh.rs, v0, pitch4), tap_ld<F16>(kh.rs, v0 + 4u, 2 * pitch4), tap_ld<F16>(kh.rs, v0 + 4u, 0));
          }
          else
          {
            const int gx = cxi + dx, gy = cyi + dy;
            if ((gx < 1 || gx >= (g.w - 1) || gy < 1 || gy >= (g.h - 1)) && (d2 > (float)(r * r)))
              continue; // quirk Q2 ('&&')
            // imageLoad semantics (0 outside the image, quirk Q2 relies on it) through the layer's buffer resource: a tap
            // outside the image gets an out-of-range offset, which the hardware answers with 0 — no branches, 32-bit offsets
            const bool xin = (unsigned)gx < (unsigned)g.w, yin = (unsigned)gy < (unsigned)g.h;
            // (each row offset from its own, in-range, row index: the 24-bit multiply must not see a negative row)
            const unsigned o0 = (__umul24((unsigned)gy, (unsigned)g.pitch) + (unsigned)gx) * 4u;
            const unsigned o_r = (yin && (unsigned)(gx + 1) < (unsigned)g.w) ? o0 + 4u : 0x80000000u;
            const unsigned o_l = (yin && (unsigned)(gx - 1) < (unsigned)g.w) ? o0 - 4u : 0x80000000u;
            const unsigned o_d = (xin && (unsigned)(gy + 1) < (unsigned)g.h) ? (__umul24((unsigned)(gy + 1), (unsigned)g.pitch) + (unsigned)gx) * 4u : 0x80000000u;
            const unsigned o_u = (xin && (unsigned)(gy - 1) < (unsigned)g.h) ? (__umul24((unsigned)(gy - 1), (unsigned)g.pitch) + (unsigned)gx) * 4u : 0x80000000u;
            accumulate(d2, tap_ld<F16>(kh.rs, o_r, 0), tap_ld<F16>(kh.rs, o_l, 0), tap_ld<F16>(kh.rs, o_d, 0), tap_ld<F16>(kh.rs, o_u, 0));
          }
        }
      };
      // (wave-uniform: one keypoint per wave) the whole window and its taps inside the image interior — all but the keypoints
      // within r + 1 texels of a border: no texel is skipped (quirk Q2's test needs a texel outside the interior) and no tap needs
      // the out-of-image handling, which is a third of the general loop's instructions
      if (cxi - r >= 1 && cxi + r <= g.w - 2 && cyi - r >= 1 && cyi + r <= g.h - 2)
        window(std::true_type{});
      else
        window(std::false_type{});
    }
    __builtin_amdgcn_wave_barrier();
    {
      // 3 x 2 box-filter passes in registers (lane i holds bin i), :130-147
      const int li = lane < 36 ? lane : 0;
      uint32_t hv = hist[li];
      const int lm = (li + 35) % 36, lp = (li + 1) % 36;
#pragma unroll
      for (int it = 0; it < 6; it++)
      {
        uint32_t hm = __shfl(hv, lm, 64), hp = __shfl(hv, lp, 64);
        hv = (uint32_t)dm_div_3((float)(hm + hv + hp)); // == / 3.f for every integer-valued float up to 2^32 (detmath.h)
      }
      uint32_t hm = __shfl(hv, lm, 64), hp = __shfl(hv, lp, 64);
      const uint32_t mx = wave_max_u32(lane < 36 ? hv : 0u);
      bool peak = lane < 36 && ((float)hv >= (0.8f * (float)mx)) && (hv > hm) && (hv > hp);
      unsigned long long pm = __ballot(peak);
      uint32_t npk = (uint32_t)__popcll(pm);
      if (peak)
      {
        uint32_t rank = ballot_rank(pm, lane);
        if (rank < a.max_keep)
        {
          uint32_t num = hm - hp;                 // quirk Q3: uint32 wrap-around
          uint32_t den = hm - (2u * hv) + hp;
          float idx = (float)lane + 0.5f * ((float)num / (float)den);
          float ang = (idx + 0.5f) * (2.f * PI_F) / 36.f;
          a.ori_ang[((size_t)b * a.ori_img_stride + k) * VKSIFT_HIP_MAX_ORI + rank] = ang;
        }
      }
      if (lane == 0)
        a.ori_cnt[(size_t)b * a.ori_img_stride + k] = npk < a.max_keep ? npk : a.max_keep;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// -------------------------------------------------------------------------------------------------
// Write main orientations in place and append the extra-orientation copies in (keypoint, bin) order
// (ComputeOrientation.comp:170-183, made deterministic). One 1024-thread block per image.
// -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_orientation_finalize(Multi<FeatArgs> m)
{
  __shared__ uint32_t wave_tot[16];
  __shared__ uint32_t carry_s;
  const VBlock vb = vblock(m); // virtual grid (images)
  const FeatArgs &a = m.oct[vb.o];
  const int b = (int)vb.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ImageView g = image_view(a, b);
  const uint32_t *cnt = a.ori_cnt + (size_t)b * a.ori_img_stride;
  const float *ang = a.ori_ang + (size_t)b * a.ori_img_stride * VKSIFT_HIP_MAX_ORI;
  if (threadIdx.x == 0)
    carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < g.n; base += 1024)
  {
    uint32_t k = base + threadIdx.x;
    uint32_t c = k < g.n ? cnt[k] : 0u;
    uint32_t v = c > 1 ? c - 1 : 0u;
    const uint32_t incl = wave_scan_incl_u32(v, lane);
    if (lane == 63)
      wave_tot[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
    for (int wv = 0; wv < wave; wv++)
      wave_base += wave_tot[wv];
    uint32_t carry = carry_s;
    uint32_t excl = carry + wave_base + incl - v;
    if (k < g.n && c >= 1)
    {
      uint32_t *rec = (uint32_t *)(g.feats + (size_t)k * VKSIFT_RECORD_BYTES);
      rec[7] = __float_as_uint(ang[(size_t)k * VKSIFT_HIP_MAX_ORI]);
      for (uint32_t j = 1; j < c; j++)
      {
        uint32_t idx = g.found + excl + (j - 1);
        if (idx < a.cap)
        {
          uint32_t *dst = (uint32_t *)(g.feats + (size_t)idx * VKSIFT_RECORD_BYTES);
#pragma unroll
          for (int q = 0; q < (int)VKSIFT_RECORD_HEAD_WORDS; q++)
            dst[q] = rec[q];
          dst[7] = __float_as_uint(ang[(size_t)k * VKSIFT_HIP_MAX_ORI + j]);
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 1023)
      carry_s = carry + wave_base + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0)
    a.found[(size_t)b * a.found_img_stride] = g.found + carry_s;
}

// -------------------------------------------------------------------------------------------------
// Descriptor (ComputeDescriptors.comp:84-274). grid = (blocks, batch); one keypoint per block.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int smod8(int v) { return v & 7; } // floored modulo for a power of two (quirk Q5, OpSMod)

// Per-pixel descriptor contribution (ComputeDescriptors.comp:139-197) for window offset (cdx, cdy).
struct DescCtx
{
  __amdgpu_buffer_rsrc_t rs; // the keypoint's Gaussian layer
  int pitch, pitch4;
  float scale_x, scale_y, rsx, rsy, kcos, ksin, kori, fp, bin_scale;
  // for the row spans: the window [-R, R]^2 clipped to the image interior, relative to the rounded position (rsx, rsy) (ComputeDescriptors.comp:151
  // skips the border texels); rounded minus exact position; 1 / kcos and 1 / -ksin
  int dx0, dx1, dy0, dy1;
  float offx, offy, ia0, ia1;
};

// The contribution of one window pixel in two straight-line halves (no branch in either, so that the scheduler can
// interleave the halves of two samples): desc_sample() = taps, gradient, angle, weight; desc_scatter() = bins + atomics.
struct DescSample
{
  float ox, oy, mag;
  float xb; // 8 * relative orientation, before the division by 2*pi
};

// the four taps of a sample: up (x, y-1), left (x-1, y), right (x+1, y), down (x, y+1)
struct DescTaps
{
  float up, lf, rt, dn;
};

// byte offset of texel (ix - 1, iy - 1) of the sample at window offset (cdx, cdy): the taps are immediate / scalar offsets from it
// (the window is clipped to the image interior, so every tap of a live sample is in range; sides < 16384: 24-bit factors)
__device__ __forceinline__ unsigned desc_tap_base(const DescCtx &c, int cdx, int cdy)
{
  const int ix = (int)c.rsx + cdx, iy = (int)c.rsy + cdy;
  return (__umul24((unsigned)(iy - 1), (unsigned)c.pitch) + (unsigned)(ix - 1)) * 4u;
}

template <bool F16>
__device__ __forceinline__ DescTaps desc_taps(const DescCtx &c, unsigned v0)
{
  DescTaps t;
  t.up = tap_ld<F16>(c.rs, v0 + 4u, 0);
  t.lf = tap_ld<F16>(c.rs, v0, c.pitch4);
  t.rt = tap_ld<F16>(c.rs, v0 + 8u, c.pitch4);
  t.dn = tap_ld<F16>(c.rs, v0 + 4u, 2 * c.pitch4);
  return t;
}

// Two samples of one lane, the second the right-hand neighbour of the first (the common case: a lane walks along a row): their
// eight taps are the texels (x, x+1) of the rows above and below and (x-1 .. x+2) of the row itself — three loads (8, 16, 8
// bytes; dword-aligned, which is all a buffer load needs) instead of eight. The descriptor kernel keeps the address path of the
// texture unit full (SQ_VMEM_TA_ADDR_FIFO_FULL 29 % of its busy cycles with one load per tap).
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void desc_taps_pair(const DescCtx &c, unsigned v0, DescTaps &a, DescTaps &b)
{
  const u32x2_t up = __builtin_amdgcn_raw_buffer_load_b64(c.rs, v0 + 4u, 0, 0);
  const u32x4_t mid = __builtin_amdgcn_raw_buffer_load_b128(c.rs, v0, c.pitch4, 0);
  const u32x2_t dn = __builtin_amdgcn_raw_buffer_load_b64(c.rs, v0 + 4u, 2 * c.pitch4, 0);
  a.up = __uint_as_float(up.x), b.up = __uint_as_float(up.y);
  a.lf = __uint_as_float(mid.x), b.lf = __uint_as_float(mid.y);
  a.rt = __uint_as_float(mid.z), b.rt = __uint_as_float(mid.w);
  a.dn = __uint_as_float(dn.x), b.dn = __uint_as_float(dn.y);
}

// INRANGE: see grad_polar (features_math.h)
template <bool INRANGE>
__device__ __forceinline__ DescSample desc_sample(const DescCtx &c, int cdx, int cdy, const DescTaps &t, bool *odd)
{
  const float es = -1.f / (2.f * 2 * 2);
  float sdx = (c.rsx + (float)cdx) - c.scale_x;
  float sdy = (c.rsy + (float)cdy) - c.scale_y;
  DescSample r;
  r.ox = c.kcos * sdx + c.ksin * sdy;
  r.oy = c.kcos * sdy - c.ksin * sdx;
  float gradX = 0.5f * (t.rt - t.lf);
  float gradY = 0.5f * (t.dn - t.up);
  float ori, root;
  grad_polar<INRANGE>(gradX, gradY, &ori, &root, odd);
  ori = wrap_2pi(ori);
  ori = wrap_2pi(ori - c.kori);
  // |ox|, |oy| < 4 for every enumerated sample: the exponent is in [-4, 0], no range handling needed
  r.mag = dm_expf_core_nonpos(es * ((r.ox * r.ox) + (r.oy * r.oy))) * root;
  r.xb = ori * c.bin_scale; // +8 (VLFeat order) or -8: (-ori) * 8 == ori * (-8) exactly
  return r;
}

// Histogram layout for 64-bit atomics: a cell is eight 8-byte slots, slot b holding the sums for the bin pair (b, b + 1 mod 8). The two
// orientation bins a sample touches are hb and hb + 1 (mod 8), so each of the four cells takes ONE ds_add_u64 into slot hb mod 8 instead of
// two ds_add_u32 (the sums stay below 2^32 by construction of the fixed-point scale, so the low half never carries into the high half),
// and the slot's byte offset is (hb & 7) * 8 — no parity split. Cell = 64 bytes. The epilogue adds the two halves that belong to a bin.
// The 4x4 grid sits inside a 6x8 array of cells (grid cell (cx, cy) = array cell (cx + 1, cy + 1)), so the 2x2 cells of a
// sample share ONE address register — the other three are immediate offsets of the ds_add_u64, and the lower corner of a sample
// one cell outside the grid still gives a non-negative address. Cells outside the grid (ComputeDescriptors.comp:189 drops
// them: 36 % of all cell updates, the enumerated footprint is 5x5 cells) are not executed at all: the add sits under the
// exec mask of its in-grid test. (Round 3's form redirected them to a per-lane dummy slot — four selects and three more
// address computations per sample, and an LDS atomic for every dropped cell. Letting them land in the border cells of
// the array instead, without any test, was measured 1.3 % SLOWER despite 6 % fewer instructions: the dropped updates then collide
// on 20 border cells like the kept ones do on the grid, and the kernel is as sensitive to same-address LDS atomics as to
// VALU issue.) Only the 16 grid cells are ever touched.
constexpr int DESC_PAD = 1, DESC_ROW_CELLS = 8; // rows of 8 cells: a grid column keeps the LDS banks it had in the dense 4x4 layout
constexpr int DESC_HIST_WORDS = (4 + 2 * DESC_PAD) * DESC_ROW_CELLS * 16; // 6 rows x 8 cells x (8 + 8) words = 3 KiB
// what a workgroup keeps of it: up to the last grid cell (the array cells behind it are never addressed by an executed add). The two-wave form holds two
// histograms; with whole arrays its 10 252 bytes of LDS would leave a CU 15 workgroups (30 waves) instead of the 16 its eight waves per SIMD allow.
constexpr int DESC_WORK_WORDS = ((4 + DESC_PAD - 1) * DESC_ROW_CELLS + (4 + DESC_PAD - 1) + 1) * 16; // 592 words
static_assert(DESC_WORK_WORDS <= DESC_HIST_WORDS && DESC_WORK_WORDS % 2 == 0, "64-bit slots");
__device__ __forceinline__ int desc_cell_word(int cell) // first word of grid cell cy * 4 + cx
{
  return (((cell >> 2) + DESC_PAD) * DESC_ROW_CELLS + (cell & 3) + DESC_PAD) * 16;
}
__device__ __forceinline__ uint32_t desc_hist_read(const uint32_t *s_work, int t) // descriptor element t = cell * 8 + bin
{
  const int cw = desc_cell_word(t >> 3), bin = t & 7;
  // slot b of a cell holds (bin b, bin b + 1 mod 8): bin = the low half of its own slot + the high half of the slot below
  return s_work[cw + 2 * bin] + s_work[cw + 2 * ((bin + 7) & 7) + 1];
}

__device__ __forceinline__ void desc_scatter(const DescCtx &c, const DescSample &r, float fbin, bool live, uint32_t *s_work)
{
  float fhx = r.ox + 2.f, fhy = r.oy + 2.f;
  // (float)(int)floorf(v) == floorf(v) for these small values: the remainders take the floor as it is, one conversion less each
  const float flx = floorf(fhx - 0.5f), fly = floorf(fhy - 0.5f), flb = floorf(fbin);
  int hx = (int)flx, hy = (int)fly, hb = (int)flb;
  float rhx = fhx - (flx + 0.5f), rhy = fhy - (fly + 0.5f), rb = fbin - flb;
  // ((w * wb) * mag) * fp == (w * wb) * (mag * fp) bit for bit: fp is a power of two (2^0 .. 2^31), so mag * fp is exact and
  // scaling by it commutes with the rounding of the product — except where (w * wb) * mag is subnormal, and there both
  // forms are far below 1 and convert to 0. One multiply per sample instead of one per bin value (8).
  // (Packed v_pk_mul_f32 for the weight products was measured 9 % slower despite 6 % fewer instructions.)
  const float magfp = r.mag * c.fp;
  const unsigned b0 = (unsigned)smod8(hb);
  const unsigned pair = b0 * 8u; // byte offset of the (hb, hb + 1) slot inside a cell
  // in-grid tests of the two columns and the two rows (a dead sample — a lane whose run has ended — fails all of them);
  // the address of a lane that fails is never used
  const bool okx[2] = {live && (unsigned)hx < 4u, live && (unsigned)(hx + 1) < 4u};
  const bool oky[2] = {(unsigned)hy < 4u, (unsigned)(hy + 1) < 4u};
  char *base = (char *)s_work + ((unsigned)((hy + DESC_PAD) * (DESC_ROW_CELLS * 64) + (hx + DESC_PAD) * 64) + pair);
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
    {
      const float w = fabsf(1.f - (float)i - rhx) * fabsf(1.f - (float)j - rhy);
      const uint32_t v0 = (uint32_t)((w * fabsf(1.f - 0.f - rb)) * magfp);
      const uint32_t v1 = (uint32_t)((w * fabsf(1.f - 1.f - rb)) * magfp);
      if (okx[i] && oky[j])
        atomicAdd((unsigned long long *)(base + (j * DESC_ROW_CELLS * 64 + i * 64)), ((unsigned long long)v1 << 32) | v0);
    }
}

// One 64 * NWV-thread workgroup per keypoint (the window of a coarse-scale keypoint has up to ~7.5k pixels; a single wave would make it the
// critical path of the whole launch). About half of the window falls outside the rotated 4x4 grid: the reference evaluates atan/exp for those
// pixels and then drops the contribution (ComputeDescriptors.comp:189); here they are never visited (analytic row spans, desc_row_spans), which
// changes no bit. The expensive part (gradient, atan2, exp, 8 fixed-point atomics) runs on full 64-lane batches.
constexpr int DESC_MAX_ROWS = 256; // window rows handled per pass (R <= 127: every stock configuration); taller windows take several passes

// ---- step: dense rows for the matcher and posting (vksift_hip_DenseRows), once per workgroup. This section's features follow the stored features
// of the sections in front of it: *s_row0 = their number (it waits in LDS for the epilogue: nothing of this stays in registers across the sample
// loop). All counters are final here (the orientation launches of every octave precede this one); uniform scalar loads. The first workgroup of
// section 0's share of an image (first_block) also writes the buffer's row count, the zero rows of quirk Q6 and the posted counters.
template <bool CAN_POST>
__device__ __forceinline__ void desc_dense_prologue(const FeatArgs &a, const vksift_hip_DenseRows &dr, int b, bool first_block, int tid, uint32_t *s_row0)
{
  if (!(dr.desc || (CAN_POST && dr.post)))
    return;
  const uint32_t *fsec = a.found + (size_t)b * a.found_img_stride - a.sec; // counter of section 0 of this image's buffer
  uint32_t row0 = 0, total = 0;
  // (constant indices into the by-value argument: a run-time index would send the struct through scratch memory — 8 bytes of scratch
  // cost this kernel 4 %, tests/test_kernel_resources.py)
#pragma unroll
  for (uint32_t j = 0; j < 16u; j++)
    if (j < dr.nsec)
    {
      const uint32_t f = fsec[j], n = f < dr.sec_cap[j] ? f : dr.sec_cap[j];
      row0 += j < a.sec ? n : 0u;
      total += n;
    }
  if (tid == 0)
    *s_row0 = row0; // read behind the barriers of the keypoint loop
  if (a.sec == 0 && first_block)
  {
    if (CAN_POST && dr.post && (uint32_t)tid < dr.found_post_n)
      dr.found_post[(size_t)b * dr.found_post_n + tid] = fsec[tid]; // the counters travel with the posted records
    if (dr.desc && tid == 0)
      dr.n[(size_t)b * dr.n_img_stride] = total;
    if (dr.desc && total < 2u && tid < 64)
    {
      uint32_t *z = (uint32_t *)(dr.desc + (size_t)b * dr.desc_img_stride);
      if (tid >= (int)total * 32)
        z[tid] = 0u;
      if (tid < 2 && tid >= (int)total)
        dr.norm[(size_t)b * dr.norm_img_stride + tid] = 128u * 128u * 128u;
    }
  }
}

// ---- step: the window radius R of a keypoint (ComputeDescriptors.comp:107-109) and the bin width lambda it comes from
__device__ __forceinline__ int desc_radius(float sigma, int octave_idx, float *lambda)
{
  float scale_factor = dm_pow2i(octave_idx);
  *lambda = 3.0f * (sigma / scale_factor);
  float radius = sqrtf(2.f) * *lambda * 5.f * 0.5f;
  return (int)floorf(radius + 0.5f);
}

// ---- step: per-keypoint set-up
__device__ __forceinline__ DescCtx desc_setup(const FeatArgs &a, const ImageView &g, const KeyHead &kh)
{
  DescCtx c;
  c.scale_x = kh.scale_x, c.scale_y = kh.scale_y, c.kori = kh.theta;
  c.rs = kh.rs;
  c.pitch = g.pitch, c.pitch4 = g.pitch * 4;
  c.bin_scale = a.use_vlfeat ? 8.f : -8.f;
  float lambda;
  const int R = desc_radius(kh.sigma, kh.octave_idx, &lambda);
  float sn, cs;
  dm_sincosf(c.kori, &sn, &cs);
  c.kcos = cs / lambda, c.ksin = sn / lambda;
  uint32_t ti = (uint32_t)(R / 2);
  c.fp = a.desc_fp_tab[ti < a.desc_fp_tab_len ? ti : a.desc_fp_tab_len - 1];
  c.rsx = roundf(c.scale_x), c.rsy = roundf(c.scale_y);

  const int cxi = (int)c.rsx, cyi = (int)c.rsy;
  c.dx0 = max(-R, 1 - cxi), c.dx1 = min(R, g.w - 2 - cxi);
  c.dy0 = max(-R, 1 - cyi), c.dy1 = min(R, g.h - 2 - cyi);
  c.offx = c.rsx - c.scale_x, c.offy = c.rsy - c.scale_y;
  // (reciprocals by v_rcp_f32, 1 ulp: the spans are conservative by 0.01 in T and 0.01 px at both ends, six orders of magnitude more than
  // that error on coordinates below 2^14 — the four IEEE divisions per row cost every wave 44 instructions per keypoint, round 6)
  c.ia0 = __builtin_amdgcn_rcpf(c.kcos), c.ia1 = __builtin_amdgcn_rcpf(-c.ksin);
  return c;
}

// The rows of one pass (at most DESC_MAX_ROWS window rows from window row y0) in LDS
struct DescRows
{
  int *lo;             // first dx of a row's span
  uint32_t *cnt;       // its length
  const uint32_t *pre; // this wave's exclusive prefix of the rows' pair slots, pre[nrows] = P (desc_row_prefix)
  int y0, nrows;
};

// ---- step: the row spans of one pass. Only pixels whose rotated position (ox, oy) lies within the 5x5-cell footprint |ox|, |oy| < 2.5 of the 4x4
// grid can touch a bin (about half of the window). Instead of testing every pixel, each window row gets its span of such pixels analytically: ox and
// oy are linear in dx, so {dx : |kcos*fx + ksin*fy| < T and |kcos*fy - ksin*fx| < T} is an interval. The spans are approximate (fused arithmetic) and
// conservative (margin): desc_scatter re-derives the cells exactly and drops the out-of-grid ones, so a false positive costs a sample slot, never a bit.
template <int NT>
__device__ __forceinline__ void desc_row_spans(const DescCtx &c, const DescRows &rows, int tid)
{
  const float T = 2.5f + 0.01f;
  for (int row = tid; row < rows.nrows; row += NT)
  {
    const float fy = (float)(rows.y0 + row) + c.offy;
    float lo = (float)c.dx0 - 0.5f, hi = (float)c.dx1 + 0.5f; // in dx
    // |a * fx + bb| < T for (a, bb) = (kcos, ksin*fy) and (-ksin, kcos*fy); fx = dx + offx
#pragma unroll
    for (int e = 0; e < 2; e++)
    {
      const float aa = e == 0 ? c.kcos : -c.ksin, ia = e == 0 ? c.ia0 : c.ia1;
      const float bb = e == 0 ? c.ksin * fy : c.kcos * fy;
      if (fabsf(aa) > 1e-12f)
      {
        const float ctr = -bb * ia - c.offx, half = T * fabsf(ia);
        lo = fmaxf(lo, ctr - half);
        hi = fminf(hi, ctr + half);
      }
      else if (!(fabsf(bb) < T))
        hi = lo - 2.f; // empty
    }
    const int ilo = (int)ceilf(lo - 0.01f), ihi = (int)floorf(hi + 0.01f);
    const int xl = max(ilo, c.dx0), xh = min(ihi, c.dx1);
    rows.lo[row] = xl;
    rows.cnt[row] = xh >= xl ? (uint32_t)(xh - xl + 1) : 0u;
  }
}

// ---- step: exclusive scan of the rows' pair slots (nrows <= DESC_MAX_ROWS), total in pre[nrows]. A slot is two row neighbours (dx, dx + 1): a span
// of cnt samples is (cnt + 1) / 2 slots, and the second half of the last slot of an odd span is dead. Every wave computes the scan for itself from
// the counts (read-only here) into its own copy of the prefix array: no workgroup barrier afterwards.
__device__ __forceinline__ void desc_row_prefix(const DescRows &rows, uint32_t *pre, int lane)
{
  uint32_t carry = 0;
  for (int base = 0; base < rows.nrows; base += 64)
  {
    const int i = base + lane;
    const uint32_t v = i < rows.nrows ? (rows.cnt[i] + 1u) >> 1 : 0u;
    const uint32_t incl = wave_scan_incl_u32(v, lane);
    if (i < rows.nrows)
      pre[i] = carry + incl - v;
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0)
    pre[rows.nrows] = carry;
}

// ---- step: the run of a wave and of a lane. The concatenated slots of the spans form the index space [0, P); the P slots need T = ceil(P / 64)
// wave-steps of two samples per lane, dealt out to the waves in whole steps (the first T % NWV waves take one more), so only the last step of the
// last wave has idle lanes. Splitting P into NWV equal parts first and rounding each up to whole steps cost up to NWV - 1 extra steps. Inside its
// wave's share lane l walks its own contiguous run — at any step the 64 lanes sit a run length apart and spread over all 16 spatial cells, so the
// 8 fixed-point LDS atomics of a step hit mostly distinct addresses (row-adjacent samples pile onto 1-2 cells and serialise: measured 8 % slower).
// Integer adds commute: the result does not depend on the order. (Enumerating samples instead of slots — 3.7 % fewer sample positions — gave a
// lane pairs that straddle two rows in 85 % of the steps: the second sample's taps loaded twice, a row advance per sample, and a last step of
// one sample per lane for runs of odd length.)
struct DescRun
{
  uint32_t steps;      // slots per lane = steps of this wave
  uint32_t sidx, send; // the lane's slots [sidx, send) of [0, P)
  int row, cdx;        // row and dx of the first sample of slot sidx
  int xend;            // lo[row] + cnt[row]: the row's span ends in front of it
};
template <int NWV>
__device__ __forceinline__ DescRun desc_run(const DescRows &rows, int wave, int lane)
{
  const uint32_t *s_pre = rows.pre;
  const uint32_t P = s_pre[rows.nrows];
  const uint32_t T = (P + 63u) / 64u, tq = T / NWV, tr = T % NWV;
  DescRun r;
  r.steps = tq + ((uint32_t)wave < tr ? 1u : 0u);
  const uint32_t step0 = (uint32_t)wave * tq + min((uint32_t)wave, tr);
  r.sidx = min(P, step0 * 64u + (uint32_t)lane * r.steps);
  r.send = min(P, r.sidx + r.steps);
  // locate the row of the first slot of this lane's run: largest row with pre[row] <= sidx. (Locating the runs of all lanes and phases in one walk
  // without dependent reads — a count per row added at the first lane it counts for, an inclusive sum over the lanes — was measured: no gain,
  // NOTEBOOK section 39.)
  int row = 0;
  if (r.sidx < r.send)
  {
    int lo_r = 0, hi_r = rows.nrows - 1;
    while (lo_r < hi_r)
    {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (s_pre[mid] <= r.sidx)
        lo_r = mid;
      else
        hi_r = mid - 1;
    }
    row = lo_r;
    while (s_pre[row + 1] <= r.sidx) // skip empty rows that share the same prefix value
      row++;
  }
  r.row = row;
  const int lo = rows.lo[row];
  r.cdx = lo + 2 * (int)(r.sidx - s_pre[row]);
  r.xend = lo + (int)rows.cnt[row];
  return r;
}

// the lane's next slot: the window offset (sx, sy) of its first sample — the second is (sx + 1, sy) — and whether each is live (neither for a
// lane whose run has ended; the second not in the last slot of an odd span). One row advance per slot: a slot never straddles two rows.
__device__ __forceinline__ void desc_next_slot(const DescRows &rows, DescRun &r, int &sx, int &sy, bool live[2])
{
  live[0] = r.sidx < r.send;
  if (live[0] && r.cdx >= r.xend)
  {
    uint32_t n;
    do
      n = rows.cnt[++r.row];
    while (n == 0u); // a live slot lies ahead: the walk ends on its row
    r.cdx = rows.lo[r.row];
    r.xend = r.cdx + (int)n;
  }
  sx = r.cdx, sy = rows.y0 + r.row;
  live[1] = live[0] && r.cdx + 1 < r.xend;
  r.cdx += 2, r.sidx++;
}

// ---- step: one slot per lane, two samples. Their (straight-line) contribution code is independent, so the scheduler interleaves the two dependency
// chains instead of padding every compare -> select and transcendental with wait states. A dead sample — both of a lane whose run has ended, the
// second of a span's odd end — takes whatever the loads return: they go through the buffer resource (any offset is safe, the texel past a span's
// end included) and no contribution is executed.
template <bool F16>
__device__ __forceinline__ void desc_step_pair(const DescCtx &c, const DescRows &rows, DescRun &run, uint32_t *s_work)
{
  int sx, sy;
  bool live[2];
  desc_next_slot(rows, run, sx, sy, live);
  DescTaps t0, t1;
  const unsigned v0 = desc_tap_base(c, sx, sy);
  if (F16)
  {
    t0 = desc_taps<F16>(c, v0);
    t1 = desc_taps<F16>(c, desc_tap_base(c, sx + 1, sy));
  }
  else
    desc_taps_pair(c, v0, t0, t1);
  bool o0, o1;
  DescSample s0 = desc_sample<true>(c, sx, sy, t0, &o0), s1 = desc_sample<true>(c, sx + 1, sy, t1, &o1);
  float f0 = angle_bin<true>(s0.xb), f1 = angle_bin<true>(s1.xb);
  o0 |= angle_bin_odd(s0.xb), o1 |= angle_bin_odd(s1.xb);
  if (__builtin_expect(__ballot(o0 || o1) != 0ull, 0))
  {
    // some lane holds a value outside the ranges of the short forms (see desc_sample): the general forms for this step
    s0 = desc_sample<false>(c, sx, sy, t0, nullptr), s1 = desc_sample<false>(c, sx + 1, sy, t1, nullptr);
    f0 = angle_bin<false>(s0.xb), f1 = angle_bin<false>(s1.xb);
  }
  desc_scatter(c, s0, f0, live[0], s_work);
  desc_scatter(c, s1, f1, live[1], s_work);
}

// ---- step: the epilogue (wave 0), in three parts.
// (1) normalise -> clamp at 0.2*norm -> renormalise -> x512 -> u8 (:200-265): lane l gets the bytes of elements l and l + 64
__device__ __forceinline__ uint32_t desc_byte(float v) { return (v != v) ? 0u : (v < 0.f ? 0u : (v > 255.f ? 255u : (uint32_t)v)); }
__device__ __forceinline__ void desc_bytes(const uint32_t *s_work, int ln, uint32_t &b0, uint32_t &b1)
{
  uint32_t w0 = desc_hist_read(s_work, ln), w1 = desc_hist_read(s_work, ln + 64);
  float norm = sqrtf((float)wave_sum_u32(w0 * w0 + w1 * w1));
  uint32_t lim = (uint32_t)(norm * 0.2f);
  w0 = w0 < lim ? w0 : lim;
  w1 = w1 < lim ? w1 : lim;
  norm = sqrtf((float)wave_sum_u32(w0 * w0 + w1 * w1));
  float scale = 512.f / norm;
  b0 = desc_byte((float)w0 * scale), b1 = desc_byte((float)w1 * scale);
}
// (2) pack 4 consecutive bytes per dword: lanes 4q..4q+3 all get dword q (of their half of the descriptor)
__device__ __forceinline__ uint32_t desc_pack4(uint32_t byte, int ln)
{
  uint32_t p = byte << ((uint32_t)(ln & 3) * 8u);
  p |= __shfl_xor(p, 1, 64);
  p |= __shfl_xor(p, 2, 64);
  return p;
}
// (3) the sinks. The descriptor's 32 dwords at dst: the first lane of every group of four stores the group's two
__device__ __forceinline__ void desc_store_dwords(uint32_t *dst, int ln, uint32_t p0, uint32_t p1)
{
  if ((ln & 3) == 0)
  {
    dst[ln >> 2] = p0;
    dst[16 + (ln >> 2)] = p1;
  }
}
// the posted record: its header words from the section record (written by the extraction and orientation launches), the descriptor's 32 words from
// the registers of the lanes that hold them
__device__ __forceinline__ void desc_post_record(const vksift_hip_DenseRows &dr, int b, uint32_t row, const float *rec, int ln, uint32_t p0, uint32_t p1)
{
  const uint32_t j = (uint32_t)ln & 15u;
  const uint32_t d0 = __shfl(p0, (int)(4u * j), 64), d1 = __shfl(p1, (int)(4u * j), 64);
  uint32_t *out = (uint32_t *)(dr.post + (size_t)b * dr.post_img_stride) + (size_t)row * VKSIFT_RECORD_WORDS;
  if (ln < 32)
    out[(int)VKSIFT_RECORD_HEAD_WORDS + ln] = ln < 16 ? d0 : d1;
  else if (ln < (int)VKSIFT_RECORD_WORDS)
    out[ln - 32] = ((const uint32_t *)rec)[ln - 32];
}
// the same 128 bytes as a dense row + |d - 128|^2 = sum d^2 - 256 sum d + 128 * 128^2 (k_shifted_norms): every lane of a group of four holds the
// group's two dwords, the sums run over the 16 groups
__device__ __forceinline__ void desc_dense_row(const vksift_hip_DenseRows &dr, int b, uint32_t row0, uint32_t k, int ln, uint32_t p0, uint32_t p1)
{
  uint32_t *dense = (uint32_t *)(dr.desc + (size_t)b * dr.desc_img_stride) + (size_t)row0 * 32;
  uint32_t *dense_norm = dr.norm + (size_t)b * dr.norm_img_stride + row0;
  uint32_t s2 = __builtin_amdgcn_udot4(p0, p0, 0u, false), s1 = __builtin_amdgcn_udot4(p0, 0x01010101u, 0u, false);
  s2 = __builtin_amdgcn_udot4(p1, p1, s2, false), s1 = __builtin_amdgcn_udot4(p1, 0x01010101u, s1, false);
#pragma unroll
  for (int dlt = 32; dlt >= 4; dlt >>= 1)
  {
    s2 += __shfl_xor(s2, dlt, 64);
    s1 += __shfl_xor(s1, dlt, 64);
  }
  desc_store_dwords(dense + (size_t)k * 32, ln, p0, p1);
  if (ln == 0)
    dense_norm[k] = s2 - 256u * s1 + 128u * 128u * 128u;
}

template <bool CAN_POST>
__device__ __forceinline__ void desc_epilogue(const vksift_hip_DenseRows &dr, const ImageView &g, int b, uint32_t k, const float *rec, const uint32_t *s_work,
                                              const uint32_t *s_row0, int lane)
{
  // (an opaque copy of the lane index for the whole epilogue: addresses and masks derived from it are recomputed per keypoint instead of being
  // hoisted out of the keypoint loop into registers the sample loop cannot spare — hoisted, one of them was spilled, and any scratch costs this
  // kernel per wave launched: tests/test_kernel_resources.py)
  int ln = lane;
  asm volatile("" : "+v"(ln));
  uint32_t b0, b1;
  desc_bytes(s_work, ln, b0, b1);
  const uint32_t p0 = desc_pack4(b0, ln), p1 = desc_pack4(b1, ln);
  desc_store_dwords((uint32_t *)(g.feats + (size_t)k * VKSIFT_RECORD_BYTES + VKSIFT_RECORD_DESC_AT), ln, p0, p1); // the section record
  if (CAN_POST && dr.post)
    desc_post_record(dr, b, *s_row0 + k, rec, ln, p0, p1);
  if (dr.desc)
    desc_dense_row(dr, b, *s_row0, k, ln, p0, p1);
}

// ---- one keypoint, set-up to epilogue, on NW waves of the workgroup (wave = 0 .. NW - 1, tid = 0 .. 64 * NW - 1 among them) with their histogram,
// row arrays of MAXR entries and prefix array (MAXR + 1). NW = 1: the wave shares nothing with its neighbours and only its own program order
// separates the steps (LDS executes a wave's operations in order); otherwise workgroup barriers do, and the first one stands between the previous
// keypoint's epilogue and the zeroing.
// NPH: every wave walks its share of the steps in NPH phases, one after the other — the runs desc_run deals out to NW * NPH waves. What costs a
// wave alone on a keypoint is not its number of steps but the length of its lanes' runs: with T steps in one phase the 64 lanes of a load sit T
// samples apart, one or two to a window row, each in a cache line of its own. Counted on 512 frames with every keypoint on one wave in one phase
// against two waves: SQ_VMEM_TA_ADDR_FIFO_FULL 2.65 G against 0.24 G cycles, L1 misses (TCP_TCC_READ_REQ) 1.24 G against 0.69 G, 5 % fewer VALU
// instructions and 11.2 ms against 6.85 (the "55 % slower" of every earlier one-wave form). Phases give the lanes the short runs of a team.
template <int NW>
__device__ __forceinline__ void desc_sync()
{
  if (NW == 1)
    __builtin_amdgcn_wave_barrier();
  else
    __syncthreads();
}
template <int NW, int NPH, int MAXR, bool PAIRS, bool CAN_POST, bool F16>
__device__ __forceinline__ void desc_keypoint(const FeatArgs &a, const vksift_hip_DenseRows &dr, const ImageView &g, int b, uint32_t k, int wave, int tid,
                                              uint32_t *s_work, int *s_lo, uint32_t *s_cnt, uint32_t *s_pre, const uint32_t *s_row0)
{
  // (PAIRS, the kernel with two call sites in its keypoint loop: opaque copies of the thread index for the steps around the sample loop, as in
  // desc_epilogue — the LDS addresses derived from it were hoisted out of the loop into registers the sample loop cannot spare, and one of them spilled)
  desc_sync<NW>(); // the previous keypoint's epilogue has read the histogram
  {
    int zt = tid;
    if (PAIRS)
      asm volatile("" : "+v"(zt));
    for (int i = zt; i < 256; i += 64 * NW)
      s_work[desc_cell_word(i >> 4) + (i & 15)] = 0; // the 16 grid cells; made visible by the barrier behind the row-span pass below
  }

  const KeyHead kh = keypoint_head<F16>(a, g, b, k);
  const DescCtx c = desc_setup(a, g, kh);
  const int bh = c.dy1 - c.dy0 + 1;
  for (int rb = 0; rb < bh; rb += MAXR)
  {
    const DescRows rows{s_lo, s_cnt, s_pre, c.dy0 + rb, min(MAXR, bh - rb)};
    int rt = tid;
    if (PAIRS)
      asm volatile("" : "+v"(rt));
    desc_sync<NW>();
    desc_row_spans<64 * NW>(c, rows, rt);
    desc_sync<NW>();
    desc_row_prefix(rows, s_pre, rt & 63);
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int ph = 0; ph < NPH; ph++)
    {
      int pt = tid;
      if (PAIRS)
        asm volatile("" : "+v"(pt));
      DescRun run = desc_run<NW * NPH>(rows, wave * NPH + ph, pt & 63);
      for (uint32_t it = 0; it < run.steps; it++)
        desc_step_pair<F16>(c, rows, run, s_work);
    }
  }
  desc_sync<NW>();
  if (wave == 0)
    desc_epilogue<CAN_POST>(dr, g, b, k, kh.rec, s_work, s_row0, tid & 63);
}

// ---- pair mode of the two-wave form: are the windows of keypoints k0 and k0 + 1 both small enough (R <= solo_r) for one wave each? Even lanes
// derive R of the first, odd lanes of the second, as desc_setup does; every wave of the workgroup gets the same answer.
// Phases of a solo wave, 512 frames, descriptor stage against the two-wave launch of the same build and call: 1: +67 %, 2: 0 %, 3: -8.2 %, 4: -9 %,
// 5: -8 %, 6: -5.5 %, 8: -1.2 % (measured when a lane walked samples and a phase of odd length ended in a one-sample step; each phase searches its
// runs. With pair slots 3, 4 and 5 phases were measured again: NOTEBOOK section 39).
#ifndef DESC_SOLO_PHASES
#define DESC_SOLO_PHASES 4
#endif
constexpr int DESC_SOLO_MAX_R = 63; // a solo wave owns half of the row arrays: 2 R + 1 <= DESC_MAX_ROWS / 2
__device__ __forceinline__ bool desc_pair_small(const ImageView &g, uint32_t k0, int lane, uint32_t solo_r)
{
  const float *rec = (const float *)(g.feats + (size_t)(k0 + ((uint32_t)lane & 1u)) * VKSIFT_RECORD_BYTES);
  float lambda;
  const int R = desc_radius(rec[6], ((const int *)rec)[5], &lambda);
  return __ballot(R > (int)solo_r) == 0ull;
}

// solo_r (two-wave form only, 0 .. DESC_SOLO_MAX_R; 0: every keypoint on the whole workgroup, one keypoint per workgroup and sweep): a workgroup owns the
// keypoints 2 kb and 2 kb + 1 of a sweep. Where both windows have R <= solo_r, wave i runs keypoint 2 kb + i alone (solo: the set-up once per keypoint
// instead of once per wave, no workgroup barrier, no wave idle during the epilogue); otherwise — and for an odd last keypoint — both waves run the
// two keypoints one after the other (team). The histogram sums are integer adds: the bytes do not depend on the split.
// LDS: 8 848 bytes per workgroup (two histograms of 2 368, row arrays 2 048, two prefix arrays 2 056, s_row0), 18 workgroups per CU by LDS: the 16 of
// eight waves per SIMD stay the limit.
template <int NWV, bool IMG_FAST, bool F16>
__global__ void __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu((NWV == 2 && !F16) ? 8 : 6, 8)))
k_descriptor(Multi<FeatArgs> m, vksift_hip_DenseRows dr, uint32_t solo_r)
{
  const VBlock vb = vblock(m); // virtual grid (images, blocks) when IMG_FAST, (blocks, images) otherwise
  const FeatArgs &a = m.oct[vb.o];
  constexpr int NSOLO = NWV == 2 ? 2 : 1; // histograms: one per solo wave
  static_assert(2 * DESC_SOLO_MAX_R + 1 <= DESC_MAX_ROWS / 2, "a solo window's rows fit half of the row arrays");
  __shared__ __attribute__((aligned(8))) uint32_t s_work[NSOLO][DESC_WORK_WORDS]; // see desc_scatter
  __shared__ int s_row_lo[DESC_MAX_ROWS];
  __shared__ uint32_t s_row_cnt[DESC_MAX_ROWS];
  __shared__ uint32_t s_row_pre[NWV][DESC_MAX_ROWS + 1];
  __shared__ uint32_t s_row0;
  const int tid = threadIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = (int)(IMG_FAST ? vb.x : vb.y);
  const ImageView g = image_view(a, b);
  const uint32_t bk = IMG_FAST ? vb.y : vb.x, nbk = IMG_FAST ? vb.gy : vb.gx;
  // (posting belongs to single-image detections, which take the four-wave form: the two-wave instantiation of batches — the kernel that
  // sits on its instruction floor with 64 VGPRs — does not carry that code)
  constexpr bool CAN_POST = NWV == 4;
  desc_dense_prologue<CAN_POST>(a, dr, b, bk == 0, tid, &s_row0);

  const uint32_t per = (NWV == 2 && solo_r != 0u) ? 2u : 1u; // keypoints per workgroup and sweep
  if (per == 2u)
    __syncthreads(); // s_row0: a solo wave 1 reads it with no other workgroup barrier behind wave 0's store
  for (uint32_t k0 = bk * per; k0 < g.n; k0 += nbk * per)
  {
    if constexpr (NWV == 2)
      if (per == 2u && k0 + 1u < g.n && desc_pair_small(g, k0, lane, solo_r))
      {
        constexpr int HALF = DESC_MAX_ROWS / 2;
        desc_keypoint<1, DESC_SOLO_PHASES, HALF, true, CAN_POST, F16>(a, dr, g, b, k0 + (uint32_t)wave, 0, lane, s_work[wave], s_row_lo + wave * HALF, s_row_cnt + wave * HALF,
                                              s_row_pre[wave], &s_row0);
        continue;
      }
    const uint32_t k1 = min(k0 + per, g.n);
    for (uint32_t k = k0; k < k1; k++)
      desc_keypoint<NWV, 1, DESC_MAX_ROWS, NWV == 2, CAN_POST, F16>(a, dr, g, b, k, wave, tid, s_work[0], s_row_lo, s_row_cnt, s_row_pre[wave], &s_row0);
  }
}

FeatArgs make_args(const vksift_hip_OctaveJob *job)
{
  FeatArgs a;
  a.gauss = job->gauss;
  a.fp16 = job->fp16;
  a.w = (int)job->w, a.h = (int)job->h, a.pitch = (int)job->pitch;
  a.plane_stride = job->plane_stride, a.img_stride = job->img_stride;
  a.feats = job->feats, a.feat_img_stride = job->feat_img_stride, a.cap = job->cap;
  a.found = job->found, a.found_img_stride = job->found_img_stride;
  a.ori_ang = job->ori_ang, a.ori_cnt = job->ori_cnt, a.ori_img_stride = job->ori_img_stride;
  uint32_t mk = job->max_ori == 0 ? VKSIFT_HIP_MAX_ORI : job->max_ori;
  a.max_keep = mk > VKSIFT_HIP_MAX_ORI ? VKSIFT_HIP_MAX_ORI : mk;
  a.use_vlfeat = job->use_vlfeat;
  a.desc_fp_tab = job->desc_fp_tab, a.desc_fp_tab_len = job->desc_fp_tab_len;
  a.sec = job->sec_index;
  return a;
}

// Work -> workgroup mapping of the per-keypoint kernels. The number of busy workgroups of an image (its keypoint count)
// is only known on the device and usually a small part of the grid. With the keypoint index fastest the busy ones form
// a run at the start of every image's row, which the dispatcher's round-robin over XCDs and shader engines can map onto a
// fraction of the machine (measured on the refinement kernels: 3x); with the image index fastest the busy workgroups
// are contiguous in dispatch order, and for batches that are multiples of 8 every image stays on one XCD (its pyramid
// planes in one L2). grid.y is limited to 65535.
bool img_fast(uint32_t batch, bool descriptor)
{
  /* Measured (128 x 640x480): orientation -5 %, descriptor +3 % (its grid is mostly busy and the keypoint-fastest order spreads the long
   * coarse-scale windows better): the orientation kernel only */
  return batch > 1 && !descriptor;
}

// an octave's share of a per-keypoint kernel's grid, in either order of the virtual grid
bool add_octave(Multi<FeatArgs> &m, const FeatArgs &a, bool img_fast, uint32_t batch, uint32_t blocks)
{
  return multi_add(m, a, img_fast ? batch : blocks, img_fast ? blocks : batch, 1u);
}

// grid sizing only (the kernels stride over the real, device-side count): a generous estimate of the keypoints of an octave
uint32_t expected_keypoints(const vksift_hip_OctaveJob *job, uint32_t batch)
{
  const uint32_t pixels_per_keypoint = 512;
  if (batch < 8u) /* a handful of images: idle workgroups cost nothing, keep the full parallelism */
    return 0xFFFFFFFFu;
  const uint64_t n = (uint64_t)job->w * job->h / pixels_per_keypoint;
  return n < 32u ? 32u : (n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n);
}

/* Workgroups per image of an octave's share, kp_per_block keypoints each, at most cap_blocks. The keypoint count is only known on the
 * device; the share is sized for a dense octave (one keypoint per 512 pixels, twice the usual yield) and strides over whatever is there.
 * Sizing it by the section capacity alone gave the coarse octaves 131 k workgroups per stage for a few hundred keypoints: 40-70 us of
 * pure dispatch each. */
uint32_t octave_blocks(const vksift_hip_OctaveJob *job, uint32_t batch, uint32_t kp_per_block, uint32_t cap_blocks)
{
  const uint32_t dense = expected_keypoints(job, batch);
  uint32_t blocks = ((job->cap < dense ? job->cap : dense) + (kp_per_block - 1)) / kp_per_block;
  if (blocks > cap_blocks)
    blocks = cap_blocks;
  return blocks == 0 ? 1 : blocks;
}

} // namespace

// the launches of one run of at most MULTI_MAX octaves
static int orientation_run(const vksift_hip_OctaveJob *jobs, uint32_t n, uint32_t batch, hipStream_t hs)
{
  Multi<FeatArgs> mo, mf;
  mo.n = mf.n = 0;
  const bool f = img_fast(batch, false);
  /* capped so that an octave's share is ~16 k workgroups whatever the batch: the workgroups stride over the keypoints,
   * and beyond that more (mostly idle) workgroups only cost dispatch — 512 frames: 1024 per image 1.97 ms, 128: 1.84, 32: 1.71 */
  uint32_t cap_blocks = 16384u / batch;
  cap_blocks = cap_blocks < 32u ? 32u : (cap_blocks > 1024u ? 1024u : cap_blocks);
  for (uint32_t i = 0; i < n; i++)
  {
    const FeatArgs a = make_args(&jobs[i]);
    if (!add_octave(mo, a, f, batch, octave_blocks(&jobs[i], batch, 4, cap_blocks)) || !multi_add(mf, a, batch, 1u, 1u))
      return (int)hipErrorInvalidValue;
  }
  const bool f16 = mo.oct[0].fp16 != 0;
  const dim3 grid(mo.start[mo.n]);
  with_bool(f, [&](auto IMG_FAST) {
    with_bool(f16, [&](auto F16) { hipLaunchKernelGGL((k_orientation<decltype(IMG_FAST)::value, decltype(F16)::value>), grid, dim3(256), 0, hs, mo); });
  });
  hipLaunchKernelGGL(k_orientation_finalize, dim3(mf.start[mf.n]), dim3(1024), 0, hs, mf);
  return (int)hipGetLastError();
}

static int descriptor_run(const vksift_hip_OctaveJob *jobs, uint32_t n, uint32_t batch, const vksift_hip_DenseRows &dr, hipStream_t hs)
{
  Multi<FeatArgs> md;
  md.n = 0;
  const bool f = img_fast(batch, true);
  /* waves per keypoint: 4 keep the critical path of a single image short (1 wave: 55 % slower, 8: no faster than 4); a batch has keypoints
   * to spare and runs 3-4 % faster with 2 (less redundant per-keypoint work, measured under the overlapped batch schedule) */
  const bool two_waves = batch >= 8u;
  /* pair mode of the two-wave form (k_descriptor): the largest R a wave takes alone; 0: none, one keypoint per workgroup as in the four-wave form.
   * Swept on 512 frames (R there is 17 .. 34): the descriptor stage falls as the threshold rises, 0: 6.96, 28: 6.78, 63: 6.36 ms */
  const int tune_r = vksift_hip_tune_get(VKSIFT_TUNE_DESC_SOLO_R);
  const uint32_t solo_r = !two_waves || tune_r <= 0 ? 0u : (tune_r > DESC_SOLO_MAX_R ? (uint32_t)DESC_SOLO_MAX_R : (uint32_t)tune_r);
  for (uint32_t i = 0; i < n; i++)
    if (!add_octave(md, make_args(&jobs[i]), f, batch, octave_blocks(&jobs[i], batch, solo_r ? 2 : 1, 2048)))
      return (int)hipErrorInvalidValue;
  if (dr.post && two_waves)
    return (int)hipErrorInvalidValue; /* posting is compiled into the four-wave form only */
  const bool f16 = md.oct[0].fp16 != 0;
  const dim3 grid(md.start[md.n]);
  with_bool(two_waves, [&](auto TWO) {
    constexpr int NWV = decltype(TWO)::value ? 2 : 4;
    with_bool(f, [&](auto IMG_FAST) {
      with_bool(f16, [&](auto F16) {
        hipLaunchKernelGGL((k_descriptor<NWV, decltype(IMG_FAST)::value, decltype(F16)::value>), grid, dim3(64 * NWV), 0, hs, md, dr, solo_r);
      });
    });
  });
  return (int)hipGetLastError();
}

template <typename F>
static int for_runs(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, F run)
{
  for (uint32_t i0 = 0; i0 < n_jobs;)
  {
    uint32_t i1 = i0 + 1;
    while (i1 < n_jobs && i1 - i0 < multi_run_max() && jobs[i1].fp16 == jobs[i0].fp16)
      i1++;
    const int e = run(jobs + i0, i1 - i0);
    if (e)
      return e;
    i0 = i1;
  }
  return 0;
}

extern "C"
{
  int vksift_hip_orientations_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s)
  {
    if (batch == 0)
      return 0;
    return for_runs(jobs, n_jobs, [&](const vksift_hip_OctaveJob *j, uint32_t n) { return orientation_run(j, n, batch, (hipStream_t)s); });
  }

  int vksift_hip_descriptors_multi_dense(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, const vksift_hip_DenseRows *dense,
                                         vksift_hip_stream s)
  {
    if (batch == 0)
      return 0;
    vksift_hip_DenseRows dr = {};
    if (dense)
    {
      const bool rows = dense->desc != NULL, post = dense->post != NULL;
      if ((!rows && !post) || (rows && (!dense->norm || !dense->n)) || (post && (!dense->found_post || dense->found_post_n > 64u)) || dense->nsec == 0 ||
          dense->nsec > 16u)
        return (int)hipErrorInvalidValue;
      for (uint32_t i = 0; i < n_jobs; i++)
        if (jobs[i].sec_index >= dense->nsec)
          return (int)hipErrorInvalidValue;
      dr = *dense;
    }
    return for_runs(jobs, n_jobs, [&](const vksift_hip_OctaveJob *j, uint32_t n) { return descriptor_run(j, n, batch, dr, (hipStream_t)s); });
  }

  int vksift_hip_descriptors_multi(const vksift_hip_OctaveJob *jobs, uint32_t n_jobs, uint32_t batch, vksift_hip_stream s)
  {
    return vksift_hip_descriptors_multi_dense(jobs, n_jobs, batch, nullptr, s);
  }

  int vksift_hip_orientations(const vksift_hip_OctaveJob *job, uint32_t batch, vksift_hip_stream s) { return vksift_hip_orientations_multi(job, 1, batch, s); }

  int vksift_hip_descriptors(const vksift_hip_OctaveJob *job, uint32_t batch, vksift_hip_stream s) { return vksift_hip_descriptors_multi(job, 1, batch, s); }
}
