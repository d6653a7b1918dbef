// extrema_refine.h — the sub-pixel refinement of a DoG extremum and what its callers share: the view of an image's octave, the two loaders of
// the 19 DoG values a step reads, refine_core(), the stored record, the arguments of the extraction launches. Included by extrema.hip (the scan
// and the four-launch tail) and extract_tail.hip (the one-launch tail of batches); see extrema.hip for the stage as a whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../detmath.h"
#include "records.h"
#include "vksift_hip.h"

struct ExtremaArgs
{
  const float *gauss; // Gaussian layer 0 of image 0 of the octave (S+3 layers, plane_stride apart)
  int fp16;           // binary16 texels (strides stay in texels)
  int w, h, pitch;
  uint64_t plane_stride, img_stride;
  int S, octave_idx;
  float seed_sigma, dog_threshold, edge_limit;
  uint64_t *seg_mask;
  uint32_t *seg_off;
  uint64_t seg_img_stride;
  int nseg;
  uint8_t *feats;
  uint64_t feat_img_stride;
  uint32_t cap;
  uint32_t *found;
  uint32_t found_img_stride;
  uint32_t *cand_xy;   // packed x | y << 14 | scale << 28, raster order
  uint32_t *cand_flag; // 1 = accepted by the refinement
  uint32_t *cand_n;    // per image: number of candidates (clamped to cand_cap)
  uint64_t cand_img_stride;
  uint32_t cand_cap;
  int band;        // rows per wave of the streaming scan
  uint32_t nsegs;  // S * h * nseg: mask segments of one image
  uint32_t nchunks; // ceil(nsegs / SEG_CHUNK)
  int scan_rev; // the streaming scan walks every XCD's share of the work space back to front (vksift_hip_OctaveJob::scan_reverse)
};

namespace
{

struct DogView
{
  const float *base; // GAUSSIAN layer 0 of the octave: DoG layer s = Gaussian layer s+1 - Gaussian layer s
  int w, h, pitch;
  size_t plane; // texels between layers
  int S;
};

// imageLoad of the DoG image with robust out-of-bounds behaviour on the layer axis (quirk Q1): layer S+2 reads 0.
// F16 (binary16 texels: widened exactly; the DoG image of such a pyramid is binary16 too) is a template parameter of everything
// that refines: a run-time flag inside this function was miscompiled (fp32 results of images >= 1 of a batch changed with
// unrelated edits of the callers).
template <bool F16>
__device__ __forceinline__ float ld(const DogView &d, int s, int x, int y)
{
  if (s < 0 || s > d.S + 1)
    return 0.f;
  if (F16)
  {
    const _Float16 *p = (const _Float16 *)d.base + (size_t)s * d.plane + (size_t)y * d.pitch + x;
    return (float)(_Float16)((float)p[d.plane] - (float)p[0]);
  }
  const float *p = d.base + (size_t)s * d.plane + (size_t)y * d.pitch + x;
  return p[d.plane] - p[0];
}

struct KpRecord
{
  float x, y, scale_x, scale_y;
  uint32_t scale_idx;
  int32_t octave_idx;
  float sigma, orientation, intensity;
};

// The 19 DoG values a refinement step reads around (x, y, s): the centre, its neighbours along each axis, and the four
// diagonal neighbours in each of the planes (s, x), (s, y) and (x, y). Named by the axis and sign of their offsets.
struct Dog19
{
  float c;
  float sp, sm, xp, xm, yp, ym;
  float sp_xp, sp_xm, sm_xp, sm_xm;
  float sp_yp, sp_ym, sm_yp, sm_ym;
  float xp_yp, xp_ym, xm_yp, xm_ym;
};

// 19 imageLoads through 64-bit pointers: serves octaves of any size. Each costs two 64-bit multiply-adds and an exec-mask branch
// for the layer test (300 of the 700 VALU instructions of a step are addressing), so the step loop stays rolled.
template <bool F16>
struct PtrLoader
{
  static constexpr int UNROLL_STEPS = 1;
  const DogView &d;
  __device__ __forceinline__ Dog19 operator()(int x, int y, int s) const
  {
    Dog19 v;
    v.c = ld<F16>(d, s, x, y);
    v.sp = ld<F16>(d, s + 1, x, y), v.sm = ld<F16>(d, s - 1, x, y);
    v.xp = ld<F16>(d, s, x + 1, y), v.xm = ld<F16>(d, s, x - 1, y);
    v.yp = ld<F16>(d, s, x, y + 1), v.ym = ld<F16>(d, s, x, y - 1);
    v.sp_xp = ld<F16>(d, s + 1, x + 1, y), v.sp_xm = ld<F16>(d, s + 1, x - 1, y), v.sm_xp = ld<F16>(d, s - 1, x + 1, y), v.sm_xm = ld<F16>(d, s - 1, x - 1, y);
    v.sp_yp = ld<F16>(d, s + 1, x, y + 1), v.sp_ym = ld<F16>(d, s + 1, x, y - 1), v.sm_yp = ld<F16>(d, s - 1, x, y + 1), v.sm_ym = ld<F16>(d, s - 1, x, y - 1);
    v.xp_yp = ld<F16>(d, s, x + 1, y + 1), v.xp_ym = ld<F16>(d, s, x + 1, y - 1), v.xm_yp = ld<F16>(d, s, x - 1, y + 1), v.xm_ym = ld<F16>(d, s, x - 1, y - 1);
    return v;
  }
};

// The same values through a BUFFER RESOURCE over the octave of one image (32-bit byte offsets, the rows as scalar offsets, the
// columns as immediates): no address arithmetic and no branch per value. A step loads the 28 GAUSSIAN texels of its neighbourhood
// once (5 + 9 + 9 + 5 over the four layers; the pointer form loads 38 + 38) and forms the 19 DoG values from them with the same
// subtraction: bit-identical. The step loop is unrolled. The caller guarantees (S + 3) * plane * texel bytes < 2^31.
template <bool F16>
struct BufLoader
{
  static constexpr int UNROLL_STEPS = 5;
  static constexpr unsigned EB = F16 ? 2u : 4u;
  const __amdgpu_buffer_rsrc_t rsrc;
  const int pitch;
  const unsigned plane;
  const int S;
  __device__ __forceinline__ float tex(unsigned base, int row_off) const
  {
    if (F16)
      return (float)__builtin_bit_cast(_Float16, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rsrc, base, row_off, 0));
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, base, row_off, 0));
  }
  static __device__ __forceinline__ float dog(float hi, float lo) { return F16 ? (float)(_Float16)(hi - lo) : hi - lo; }
  __device__ __forceinline__ Dog19 operator()(int x, int y, int s) const
  {
    const int pitch_b = pitch * (int)EB;
    const unsigned plane_b = plane * EB;
    // byte offset of Gaussian texel (x - 1, y - 1) of layer s; s >= 1, x >= 1, y >= 1 always
    const unsigned b0 = ((unsigned)s * plane + (unsigned)(y - 1) * (unsigned)pitch + (unsigned)(x - 1)) * EB;
    const unsigned bm = b0 - plane_b, b1 = b0 + plane_b, b2 = b1 + plane_b; // layers s - 1, s + 1, s + 2 (past the last layer: reads 0)
    // Gaussian texels: the full 3x3 of layers s and s + 1, the cross of layers s - 1 and s + 2
    float g0[3][3], g1[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++)
      {
        g0[j][i] = tex(b0 + (unsigned)i * EB, j * pitch_b);
        g1[j][i] = tex(b1 + (unsigned)i * EB, j * pitch_b);
      }
    const float gm_c = tex(bm + EB, pitch_b), gm_xm = tex(bm, pitch_b), gm_xp = tex(bm + 2u * EB, pitch_b), gm_ym = tex(bm + EB, 0), gm_yp = tex(bm + EB, 2 * pitch_b);
    const float g2_c = tex(b2 + EB, pitch_b), g2_xm = tex(b2, pitch_b), g2_xp = tex(b2 + 2u * EB, pitch_b), g2_ym = tex(b2 + EB, 0), g2_yp = tex(b2 + EB, 2 * pitch_b);
    // DoG layer s + 1 exists up to S + 1 (quirk Q1: beyond it the reference's image load returns 0)
    const bool up = s + 1 <= S + 1;
    Dog19 v;
    v.sp = up ? dog(g2_c, g1[1][1]) : 0.f, v.sm = dog(g0[1][1], gm_c);
    v.sp_xp = up ? dog(g2_xp, g1[1][2]) : 0.f, v.sp_xm = up ? dog(g2_xm, g1[1][0]) : 0.f;
    v.sp_yp = up ? dog(g2_yp, g1[2][1]) : 0.f, v.sp_ym = up ? dog(g2_ym, g1[0][1]) : 0.f;
    v.sm_xp = dog(g0[1][2], gm_xp), v.sm_xm = dog(g0[1][0], gm_xm), v.sm_yp = dog(g0[2][1], gm_yp), v.sm_ym = dog(g0[0][1], gm_ym);
    float d0[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++)
        d0[j][i] = dog(g1[j][i], g0[j][i]);
    v.c = d0[1][1];
    v.xp = d0[1][2], v.xm = d0[1][0], v.yp = d0[2][1], v.ym = d0[0][1];
    v.xp_yp = d0[2][2], v.xp_ym = d0[0][2], v.xm_yp = d0[2][0], v.xm_ym = d0[0][0];
    return v;
  }
};

// Refinement + acceptance tests (ExtractKeypoints.comp:121-224) of the candidate at (x, y, s) of a W x H octave with S scales.
template <class Load>
__device__ bool refine_core(const Load &load, int W, int H, int S, int x, int y, int s, float dog_threshold, float edge_limit, float seed_sigma, int octave_idx,
                            KpRecord *kp)
{
  float oX = 0.f, oY = 0.f, oS = 0.f, gX = 0.f, gY = 0.f, gS = 0.f;
  float vc = 0.f, xp = 0.f, xm = 0.f, yp = 0.f, ym = 0.f, h23 = 0.f;
  int rx = x, ry = y, rs = s;
#pragma unroll Load::UNROLL_STEPS
  for (int step = 0; step < 5; step++)
  {
    const Dog19 v = load(rx, ry, rs);
    vc = v.c;
    xp = v.xp, xm = v.xm, yp = v.yp, ym = v.ym;
    gS = 0.5f * (v.sp - v.sm);
    gX = 0.5f * (xp - xm);
    gY = 0.5f * (yp - ym);
    float h11 = v.sp + v.sm - 2.f * vc;
    float h22 = xp + xm - 2.f * vc;
    float h33 = yp + ym - 2.f * vc;
    float h12 = 0.25f * (v.sp_xp - v.sp_xm - v.sm_xp + v.sm_xm);
    float h13 = 0.25f * (v.sp_yp - v.sp_ym - v.sm_yp + v.sm_ym);
    h23 = 0.25f * (v.xp_yp - v.xp_ym - v.xm_yp + v.xm_ym);

    float det = h11 * ((h22 * h33) - (h23 * h23)) - h12 * ((h12 * h33) - (h13 * h23)) + h13 * ((h12 * h23) - (h13 * h22));
    if (det == 0.0f)
      return false;
    float i11 = ((h22 * h33) - (h23 * h23)) / det;
    float i12 = -1.f * ((h12 * h33) - (h13 * h23)) / det;
    float i13 = ((h12 * h23) - (h13 * h22)) / det;
    float i22 = ((h11 * h33) - (h13 * h13)) / det;
    float i23 = -1.f * ((h11 * h23) - (h13 * h12)) / det;
    float i33 = ((h11 * h22) - (h12 * h12)) / det;
    oS = -i11 * gS - i12 * gX - i13 * gY;
    oX = -i12 * gS - i22 * gX - i23 * gY;
    oY = -i13 * gS - i23 * gX - i33 * gY;

    if (fabsf(oX) < 0.6f && fabsf(oY) < 0.6f && fabsf(oS) < 0.6f)
      break;
    else if (step < 4)
    {
      rx += ((oX >= 0.6f && rx < (W - 2)) ? 1 : 0) + ((oX <= -0.6f && rx > 1) ? -1 : 0);
      ry += ((oY >= 0.6f && ry < (H - 2)) ? 1 : 0) + ((oY <= -0.6f && ry > 1) ? -1 : 0);
      rs += ((oS >= 0.6f && rs < (S + 1)) ? 1 : 0) + ((oS <= -0.6f && rs > 1) ? -1 : 0);
    }
  }
  // (rx, ry, rs) is where the last neighbourhood was loaded (the position does not move after the last loads): vc, the axis
  // neighbours and h23's diagonal differences are the values the acceptance and edge tests read
  float sx = (float)rx + oX, sy = (float)ry + oY, ss = (float)rs + oS;
  float nv = vc + 0.5f * (gX * oX + gY * oY + gS * oS);
  if (!(fabsf(nv) > dog_threshold && fabsf(oX) < 1.5f && fabsf(oY) < 1.5f && fabsf(oS) < 1.5f && sx >= 0 && sx < (float)W && sy >= 0 && sy < (float)H &&
        ss >= 0 && ss <= (float)(S + 1)))
    return false;
  float e11 = xp + xm - 2.f * vc;
  float e22 = yp + ym - 2.f * vc;
  float e12 = h23;
  float edgeness = ((e11 + e22) * (e11 + e22)) / ((e11 * e22) - (e12 * e12));
  if (!((edgeness < edge_limit) && (edgeness >= 0)))
    return false;

  float scale_factor = octave_idx >= 0 ? dm_pow2i(octave_idx) : 1.f / dm_pow2i(-octave_idx);
  kp->scale_x = sx;
  kp->scale_y = sy;
  kp->scale_idx = (uint32_t)roundf(ss);
  kp->octave_idx = octave_idx;
  kp->sigma = seed_sigma * dm_exp2f(ss / (float)S) * scale_factor;
  kp->orientation = 0.f;
  kp->intensity = nv;
  kp->x = sx * scale_factor;
  kp->y = sy * scale_factor;
  return true;
}

__device__ __forceinline__ void store_record(uint32_t *rec, const KpRecord &kp)
{
  static_assert(sizeof(KpRecord) == VKSIFT_RECORD_HEAD_WORDS * 4u, "the header words of a stored record");
  rec[0] = __float_as_uint(kp.x);
  rec[1] = __float_as_uint(kp.y);
  rec[2] = __float_as_uint(kp.scale_x);
  rec[3] = __float_as_uint(kp.scale_y);
  rec[4] = kp.scale_idx;
  rec[5] = (uint32_t)kp.octave_idx;
  rec[6] = __float_as_uint(kp.sigma);
  rec[7] = __float_as_uint(kp.orientation);
  rec[8] = __float_as_uint(kp.intensity);
}

// What both refinement kernels derive from their octave and image: the candidate list and its (clamped) length, the image's octave as
// a view and as one buffer resource (BUF: the launcher has checked that it stays below 2 GiB), the accept flags and per-chunk accept counts
// (in the segment-offset array, free again after k_cand_list).
struct RefineCtx
{
  const ExtremaArgs &a;
  uint32_t n, nch; // candidates, chunks of 256
  DogView d;
  __amdgpu_buffer_rsrc_t rsrc;
  const uint32_t *xy;
  uint32_t *flag, *chunk_sum;
};

template <bool F16>
__device__ __forceinline__ RefineCtx refine_ctx(const ExtremaArgs &a, int b)
{
  constexpr unsigned EB = F16 ? 2u : 4u;
  const uint32_t found = a.cand_n[b], n = found < a.cand_cap ? found : a.cand_cap;
  const DogView d{(const float *)((const uint8_t *)a.gauss + (size_t)b * a.img_stride * EB), a.w, a.h, a.pitch, (size_t)a.plane_stride, a.S};
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)d.base, 0, (int)((unsigned)(a.S + 3) * (unsigned)a.plane_stride * EB), 0x00020000);
  const size_t at = (size_t)b * a.cand_img_stride;
  return RefineCtx{a, n, (n + 255u) / 256u, d, rsrc, a.cand_xy + at, a.cand_flag + at, a.seg_off + (size_t)b * a.seg_img_stride};
}

// refine the candidate packed as x | y << 14 | scale << 28 (k_cand_list)
template <bool F16, bool BUF>
__device__ __forceinline__ bool refine_candidate(const RefineCtx &c, uint32_t packed, KpRecord *kp)
{
  const ExtremaArgs &a = c.a;
  const int x = (int)(packed & 0x3fffu), y = (int)((packed >> 14) & 0x3fffu), s = (int)(packed >> 28);
  if constexpr (BUF)
    return refine_core(BufLoader<F16>{c.rsrc, a.pitch, (unsigned)a.plane_stride, a.S}, a.w, a.h, a.S, x, y, s, a.dog_threshold, a.edge_limit, a.seed_sigma, a.octave_idx, kp);
  else
    return refine_core(PtrLoader<F16>{c.d}, a.w, a.h, a.S, x, y, s, a.dog_threshold, a.edge_limit, a.seed_sigma, a.octave_idx, kp);
}

} // namespace

/* extract_tail.hip: the tail of a run of octaves (ballots -> records) as ONE launch, one workgroup per (image, octave); args as extract_run() holds them;
 * small_wg: 512-thread workgroups whatever the size of the launch */
int extract_tail_launch(const ExtremaArgs *args, uint32_t n, uint32_t batch, bool f16, bool buf, bool small_wg, hipStream_t hs);
