// place.hip — caller-supplied keypoints (vksift_ext_describeKeypoints; OpenCV's detectAndCompute(useProvidedKeypoints), SiftGPU's
// SetKeypointList, VLFeat's vl_sift with frames; no counterpart in the reference, which describes only what it detected): the inverse of the
// last lines of the refinement (extrema_refine.h: refine_core). A keypoint (x, y, sigma) in image pixels becomes the nine header words of a
// record that the orientation and descriptor launchers accept, in the octave section of its image's SIFT buffer.
// One workgroup per image walks the image's keypoints in chunks of its own size, in input order:
//   1. classify: octave = the first whose relative scale sigma * 2^-octave_idx lies below the top threshold (the last otherwise), scale index =
//      the thresholds at or below it — comparisons against a host-made table, no logarithm; position = x * 2^-octave_idx, exact
//   2. one ballot per octave over the admissible keypoints of the chunk, rank inside the wave, the wave totals through LDS, the running
//      count of every octave in LDS: record index = keypoints of the same octave in front of this one. No atomics: deterministic
//   3. header words as plain stores, dropped at and beyond the section's capacity
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../detmath.h"
#include "records.h"
#include "vksift_hip.h"
#include "wave.h"

#define PLACE_WAVES (VKSIFT_HIP_PLACE_WG / 64u)
#define PLACE_MAX_STEPS 14u /* S + 1 thresholds, S <= 13 */

namespace
{

struct PlaceTable // the launch's octaves, by value
{
  uint32_t n_oct, S, keep_orientation;
  float steps[PLACE_MAX_STEPS];
  uint32_t w[VKSIFT_MAX_SECTIONS], h[VKSIFT_MAX_SECTIONS], cap[VKSIFT_MAX_SECTIONS], found_img_stride[VKSIFT_MAX_SECTIONS];
  int32_t octave_idx[VKSIFT_MAX_SECTIONS];
  uint8_t *feats[VKSIFT_MAX_SECTIONS];
  uint64_t feat_img_stride[VKSIFT_MAX_SECTIONS];
  uint32_t *found[VKSIFT_MAX_SECTIONS];
};

__device__ __forceinline__ bool finite_bits(uint32_t v) { return (v & 0x7F800000u) != 0x7F800000u; }

__global__ void __launch_bounds__(VKSIFT_HIP_PLACE_WG) k_place_keypoints(const uint32_t *__restrict__ kps, const uint32_t *__restrict__ kp_first, PlaceTable t,
                                                                         uint32_t *__restrict__ placed)
{
  __shared__ uint32_t wave_tot[PLACE_WAVES][VKSIFT_MAX_SECTIONS], base_s[VKSIFT_MAX_SECTIONS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, b = blockIdx.x;
  const uint32_t first = kp_first[b], end = kp_first[b + 1u], n = end > first ? end - first : 0u;
  if (tid < VKSIFT_MAX_SECTIONS)
    base_s[tid] = 0u;
  __syncthreads();
  const float top = t.steps[t.S];
  for (uint32_t base = 0; base < n; base += VKSIFT_HIP_PLACE_WG)
  {
    const uint32_t i = base + tid;
    bool adm = false;
    uint32_t oct = 0, scale_idx = 0, kw[5] = {0, 0, 0, 0, 0};
    float sx = 0.f, sy = 0.f;
    // ---- 1
    if (i < n)
    {
      const uint32_t *kp = kps + (size_t)(first + i) * 5u;
      for (uint32_t k = 0; k < 5u; k++)
        kw[k] = kp[k];
      const float x = dm_u2f(kw[0]), y = dm_u2f(kw[1]), sigma = dm_u2f(kw[2]), ori = dm_u2f(kw[3]);
      float rel = 0.f, inv = 0.f, wf = 0.f, hf = 0.f;
      // from the last octave down: the last assignment is the first octave that qualifies, the last octave when none does
      for (uint32_t q = 0; q < t.n_oct; q++)
      {
        const uint32_t o = t.n_oct - 1u - q;
        const float f = dm_pow2i(-t.octave_idx[o]), r = sigma * f;
        if (q == 0u || r < top)
          oct = o, rel = r, inv = f, wf = (float)t.w[o], hf = (float)t.h[o];
      }
      for (uint32_t j = 0; j <= t.S; j++)
        scale_idx += rel >= t.steps[j] ? 1u : 0u;
      sx = x * inv, sy = y * inv;
      adm = finite_bits(kw[0]) && finite_bits(kw[1]) && finite_bits(kw[2]) && rel >= 0.02f && rel <= 29.f && sx >= 0.f && sx < wf && sy >= 0.f && sy < hf &&
            (!t.keep_orientation || (ori >= 0.f && ori <= DM_TWO_PI_F));
    }
    // ---- 2
    uint32_t rank = 0;
    for (uint32_t o = 0; o < t.n_oct; o++)
    {
      const unsigned long long bal = __ballot(adm && oct == o);
      if (oct == o)
        rank = ballot_rank(bal, (int)lane);
      if (lane == 0u)
        wave_tot[wave][o] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    // ---- 3
    if (adm)
    {
      uint32_t idx = base_s[oct] + rank;
      for (uint32_t wv = 0; wv < PLACE_WAVES; wv++)
        idx += wv < wave ? wave_tot[wv][oct] : 0u;
      if (idx < t.cap[oct])
      {
        uint32_t *rec = (uint32_t *)(t.feats[oct] + (size_t)b * t.feat_img_stride[oct] + (size_t)idx * VKSIFT_RECORD_BYTES);
        rec[0] = kw[0], rec[1] = kw[1];
        rec[2] = dm_f2u(sx), rec[3] = dm_f2u(sy);
        rec[4] = scale_idx, rec[5] = (uint32_t)t.octave_idx[oct];
        rec[6] = kw[2];
        rec[7] = t.keep_orientation ? kw[3] : 0u;
        rec[8] = kw[4];
      }
    }
    __syncthreads(); // every thread has read the running counts and the wave totals of this chunk
    if (tid < t.n_oct)
    {
      uint32_t sum = 0;
      for (uint32_t wv = 0; wv < PLACE_WAVES; wv++)
        sum += wave_tot[wv][tid];
      base_s[tid] += sum;
    }
    __syncthreads();
  }
  if (tid < t.n_oct)
    t.found[tid][(size_t)b * t.found_img_stride[tid]] = base_s[tid];
  if (tid == 0u)
  {
    uint32_t stored = 0;
    for (uint32_t o = 0; o < t.n_oct; o++)
      stored += section_stored(base_s[o], t.cap[o]);
    placed[b] = stored;
  }
}

} // namespace

extern "C" int vksift_hip_place_keypoints(const vksift_hip_Keypoint *kps, const uint32_t *kp_first, const vksift_hip_PlaceOctave *oct, uint32_t n_oct,
                                          const float *sigma_steps, uint32_t S, uint32_t keep_orientation, uint32_t batch, uint32_t *placed, vksift_hip_stream s)
{
  if (n_oct < 1 || n_oct > VKSIFT_MAX_SECTIONS || S < 1 || S + 1u > PLACE_MAX_STEPS || !oct || !sigma_steps || !kp_first || !placed)
    return (int)hipErrorInvalidValue;
  for (uint32_t o = 0; o < n_oct; o++) /* records are stored dword by dword; 2^-octave_idx is formed from the exponent bits */
    if (!oct[o].feats || !oct[o].found || ((uintptr_t)oct[o].feats & 3u) || (oct[o].feat_img_stride & 3u) || oct[o].octave_idx < -31 || oct[o].octave_idx > 31)
      return (int)hipErrorInvalidValue;
  if (batch == 0)
    return 0;
  PlaceTable t = {};
  t.n_oct = n_oct, t.S = S, t.keep_orientation = keep_orientation ? 1u : 0u;
  for (uint32_t j = 0; j <= S; j++)
    t.steps[j] = sigma_steps[j];
  for (uint32_t o = 0; o < n_oct; o++)
  {
    t.w[o] = oct[o].w, t.h[o] = oct[o].h, t.cap[o] = oct[o].cap, t.found_img_stride[o] = oct[o].found_img_stride;
    t.octave_idx[o] = oct[o].octave_idx;
    t.feats[o] = oct[o].feats, t.feat_img_stride[o] = oct[o].feat_img_stride, t.found[o] = oct[o].found;
  }
  hipLaunchKernelGGL(k_place_keypoints, dim3(batch), dim3(VKSIFT_HIP_PLACE_WG), 0, (hipStream_t)s, (const uint32_t *)kps, kp_first, t, placed);
  return (int)hipGetLastError();
}
