// two_view.h — the test "does the pair (a, b) agree with the model M", once for both users: the RANSAC of verify.hip counts inliers with it
// (scaled coordinates, the sampled model) and the sweep of guided.hip admits candidates with it (pixel coordinates, the published model).
// MODEL is VKSIFT_HIP_GUIDE_HOMOGRAPHY or VKSIFT_HIP_GUIDE_FUNDAMENTAL; M is row-major; t2 the squared threshold in the coordinates' unit.
//   homography:   forward transfer error without a division: with (u, v, d) = M (xa, ya, 1) the pair passes iff
//                 d > 0 and (u - xb d)^2 + (v - yb d)^2 < (d d) t2
//   fundamental:  Sampson distance without a division: with l = M (xa, ya, 1), m = M^T (xb, yb, 1) and r = (xb, yb, 1) l the pair passes
//                 iff r r < t2 ((l0 l0 + l1 l1) + (m0 m0 + m1 m1))
// The test is split into what depends on a alone (side_a), on b alone (side_b) and the rest (admissible), four floats per side:
//   homography:   A {u, v, d, lim} with lim = (d d) t2, replaced by -1 when d > 0 fails; B {xb, yb}
//   fundamental:  A {l0, l1, l2, l0 l0 + l1 l1}; B {xb, yb, m0 m0 + m1 m1}
// so that a sweep computes each side once (guided.hip: in the owner's registers, or while the other side is staged in LDS) and
// admissible(side_a(M, a, t2), side_b(M, b), t2) is the whole test where nothing is reused (verify.hip). Splitting changes no bit: every
// value is the same correctly rounded fp32 add / sub / mul in the same order wherever it is formed (the tree is built with
// -ffp-contract=off), and "d > 0 && e2 < lim" equals "e2 < (d > 0 ? lim : -1)" for every input: e2 is a sum of squares, so it is NaN or
// not below -1, and with d > 0 both sides compare e2 with lim. A NaN anywhere (a row a side does not hold, a degenerate model) fails the
// comparison. tests/np_verify.py, tests/np_verify_f.py and tests/np_guided.py restate the test bit for bit.
#ifndef VKSIFT_TWO_VIEW_H
#define VKSIFT_TWO_VIEW_H

#include <hip/hip_runtime.h>

#include "vksift_hip.h"

template <int MODEL> __device__ __forceinline__ float4 side_a(const float (&M)[9], float2 p, float t2)
{
  const float r0 = (M[0] * p.x + M[1] * p.y) + M[2];
  const float r1 = (M[3] * p.x + M[4] * p.y) + M[5];
  const float r2 = (M[6] * p.x + M[7] * p.y) + M[8];
  if (MODEL == (int)VKSIFT_HIP_GUIDE_HOMOGRAPHY)
  {
    const float lim = (r2 * r2) * t2;
    return float4{r0, r1, r2, r2 > 0.f ? lim : -1.f};
  }
  return float4{r0, r1, r2, r0 * r0 + r1 * r1};
}

template <int MODEL> __device__ __forceinline__ float4 side_b(const float (&M)[9], float2 p)
{
  if (MODEL == (int)VKSIFT_HIP_GUIDE_HOMOGRAPHY)
    return float4{p.x, p.y, 0.f, 0.f};
  const float m0 = (M[0] * p.x + M[3] * p.y) + M[6];
  const float m1 = (M[1] * p.x + M[4] * p.y) + M[7];
  return float4{p.x, p.y, m0 * m0 + m1 * m1, 0.f};
}

template <int MODEL> __device__ __forceinline__ bool admissible(float4 qa, float4 qb, float t2)
{
  if (MODEL == (int)VKSIFT_HIP_GUIDE_HOMOGRAPHY)
  {
    const float ru = qa.x - qb.x * qa.z, rv = qa.y - qb.y * qa.z;
    const float e2 = ru * ru + rv * rv;
    return e2 < qa.w;
  }
  const float r = (qb.x * qa.x + qb.y * qa.y) + qa.z;
  const float g = qa.w + qb.z;
  return r * r < t2 * g;
}

#endif
