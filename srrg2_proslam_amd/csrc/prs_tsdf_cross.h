// prs_tsdf_cross.h -- a taken crossing of a TSDF volume as the surface call and the mesh call both state it
// (include/proslam_hip_tsdf.h, "crossing", "point", "normal"): the band test, the point on the edge and the normal at its nearer
// end.  tsdf.hip and tsdf_mesh.hip run these expressions and no others, so a mesh face and a surface row agree byte for byte.
// Explicit two-operand float32 in the order the header writes; the axis e may be a constant or a lane's own value.
#pragma once
#include <float.h>
#include <math.h>

#include "prs_device.h"

namespace prs {

__device__ __forceinline__ bool in_band(const float2 c, const float min_weight) {
  return c.y >= min_weight && fabsf(c.x) < 1.0f;
}

// the xyz row of the crossing between voxel a = (i, j, k), value va, and its next voxel along e, value vn: a's centre moved along
// e by s * voxel_size, and the smaller weight.  o: origin[b]
__device__ __forceinline__ float4 crossing_point(const float* o, const int i, const int j, const int k, const int e, const float2 va, const float2 vn,
                                                 const float vs) {
  const float ta = va.x, tn = vn.x;
  const float sfrac = ta / (ta - tn);
  float p0 = o[0] + ((float) i + 0.5f) * vs;
  float p1 = o[1] + ((float) j + 0.5f) * vs;
  float p2 = o[2] + ((float) k + 0.5f) * vs;
  const float moved = (e == 0 ? p0 : (e == 1 ? p1 : p2)) + sfrac * vs;
  p0 = e == 0 ? moved : p0;
  p1 = e == 1 ? moved : p1;
  p2 = e == 2 ? moved : p2;
  const float wa = va.y, wn = vn.y;
  return make_float4(p0, p1, p2, wn < wa ? wn : wa);
}

// the normal row of the same crossing: central differences of tsdf at the end whose |tsdf| is smaller (a tie goes to a), an
// unobserved or absent neighbour replaced by that end's own value.  vol: the sequence's volume, lin: a's linear index, stride_e: the
// linear step along e
__device__ __forceinline__ float4 crossing_normal(const float2* vol, const int lin, const int i, const int j, const int k, const int e,
                                                  const int stride_e, const float ta, const float tn, const int nx, const int ny, const int nz,
                                                  const float mw) {
  const int n[3]      = {nx, ny, nz};
  const int stride[3] = {1, nx, nx * ny};
  const int at[3]     = {i, j, k};
  const bool at_n = fabsf(tn) < fabsf(ta);
  const int g     = at_n ? lin + stride_e : lin;
  const float tg  = at_n ? tn : ta;
  float m[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int gd = at[d] + ((at_n && d == e) ? 1 : 0);
    float hi = tg, lo = tg;
    if (gd + 1 < n[d]) {
      const float2 h = vol[g + stride[d]];
      hi = h.y >= mw ? h.x : tg;
    }
    if (gd >= 1) {
      const float2 l = vol[g - stride[d]];
      lo = l.y >= mw ? l.x : tg;
    }
    m[d] = hi - lo;
  }
  const float len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  float4 nrm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (len2 > 0.0f && len2 <= FLT_MAX) {
    const float len = sqrtf(len2);
    nrm = make_float4(m[0] / len, m[1] / len, m[2] / len, 1.0f);
  }
  return nrm;
}

}  // namespace prs
