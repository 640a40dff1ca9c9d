// prs_depth.h -- what the stages that read depth images through the trajectory share (depth_cloud.hip, depth_consistency.hip): which
// frame has a usable pose, which depth element is valid, and a pixel's point in its camera.  One written expression order for both.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "prs_compact.h"

namespace prs {

// the pose row k of image f of sequence b when the frame is usable, -1 otherwise: k = frame_index[b][f] (f when frame_index is
// NULL) inside [0, pose_stride) and the twelve entries of the top three rows of pose[b][k] finite
__device__ __forceinline__ int depth_pose_row(const int32_t* frame_index, const float* pose, const int frames, const int pose_stride, const int b,
                                              const int f) {
  const int k = frame_index ? frame_index[(size_t) b * frames + f] : f;
  if (k < 0 || k >= pose_stride) {
    return -1;
  }
  const float* P = pose + ((size_t) b * pose_stride + k) * 16;
  bool finite    = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    finite = finite && finite_bits(P[i]);
  }
  return finite ? k : -1;
}

// d = scale * raw, and whether the element is valid: raw > 0 (which drops NaN, -0, 0 and negative values) and d inside
// [range_min, range_max] (which drops +inf)
__device__ __forceinline__ bool depth_valid(const float raw, const float scale, const float range_min, const float range_max, float& d) {
  d = scale * raw;
  return raw > 0.0f && d >= range_min && d <= range_max;
}

// the point of pixel (v, u) at depth d in its camera
__device__ __forceinline__ void depth_point(const int u, const int v, const float d, const float fx, const float fy, const float cx, const float cy,
                                            float* p) {
  p[0] = ((float) u - cx) / fx * d;
  p[1] = ((float) v - cy) / fy * d;
  p[2] = d;
}

}  // namespace prs
