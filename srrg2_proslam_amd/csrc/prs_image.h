// prs_image.h -- the rules of include/proslam_hip.h that the stages of a [batch][frames][rows][cols] call share, each stated once: what
// a pitch and a call's size may be (host), which frames of a sequence are served and the record of a stereo winner (device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/proslam_hip.h"

namespace prs {

// bytes of an element of a PRS_PIXEL_* / PRS_DEPTH_* type, 0 for a type that is not one
inline int64_t pixel_bytes(const int type) { return type == PRS_PIXEL_U8 ? 1 : type == PRS_PIXEL_U16 ? 2 : type == PRS_PIXEL_F32 ? 4 : 0; }
inline int64_t depth_bytes(const int type) { return type == PRS_DEPTH_U16 ? 2 : type == PRS_DEPTH_F32 ? 4 : 0; }

// a row pitch in bytes holds whole elements and at least cols of them
inline bool pitch_ok(const int64_t pitch, const int64_t cols, const int64_t elem) {
  return pitch % elem == 0 && pitch >= cols * elem;
}

// pixels of a call, 0 when it is refused: a size below 1, or batch * frames, rows * cols or their product (each below 2^62) above 2^31 - 1
inline uint64_t image_pixels(const int64_t batch, const int64_t frames, const int64_t rows, const int64_t cols) {
  if (batch < 1 || frames < 1 || rows < 1 || cols < 1) {
    return 0;
  }
  if (batch * frames > 0x7fffffffll || rows * cols > 0x7fffffffll || batch * frames * rows * cols > 0x7fffffffll) {
    return 0;
  }
  return (uint64_t) (batch * frames * rows * cols);
}

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// the images of sequence b a call on batch o (a struct with n_images and frames) works on; -1: n_images[b] is outside [0, frames]
template <class Batch>
__device__ __forceinline__ int images_of(const Batch& o, const int b) {
  const int n = o.n_images ? o.n_images[b] : o.frames;
  return (n < 0 || n > o.frames) ? -1 : n;
}

// image = b * frames + f
__device__ __forceinline__ int frame_of(const uint32_t image, const int frames) { return (int) (image % (uint32_t) frames); }
__device__ __forceinline__ int sequence_of(const uint32_t image, const int frames) { return (int) (image / (uint32_t) frames); }

// whether the call works on image `image` (its sequence is in range and long enough)
template <class Batch>
__device__ __forceinline__ bool image_served(const Batch& o, const uint32_t image) {
  const int f = frame_of(image, o.frames), b = sequence_of(image, o.frames);
  return f < images_of(o, b);
}

// The record of a left pixel's winner, (the bits of s, i*), from best = (A0 << 16) | i* over the admissible disparity indices i < i_end
// (kStereoNoBest: none), a2 = the least cost two or more indices from i* (kStereoNoCost: none) and Am, Ap = the costs at i* - 1 and
// i* + 1 (read only where both are admissible).  s is 0 when the uniqueness test 100 * A0 < (100 - q) * a2 drops the pixel, else d0 + i*
// + the parabola's (Am - Ap) / (2 * den), den = Am + Ap - 2 * A0 > 0.  The float operations keep their written order (-ffp-contract=off).
constexpr uint32_t kStereoNoCost = 0xffffu;      // above every aggregated cost
constexpr uint32_t kStereoNoBest = 0xffffffffu;  // above every (cost << 16) | i
__device__ __forceinline__ uint2 stereo_winner_record(const uint32_t best, const uint32_t a2, const int Am, const int Ap, const int i_end,
                                                      const int d0, const int q) {
  const bool has  = best != kStereoNoBest;
  const int istar = (int) (best & 0xffffu);
  float s = 0.0f;
  if (has) {
    const int A0    = (int) (best >> 16);
    const bool keep = q == 0 || a2 == kStereoNoCost || 100 * A0 < (100 - q) * (int) a2;
    if (keep) {
      float delta = 0.0f;
      if (istar >= 1 && istar + 1 < i_end) {  // both neighbours in the range and admissible
        const int den = (Am + Ap) - 2 * A0;
        if (den > 0) {
          delta = (float) (Am - Ap) / (float) (2 * den);
        }
      }
      s = (float) (d0 + istar) + delta;
    }
  }
  return make_uint2(__float_as_uint(s), has ? (uint32_t) istar : 0xffffffffu);
}

}  // namespace prs
