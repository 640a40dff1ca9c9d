// depth_consistency.hip -- the depth consistency filter on the device: every depth pixel of a frame is projected into the neighbouring
// frames through the trajectory and kept when enough of them see it at the same place and few enough see past it
// (prs_depth_consistency_batch_run; the rule is stated in include/proslam_hip.h, BUILD-DEFINED, and restated in
// tests/depth_consistency_ref.py).  Two launches:
//   prepare  one workgroup per sequence: validation, status, n_skipped, zeroes in n_kept / n_removed, and one record per image and
//            slot in the workspace: the relative transform M = C_g^-1 C_f (float64 from the float32 camera poses, rounded to float32),
//            whether the slot exists and, in slot 0, the state of the image.  The float64 work is done here, once per slot
//   filter   one workgroup per 64 x 32 pixels of one image, in eight steps of 64 x 4, a lane per pixel: the image's records through LDS
//            once (uniform over the workgroup), the slots in a uniform loop with one gather each, the decision, the counts by wave
//            ballots summed over the steps and one integer atomic add a workgroup and counter (a workgroup per 64 x 4 pixels, built
//            first, spent a third of the call on those adds: 1200 an image on one word; profiles/depth_consistency/README.md)
// The only atomics are integer adds, so no output byte depends on the order they arrive in.
#include <math.h>
#include <stddef.h>

#include <string>

#include "prs_depth.h"
#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kThreads  = 256;
constexpr int kTileW    = 64;  // a wave is one row of the tile
constexpr int kTileH    = kThreads / kTileW;
constexpr int kGroups   = 8;   // steps of a workgroup, one below the other: it owns kTileW x (kTileH * kGroups) pixels
constexpr int kWaves    = kThreads / PRS_WAVE;
constexpr int kMaxSlots = 16;  // 2 * window, window <= 8
constexpr int kRecWords = 16;  // a record: 64 bytes

// a record of the workspace, [batch][frames][2 * window]
struct SlotRecord {
  float M[12];      // the top three rows of C_g^-1 C_f
  int32_t exists;   // the slot votes
  int32_t state;    // slot 0 alone: the image's state
  int32_t unused[2];
};
static_assert(sizeof(SlotRecord) == 4 * kRecWords, "a slot record is 64 bytes");
enum { kImageUntouched = 0, kImageFiltered = 1, kImageSkipped = 2 };

struct DepthConsistencyArgs {
  prs_depth_consistency_params p;
  prs_depth_consistency_batch o;
  int32_t slots;             // 2 * window
  int32_t tiles_x, tiles_y;  // of an image
  SlotRecord* rec;
};

__device__ __forceinline__ int pose_row_of(const DepthConsistencyArgs& a, const int b, const int f) {
  return depth_pose_row(a.o.frame_index, a.o.pose, a.o.frames, a.o.pose_stride, b, f);
}

// C = pose[b][k] * sensor_in_robot, the top three rows
__device__ __forceinline__ void camera_pose(const DepthConsistencyArgs& a, const int b, const int k, float* C) {
  se3_mul<false>(a.o.pose + ((size_t) b * a.o.pose_stride + k) * 16, a.p.sensor_in_robot, C);
}

// ---- prepare: blockIdx.x = b ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void depth_consistency_prepare_kernel(const DepthConsistencyArgs a) {
  __shared__ int s_skipped;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int frames = a.o.frames, slots = a.slots;
  const int n_img  = a.o.n_images ? a.o.n_images[b] : frames;
  SlotRecord* rec  = a.rec + (size_t) b * frames * slots;
  if (n_img < 0 || n_img > frames) {
    for (int f = tid; f < frames; f += kThreads) {
      rec[(size_t) f * slots].state = kImageUntouched;
    }
    if (tid == 0) {
      a.o.status[b] = PRS_ERR_RANGE;
      if (a.o.n_skipped) {
        a.o.n_skipped[b] = 0;
      }
    }
    return;
  }
  if (tid == 0) {
    s_skipped = 0;
  }
  __syncthreads();
  int skipped = 0;
  for (int f = tid; f < frames; f += kThreads) {
    int state = kImageUntouched;
    if (f < n_img) {
      state = pose_row_of(a, b, f) >= 0 ? kImageFiltered : kImageSkipped;
      skipped += state == kImageSkipped ? 1 : 0;
      if (a.o.n_kept) {
        a.o.n_kept[(size_t) b * frames + f] = 0;
      }
      if (a.o.n_removed) {
        a.o.n_removed[(size_t) b * frames + f] = 0;
      }
    }
    rec[(size_t) f * slots].state = state;
  }
  if (skipped) {
    atomicAdd(&s_skipped, skipped);
  }
  // the records of the images that are filtered: a thread per (f, slot)
  const int window = a.p.window;
  for (long long i = tid; i < (long long) n_img * slots; i += kThreads) {
    const int f = (int) (i / slots), s = (int) (i - (long long) f * slots);
    const int j = s < window ? s + 1 : s - window + 1;
    const long long g = s < window ? (long long) f - (long long) j * a.p.stride : (long long) f + (long long) j * a.p.stride;
    SlotRecord& r = rec[i];
    const int kf  = pose_row_of(a, b, f);
    const int kg  = (kf >= 0 && g >= 0 && g < n_img) ? pose_row_of(a, b, (int) g) : -1;
    r.exists      = kg >= 0 ? 1 : 0;
    if (kg >= 0) {
      float Cf[12], Cg[12];
      camera_pose(a, b, kf, Cf);
      camera_pose(a, b, kg, Cg);
      double dt[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        dt[c] = (double) Cf[4 * c + 3] - (double) Cg[4 * c + 3];
      }
#pragma unroll
      for (int row = 0; row < 3; ++row) {
        const double g0 = (double) Cg[0 + row], g1 = (double) Cg[4 + row], g2 = (double) Cg[8 + row];  // column `row` of R_g
#pragma unroll
        for (int col = 0; col < 3; ++col) {
          r.M[4 * row + col] = (float) ((g0 * (double) Cf[0 + col] + g1 * (double) Cf[4 + col]) + g2 * (double) Cf[8 + col]);
        }
        r.M[4 * row + 3] = (float) ((g0 * dt[0] + g1 * dt[1]) + g2 * dt[2]);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.o.status[b] = PRS_OK;
    if (a.o.n_skipped) {
      a.o.n_skipped[b] = s_skipped;
    }
  }
}

// ---- filter: blockIdx.x = ((b * frames + f) * tiles_y + ty) * tiles_x + tx ----------------------------------------------------------
template <typename E>
__device__ __forceinline__ float element_at(const void* depth, const size_t row_bytes, const int u) {
  return (float) reinterpret_cast<const E*>(static_cast<const uint8_t*>(depth) + row_bytes)[u];
}

template <typename E>
__global__ __launch_bounds__(kThreads) void depth_consistency_filter_kernel(const DepthConsistencyArgs a) {
  __shared__ uint32_t s_rec[kMaxSlots * kRecWords];
  __shared__ int s_kept[kWaves], s_removed[kWaves];
  const int tid       = threadIdx.x;
  const uint32_t tx_n = (uint32_t) a.tiles_x, ty_n = (uint32_t) a.tiles_y;
  uint32_t id         = blockIdx.x;
  const int tx = (int) (id % tx_n);
  id /= tx_n;
  const int ty = (int) (id % ty_n);
  const uint32_t image = id / ty_n;  // b * frames + f
  const int slots      = a.slots;
  if (tid < slots * kRecWords) {
    s_rec[tid] = reinterpret_cast<const uint32_t*>(a.rec + (size_t) image * slots)[tid];
  }
  __syncthreads();
  const int state = (int) s_rec[13];
  if (state == kImageUntouched) {
    return;  // behind n_images, or a refused sequence: no depth is read
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const int u = tx * kTileW + (tid & (kTileW - 1));
  const size_t image_row0 = (size_t) image * (size_t) rows;
  const bool counting = a.o.n_kept || a.o.n_removed;
  int kept = 0, gone = 0;  // the wave's
  for (int group = 0; group < kGroups; ++group) {
    const int v0 = (ty * kGroups + group) * kTileH;  // ty * kGroups * kTileH < rows
    if (v0 >= rows) {
      break;  // uniform
    }
    const int v = v0 + tid / kTileW;
    const bool inside = u < cols && v < rows;
    const size_t row = image_row0 + (size_t) (inside ? v : 0);
    E own = E(0);
    float d = 0.0f;
    bool valid = false;
    if (inside && (state == kImageFiltered || a.o.n_removed)) {  // a skipped frame reads its depth only to count what it drops
      own   = reinterpret_cast<const E*>(static_cast<const uint8_t*>(a.o.depth) + row * (size_t) a.o.pitch)[u];
      valid = depth_valid((float) own, a.p.depth_scaling_factor_to_meters, a.p.range_min, a.p.range_max, d);
    }
    int support = 0, violation = 0;
    if (state == kImageFiltered) {
      float p[3];
      depth_point(u, v, d, a.p.fx, a.p.fy, a.p.cx, a.p.cy, p);
      const int f = frame_of(image, a.o.frames);
      const int window = a.p.window;
      for (int s = 0; s < slots; ++s) {
        const float* M = reinterpret_cast<const float*>(s_rec + s * kRecWords);
        if (s_rec[s * kRecWords + 12] == 0) {  // uniform
          continue;
        }
        const int g = s < window ? f - (s + 1) * a.p.stride : f + (s - window + 1) * a.p.stride;  // exists: inside [0, n_images)
        float q[3];
        se3_apply(M, p, q);
        if (!(valid && q[2] > 0.0f)) {
          continue;
        }
        const float x = floorf((q[0] / q[2] * a.p.fx + a.p.cx) + 0.5f);
        const float y = floorf((q[1] / q[2] * a.p.fy + a.p.cy) + 0.5f);
        if (!(x >= 0.0f && x < (float) cols && y >= 0.0f && y < (float) rows)) {
          continue;
        }
        const size_t grow = (size_t) ((long long) image_row0 + (long long) (g - f) * rows) + (size_t) (int) y;
        float dg;
        if (!depth_valid(element_at<E>(a.o.depth, grow * (size_t) a.o.pitch, (int) x), a.p.depth_scaling_factor_to_meters, a.p.range_min, a.p.range_max,
                         dg)) {
          continue;
        }
        const float e = dg - q[2], tol = a.p.max_rel_diff * q[2];
        support += (e >= -tol && e <= tol) ? 1 : 0;
        violation += e > tol ? 1 : 0;
      }
    }
    const bool keep = valid && state == kImageFiltered && support >= a.p.min_support && violation <= a.p.max_violation;
    if (inside) {
      reinterpret_cast<E*>(static_cast<uint8_t*>(a.o.out) + row * (size_t) a.o.out_pitch)[u] = keep ? own : E(0);
      if (a.o.support) {
        a.o.support[row * (size_t) a.o.count_pitch + u] = (uint8_t) support;
      }
      if (a.o.violation) {
        a.o.violation[row * (size_t) a.o.count_pitch + u] = (uint8_t) violation;
      }
    }
    if (counting) {  // uniform
      kept += (int) __popcll(__ballot(keep));
      gone += (int) __popcll(__ballot(valid && !keep));
    }
  }
  if (counting) {
    if ((tid & (PRS_WAVE - 1)) == 0) {
      s_kept[tid >> 6]    = kept;
      s_removed[tid >> 6] = gone;
    }
    __syncthreads();
    if (tid == 0) {
      int sum_kept = 0, sum_removed = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        sum_kept += s_kept[w];
        sum_removed += s_removed[w];
      }
      if (a.o.n_kept && sum_kept != 0) {
        atomicAdd(a.o.n_kept + image, sum_kept);
      }
      if (a.o.n_removed && sum_removed != 0) {
        atomicAdd(a.o.n_removed + image, sum_removed);
      }
    }
  }
}

// records of a call; 0 when a size is not one the launcher takes
uint64_t records_of(const int64_t batch, const int64_t frames, const int64_t window) {
  if (batch < 1 || frames < 1 || window < 1 || window > kMaxSlots / 2 || batch * frames > 0x7fffffffll) {  // the product is below 2^62
    return 0;
  }
  return (uint64_t) (batch * frames * (2 * window));
}

}  // namespace

int depth_consistency_launch(prs_context* ctx, const prs_depth_consistency_params* params, const prs_depth_consistency_batch* batch) {
  const std::string who = "prs_depth_consistency_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_depth_consistency_params& p = *params;
  const prs_depth_consistency_batch& o  = *batch;
  if (!o.depth || !o.pose || !o.out || !o.status || !o.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": depth, pose, out, status or the workspace not set").c_str());
  }
  const int64_t elem = depth_bytes(p.depth_type);
  if (elem == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": unknown depth_type").c_str());
  }
  bool finite        = std::isfinite(p.depth_scaling_factor_to_meters) && std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) &&
                std::isfinite(p.cy) && std::isfinite(p.range_min) && std::isfinite(p.range_max) && std::isfinite(p.max_rel_diff);
  for (int i = 0; i < 16; ++i) {
    finite = finite && std::isfinite(p.sensor_in_robot[i]);
  }
  if (o.batch < 1 || o.frames < 1 || o.rows < 1 || o.cols < 1 || o.pose_stride < 1 || p.window < 1 || p.window > kMaxSlots / 2 || p.stride < 1 ||
      p.min_support < 0 || p.min_support > kMaxSlots || p.max_violation < 0 || p.max_violation > kMaxSlots || !finite || p.max_rel_diff < 0.0f ||
      !(p.depth_scaling_factor_to_meters > 0.0f) || p.range_min < 0.0f || p.range_min > p.range_max || !pitch_ok(o.pitch, o.cols, elem) ||
      !pitch_ok(o.out_pitch, o.cols, elem) ||
      ((o.support || o.violation) && o.count_pitch < o.cols)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size or stride below 1, window outside 1 .. 8, min_support or max_violation outside 0 .. 16, a parameter not finite, max_rel_diff below 0, a scale not positive, range_min negative or above range_max, or a pitch below the row's bytes or not a multiple of the element").c_str());
  }
  if (!aligned_to(o.depth, (uintptr_t) elem) || !aligned_to(o.out, (uintptr_t) elem) || !aligned_to(o.workspace, 16) || !aligned_to(o.n_images, 4) ||
      !aligned_to(o.pose, 4) || !aligned_to(o.frame_index, 4) || !aligned_to(o.n_kept, 4) || !aligned_to(o.n_removed, 4) ||
      !aligned_to(o.n_skipped, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": the workspace must be 16-byte aligned, depth and out to their element, the other arrays but support and violation 4-byte").c_str());
  }
  const int64_t images = (int64_t) o.batch * o.frames;  // below 2^62
  if (o.rows > (1 << 24) || o.cols > (1 << 24) || images > 0x7fffffffll || images * o.rows > 0x7fffffffll ||
      images * o.rows * o.cols > 0x7fffffffll) {  // each factor of the last product is below 2^31, the product before it too
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": rows or cols above 2^24, or batch * frames * rows * cols beyond 2^31 - 1").c_str());
  }
  const uint64_t image_rows = (uint64_t) images * (uint64_t) o.rows, depth_bytes = image_rows * (uint64_t) o.pitch;
  if (overlap(o.depth, depth_bytes, o.out, image_rows * (uint64_t) o.out_pitch) ||
      (o.support && overlap(o.depth, depth_bytes, o.support, image_rows * (uint64_t) o.count_pitch)) ||
      (o.violation && overlap(o.depth, depth_bytes, o.violation, image_rows * (uint64_t) o.count_pitch))) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": out, support and violation must not overlap depth, which is read while they are written").c_str());
  }
  DepthConsistencyArgs a = {};
  a.p = p;
  a.o = o;
  a.slots   = 2 * p.window;
  a.tiles_x = (o.cols + kTileW - 1) / kTileW;
  a.tiles_y = (o.rows + kTileH * kGroups - 1) / (kTileH * kGroups);
  a.rec     = static_cast<SlotRecord*>(o.workspace);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid prepare = on.grid(o.batch, kThreads);
  const Grid filter  = on.grid(images * a.tiles_x * a.tiles_y, kThreads);  // images * tiles_y <= images * rows < 2^31, tiles_x < 2^19
  PRS_TRY(on.check());
  on.launch(depth_consistency_prepare_kernel, prepare, 0, a);
  on.launch(p.depth_type == PRS_DEPTH_U16 ? depth_consistency_filter_kernel<uint16_t> : depth_consistency_filter_kernel<float>, filter, 0, a);
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_depth_consistency_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_depth_consistency_params);
  sizes2[1] = sizeof(prs_depth_consistency_batch);
}

uint64_t prs_depth_consistency_workspace_bytes(int32_t batch, int32_t frames, int32_t window) {
  return records_of(batch, frames, window) * sizeof(SlotRecord);
}

int prs_depth_consistency_batch_run(prs_context* ctx, const prs_depth_consistency_params* params, const prs_depth_consistency_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return depth_consistency_launch(ctx, params, batch);
}

}  // extern "C"
