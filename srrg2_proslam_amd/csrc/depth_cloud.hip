// depth_cloud.hip -- the dense RGB-D cloud on the device: every sampled depth pixel of a sequence's frames, placed in the world by the
// trajectory (prs_depth_cloud_batch_run; the rule is stated in include/proslam_hip.h, BUILD-DEFINED, and restated in
// tests/depth_cloud_ref.py).  The stable stream compaction of world_map.hip over the pixels, in chunks that never span two images:
//   count    one workgroup per chunk of 1024 sampled pixels, four consecutive samples a lane: the depth test, four wave ballots, the
//            chunk's count.  A frame behind n_images, or without a usable pose, counts 0 and reads no pixel
//   scan     one workgroup per sequence: validation, the skipped frames, n_base, truncation, the chunk bases (an exclusive scan).  A
//            chunk that keeps nothing, starts behind out_stride or belongs to a refused sequence gets the base -1
//   scatter  one workgroup per chunk with a base: T = pose * sensor_in_robot once, by twelve lanes through LDS; the same ballots give
//            every kept pixel its place in the chunk; the rows are staged in LDS in that order and written from the scanned base on,
//            one 16-byte store a row, 4 KB in one piece per store instruction of the workgroup (a lane that stores its own four
//            rows writes 16 bytes every 64: measured 1.87 against 1.48 ms at 1024 frames, profiles/depth_cloud/README.md)
// No atomic anywhere: a row's position depends on the pixels before it alone.
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <string>

#include "prs_compact.h"
#include "prs_depth.h"
#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;                    // consecutive samples of a lane
constexpr int kChunk   = kThreads * kPerLane;  // sampled pixels per workgroup
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kWideThreads = 1024;  // the scan at one long sequence

struct DepthCloudArgs {
  prs_depth_cloud_params p;
  prs_depth_cloud_batch o;
  int32_t srows, scols;      // sampled rows and columns of an image
  int32_t samples;           // srows * scols
  int32_t chunks_per_frame;  // ceil(samples / kChunk)
  int32_t chunks;            // frames * chunks_per_frame: the chunks of a sequence
  int32_t write_out;
  int32_t* ws_count;  // [batch][chunks] kept pixels of the chunk; after the scan: the chunk's first output row, -1 = keep out
};

// the pose row of image f of sequence b when the frame gives rows, -1 when it is skipped.  Uniform over the workgroup
__device__ __forceinline__ int pose_row_of(const DepthCloudArgs& a, const int b, const int f) {
  return depth_pose_row(a.o.frame_index, a.o.pose, a.o.frames, a.o.pose_stride, b, f);
}

// blockIdx.x = (b * frames + f) * chunks_per_frame + c.  E: the depth element; VEC: a lane's four samples are one aligned load (step 1,
// cols a multiple of 4, rows and the base aligned to the load); SCATTER: write the rows (else: count them)
template <typename E, bool VEC, bool SCATTER>
__global__ __launch_bounds__(kThreads) void depth_cloud_kernel(const DepthCloudArgs a) {
  __shared__ int s_wave[kWaves];
  __shared__ float s_T[12];
  __shared__ float4 s_row[SCATTER ? kChunk : 1];  // the chunk's rows in their order
  __shared__ int32_t s_pix[SCATTER ? kChunk : 1];
  const int tid     = threadIdx.x;
  const uint32_t id = blockIdx.x;
  const uint32_t cf = (uint32_t) a.chunks_per_frame;
  const uint32_t image = id / cf;  // b * frames + f
  const int c = (int) (id % cf);
  const int f = frame_of(image, a.o.frames), b = sequence_of(image, a.o.frames);
  int base = 0;
  if (SCATTER) {
    base = __builtin_amdgcn_readfirstlane(a.ws_count[id]);
    if (base < 0) {
      return;  // nothing kept, behind out_stride, a skipped frame or a refused sequence: no pixel is read
    }
    if (tid < 12) {  // a chunk with rows has a usable pose
      const int k    = a.o.frame_index ? a.o.frame_index[image] : f;
      const float* A = a.o.pose + ((size_t) b * a.o.pose_stride + k) * 16 + 4 * (tid >> 2);
      const float* B = a.p.sensor_in_robot + (tid & 3);
      float t        = (A[0] * B[0] + A[1] * B[4]) + A[2] * B[8];
      if ((tid & 3) == 3) {
        t = t + A[3];
      }
      s_T[tid] = t;
    }
  } else {
    const int n_img = a.o.n_images[b];
    if (n_img < 0 || n_img > a.o.frames || f >= n_img || pose_row_of(a, b, f) < 0) {
      if (tid == 0) {
        a.ws_count[id] = 0;
      }
      return;
    }
  }
  // the lane's samples s0 .. s0 + 3 of the image, sample s = (s / scols, s % scols) of the sampled grid
  const int s0 = c * kChunk + tid * kPerLane;
  const uint8_t* img = static_cast<const uint8_t*>(a.o.depth) + (size_t) image * (size_t) a.o.rows * (size_t) a.o.pitch;
  float raw[kPerLane] = {};
  int u[kPerLane] = {}, v[kPerLane] = {};
  if (s0 < a.samples) {
    int sr = s0 / a.scols, sc = s0 - sr * a.scols;
    if (VEC) {
      const E* at = reinterpret_cast<const E*>(img + (size_t) sr * (size_t) a.o.pitch) + sc;
      E e[kPerLane];
      if (sizeof(E) == 2) {
        *reinterpret_cast<uint2*>(e) = *reinterpret_cast<const uint2*>(at);
      } else {
        *reinterpret_cast<uint4*>(e) = *reinterpret_cast<const uint4*>(at);
      }
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        raw[j] = (float) e[j];
        u[j] = sc + j, v[j] = sr;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        if (s0 + j < a.samples) {
          u[j] = sc * a.p.step, v[j] = sr * a.p.step;
          raw[j] = (float) reinterpret_cast<const E*>(img + (size_t) v[j] * (size_t) a.o.pitch)[u[j]];
        }
        if (++sc == a.scols) {
          sc = 0, ++sr;
        }
      }
    }
  }
  bool keep[kPerLane];
  float d[kPerLane];
  uint64_t mask[kPerLane];
  int kept = 0, below = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    keep[j] = depth_valid(raw[j], a.p.depth_scaling_factor_to_meters, a.p.range_min, a.p.range_max, d[j]);  // a sample behind the image has raw 0
    mask[j] = __ballot(keep[j]);
    kept += __popcll(mask[j]);
    below = lanes_below(mask[j], below);
  }
  if ((tid & (PRS_WAVE - 1)) == 0) {
    s_wave[tid >> 6] = kept;
  }
  __syncthreads();
  if (!SCATTER) {
    if (tid == 0) {
      int k = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        k += s_wave[w];
      }
      a.ws_count[id] = k;
    }
    return;
  }
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    T[i] = s_T[i];
  }
  const size_t out0 = (size_t) b * (size_t) a.o.out_stride;
  const uint8_t* gray = a.o.gray ? a.o.gray + (size_t) image * (size_t) a.o.rows * (size_t) a.o.gray_pitch : nullptr;
  // the lane's first row among the chunk's: the kept samples of the waves before this one and of the lanes below this one
  int at = below, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    at += w < (tid >> 6) ? s_wave[w] : 0;
    total += s_wave[w];
  }
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    if (keep[j]) {
      float p[3], w[3];
      depth_point(u[j], v[j], d[j], a.p.fx, a.p.fy, a.p.cx, a.p.cy, p);
      se3_apply(T, p, w);
      float intensity = 0.0f;
      if (gray) {
        intensity = (float) gray[(size_t) v[j] * (size_t) a.o.gray_pitch + u[j]] * (1.0f / 255.0f);
      }
      s_row[at] = make_float4(w[0], w[1], w[2], intensity);
      s_pix[at] = v[j] * a.o.cols + u[j];
      ++at;
    }
  }
  __syncthreads();
  const int n = min(total, a.o.out_stride - base);  // the scan gives a chunk behind out_stride no base
  for (int i = tid; i < n; i += kThreads) {
    const size_t to = out0 + (size_t) base + (size_t) i;
    reinterpret_cast<float4*>(a.o.xyz)[to] = s_row[i];
    if (a.o.frame) {
      a.o.frame[to] = f;
    }
    if (a.o.pixel) {
      a.o.pixel[to] = s_pix[i];
    }
  }
}

// ---- scan: one workgroup per sequence, of 64 .. kWideThreads threads as the chunks ask ---------------------------------------------
__global__ __launch_bounds__(kWideThreads) void depth_cloud_scan_kernel(const DepthCloudArgs a) {
  __shared__ uint64_t s_scan[17];
  const int tid = threadIdx.x, threads = blockDim.x, b = blockIdx.x;
  const int C   = a.chunks;
  int32_t* cnt  = a.ws_count + (size_t) b * C;
  const int n_img  = a.o.n_images[b];
  const int n_base = a.o.n_base ? a.o.n_base[b] : 0;
  const int cap    = a.o.out_stride > 0 ? a.o.out_stride : 0;
  __syncthreads();  // n_base may be n_out: every lane has read it before lane 0 writes it
  if (n_img < 0 || n_img > a.o.frames || n_base < 0 || n_base > cap) {
    for (int c = tid; c < C; c += threads) {
      cnt[c] = -1;
    }
    if (tid == 0) {
      a.o.status[b]    = PRS_ERR_RANGE;
      a.o.n_out[b]     = n_base < 0 ? 0 : (n_base > cap ? cap : n_base);
      a.o.n_total[b]   = 0;
      a.o.n_skipped[b] = 0;
    }
    return;
  }
  uint64_t skipped = 0, frames_skipped = 0;
  for (int f = tid; f < n_img; f += threads) {
    skipped += pose_row_of(a, b, f) < 0 ? 1u : 0u;
  }
  (void) block_exclusive_scan_u64(skipped, s_scan, frames_skipped);
  // every thread kCompactBatch consecutive chunks of a tile, their sum scanned over the tile and carried from tile to tile
  uint64_t carry = (uint64_t) n_base;
  for (int t0 = 0; t0 < C; t0 += threads * kCompactBatch) {
    const int c0 = t0 + tid * kCompactBatch;
    int32_t k[kCompactBatch] = {};
    uint64_t sum = 0;
    if (c0 < C) {
      load_counts(cnt, c0, C, k);
#pragma unroll
      for (int j = 0; j < kCompactBatch; ++j) {
        sum += (uint64_t) k[j];
      }
    }
    uint64_t tile = 0;
    uint64_t at   = carry + block_exclusive_scan_u64(sum, s_scan, tile);
#pragma unroll
    for (int j = 0; j < kCompactBatch; ++j) {
      if (c0 + j < C) {
        cnt[c0 + j] = (k[j] == 0 || at >= (uint64_t) cap) ? -1 : (int32_t) at;
      }
      at += (uint64_t) k[j];
    }
    carry += tile;
  }
  if (tid == 0) {
    const int32_t total = carry > 0x7fffffffull ? 0x7fffffff : (int32_t) carry;
    a.o.n_total[b]      = total;
    a.o.n_skipped[b]    = (int32_t) frames_skipped;
    a.o.n_out[b]        = a.write_out ? (total < cap ? total : cap) : n_base;
    a.o.status[b]       = (a.write_out && total > cap) ? PRS_ERR_CAPACITY : PRS_OK;
  }
}

// the sampled grid of an image and its chunks; samples 0 when a size is not one the launcher takes
struct Layout {
  int64_t srows, scols, samples, chunks_per_frame;
  uint64_t counts;  // bytes
};

Layout layout_of(const int64_t batch, const int64_t frames, const int64_t rows, const int64_t cols, const int64_t step) {
  Layout l = {};
  if (batch < 1 || frames < 1 || rows < 1 || cols < 1 || step < 1) {
    return l;
  }
  l.srows = (rows + step - 1) / step;
  l.scols = (cols + step - 1) / step;
  if (l.srows * l.scols > 0x7fffffffll || frames * l.srows * l.scols > 0x7fffffffll) {  // the first product is below 2^62
    return l;
  }
  l.samples          = l.srows * l.scols;
  l.chunks_per_frame = (l.samples + kChunk - 1) / kChunk;
  l.counts           = (uint64_t) batch * (uint64_t) frames * (uint64_t) l.chunks_per_frame * 4;
  return l;
}

template <typename E>
void launch_pass(const Launches& on, const Grid& grid, const DepthCloudArgs& a, const bool vec, const bool scatter) {
  if (vec) {
    if (scatter) {
      on.launch(depth_cloud_kernel<E, true, true>, grid, 0, a);
    } else {
      on.launch(depth_cloud_kernel<E, true, false>, grid, 0, a);
    }
  } else {
    if (scatter) {
      on.launch(depth_cloud_kernel<E, false, true>, grid, 0, a);
    } else {
      on.launch(depth_cloud_kernel<E, false, false>, grid, 0, a);
    }
  }
}

}  // namespace

int depth_cloud_launch(prs_context* ctx, const prs_depth_cloud_params* params, const prs_depth_cloud_batch* batch) {
  const std::string who = "prs_depth_cloud_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_depth_cloud_params& p = *params;
  const prs_depth_cloud_batch& o  = *batch;
  if (!o.depth || !o.n_images || !o.pose || !o.n_out || !o.n_total || !o.n_skipped || !o.status || !o.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": depth, n_images, pose, a per-sequence output or the workspace not set").c_str());
  }
  const int64_t elem = depth_bytes(p.depth_type);
  if (elem == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": unknown depth_type").c_str());
  }
  bool finite        = std::isfinite(p.depth_scaling_factor_to_meters) && std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) &&
                std::isfinite(p.cy) && std::isfinite(p.range_min) && std::isfinite(p.range_max);
  for (int i = 0; i < 16; ++i) {
    finite = finite && std::isfinite(p.sensor_in_robot[i]);
  }
  if (o.batch < 1 || o.frames < 1 || o.rows < 1 || o.cols < 1 || o.pose_stride < 1 || p.step < 1 || !pitch_ok(o.pitch, o.cols, elem) ||
      (o.gray && o.gray_pitch < o.cols) || !finite || !(p.depth_scaling_factor_to_meters > 0.0f) ||
      p.range_min < 0.0f || p.range_min > p.range_max || (o.xyz && o.out_stride < 1)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size or step below 1, a pitch below the row's bytes or not a multiple of the element, a parameter not finite, a scale not positive, range_min negative or above range_max, or out_stride below 1 with xyz set").c_str());
  }
  if (!aligned_to(o.xyz, 16) || !aligned_to(o.workspace, 16) || !aligned_to(o.depth, (uintptr_t) elem) || !aligned_to(o.n_images, 4) ||
      !aligned_to(o.pose, 4) || !aligned_to(o.frame_index, 4) || !aligned_to(o.n_base, 4) || !aligned_to(o.frame, 4) || !aligned_to(o.pixel, 4) ||
      !aligned_to(o.n_out, 4) || !aligned_to(o.n_total, 4) || !aligned_to(o.n_skipped, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": xyz and the workspace must be 16-byte aligned, depth to its element, the other arrays but gray 4-byte").c_str());
  }
  const Layout l = layout_of(o.batch, o.frames, o.rows, o.cols, p.step);
  if (l.samples < 1 || (int64_t) o.rows * (int64_t) o.cols > 0x7fffffffll) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": rows * cols or frames * sampled pixels beyond 2^31 - 1").c_str());
  }
  const int64_t C = (int64_t) o.frames * l.chunks_per_frame, blocks = (int64_t) o.batch * C;  // C <= frames * samples < 2^31
  const int wide = (int) std::min<long long>(kWideThreads, ((C + kCompactBatch - 1) / kCompactBatch + PRS_WAVE - 1) / PRS_WAVE * PRS_WAVE);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid pass = on.grid(blocks, kThreads), scan = on.grid(o.batch, wide);  // the two passes: batch * frames * chunks of 1024 sampled pixels
  PRS_TRY(on.check());
  DepthCloudArgs a = {};
  a.p = p;
  a.o = o;
  a.srows = (int32_t) l.srows, a.scols = (int32_t) l.scols, a.samples = (int32_t) l.samples;
  a.chunks_per_frame = (int32_t) l.chunks_per_frame, a.chunks = (int32_t) C;
  a.write_out = o.xyz != nullptr;
  a.ws_count  = static_cast<int32_t*>(o.workspace);
  // a lane's four samples in one load: they lie in one row (cols a multiple of 4) at an address that is a multiple of the load
  const uintptr_t load = (uintptr_t) elem * kPerLane;
  const bool vec       = p.step == 1 && o.cols % kPerLane == 0 && (uintptr_t) o.pitch % load == 0 && aligned_to(o.depth, load);
  const bool u16       = p.depth_type == PRS_DEPTH_U16;
  if (u16) {
    launch_pass<uint16_t>(on, pass, a, vec, false);
  } else {
    launch_pass<float>(on, pass, a, vec, false);
  }
  on.launch(depth_cloud_scan_kernel, scan, 0, a);
  if (a.write_out) {
    if (u16) {
      launch_pass<uint16_t>(on, pass, a, vec, true);
    } else {
      launch_pass<float>(on, pass, a, vec, true);
    }
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_depth_cloud_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_depth_cloud_params);
  sizes2[1] = sizeof(prs_depth_cloud_batch);
}

uint64_t prs_depth_cloud_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols, int32_t step) {
  return (layout_of(batch, frames, rows, cols, step).counts + 15) & ~(uint64_t) 15;
}

int prs_depth_cloud_batch_run(prs_context* ctx, const prs_depth_cloud_params* params, const prs_depth_cloud_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return depth_cloud_launch(ctx, params, batch);
}

}  // extern "C"
