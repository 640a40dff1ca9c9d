// depth_normals.hip -- surface normals of depth images on the device: one oriented (n0, n1, n2, w) a pixel in the camera frame and,
// optionally, one world-frame normal per row of the dense cloud made of the same images (prs_depth_normals_batch_run; the rule is
// stated in include/proslam_hip_normals.h, BUILD-DEFINED, and restated in tests/depth_normals_ref.py).
//   head     a thread an image: status[b] and n_bad_rows[b] = 0 by the thread of the sequence's first image, 0 into n_normal of a
//            served image (the tiles add to it)
//   tiles    one workgroup per 64 x 16 tile of one image (the speckle filter's tile).  The tile's depths in metres with a halo of
//            radius + smooth go into LDS once, NaN for an invalid pixel or one outside the image: a valid depth can be 0 (a product
//            that underflows with range_min 0), a NaN fails every comparison, so fabsf(d_q - d_c) <= gate is the whole usable test.
//            (u - cx) / fx and (v - cy) / fy are divided once per column and row of that region, not per point.  Without smoothing a
//            lane computes its pixel's normal from LDS and stores it.  With smoothing the raw normals of the tile and a halo of
//            `smooth` go into LDS as four planes of floats (consecutive lanes on consecutive banks), (0, 0, 0, 0) where there is none;
//            the window sum adds a zero for a pixel that is gated out or has no normal, which leaves every bit of the sum as skipping
//            the pixel would: a + (+0) = a for every a but -0, and a sum that starts at +0 never is -0 (x + y = -0 only for
//            x = y = -0).  One 16-byte store a pixel, consecutive lanes on consecutive pixels; n_normal by wave ballots and one
//            integer atomic add a workgroup
//   rows     one workgroup per 256 cloud rows of a sequence: the row's frame and pixel, the rotation of T = pose * sensor_in_robot,
//            one 16-byte load, one 16-byte store; n_bad_rows by wave ballots and one integer atomic add a workgroup
// The atomics are integer adds: the sums are the same whatever order they arrive in.
#include <float.h>
#include <math.h>
#include <stddef.h>

#include <string>

#include "../../include/proslam_hip_normals.h"
#include "prs_depth.h"
#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kTileW   = PRS_WAVE;  // a lane a column
constexpr int kTileH   = 16;
constexpr int kMaxRadius = 8, kMaxSmooth = 3;

struct DepthNormalsArgs {
  prs_depth_normals_params p;
  prs_depth_normals_batch o;
  int32_t tiles_x, tiles_y;
  int32_t images;      // batch * frames
  int32_t with_rows;
  int32_t row_blocks;  // ceil(row_stride / kThreads)
};

// floats of LDS a tile workgroup uses: the depth region with its column and row factors, and the four planes of raw normals
inline size_t tile_floats(const int radius, const int smooth) {
  const int h = radius + smooth;
  const size_t depth = (size_t) (kTileH + 2 * h) * (kTileW + 2 * h) + (kTileW + 2 * h) + (kTileH + 2 * h);
  return depth + (smooth > 0 ? 4 * (size_t) (kTileH + 2 * smooth) * (kTileW + 2 * smooth) : 0);
}

// the images of sequence b the call works on; -1: the sequence is refused (n_images[b], or with rows row_base[b] / row_n[b])
__device__ __forceinline__ int sequence_images(const DepthNormalsArgs& a, const int b) {
  int n = images_of(a.o, b);
  if (a.with_rows && n >= 0) {
    const int base = a.o.row_base ? a.o.row_base[b] : 0, rows = a.o.row_n[b];
    if (base < 0 || rows < 0 || base > a.o.row_stride || rows > a.o.row_stride || base > rows) {
      n = -1;
    }
  }
  return n;
}

// ---- head: a thread an image ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void depth_normals_head_kernel(const DepthNormalsArgs a) {
  const uint32_t image = blockIdx.x * (uint32_t) kThreads + threadIdx.x;  // images < 2^31
  if (image >= (uint32_t) a.images) {
    return;
  }
  const int f = frame_of(image, a.o.frames), b = sequence_of(image, a.o.frames);
  const int n_img = sequence_images(a, b);
  if (f == 0) {
    a.o.status[b] = n_img < 0 ? PRS_ERR_RANGE : PRS_OK;
    if (n_img >= 0 && a.with_rows) {
      a.o.n_bad_rows[b] = 0;
    }
  }
  if (f < n_img && a.o.n_normal) {
    a.o.n_normal[image] = 0;
  }
}

// len2 > 0 && len2 <= FLT_MAX: a length that can be divided by (false for NaN and +inf)
__device__ __forceinline__ bool length_ok(const float len2) {
  return len2 > 0.0f && len2 <= FLT_MAX;
}

// The raw normal (n0, n1, n2, w) of the pixel at (ly, lx) of the depth region s_d (dw floats a row), (0, 0, 0, 0) when it has none.
// s_kx, s_ky: ((float) u - cx) / fx and ((float) v - cy) / fy of the region's columns and rows.  (ly, lx) lies at least r inside
__device__ __forceinline__ float4 raw_normal(const float* s_d, const float* s_kx, const float* s_ky, const int dw, const int ly, const int lx,
                                             const int r, const float max_rel_diff) {
  const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float* at  = s_d + ly * dw + lx;
  const float dc   = at[0];
  const float gate = max_rel_diff * dc;  // NaN at an invalid centre: nothing is usable
  const float dl = at[-r], dr = at[r], du = at[-r * dw], dd = at[r * dw];
  const bool ul = fabsf(dl - dc) <= gate, ur = fabsf(dr - dc) <= gate, uu = fabsf(du - dc) <= gate, ud = fabsf(dd - dc) <= gate;
  if (!((ul || ur) && (uu || ud))) {
    return none;
  }
  const float kx = s_kx[lx], ky = s_ky[ly];
  const float p[3] = {kx * dc, ky * dc, dc};
  float tx[3], ty[3];
  {
    const float kr = s_kx[lx + r], kl = s_kx[lx - r];
    const float R[3] = {ur ? kr * dr : p[0], ur ? ky * dr : p[1], ur ? dr : p[2]};
    const float L[3] = {ul ? kl * dl : p[0], ul ? ky * dl : p[1], ul ? dl : p[2]};
    const float kd = s_ky[ly + r], ku = s_ky[ly - r];
    const float D[3] = {ud ? kx * dd : p[0], ud ? kd * dd : p[1], ud ? dd : p[2]};
    const float U[3] = {uu ? kx * du : p[0], uu ? ku * du : p[1], uu ? du : p[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      tx[i] = R[i] - L[i];
      ty[i] = D[i] - U[i];
    }
  }
  const float m0 = ty[1] * tx[2] - ty[2] * tx[1];
  const float m1 = ty[2] * tx[0] - ty[0] * tx[2];
  const float m2 = ty[0] * tx[1] - ty[1] * tx[0];
  const float len2 = (m0 * m0 + m1 * m1) + m2 * m2;
  if (!length_ok(len2)) {
    return none;
  }
  const float len = sqrtf(len2);
  float n0 = m0 / len, n1 = m1 / len, n2 = m2 / len;
  const float dot = (n0 * p[0] + n1 * p[1]) + n2 * p[2];
  if (dot > 0.0f) {
    n0 = -n0, n1 = -n1, n2 = -n2;
  }
  return make_float4(n0, n1, n2, (float) ((int) ul + (int) ur + (int) uu + (int) ud));
}

// ---- tiles: blockIdx.x = (image * tiles_y + ty) * tiles_x + tx.  E: the depth element; SMOOTH: smooth > 0 ----------------------------
template <typename E, bool SMOOTH>
__global__ __launch_bounds__(kThreads) void depth_normals_kernel(const DepthNormalsArgs a) {
  extern __shared__ float s_mem[];
  __shared__ int s_count[kWaves];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), w = tid >> 6;
  uint32_t id  = blockIdx.x;
  const int tx = (int) (id % (uint32_t) a.tiles_x);
  id /= (uint32_t) a.tiles_x;
  const int ty         = (int) (id % (uint32_t) a.tiles_y);
  const uint32_t image = id / (uint32_t) a.tiles_y;
  const int f = frame_of(image, a.o.frames), b = sequence_of(image, a.o.frames);
  if (f >= sequence_images(a, b)) {
    return;
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const int r = a.p.radius, s = SMOOTH ? a.p.smooth : 0, h = r + s;
  const int dw = kTileW + 2 * h, dh = kTileH + 2 * h;  // the depth region: the tile and a halo of h
  float* s_d  = s_mem;
  float* s_kx = s_d + dh * dw;
  float* s_ky = s_kx + dw;
  float* s_n  = s_ky + dh;                             // SMOOTH: four planes of nh * nw floats
  const int x0 = tx * kTileW - h, y0 = ty * kTileH - h;  // the region's first column and row in the image
  for (int i = tid; i < dw + dh; i += kThreads) {
    if (i < dw) {
      s_kx[i] = ((float) (x0 + i) - a.p.cx) / a.p.fx;
    } else {
      s_ky[i - dw] = ((float) (y0 + i - dw) - a.p.cy) / a.p.fy;
    }
  }
  const uint8_t* img = static_cast<const uint8_t*>(a.o.depth) + (size_t) image * (size_t) rows * (size_t) a.o.pitch;
  for (int i = tid; i < dh * dw; i += kThreads) {
    const int ly = (int) ((uint32_t) i / (uint32_t) dw), lx = i - ly * dw;
    const int y = y0 + ly, x = x0 + lx;
    float d = __builtin_nanf("");
    if (y >= 0 && y < rows && x >= 0 && x < cols) {
      const float raw = (float) reinterpret_cast<const E*>(img + (size_t) y * (size_t) a.o.pitch)[x];
      float metres;
      if (depth_valid(raw, a.p.depth_scaling_factor_to_meters, a.p.range_min, a.p.range_max, metres)) {
        d = metres;
      }
    }
    s_d[i] = d;
  }
  __syncthreads();
  const int nw = kTileW + 2 * s, nh = kTileH + 2 * s, plane = nw * nh;
  if (SMOOTH) {  // the raw normals of the tile and a halo of s; a pixel outside the image has a NaN depth and so none
    for (int i = tid; i < plane; i += kThreads) {
      const int ny = (int) ((uint32_t) i / (uint32_t) nw), nx = i - ny * nw;
      const float4 n = raw_normal(s_d, s_kx, s_ky, dw, ny + r, nx + r, r, a.p.max_rel_diff);
      s_n[i] = n.x, s_n[plane + i] = n.y, s_n[2 * plane + i] = n.z, s_n[3 * plane + i] = n.w;
    }
    __syncthreads();
  }
  const int x = tx * kTileW + lane;
  float4* out = reinterpret_cast<float4*>(a.o.normal);
  int have = 0;  // the wave's pixels with a normal
  for (int ly = w; ly < kTileH; ly += kWaves) {
    const int y = ty * kTileH + ly;
    const bool inside = y < rows && x < cols;
    float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside) {
      if (!SMOOTH) {
        n = raw_normal(s_d, s_kx, s_ky, dw, ly + r, lane + r, r, a.p.max_rel_diff);
      } else {
        const int c = (ly + s) * nw + lane + s;
        const float wc = s_n[3 * plane + c];
        if (wc > 0.0f) {
          const float* at  = s_d + (ly + h) * dw + lane + h;
          const float dc   = at[0];
          const float gate = a.p.max_rel_diff * dc;
          float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
          for (int dv = -s; dv <= s; ++dv) {
            for (int du = -s; du <= s; ++du) {
              const int q    = c + dv * nw + du;
              const bool use = fabsf(at[dv * dw + du] - dc) <= gate;
              a0 = a0 + (use ? s_n[q] : 0.0f);
              a1 = a1 + (use ? s_n[plane + q] : 0.0f);
              a2 = a2 + (use ? s_n[2 * plane + q] : 0.0f);
            }
          }
          const float len2 = (a0 * a0 + a1 * a1) + a2 * a2;
          if (length_ok(len2)) {
            const float len = sqrtf(len2);
            n = make_float4(a0 / len, a1 / len, a2 / len, wc);
          }
        }
      }
      out[((size_t) image * (size_t) rows + (size_t) y) * (size_t) cols + (size_t) x] = n;
    }
    have += (int) __popcll(__ballot(inside && n.w > 0.0f));
  }
  if (a.o.n_normal) {  // one integer atomic add a workgroup: the sum does not depend on the order
    if (lane == 0) {
      s_count[w] = have;
    }
    __syncthreads();
    if (tid == 0) {
      int sum = 0;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) {
        sum += s_count[i];
      }
      if (sum != 0) {
        atomicAdd(a.o.n_normal + image, sum);
      }
    }
  }
}

// ---- rows: blockIdx.x = b * row_blocks + block; a thread a cloud row ---------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void depth_normals_rows_kernel(const DepthNormalsArgs a) {
  __shared__ int s_bad[kWaves];
  const int tid   = threadIdx.x;
  const int block = (int) (blockIdx.x % (uint32_t) a.row_blocks), b = (int) (blockIdx.x / (uint32_t) a.row_blocks);
  const int n_img = sequence_images(a, b);
  if (n_img < 0) {
    return;
  }
  const int64_t base = a.o.row_base ? a.o.row_base[b] : 0, end = min(a.o.row_n[b], a.o.row_stride);
  const int64_t j = (int64_t) block * kThreads + tid;
  bool bad = false;
  if (j >= base && j < end) {
    const size_t at = (size_t) b * (size_t) a.o.row_stride + (size_t) j;
    const int f = a.o.row_frame[at], q = a.o.row_pixel[at];
    const int pixels = a.o.rows * a.o.cols;  // below 2^31
    int k = -1;
    if (f >= 0 && f < n_img && q >= 0 && q < pixels) {
      k = depth_pose_row(a.o.frame_index, a.o.pose, a.o.frames, a.o.pose_stride, b, f);
    }
    float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (k >= 0) {
      float T[12];
      se3_mul<false>(a.o.pose + ((size_t) b * (size_t) a.o.pose_stride + (size_t) k) * 16, a.p.sensor_in_robot, T);
      const size_t image = (size_t) b * (size_t) a.o.frames + (size_t) f;
      const float4 n = reinterpret_cast<const float4*>(a.o.normal)[image * (size_t) pixels + (size_t) q];
      row.x = (T[0] * n.x + T[1] * n.y) + T[2] * n.z;
      row.y = (T[4] * n.x + T[5] * n.y) + T[6] * n.z;
      row.z = (T[8] * n.x + T[9] * n.y) + T[10] * n.z;
      row.w = n.w;
    } else {
      bad = true;
    }
    reinterpret_cast<float4*>(a.o.row_normal)[at] = row;
  }
  const int n_bad = (int) __popcll(__ballot(bad));
  if ((tid & (PRS_WAVE - 1)) == 0) {
    s_bad[tid >> 6] = n_bad;
  }
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
      sum += s_bad[i];
    }
    if (sum != 0) {
      atomicAdd(a.o.n_bad_rows + b, sum);
    }
  }
}

template <typename E>
void launch_tiles(const Launches& on, const Grid& grid, const size_t lds, const DepthNormalsArgs& a) {
  if (a.p.smooth > 0) {
    on.launch(depth_normals_kernel<E, true>, grid, lds, a);
  } else {
    on.launch(depth_normals_kernel<E, false>, grid, lds, a);
  }
}

}  // namespace

int depth_normals_launch(prs_context* ctx, const prs_depth_normals_params* params, const prs_depth_normals_batch* batch) {
  const std::string who = "prs_depth_normals_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_depth_normals_params& p = *params;
  const prs_depth_normals_batch& o  = *batch;
  const int row_pointers = (o.row_frame != nullptr) + (o.row_pixel != nullptr) + (o.row_n != nullptr) + (o.row_normal != nullptr) +
                           (o.n_bad_rows != nullptr);
  const bool with_rows = row_pointers == 5;
  if (!o.depth || !o.normal || !o.status || (row_pointers != 0 && !with_rows) || (with_rows && !o.pose)) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": depth, normal or status not set, or row_frame, row_pixel, row_n, row_normal, n_bad_rows and pose set only in part").c_str());
  }
  const int64_t elem = depth_bytes(p.depth_type);
  if (elem == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": unknown depth_type").c_str());
  }
  bool finite = std::isfinite(p.depth_scaling_factor_to_meters) && std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) &&
                std::isfinite(p.cy) && std::isfinite(p.range_min) && std::isfinite(p.range_max) && std::isfinite(p.max_rel_diff);
  for (int i = 0; i < 16; ++i) {
    finite = finite && std::isfinite(p.sensor_in_robot[i]);
  }
  if (o.batch < 1 || o.frames < 1 || o.rows < 1 || o.cols < 1 || (with_rows && (o.pose_stride < 1 || o.row_stride < 1)) ||
      !pitch_ok(o.pitch, o.cols, elem) || p.radius < 1 || p.radius > kMaxRadius || p.smooth < 0 || p.smooth > kMaxSmooth || !finite ||
      !(p.depth_scaling_factor_to_meters > 0.0f) || p.range_min < 0.0f || p.range_min > p.range_max || p.max_rel_diff < 0.0f) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size below 1, a pitch below the row's bytes or not a multiple of the element, radius outside 1 .. 8, smooth outside 0 .. 3, a parameter not finite, a scale not positive, range_min negative or above range_max, or max_rel_diff negative").c_str());
  }
  if (!aligned_to(o.normal, 16) || !aligned_to(o.row_normal, 16) || !aligned_to(o.depth, (uintptr_t) elem) || !aligned_to(o.n_images, 4) ||
      !aligned_to(o.pose, 4) || !aligned_to(o.frame_index, 4) || !aligned_to(o.row_frame, 4) || !aligned_to(o.row_pixel, 4) ||
      !aligned_to(o.row_n, 4) || !aligned_to(o.row_base, 4) || !aligned_to(o.n_normal, 4) || !aligned_to(o.n_bad_rows, 4) ||
      !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": normal and row_normal must be 16-byte aligned, depth to its element, the other arrays 4-byte").c_str());
  }
  if (image_pixels(o.batch, o.frames, o.rows, o.cols) < 1) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": rows * cols or batch * frames * rows * cols beyond 2^31 - 1").c_str());
  }
  DepthNormalsArgs a = {};
  a.p = p;
  a.o = o;
  a.tiles_x    = (o.cols + kTileW - 1) / kTileW;
  a.tiles_y    = (o.rows + kTileH - 1) / kTileH;
  a.images     = (int32_t) ((int64_t) o.batch * o.frames);
  a.with_rows  = with_rows;
  a.row_blocks = with_rows ? (int32_t) (((int64_t) o.row_stride + kThreads - 1) / kThreads) : 0;
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid head  = on.grid(((int64_t) a.images + kThreads - 1) / kThreads, kThreads);
  const Grid tiles = on.grid((int64_t) a.images * a.tiles_x * a.tiles_y, kThreads);
  const Grid rows  = with_rows ? on.grid((int64_t) o.batch * a.row_blocks, kThreads) : Grid();
  PRS_TRY(on.check());
  const size_t lds = tile_floats(p.radius, p.smooth) * sizeof(float);  // at most 38208 bytes: no request is needed
  on.launch(depth_normals_head_kernel, head, 0, a);
  if (p.depth_type == PRS_DEPTH_U16) {
    launch_tiles<uint16_t>(on, tiles, lds, a);
  } else {
    launch_tiles<float>(on, tiles, lds, a);
  }
  if (with_rows) {
    on.launch(depth_normals_rows_kernel, rows, 0, a);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_depth_normals_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_depth_normals_params);
  sizes2[1] = sizeof(prs_depth_normals_batch);
}

int prs_depth_normals_batch_run(prs_context* ctx, const prs_depth_normals_params* params, const prs_depth_normals_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return depth_normals_launch(ctx, params, batch);
}

}  // extern "C"
