// tsdf_raycast.hip -- a TSDF volume rendered into depth and normal images on the device (prs_tsdf_raycast_batch_run; the rule is
// stated in include/proslam_hip_tsdf_raycast.h, BUILD-DEFINED, and restated in tests/tsdf_raycast_ref.py).
//   head   one workgroup per sequence, a thread a view: status[b], n_skipped[b] (ballot counts through LDS), 0 into n_hit, and per
//          view T = pose * sensor_in_robot with a flag (kSkipped, kServed, kUntouched) into the workspace (16 floats a view)
//   rays   one workgroup per tile of 16 x 16 pixels of one view, a wave per 8 x 8 pixels of it: the 64 rays of a wave leave the camera
//          in a narrow bundle, so the eight voxels a lane gathers a sample lie next to its neighbours' and share their cache lines.
//          T and the flag are wave-uniform reads of the workspace.  A lane marches its own ray; the wave leaves the loop when a
//          ballot shows no live lane.  A voxel is one 8-byte load, the two corners along x follow one another in memory.  The hit
//          count is a ballot count a wave, summed through LDS, and one global integer atomic add a workgroup.
// A gather-bound kernel: no LDS staging of the volume (a tile's rays cross bricks no workgroup could name in advance), no empty-space
// skipping.  The only atomic is an integer add: the sums are the same whatever order they arrive in.
#include <float.h>
#include <math.h>
#include <stddef.h>

#include <string>

#include "../../include/proslam_hip_tsdf_raycast.h"
#include "prs_compact.h"
#include "prs_depth.h"
#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kTile    = 16;                      // pixels of a workgroup's tile along u and along v
constexpr int kSub     = 8;                       // pixels of a wave's part of it along u and along v
constexpr int kWsFloats = 16;                     // floats of workspace a view: T[12], the flag (an int), three unused
constexpr int kSkipped = 0, kServed = 1, kUntouched = 2;
constexpr float kMaxSteps = 1048576.0f;           // steps the diagonal of a volume may hold, and a ray's trip count less two
constexpr int64_t kMaxVoxels = 0x7fffffffll / 3;  // the limit of the other TSDF calls

struct RaycastArgs {
  prs_tsdf_raycast_params p;
  prs_tsdf_raycast_batch o;
  int32_t tiles_x;  // tiles of a view along u
  float* ws;        // [batch][views][kWsFloats]
};

// the views of sequence b the call works on; -1: n_views[b] is outside [0, views]
__device__ __forceinline__ int views_of(const prs_tsdf_raycast_batch& o, const int b) {
  const int n = o.n_views ? o.n_views[b] : o.views;
  return (n < 0 || n > o.views) ? -1 : n;
}

// ---- head: blockIdx.x = b; thread t on views t, t + kThreads, ... -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_raycast_head_kernel(const RaycastArgs a) {
  __shared__ int s_skipped[kWaves];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int views = a.o.views;
  const int n_v   = views_of(a.o, b);
  int skipped = 0;
  for (int r0 = 0; r0 < views; r0 += kThreads) {  // uniform trip count: the ballot below is the whole wave's
    const int r = r0 + tid;
    bool skip = false;
    if (r < views) {
      const size_t view = (size_t) b * (size_t) views + (size_t) r;
      float* ws = a.ws + view * kWsFloats;
      int flag  = kUntouched;
      float T[12] = {};
      if (r < n_v) {
        const int k = depth_pose_row(a.o.view_index, a.o.pose, views, a.o.pose_stride, b, r);
        if (k >= 0) {
          se3_mul<false>(a.o.pose + ((size_t) b * (size_t) a.o.pose_stride + (size_t) k) * 16, a.p.sensor_in_robot, T);
          flag = kServed;
        } else {
          flag = kSkipped;
          skip = true;
        }
        if (a.o.n_hit) {
          a.o.n_hit[view] = 0;
        }
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        ws[i] = T[i];
      }
      ws[12] = __int_as_float(flag);
    }
    skipped += (int) __popcll(__ballot(skip));
  }
  if ((tid & (PRS_WAVE - 1)) == 0) {
    s_skipped[tid >> 6] = skipped;
  }
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      sum += s_skipped[w];
    }
    a.o.status[b]    = n_v < 0 ? PRS_ERR_RANGE : PRS_OK;
    a.o.n_skipped[b] = n_v < 0 ? 0 : sum;
  }
}

// a sequence's volume as the sample rule sees it
struct Volume {
  const float2* at;     // voxel (0, 0, 0)
  int nx, ny, nz;
  float mx, my, mz;     // (float) (n_a - 2): the last cell along the axis
  float min_weight;
};

// two voxels that follow one another along x, (tsdf, w) of x0 and (tsdf, w) of x1, as one vector load of 16 bytes at the alignment of a
// voxel (a struct of four floats is taken apart into four loads)
typedef float float4_a8 __attribute__((ext_vector_type(4), aligned(8)));
struct VoxelPair {
  float t0, w0, t1, w1;
};
__device__ __forceinline__ VoxelPair load_pair(const float2* at) {
  const float4_a8 v = *reinterpret_cast<const float4_a8*>(at);
  return {v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ float lerp(const float p, const float q, const float f) {
  return p + f * (q - p);
}

// the sample rule at the grid coordinate (g0, g1, g2): whether the sample is valid, and then its value
__device__ __forceinline__ bool tsdf_sample(const Volume& V, const float g0, const float g1, const float g2, float& value) {
  const float i0 = floorf(g0), i1 = floorf(g1), i2 = floorf(g2);
  const bool inside = finite_bits(g0) && finite_bits(g1) && finite_bits(g2) && i0 >= 0.0f && i0 <= V.mx && i1 >= 0.0f && i1 <= V.my &&
                      i2 >= 0.0f && i2 <= V.mz;
  if (!inside) {
    return false;
  }
  const int j0 = (int) i0, j1 = (int) i1, j2 = (int) i2;  // below 2^31: i_a <= (float) (n_a - 2)
  if (j0 > V.nx - 2 || j1 > V.ny - 2 || j2 > V.nz - 2) {
    return false;  // only where (float) (n_a - 2) rounds up, beyond 2^24 voxels along an axis
  }
  const size_t nx = (size_t) V.nx, row = nx, layer = nx * (size_t) V.ny;
  const float2* c = V.at + (((size_t) j2 * (size_t) V.ny + (size_t) j1) * nx + (size_t) j0);
  // the corners x0 and x1 of a pair (dy, dz) are 16 contiguous bytes, 8-byte aligned: one load each; the weights are tested without
  // short-circuit, so the four loads are issued together
  const VoxelPair p00 = load_pair(c), p10 = load_pair(c + row), p01 = load_pair(c + layer), p11 = load_pair(c + layer + row);
  const float mw = V.min_weight;
  const bool observed = (p00.w0 >= mw) & (p00.w1 >= mw) & (p10.w0 >= mw) & (p10.w1 >= mw) & (p01.w0 >= mw) & (p01.w1 >= mw) & (p11.w0 >= mw) &
                        (p11.w1 >= mw);
  if (!observed) {
    return false;
  }
  const float f0 = g0 - i0, f1 = g1 - i1, f2 = g2 - i2;
  const float c00 = lerp(p00.t0, p00.t1, f0), c10 = lerp(p10.t0, p10.t1, f0);
  const float c01 = lerp(p01.t0, p01.t1, f0), c11 = lerp(p11.t0, p11.t1, f0);
  const float c0 = lerp(c00, c10, f1), c1 = lerp(c01, c11, f1);
  value = lerp(c0, c1, f2);
  return true;
}

// ---- rays: blockIdx.x = the tile (ty * tiles_x + tx), blockIdx.y = b * views + r ---------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_raycast_rays_kernel(const RaycastArgs a) {
  __shared__ int s_hit[kWaves];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), wave = tid >> 6;
  const size_t view = blockIdx.y;
  const float* ws = a.ws + view * kWsFloats;
  const int flag  = __float_as_int(ws[12]);
  if (flag == kUntouched) {
    return;  // a view from n_views on, or a refused sequence (uniform over the workgroup)
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const int tx = (int) (blockIdx.x % (uint32_t) a.tiles_x), ty = (int) (blockIdx.x / (uint32_t) a.tiles_x);
  const int u = tx * kTile + (wave & 1) * kSub + (lane & (kSub - 1));
  const int v = ty * kTile + (wave >> 1) * kSub + (lane >> 3);
  const bool inside = u < cols && v < rows;
  const size_t line = view * (size_t) rows + (size_t) v;
  float* depth_at  = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(a.o.depth) + line * (size_t) a.o.pitch) + u;
  float4* normal_at = reinterpret_cast<float4*>(a.o.normal) + (line * (size_t) cols + (size_t) u);
  if (flag == kSkipped) {
    if (inside) {
      *depth_at = 0.0f;
      if (a.o.normal) {
        *normal_at = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
    return;
  }
  const int b = (int) (view / (size_t) a.o.views);
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    T[i] = ws[i];
  }
  const float vs = a.p.voxel_size, step = a.p.step;
  const float* org = a.o.origin + (size_t) b * 4;
  const float o[3] = {org[0], org[1], org[2]};
  const int n[3]   = {a.o.nx, a.o.ny, a.o.nz};
  Volume V;
  V.at = reinterpret_cast<const float2*>(a.o.volume) + (size_t) b * ((size_t) n[0] * (size_t) n[1] * (size_t) n[2]);
  V.nx = n[0], V.ny = n[1], V.nz = n[2];
  V.mx = (float) (n[0] - 2), V.my = (float) (n[1] - 2), V.mz = (float) (n[2] - 2);
  V.min_weight = a.p.min_weight;

  // the ray and its stretch inside the box of the voxel centres
  const float dc0 = ((float) u - a.p.cx) / a.p.fx, dc1 = ((float) v - a.p.cy) / a.p.fy;
  float c[3], dw[3];
  float l_in = a.p.range_min, l_out = a.p.range_max;
  bool miss = false;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    c[e]  = T[4 * e + 3];
    dw[e] = (T[4 * e + 0] * dc0 + T[4 * e + 1] * dc1) + T[4 * e + 2] * 1.0f;
    const float lo = o[e] + 0.5f * vs, hi = o[e] + ((float) n[e] - 0.5f) * vs;
    if (dw[e] == 0.0f) {
      miss = miss || c[e] < lo || c[e] > hi;
    } else {
      const float t1 = (lo - c[e]) / dw[e], t2 = (hi - c[e]) / dw[e];
      const float t_near = t2 < t1 ? t2 : t1, t_far = t2 < t1 ? t1 : t2;
      l_in  = t_near > l_in ? t_near : l_in;
      l_out = t_far < l_out ? t_far : l_out;
    }
  }
  int trips = 0;
  if (inside && !miss && l_in <= l_out) {
    const float q = (l_out - l_in) / step;
    if (q >= 0.0f) {  // false for a NaN
      trips = (int) (q < kMaxSteps ? q : kMaxSteps) + 2;
    }
  }

  // the march: a lane is live until its ray ends, the wave goes on while one lane is
  bool hit = false, prev_valid = false;
  float prev_t = 0.0f, prev_l = 0.0f, l_star = 0.0f;
  bool live = trips > 0;
  for (int k = 0; __ballot(live) != 0ull; ++k) {
    if (live) {
      const float l = l_in + (float) k * step;
      if (!(l <= l_out)) {
        live = false;
      } else {
        float t = 0.0f;
        const bool valid = tsdf_sample(V, ((c[0] + l * dw[0]) - o[0]) / vs - 0.5f, ((c[1] + l * dw[1]) - o[1]) / vs - 0.5f,
                                       ((c[2] + l * dw[2]) - o[2]) / vs - 0.5f, t);
        if (valid && t <= 0.0f) {
          if (prev_valid && prev_t > 0.0f) {  // prev_valid is false at k = 0
            hit    = true;
            l_star = prev_l + step * (prev_t / (prev_t - t));
          }
          live = false;
        } else {
          prev_valid = valid, prev_t = t, prev_l = l;
          live = k + 1 < trips;
        }
      }
    }
  }
  const float d = (hit && l_star >= a.p.range_min && l_star <= a.p.range_max) ? l_star : 0.0f;
  const bool counted = inside && d > 0.0f;
  if (inside) {
    *depth_at = d;
    if (a.o.normal) {
      float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (counted) {
        const float g[3] = {((c[0] + d * dw[0]) - o[0]) / vs - 0.5f, ((c[1] + d * dw[1]) - o[1]) / vs - 0.5f,
                            ((c[2] + d * dw[2]) - o[2]) / vs - 0.5f};
        float m[3];
        bool all = true;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          float hi = 0.0f, lo = 0.0f;
          const bool ok_hi = tsdf_sample(V, e == 0 ? g[0] + 1.0f : g[0], e == 1 ? g[1] + 1.0f : g[1], e == 2 ? g[2] + 1.0f : g[2], hi);
          const bool ok_lo = tsdf_sample(V, e == 0 ? g[0] - 1.0f : g[0], e == 1 ? g[1] - 1.0f : g[1], e == 2 ? g[2] - 1.0f : g[2], lo);
          all  = all && ok_hi && ok_lo;
          m[e] = hi - lo;
        }
        const float len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
        if (all && len2 > 0.0f && len2 <= FLT_MAX) {
          const float len = sqrtf(len2);
          const float q0 = m[0] / len, q1 = m[1] / len, q2 = m[2] / len;
          row = make_float4((T[0] * q0 + T[4] * q1) + T[8] * q2, (T[1] * q0 + T[5] * q1) + T[9] * q2, (T[2] * q0 + T[6] * q1) + T[10] * q2,
                            1.0f);
        }
      }
      *normal_at = row;
    }
  }
  if (a.o.n_hit) {  // uniform
    const int in_wave = (int) __popcll(__ballot(counted));
    if (lane == 0) {
      s_hit[wave] = in_wave;
    }
    __syncthreads();
    if (tid == 0) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        sum += s_hit[w];
      }
      if (sum != 0) {
        atomicAdd(a.o.n_hit + view, sum);
      }
    }
  }
}

}  // namespace

int tsdf_raycast_launch(prs_context* ctx, const prs_tsdf_raycast_params* params, const prs_tsdf_raycast_batch* batch) {
  const std::string who = "prs_tsdf_raycast_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_tsdf_raycast_params& p = *params;
  const prs_tsdf_raycast_batch& o  = *batch;
  if (!o.origin || !o.volume || !o.pose || !o.depth || !o.n_skipped || !o.status || !o.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": origin, volume, pose, depth, n_skipped, status or the workspace not set").c_str());
  }
  bool finite = std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) && std::isfinite(p.cy) && std::isfinite(p.range_min) &&
                std::isfinite(p.range_max) && std::isfinite(p.voxel_size) && std::isfinite(p.min_weight) && std::isfinite(p.step);
  for (int i = 0; i < 16; ++i) {
    finite = finite && std::isfinite(p.sensor_in_robot[i]);
  }
  if (o.batch < 1 || o.views < 1 || o.rows < 1 || o.cols < 1 || o.pose_stride < 1 || o.nx < 1 || o.ny < 1 || o.nz < 1 ||
      !pitch_ok(o.pitch, o.cols, 4) || !finite || p.range_min < 0.0f || p.range_min > p.range_max || !(p.voxel_size > 0.0f) || !(p.step > 0.0f)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size below 1, a pitch below 4 * cols or not a multiple of 4, a parameter not finite, range_min negative or above range_max, or voxel_size or step not positive").c_str());
  }
  const float steps = (((float) o.nx + (float) o.ny) + (float) o.nz) * p.voxel_size / p.step;
  if (!(steps <= kMaxSteps)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": the volume's diagonal holds more than 1048576 steps").c_str());
  }
  if (!aligned_to(o.volume, 16) || !aligned_to(o.normal, 16) || !aligned_to(o.workspace, 16) || !aligned_to(o.depth, 4) || !aligned_to(o.origin, 4) ||
      !aligned_to(o.pose, 4) || !aligned_to(o.view_index, 4) || !aligned_to(o.n_views, 4) || !aligned_to(o.n_hit, 4) || !aligned_to(o.n_skipped, 4) ||
      !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": volume, normal and the workspace must be 16-byte aligned, the other arrays 4-byte").c_str());
  }
  if ((int64_t) o.nx * o.ny > kMaxVoxels || (int64_t) o.nx * o.ny * o.nz > kMaxVoxels || (int64_t) o.rows * o.cols > 0x7fffffffll ||
      (int64_t) o.batch * o.views > 0x7fffffffll) {  // the first product is below 2^62
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": nx * ny * nz beyond (2^31 - 1) / 3, or rows * cols or batch * views beyond 2^31 - 1").c_str());
  }
  RaycastArgs a = {};
  a.p = p;
  a.o = o;
  const int64_t tiles_x = ((int64_t) o.cols + kTile - 1) / kTile, tiles_y = ((int64_t) o.rows + kTile - 1) / kTile;
  a.tiles_x = (int32_t) tiles_x;
  a.ws      = static_cast<float*>(o.workspace);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid head = on.grid(o.batch, kThreads);
  const Grid rays = on.grid(tiles_x * tiles_y, (int64_t) o.batch * o.views, kThreads);
  PRS_TRY(on.check());
  on.launch(tsdf_raycast_head_kernel, head, 0, a);
  on.launch(tsdf_raycast_rays_kernel, rays, 0, a);
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_tsdf_raycast_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_tsdf_raycast_params);
  sizes2[1] = sizeof(prs_tsdf_raycast_batch);
}

uint64_t prs_tsdf_raycast_workspace_bytes(int32_t batch, int32_t views) {
  if (batch < 1 || views < 1 || (int64_t) batch * views > 0x7fffffffll) {
    return 0;
  }
  return (uint64_t) batch * (uint64_t) views * kWsFloats * sizeof(float);
}

int prs_tsdf_raycast_batch_run(prs_context* ctx, const prs_tsdf_raycast_params* params, const prs_tsdf_raycast_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return tsdf_raycast_launch(ctx, params, batch);
}

}  // extern "C"
