// tsdf.hip -- TSDF fusion on the device: depth images averaged along the viewing ray into a truncated signed distance volume per
// sequence (prs_tsdf_integrate_batch_run) and the zero crossings of that volume as points with normals (prs_tsdf_surface_batch_run;
// the rule is stated in include/proslam_hip_tsdf.h, BUILD-DEFINED, and restated in tests/tsdf_ref.py).
//   integrate
//     head     one workgroup per sequence, a thread an image: status[b], n_skipped[b] (ballot counts through LDS), 0 into n_updates,
//              and per image Ti = se3_inverse(pose * sensor_in_robot) with a served flag into the workspace (16 floats an image)
//     bricks   one workgroup per brick of 32 x 4 x 4 voxels of one sequence: a lane holds the (tsdf, w) of its two voxels (the same
//              i and j, k two apart) in registers over the whole frame loop, so a voxel is loaded once and stored at most once a call.
//              A half-wave reads 256 consecutive bytes of the volume, the natural width for volumes whose nx is no multiple of 64.
//              Ti comes through LDS, 32 images at a time (a read of one address by every lane is a broadcast); the images' update
//              counts are gathered there too (a ballot count a wave, an LDS integer add) and leave as one global integer atomic add
//              a workgroup and image.  No brick is tested against a frustum: every voxel runs the rule itself.
//   surface    the stable stream compaction of depth_cloud.hip over the voxels in raster order, which is the order of the rows, in
//              chunks of 1024 consecutive voxels, lane t on voxels t, t + 256, t + 512 and t + 768 of the chunk:
//     count    three wave ballots a voxel (one an axis), the chunk's count into the workspace
//     scan     one workgroup per sequence: the chunk bases (an exclusive scan), n_total, n_out, status
//     scatter  the same ballots give every crossing its row; point, normal and cell are stored where the row belongs
// The only atomics are integer adds: the sums are the same whatever order they arrive in.
#include <float.h>
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <string>

#include "../../include/proslam_hip_tsdf.h"
#include "prs_compact.h"
#include "prs_depth.h"
#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"
#include "prs_se3.h"
#include "prs_tsdf_cross.h"

namespace prs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kBrickX = 32, kBrickY = 4, kBrickZ = 4;
constexpr int kPerLane = kBrickX * kBrickY * kBrickZ / kThreads;  // 2: the same (i, j), k and k + kBrickZ / 2
constexpr int kFrameTile = 32;     // images whose Ti lie in LDS at a time
constexpr int kWsFloats  = 16;     // floats of workspace an image: Ti[12], the served flag (an int), three unused
constexpr int kSurfPerLane = 4;
constexpr int kSurfChunk   = kThreads * kSurfPerLane;  // voxels per workgroup of the surface passes
constexpr int kWideThreads = 1024;                     // the scan at one large volume
constexpr int64_t kMaxVoxels = 0x7fffffffll / 3;       // cell = 3 * index + e stays an int32

struct TsdfArgs {
  prs_tsdf_params p;
  prs_tsdf_batch o;
  int32_t bx, by, bz;  // bricks of a sequence along x, y and z
  float* ws;           // [batch][frames][kWsFloats]
};

// ---- head: blockIdx.x = b; thread t on images t, t + kThreads, ... ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_head_kernel(const TsdfArgs a) {
  __shared__ int s_skipped[kWaves];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int frames = a.o.frames;
  const int n_img  = images_of(a.o, b);
  int skipped = 0;
  for (int f0 = 0; f0 < frames; f0 += kThreads) {  // uniform trip count: the ballot below is the whole wave's
    const int f = f0 + tid;
    bool skip = false;
    if (f < frames) {
      const size_t image = (size_t) b * (size_t) frames + (size_t) f;
      float* ws  = a.ws + image * kWsFloats;
      int served = 0;
      float Ti[12] = {};
      if (f < n_img) {
        const int k = depth_pose_row(a.o.frame_index, a.o.pose, frames, a.o.pose_stride, b, f);
        if (k >= 0) {
          float T[12];
          se3_mul<false>(a.o.pose + ((size_t) b * (size_t) a.o.pose_stride + (size_t) k) * 16, a.p.sensor_in_robot, T);
          se3_inverse<false>(T, Ti);
          served = 1;
        } else {
          skip = true;
        }
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        ws[i] = Ti[i];
      }
      ws[12] = __int_as_float(served);
      if (n_img >= 0 && a.o.n_updates) {
        a.o.n_updates[image] = 0;
      }
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
    a.o.status[b]    = n_img < 0 ? PRS_ERR_RANGE : PRS_OK;
    a.o.n_skipped[b] = n_img < 0 ? 0 : sum;
  }
}

// ---- bricks: blockIdx.x = ((b * bz + z) * by + y) * bx + x.  E: the depth element -----------------------------------------------------
template <typename E>
__global__ __launch_bounds__(kThreads) void tsdf_integrate_kernel(const TsdfArgs a) {
  __shared__ float s_T[kFrameTile * kWsFloats];
  __shared__ int s_upd[kFrameTile];
  const int tid = threadIdx.x;
  uint32_t id   = blockIdx.x;
  const int x = (int) (id % (uint32_t) a.bx);
  id /= (uint32_t) a.bx;
  const int y = (int) (id % (uint32_t) a.by);
  id /= (uint32_t) a.by;
  const int z = (int) (id % (uint32_t) a.bz);
  const int b = (int) (id / (uint32_t) a.bz);
  const int n_img = images_of(a.o, b);
  if (n_img <= 0) {
    return;  // refused, or no image: nothing of the volume is touched (uniform over the workgroup)
  }
  const int nx = a.o.nx, ny = a.o.ny, nz = a.o.nz;
  const int i = x * kBrickX + (tid & (kBrickX - 1));
  const int j = y * kBrickY + ((tid >> 5) & (kBrickY - 1));
  const int k0 = z * kBrickZ + (tid >> 7);  // the lane's voxels: k0 and k0 + 2
  const float vs = a.p.voxel_size;
  const float* o = a.o.origin + (size_t) b * 4;
  const float c0 = o[0] + ((float) i + 0.5f) * vs;
  const float c1 = o[1] + ((float) j + 0.5f) * vs;
  float c2[kPerLane];
  bool live[kPerLane], touched[kPerLane];
  float2 cell[kPerLane];
  float2* at[kPerLane];
#pragma unroll
  for (int v = 0; v < kPerLane; ++v) {
    const int k = k0 + v * (kBrickZ / kPerLane);
    c2[v]      = o[2] + ((float) k + 0.5f) * vs;
    live[v]    = i < nx && j < ny && k < nz;
    touched[v] = false;
    cell[v]    = make_float2(0.0f, 0.0f);
    at[v] = reinterpret_cast<float2*>(a.o.volume) + ((((size_t) b * (size_t) nz + (size_t) k) * (size_t) ny + (size_t) j) * (size_t) nx + (size_t) i);
    if (live[v]) {
      cell[v] = *at[v];
    }
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const float fcols = (float) cols, frows = (float) rows;
  const float fx = a.p.fx, fy = a.p.fy, cx = a.p.cx, cy = a.p.cy;
  const float scale = a.p.depth_scaling_factor_to_meters, rmin = a.p.range_min, rmax = a.p.range_max;
  const float trunc = a.p.truncation, wmax = a.p.max_weight;
  const size_t image_bytes = (size_t) rows * (size_t) a.o.pitch;
  const size_t image0      = (size_t) b * (size_t) a.o.frames;
  for (int f0 = 0; f0 < n_img; f0 += kFrameTile) {
    const int tile = min(kFrameTile, n_img - f0);
    __syncthreads();  // the tile before this one has been read
    for (int t = tid; t < tile * kWsFloats; t += kThreads) {
      s_T[t] = a.ws[(image0 + (size_t) f0) * kWsFloats + (size_t) t];
    }
    if (tid < kFrameTile) {
      s_upd[tid] = 0;
    }
    __syncthreads();
    for (int ff = 0; ff < tile; ++ff) {
      const float* Ti = s_T + ff * kWsFloats;
      if (__float_as_int(Ti[12]) == 0) {
        continue;  // a skipped frame (uniform)
      }
      const uint8_t* img = static_cast<const uint8_t*>(a.o.depth) + (image0 + (size_t) (f0 + ff)) * image_bytes;
      int updated = 0;
#pragma unroll
      for (int v = 0; v < kPerLane; ++v) {
        bool hit = false;
        if (live[v]) {
          const float c[3] = {c0, c1, c2[v]};
          float q[3];
          se3_apply(Ti, c, q);
          const float zc = q[2];
          if (zc > 0.0f && zc >= rmin && zc <= rmax) {
            const float uf = floorf((q[0] / zc * fx + cx) + 0.5f);
            const float vf = floorf((q[1] / zc * fy + cy) + 0.5f);
            if (uf >= 0.0f && uf < fcols && vf >= 0.0f && vf < frows) {
              const int u = (int) uf, r = (int) vf;
              const float raw = (float) reinterpret_cast<const E*>(img + (size_t) r * (size_t) a.o.pitch)[u];
              float d;
              if (depth_valid(raw, scale, rmin, rmax, d)) {
                const float sdf = d - zc;
                if (sdf >= -trunc) {
                  float t = sdf / trunc;
                  t = t > 1.0f ? 1.0f : t;
                  const float w1 = cell[v].y + 1.0f;
                  cell[v].x = (cell[v].x * cell[v].y + t) / w1;
                  cell[v].y = w1 > wmax ? wmax : w1;
                  hit = true;
                }
              }
            }
          }
        }
        touched[v] = touched[v] || hit;
        updated += (int) __popcll(__ballot(hit));
      }
      if (a.o.n_updates && updated != 0 && (tid & (PRS_WAVE - 1)) == 0) {
        atomicAdd(s_upd + ff, updated);
      }
    }
    if (a.o.n_updates) {
      __syncthreads();
      if (tid < tile && s_upd[tid] != 0) {
        atomicAdd(a.o.n_updates + image0 + (size_t) (f0 + tid), s_upd[tid]);
      }
    }
  }
#pragma unroll
  for (int v = 0; v < kPerLane; ++v) {
    if (touched[v]) {
      *at[v] = cell[v];
    }
  }
}

// =====================================================================================================================================
struct SurfaceArgs {
  prs_tsdf_params p;
  prs_tsdf_surface_batch o;
  int32_t voxels;     // nx * ny * nz
  int32_t chunks;     // ceil(voxels / kSurfChunk): the chunks of a sequence
  int32_t write_out;
  int32_t* ws_count;  // [batch][chunks] crossings of the chunk; after the scan: the chunk's first output row, -1 = keep out
};

// blockIdx.x = b * chunks + c.  SCATTER: write the rows (else: count them)
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void tsdf_surface_kernel(const SurfaceArgs a) {
  __shared__ int s_wave[kSurfPerLane][kWaves];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), wave = tid >> 6;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), b = (int) (id / (uint32_t) a.chunks);
  int base = 0;
  if (SCATTER) {
    base = __builtin_amdgcn_readfirstlane(a.ws_count[id]);
    if (base < 0) {
      return;  // no crossing, or behind out_stride
    }
  }
  const int nx = a.o.nx, ny = a.o.ny, nz = a.o.nz;
  const int n[3]      = {nx, ny, nz};
  const int stride[3] = {1, nx, nx * ny};
  const float mw = a.p.min_weight;
  const float2* vol = reinterpret_cast<const float2*>(a.o.volume) + (size_t) b * (size_t) a.voxels;
  float2 va[kSurfPerLane];
  float2 vn[kSurfPerLane][3];
  uint64_t mask[kSurfPerLane][3];
  int at[kSurfPerLane][3];  // the voxel's coordinates
  int kept[kSurfPerLane];
#pragma unroll
  for (int s = 0; s < kSurfPerLane; ++s) {
    const int lin = c * kSurfChunk + s * kThreads + tid;  // below 2^31: voxels <= (2^31 - 1) / 3, rounded up to a chunk
    const bool inside = lin < a.voxels;
    const int k = lin / stride[2], rem = lin - k * stride[2], j = rem / nx;
    at[s][0] = rem - j * nx, at[s][1] = j, at[s][2] = k;
    va[s] = inside ? vol[lin] : make_float2(0.0f, 0.0f);
    const bool band_a = inside && in_band(va[s], mw);
    kept[s] = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      bool cross = false;
      vn[s][e] = make_float2(0.0f, 0.0f);
      if (band_a && at[s][e] + 1 < n[e]) {
        vn[s][e] = vol[lin + stride[e]];
        cross = in_band(vn[s][e], mw) && ((va[s].x < 0.0f) != (vn[s][e].x < 0.0f));
      }
      mask[s][e] = __ballot(cross);
      kept[s] += (int) __popcll(mask[s][e]);
    }
    if (lane == 0) {
      s_wave[s][wave] = kept[s];
    }
  }
  __syncthreads();
  if (!SCATTER) {
    if (tid == 0) {
      int sum = 0;
#pragma unroll
      for (int s = 0; s < kSurfPerLane; ++s) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          sum += s_wave[s][w];
        }
      }
      a.ws_count[id] = sum;
    }
    return;
  }
  const int cap    = a.o.out_stride;
  const size_t out0 = (size_t) b * (size_t) cap;
  const float vs = a.p.voxel_size;
  const float* o = a.o.origin + (size_t) b * 4;
  int before = base;  // the rows of the chunk's voxels that come before the slot's
#pragma unroll
  for (int s = 0; s < kSurfPerLane; ++s) {
    int pos = before;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      pos += w < wave ? s_wave[s][w] : 0;
      before += s_wave[s][w];
    }
    // the rows of the lanes below this one, on every axis, then this voxel's own in the order of the axes
    pos = lanes_below(mask[s][0], pos);
    pos = lanes_below(mask[s][1], pos);
    pos = lanes_below(mask[s][2], pos);
    const int lin = c * kSurfChunk + s * kThreads + tid;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      if (!((mask[s][e] >> lane) & 1ull)) {
        continue;
      }
      const int row = pos++;
      if (row >= cap) {
        continue;
      }
      // the crossing's point and normal: prs_tsdf_cross.h, which the mesh call runs too
      reinterpret_cast<float4*>(a.o.xyz)[out0 + (size_t) row] = crossing_point(o, at[s][0], at[s][1], at[s][2], e, va[s], vn[s][e], vs);
      if (a.o.cell) {
        a.o.cell[out0 + (size_t) row] = 3 * lin + e;
      }
      if (a.o.normal) {
        reinterpret_cast<float4*>(a.o.normal)[out0 + (size_t) row] =
            crossing_normal(vol, lin, at[s][0], at[s][1], at[s][2], e, stride[e], va[s].x, vn[s][e].x, nx, ny, nz, mw);
      }
    }
  }
}

// ---- scan: one workgroup per sequence, of 64 .. kWideThreads threads as the chunks ask -------------------------------------------------
__global__ __launch_bounds__(kWideThreads) void tsdf_surface_scan_kernel(const SurfaceArgs a) {
  __shared__ uint64_t s_scan[17];
  const int tid = threadIdx.x, threads = blockDim.x, b = blockIdx.x;
  const int C   = a.chunks;
  int32_t* cnt  = a.ws_count + (size_t) b * C;
  const int cap = a.write_out ? a.o.out_stride : 0;
  // every thread kCompactBatch consecutive chunks of a tile, their sum scanned over the tile and carried from tile to tile
  uint64_t carry = 0;
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
    const int32_t total = carry > 0x7fffffffull ? 0x7fffffff : (int32_t) carry;  // at most 3 * voxels
    a.o.n_total[b]      = total;
    a.o.n_out[b]        = total < cap ? total : cap;
    a.o.status[b]       = (a.write_out && total > cap) ? PRS_ERR_CAPACITY : PRS_OK;
  }
}

// chunks of a sequence's volume for the surface passes, 0 when the sizes are not ones the launcher takes
int64_t surface_chunks(const int64_t batch, const int64_t nx, const int64_t ny, const int64_t nz) {
  if (batch < 1 || nx < 1 || ny < 1 || nz < 1 || nx * ny > kMaxVoxels || nx * ny * nz > kMaxVoxels) {  // the first product is below 2^62
    return 0;
  }
  return (nx * ny * nz + kSurfChunk - 1) / kSurfChunk;
}

}  // namespace

int tsdf_integrate_launch(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_batch* batch) {
  const std::string who = "prs_tsdf_integrate_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_tsdf_params& p = *params;
  const prs_tsdf_batch& o  = *batch;
  if (!o.depth || !o.pose || !o.origin || !o.volume || !o.n_skipped || !o.status || !o.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": depth, pose, origin, volume, n_skipped, status or the workspace not set").c_str());
  }
  const int64_t elem = depth_bytes(p.depth_type);
  if (elem == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": unknown depth_type").c_str());
  }
  bool finite = std::isfinite(p.depth_scaling_factor_to_meters) && std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) &&
                std::isfinite(p.cy) && std::isfinite(p.range_min) && std::isfinite(p.range_max) && std::isfinite(p.voxel_size) &&
                std::isfinite(p.truncation) && std::isfinite(p.max_weight);
  for (int i = 0; i < 16; ++i) {
    finite = finite && std::isfinite(p.sensor_in_robot[i]);
  }
  if (o.batch < 1 || o.frames < 1 || o.rows < 1 || o.cols < 1 || o.pose_stride < 1 || o.nx < 1 || o.ny < 1 || o.nz < 1 ||
      !pitch_ok(o.pitch, o.cols, elem) || !finite || !(p.depth_scaling_factor_to_meters > 0.0f) || p.range_min < 0.0f ||
      p.range_min > p.range_max || !(p.voxel_size > 0.0f) || !(p.truncation > 0.0f) || !(p.max_weight >= 1.0f)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size below 1, a pitch below the row's bytes or not a multiple of the element, a parameter not finite, a scale, voxel_size or truncation not positive, range_min negative or above range_max, or max_weight below 1").c_str());
  }
  if (!aligned_to(o.volume, 16) || !aligned_to(o.workspace, 16) || !aligned_to(o.depth, (uintptr_t) elem) || !aligned_to(o.n_images, 4) ||
      !aligned_to(o.pose, 4) || !aligned_to(o.frame_index, 4) || !aligned_to(o.origin, 4) || !aligned_to(o.n_updates, 4) ||
      !aligned_to(o.n_skipped, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": volume and the workspace must be 16-byte aligned, depth to its element, the other arrays 4-byte").c_str());
  }
  if (surface_chunks(o.batch, o.nx, o.ny, o.nz) < 1 || (int64_t) o.rows * o.cols > 0x7fffffffll || (int64_t) o.batch * o.frames > 0x7fffffffll) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": nx * ny * nz beyond (2^31 - 1) / 3, or rows * cols or batch * frames beyond 2^31 - 1").c_str());
  }
  TsdfArgs a = {};
  a.p  = p;
  a.o  = o;
  a.bx = (o.nx + kBrickX - 1) / kBrickX;
  a.by = (o.ny + kBrickY - 1) / kBrickY;
  a.bz = (o.nz + kBrickZ - 1) / kBrickZ;
  a.ws = static_cast<float*>(o.workspace);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid head   = on.grid(o.batch, kThreads);
  const Grid bricks = on.grid((int64_t) o.batch * a.bx * a.by * a.bz, kThreads);  // below 2^31 * 2^31
  PRS_TRY(on.check());
  on.launch(tsdf_head_kernel, head, 0, a);
  if (p.depth_type == PRS_DEPTH_U16) {
    on.launch(tsdf_integrate_kernel<uint16_t>, bricks, 0, a);
  } else {
    on.launch(tsdf_integrate_kernel<float>, bricks, 0, a);
  }
  return on.finish();
}

int tsdf_surface_launch(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_surface_batch* batch) {
  const std::string who = "prs_tsdf_surface_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_tsdf_params& p        = *params;
  const prs_tsdf_surface_batch& o = *batch;
  if (!o.origin || !o.volume || !o.n_out || !o.n_total || !o.status || !o.workspace || (!o.xyz && (o.normal || o.cell))) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": origin, volume, a per-sequence output or the workspace not set, or normal or cell set without xyz").c_str());
  }
  if (o.batch < 1 || o.nx < 1 || o.ny < 1 || o.nz < 1 || (o.xyz && o.out_stride < 1) || !std::isfinite(p.voxel_size) || !(p.voxel_size > 0.0f) ||
      !std::isfinite(p.min_weight)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size below 1, out_stride below 1 with xyz set, voxel_size not finite or not positive, or min_weight not finite").c_str());
  }
  if (!aligned_to(o.volume, 16) || !aligned_to(o.xyz, 16) || !aligned_to(o.normal, 16) || !aligned_to(o.workspace, 16) || !aligned_to(o.origin, 4) ||
      !aligned_to(o.cell, 4) || !aligned_to(o.n_out, 4) || !aligned_to(o.n_total, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": volume, xyz, normal and the workspace must be 16-byte aligned, the other arrays 4-byte").c_str());
  }
  const int64_t C = surface_chunks(o.batch, o.nx, o.ny, o.nz);
  if (C < 1) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": nx * ny * nz beyond (2^31 - 1) / 3").c_str());
  }
  const int wide = (int) std::min<long long>(kWideThreads, ((C + kCompactBatch - 1) / kCompactBatch + PRS_WAVE - 1) / PRS_WAVE * PRS_WAVE);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid pass = on.grid((int64_t) o.batch * C, kThreads), scan = on.grid(o.batch, wide);
  PRS_TRY(on.check());
  SurfaceArgs a = {};
  a.p = p;
  a.o = o;
  a.voxels    = (int32_t) ((int64_t) o.nx * o.ny * o.nz);
  a.chunks    = (int32_t) C;
  a.write_out = o.xyz != nullptr;
  a.ws_count  = static_cast<int32_t*>(o.workspace);
  on.launch(tsdf_surface_kernel<false>, pass, 0, a);
  on.launch(tsdf_surface_scan_kernel, scan, 0, a);
  if (a.write_out) {
    on.launch(tsdf_surface_kernel<true>, pass, 0, a);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_tsdf_struct_sizes(uint64_t* sizes3) {
  sizes3[0] = sizeof(prs_tsdf_params);
  sizes3[1] = sizeof(prs_tsdf_batch);
  sizes3[2] = sizeof(prs_tsdf_surface_batch);
}

uint64_t prs_tsdf_workspace_bytes(int32_t batch, int32_t frames) {
  if (batch < 1 || frames < 1 || (int64_t) batch * frames > 0x7fffffffll) {
    return 0;
  }
  return (uint64_t) batch * (uint64_t) frames * kWsFloats * sizeof(float);
}

uint64_t prs_tsdf_surface_workspace_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t nz) {
  const uint64_t counts = (uint64_t) batch * (uint64_t) surface_chunks(batch, nx, ny, nz) * 4;  // 0 chunks: 0 bytes
  return (counts + 15) & ~(uint64_t) 15;
}

int prs_tsdf_integrate_batch_run(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return tsdf_integrate_launch(ctx, params, batch);
}

int prs_tsdf_surface_batch_run(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_surface_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return tsdf_surface_launch(ctx, params, batch);
}

}  // extern "C"
