// tsdf_mesh.hip -- a TSDF volume as an indexed quad mesh on the device, by surface nets (prs_tsdf_mesh_batch_run; the rule is stated in
// include/proslam_hip_tsdf_mesh.h, BUILD-DEFINED, and restated in tests/tsdf_mesh_ref.py).  The voxels are walked as the surface call
// walks them: chunks of 1024 consecutive voxels in raster order, lane t on voxels t, t + 256, t + 512 and t + 768 of the chunk.  A lane
// whose voxel q is the low corner of a cube reads the cube's eight corners in place and keeps a band bit and a sign bit of each: the
// twelve edges of the cube, and with them q's own three crossings, are integer logic on those sixteen bits.
//     count     a ballot for the active cubes and one an axis for the interior crossings: two counts a chunk into the workspace
//     scan      one workgroup per sequence: both rows of chunk bases (exclusive scans), the four counts and the status
//     vertices  the same ballot gives every active cube its rank, which goes into the rank map (an int32 a voxel of the workspace)
//               whether or not its row fits; the lanes of active cubes whose row fits walk their crossings in ascending id
//     quads     the same ballots give every interior crossing its row; four ranks gathered from the map, one 16-byte store
// No atomic at all.  The crossing's point and normal are those of prs_tsdf_cross.h, which the surface call runs too.
#include <float.h>
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <string>

#include "../../include/proslam_hip_tsdf_mesh.h"
#include "prs_compact.h"
#include "prs_device.h"
#include "prs_host.h"
#include "prs_tsdf_cross.h"

namespace prs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kPerLane = 4;
constexpr int kChunk   = kThreads * kPerLane;       // voxels per workgroup: the surface call's chunk
constexpr int kWideThreads = 1024;                  // the scan at one large volume
constexpr int64_t kMaxVoxels = 0x7fffffffll / 3;    // the crossing's id 3 * index + e stays an int32

// the twelve edges of a cube in ascending id, four bits an edge: the corner (dx + 2 * dy + 4 * dz) its voxel a is, and its axis
constexpr uint64_t kEdgeCorner = 0x654432211000ull;
constexpr uint64_t kEdgeAxis   = 0x011022021210ull;

struct MeshArgs {
  prs_tsdf_mesh_batch o;
  float voxel_size, min_weight;
  int32_t voxels;      // nx * ny * nz
  int32_t chunks;      // ceil(voxels / kChunk): the chunks of a sequence
  int32_t write_out;
  int32_t* ws_vcount;  // [batch][chunks] active cubes of the chunk; after the scan: the rank of its first one, -1 = it has none
  int32_t* ws_qcount;  // [batch][chunks] interior crossings of the chunk; after the scan: its first row, -1 = keep out
  int32_t* ws_rank;    // [batch][voxels] the rank of the active cube at a voxel; written and read at active cubes alone
};

// what a lane knows of its voxel q = (i, j, k), linear index lin
struct Cell {
  int lin, i, j, k;
  uint32_t edges;  // the cube's taken crossings, bit = the edge's place in ascending id (0 when q is no cube's low corner)
  uint32_t quads;  // q's own interior crossings, bit = axis
  bool negative;   // t_q < 0.0f
};

__device__ __forceinline__ Cell cell_of(const MeshArgs& a, const float2* vol, const int lin) {
  const int nx = a.o.nx, ny = a.o.ny, nz = a.o.nz, nxny = nx * ny;
  Cell q;
  q.lin = lin;
  q.k   = lin / nxny;
  const int rem = lin - q.k * nxny;
  q.j = rem / nx;
  q.i = rem - q.j * nx;
  q.edges = 0, q.quads = 0, q.negative = false;
  if (lin < a.voxels && q.i + 1 < nx && q.j + 1 < ny && q.k + 1 < nz) {  // the eight corners lie in the grid
    uint32_t band = 0, neg = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float2 v = vol[lin + (c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nxny];
      band |= (in_band(v, a.min_weight) ? 1u : 0u) << c;
      neg |= (v.x < 0.0f ? 1u : 0u) << c;
    }
    if (band != 0) {
      // an edge is taken iff both ends are in band and their signs differ; the low ends of the x edges are corners 0, 2, 4, 6, of
      // the y edges 0, 1, 4, 5, of the z edges 0, 1, 2, 3
      const uint32_t x = band & (band >> 1) & (neg ^ (neg >> 1)) & 0x55u;
      const uint32_t y = band & (band >> 2) & (neg ^ (neg >> 2)) & 0x33u;
      const uint32_t z = band & (band >> 4) & (neg ^ (neg >> 4)) & 0x0fu;
      q.edges = (x & 1u) | ((y & 1u) << 1) | ((z & 1u) << 2) | (((y >> 1) & 1u) << 3) | (((z >> 1) & 1u) << 4) | (((x >> 2) & 1u) << 5) |
                (((z >> 2) & 1u) << 6) | (((z >> 3) & 1u) << 7) | (((x >> 4) & 1u) << 8) | (((y >> 4) & 1u) << 9) | (((y >> 5) & 1u) << 10) |
                (((x >> 6) & 1u) << 11);
      // q's own crossings, interior iff q is at least 1 on the two other axes (it is at most n - 2 on every axis already)
      q.quads = ((x & 1u) && q.j >= 1 && q.k >= 1 ? 1u : 0u) | ((y & 1u) && q.k >= 1 && q.i >= 1 ? 2u : 0u) |
                ((z & 1u) && q.i >= 1 && q.j >= 1 ? 4u : 0u);
      q.negative = (neg & 1u) != 0;
    }
  }
  return q;
}

// ---- count: blockIdx.x = b * chunks + c -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_mesh_count_kernel(const MeshArgs a) {
  __shared__ int s_v[kWaves], s_q[kWaves];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), wave = tid >> 6;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), b = (int) (id / (uint32_t) a.chunks);
  const float2* vol = reinterpret_cast<const float2*>(a.o.volume) + (size_t) b * (size_t) a.voxels;
  int cubes = 0, quads = 0;
#pragma unroll
  for (int s = 0; s < kPerLane; ++s) {
    const Cell q = cell_of(a, vol, c * kChunk + s * kThreads + tid);  // below 2^31: voxels <= (2^31 - 1) / 3, rounded up to a chunk
    cubes += (int) __popcll(__ballot(q.edges != 0));
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      quads += (int) __popcll(__ballot(((q.quads >> e) & 1u) != 0));
    }
  }
  if (lane == 0) {
    s_v[wave] = cubes;
    s_q[wave] = quads;
  }
  __syncthreads();
  if (tid == 0) {
    int sv = 0, sq = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      sv += s_v[w];
      sq += s_q[w];
    }
    a.ws_vcount[id] = sv;
    a.ws_qcount[id] = sq;
  }
}

// ---- scan: one workgroup per sequence, of 64 .. kWideThreads threads as the chunks ask ------------------------------------------------
// the C counts at cnt become chunk bases: -1 for a chunk without a row, and with `gate` for one whose first row lies behind cap -> total
__device__ __forceinline__ uint64_t scan_counts(int32_t* cnt, const int C, const int cap, const bool gate, uint64_t* s_scan) {
  const int tid = threadIdx.x, threads = blockDim.x;
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
        cnt[c0 + j] = (k[j] == 0 || (gate && at >= (uint64_t) cap)) ? -1 : (int32_t) at;
      }
      at += (uint64_t) k[j];
    }
    carry += tile;
  }
  return carry;
}

__global__ __launch_bounds__(kWideThreads) void tsdf_mesh_scan_kernel(const MeshArgs a) {
  __shared__ uint64_t s_scan[17];
  const int b = blockIdx.x, C = a.chunks;
  const int vcap = a.write_out ? a.o.vertex_stride : 0, qcap = a.write_out ? a.o.quad_stride : 0;
  // a cube behind vertex_stride keeps its rank, which a quad may name: the vertex bases are not gated
  const uint64_t cubes = scan_counts(a.ws_vcount + (size_t) b * C, C, vcap, false, s_scan);
  const uint64_t quads = scan_counts(a.ws_qcount + (size_t) b * C, C, qcap, true, s_scan);
  if (threadIdx.x == 0) {
    const int32_t nv = (int32_t) cubes, nq = (int32_t) quads;  // at most voxels and 3 * voxels
    a.o.n_vertices_total[b] = nv;
    a.o.n_quads_total[b]    = nq;
    a.o.n_vertices[b]       = nv < vcap ? nv : vcap;
    a.o.n_quads[b]          = nq < qcap ? nq : qcap;
    a.o.status[b]           = (a.write_out && (nv > vcap || nq > qcap)) ? PRS_ERR_CAPACITY : PRS_OK;
  }
}

// ---- vertices: blockIdx.x = b * chunks + c --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_mesh_vertices_kernel(const MeshArgs a) {
  __shared__ int s_wave[kPerLane][kWaves];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), wave = tid >> 6;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), b = (int) (id / (uint32_t) a.chunks);
  const int base = __builtin_amdgcn_readfirstlane(a.ws_vcount[id]);
  if (base < 0) {
    return;  // no active cube
  }
  const float2* vol = reinterpret_cast<const float2*>(a.o.volume) + (size_t) b * (size_t) a.voxels;
  Cell q[kPerLane];
  uint64_t active[kPerLane];
#pragma unroll
  for (int s = 0; s < kPerLane; ++s) {
    q[s]      = cell_of(a, vol, c * kChunk + s * kThreads + tid);
    active[s] = __ballot(q[s].edges != 0);
    if (lane == 0) {
      s_wave[s][wave] = (int) __popcll(active[s]);
    }
  }
  __syncthreads();
  const int nx = a.o.nx, ny = a.o.ny, nz = a.o.nz, nxny = nx * ny;
  const int cap = a.o.vertex_stride;
  const size_t out0 = (size_t) b * (size_t) cap;
  int32_t* rank_of = a.ws_rank + (size_t) b * (size_t) a.voxels;
  const float vs = a.voxel_size, mw = a.min_weight;
  const float* o = a.o.origin + (size_t) b * 4;
  int before = base;  // the ranks of the chunk's cubes that come before the slot's
#pragma unroll
  for (int s = 0; s < kPerLane; ++s) {
    int rank = before;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      rank += w < wave ? s_wave[s][w] : 0;
      before += s_wave[s][w];
    }
    rank = lanes_below(active[s], rank);
    if (q[s].edges == 0) {
      continue;
    }
    rank_of[q[s].lin] = rank;
    if (rank >= cap) {
      continue;
    }
    const int m = __popc(q[s].edges);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    for (uint32_t left = q[s].edges; left != 0; left &= left - 1) {  // ascending id
      const int edge   = __ffs((int) left) - 1;
      const int corner = (int) ((kEdgeCorner >> (4 * edge)) & 7u), e = (int) ((kEdgeAxis >> (4 * edge)) & 3u);
      const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
      const int lin      = q[s].lin + dx + dy * nx + dz * nxny;
      const int stride_e = e == 0 ? 1 : (e == 1 ? nx : nxny);
      const float2 va = vol[lin], vn = vol[lin + stride_e];
      const float4 P = crossing_point(o, q[s].i + dx, q[s].j + dy, q[s].k + dz, e, va, vn, vs);
      s0 = s0 + P.x;
      s1 = s1 + P.y;
      s2 = s2 + P.z;
      if (a.o.normal) {
        const float4 N = crossing_normal(vol, lin, q[s].i + dx, q[s].j + dy, q[s].k + dz, e, stride_e, va.x, vn.x, nx, ny, nz, mw);
        if (N.w != 0.0f) {
          g0 = g0 + N.x;
          g1 = g1 + N.y;
          g2 = g2 + N.z;
        }
      }
    }
    const float fm = (float) m;
    reinterpret_cast<float4*>(a.o.vertex)[out0 + (size_t) rank] = make_float4(s0 / fm, s1 / fm, s2 / fm, fm);
    if (a.o.cube) {
      a.o.cube[out0 + (size_t) rank] = q[s].lin;
    }
    if (a.o.normal) {
      const float len2 = (g0 * g0 + g1 * g1) + g2 * g2;
      float4 nrm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (len2 > 0.0f && len2 <= FLT_MAX) {
        const float len = sqrtf(len2);
        nrm = make_float4(g0 / len, g1 / len, g2 / len, 1.0f);
      }
      reinterpret_cast<float4*>(a.o.normal)[out0 + (size_t) rank] = nrm;
    }
  }
}

// ---- quads: blockIdx.x = b * chunks + c -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tsdf_mesh_quads_kernel(const MeshArgs a) {
  __shared__ int s_wave[kPerLane][kWaves];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), wave = tid >> 6;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), b = (int) (id / (uint32_t) a.chunks);
  const int base = __builtin_amdgcn_readfirstlane(a.ws_qcount[id]);
  if (base < 0) {
    return;  // no interior crossing, or behind quad_stride
  }
  const float2* vol = reinterpret_cast<const float2*>(a.o.volume) + (size_t) b * (size_t) a.voxels;
  Cell q[kPerLane];
  uint64_t mask[kPerLane][3];
#pragma unroll
  for (int s = 0; s < kPerLane; ++s) {
    q[s] = cell_of(a, vol, c * kChunk + s * kThreads + tid);
    int kept = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      mask[s][e] = __ballot(((q[s].quads >> e) & 1u) != 0);
      kept += (int) __popcll(mask[s][e]);
    }
    if (lane == 0) {
      s_wave[s][wave] = kept;
    }
  }
  __syncthreads();
  const int nx = a.o.nx, ny = a.o.ny;
  const int stride[3] = {1, nx, nx * ny};
  const int cap = a.o.quad_stride;
  const size_t out0 = (size_t) b * (size_t) cap;
  const int32_t* rank_of = a.ws_rank + (size_t) b * (size_t) a.voxels;
  int before = base;  // the rows of the chunk's voxels that come before the slot's
#pragma unroll
  for (int s = 0; s < kPerLane; ++s) {
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
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      if (!((q[s].quads >> e) & 1u)) {
        continue;
      }
      const int row = pos++;
      if (row >= cap) {
        continue;
      }
      // the four cubes around the edge: each is active, so this call's vertices pass wrote its rank
      const int lin = q[s].lin, sb = stride[(e + 1) % 3], sc = stride[(e + 2) % 3];
      const int r00 = rank_of[lin - sb - sc], r10 = rank_of[lin - sc], r11 = rank_of[lin], r01 = rank_of[lin - sb];
      reinterpret_cast<int4*>(a.o.quad)[out0 + (size_t) row] = q[s].negative ? make_int4(r00, r10, r11, r01) : make_int4(r00, r01, r11, r10);
      if (a.o.edge) {
        a.o.edge[out0 + (size_t) row] = 3 * lin + e;
      }
    }
  }
}

// chunks of a sequence's volume, 0 when the sizes are not ones the launcher takes
int64_t mesh_chunks(const int64_t batch, const int64_t nx, const int64_t ny, const int64_t nz) {
  if (batch < 1 || nx < 1 || ny < 1 || nz < 1 || nx * ny > kMaxVoxels || nx * ny * nz > kMaxVoxels) {  // the first product is below 2^62
    return 0;
  }
  return (nx * ny * nz + kChunk - 1) / kChunk;
}

// the workspace: [batch][chunks] int32 twice, each rounded up to 16 bytes, then [batch][voxels] int32
uint64_t mesh_count_bytes(const int64_t batch, const int64_t chunks) {
  return up16((uint64_t) batch * (uint64_t) chunks * 4);
}

}  // namespace

int tsdf_mesh_launch(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_mesh_batch* batch) {
  const std::string who = "prs_tsdf_mesh_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_tsdf_params& p     = *params;
  const prs_tsdf_mesh_batch& o = *batch;
  const bool write_out = o.vertex && o.quad;
  if (!o.origin || !o.volume || !o.n_vertices || !o.n_vertices_total || !o.n_quads || !o.n_quads_total || !o.status || !o.workspace ||
      (o.vertex != nullptr) != (o.quad != nullptr) || (!write_out && (o.normal || o.cube || o.edge))) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": origin, volume, a per-sequence output or the workspace not set, only one of vertex and quad set, or normal, cube or edge set without them").c_str());
  }
  if (o.batch < 1 || o.nx < 1 || o.ny < 1 || o.nz < 1 || (write_out && (o.vertex_stride < 1 || o.quad_stride < 1)) || !std::isfinite(p.voxel_size) ||
      !(p.voxel_size > 0.0f) || !std::isfinite(p.min_weight)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size below 1, a stride below 1 with outputs set, voxel_size not finite or not positive, or min_weight not finite").c_str());
  }
  if (!aligned_to(o.volume, 16) || !aligned_to(o.vertex, 16) || !aligned_to(o.normal, 16) || !aligned_to(o.quad, 16) || !aligned_to(o.workspace, 16) ||
      !aligned_to(o.origin, 4) || !aligned_to(o.cube, 4) || !aligned_to(o.edge, 4) || !aligned_to(o.n_vertices, 4) ||
      !aligned_to(o.n_vertices_total, 4) || !aligned_to(o.n_quads, 4) || !aligned_to(o.n_quads_total, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": volume, vertex, normal, quad and the workspace must be 16-byte aligned, the other arrays 4-byte").c_str());
  }
  const int64_t C = mesh_chunks(o.batch, o.nx, o.ny, o.nz);
  if (C < 1) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": nx * ny * nz beyond (2^31 - 1) / 3").c_str());
  }
  const int wide = (int) std::min<long long>(kWideThreads, ((C + kCompactBatch - 1) / kCompactBatch + PRS_WAVE - 1) / PRS_WAVE * PRS_WAVE);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid pass = on.grid((int64_t) o.batch * C, kThreads), scan = on.grid(o.batch, wide);
  PRS_TRY(on.check());
  MeshArgs a = {};
  a.o = o;
  a.voxel_size = p.voxel_size;
  a.min_weight = p.min_weight;
  a.voxels     = (int32_t) ((int64_t) o.nx * o.ny * o.nz);
  a.chunks     = (int32_t) C;
  a.write_out  = write_out;
  uint8_t* ws  = static_cast<uint8_t*>(o.workspace);
  const uint64_t counts = mesh_count_bytes(o.batch, C);
  a.ws_vcount = reinterpret_cast<int32_t*>(ws);
  a.ws_qcount = reinterpret_cast<int32_t*>(ws + counts);
  a.ws_rank   = reinterpret_cast<int32_t*>(ws + 2 * counts);
  on.launch(tsdf_mesh_count_kernel, pass, 0, a);
  on.launch(tsdf_mesh_scan_kernel, scan, 0, a);
  if (write_out) {
    on.launch(tsdf_mesh_vertices_kernel, pass, 0, a);
    on.launch(tsdf_mesh_quads_kernel, pass, 0, a);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_tsdf_mesh_struct_sizes(uint64_t* sizes1) {
  sizes1[0] = sizeof(prs_tsdf_mesh_batch);
}

uint64_t prs_tsdf_mesh_workspace_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t nz) {
  const int64_t C = mesh_chunks(batch, nx, ny, nz);
  if (C < 1 || !grid_fits((int64_t) batch * C, kThreads)) {
    return 0;
  }
  return 2 * mesh_count_bytes(batch, C) + up16((uint64_t) batch * (uint64_t) nx * (uint64_t) ny * (uint64_t) nz * 4);
}

int prs_tsdf_mesh_batch_run(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_mesh_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return tsdf_mesh_launch(ctx, params, batch);
}

}  // extern "C"
