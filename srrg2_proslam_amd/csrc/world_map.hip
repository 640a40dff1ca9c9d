// world_map.hip -- the world map on the device: the landmarks of every archived map and of the live one, carried into the world frame
// by the float64 node poses of the pose graph as they stand, filtered and compacted into one cloud per sequence in node order
// (prs_world_map_batch_run; the rule is stated in include/proslam_hip.h, BUILD-DEFINED, and restated in tests/world_map_ref.py).
// A stable stream compaction over batch x maps x capacity rows, spread over (sequence, map, chunk of kChunk rows) so that one
// sequence of hundreds of maps fills the device as well as thousands of sequences of a few maps do:
//   count    one workgroup per chunk: the rows it keeps and the rows it drops as not finite, into the workspace
//   scan     one workgroup per sequence: validates the sequence, gives every chosen map its node, turns the counts into chunk bases
//            in node order (an exclusive scan) and writes the per-sequence counts and status
//   scatter  one workgroup per chunk: positions inside the chunk from wave ballots, wave totals through LDS, the base from the scan;
//            writes the cloud, refreshes `state`, and leaves the chunk's bounds in the workspace
//   bounds   one workgroup per sequence: min / max over the chunks' bounds
// No atomic decides a position or a value; the output bytes depend neither on the batch nor on the grid nor on the run.
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <string>

#include "prs_compact.h"
#include "prs_device.h"
#include "prs_host.h"

namespace prs {

namespace {

constexpr int kThreads = 256;
constexpr int kChunk   = kThreads;  // rows per workgroup: one row per thread, a wave's rows are 64 consecutive ones
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kWideThreads = 1024;  // the per-sequence kernels at one long sequence: as many threads as it has nodes, or chunks
constexpr int kBatch   = kCompactBatch;

struct WorldMapArgs {
  prs_world_map_params p;
  prs_world_map_batch o;
  int32_t batch, capacity, node_stride, slot_stride;
  int32_t maps;    // map entries per sequence: the archive's slots, then the live map (entry slot_stride)
  int32_t chunks;  // chunks per map
  int32_t write_out;
  // the live map
  const float* live_coords;
  const uint8_t* live_desc;
  const int32_t* live_n_points;
  const uint32_t* live_n_opt;
  const uint8_t* live_inlier;
  float* live_state;
  // the archive
  const float* ar_coords;
  const uint8_t* ar_desc;
  const uint32_t* ar_n_opt;
  const uint8_t* ar_inlier;
  float* ar_state;
  const int32_t* ar_n_points;
  const int32_t* slot_of_node;
  // the graph
  const double* graph_X;
  const int32_t* n_nodes;
  const int32_t* cur_node;
  // the workspace
  int32_t* ws_count;      // [batch][maps][chunks] kept rows of the chunk; after the scan: the chunk's first output row
  int32_t* ws_nonfinite;  // [batch][maps][chunks]
  float* ws_bounds;       // [batch][maps][chunks][6]
  int32_t* ws_node;       // [batch][maps] node of the map, -1 = not chosen (or the sequence is refused)
};

// the rows of map entry m of sequence b
struct MapRows {
  const float4* coords;
  const uint4* desc;
  const uint32_t* n_opt;
  const uint8_t* inlier;
  float4* state;
};

__device__ __forceinline__ MapRows map_rows(const WorldMapArgs& a, const int b, const int m) {
  MapRows r;
  if (m == a.slot_stride) {
    const size_t at = (size_t) b * a.capacity;
    r.coords = reinterpret_cast<const float4*>(a.live_coords) + at;
    r.desc   = reinterpret_cast<const uint4*>(a.live_desc) + 2 * at;
    r.n_opt  = a.live_n_opt + at;
    r.inlier = a.live_inlier + at;
    r.state  = reinterpret_cast<float4*>(a.live_state) + at;
  } else {
    const size_t at = ((size_t) b * a.slot_stride + m) * a.capacity;
    r.coords = reinterpret_cast<const float4*>(a.ar_coords) + at;
    r.desc   = reinterpret_cast<const uint4*>(a.ar_desc) + 2 * at;
    r.n_opt  = a.ar_n_opt + at;
    r.inlier = a.ar_inlier + at;
    r.state  = reinterpret_cast<float4*>(a.ar_state) + at;
  }
  return r;
}

// one landmark in the world: float64 products and sums in the order the header writes them, one rounding to float each
struct WorldRow {
  float4 c;
  float wx, wy, wz;
  uint32_t n_opt;
  bool finite;  // all three world coordinates
  bool passes;  // the filter, the finiteness aside
};

// what the filter and the transform read of row r: 21 bytes
struct RowIn {
  float4 c;
  uint32_t n_opt;
  uint8_t inlier;
};

__device__ __forceinline__ RowIn row_in(const MapRows& rows, const int r) {
  RowIn in;
  in.c      = rows.coords[r];
  in.n_opt  = rows.n_opt[r];
  in.inlier = rows.inlier[r];
  return in;
}

__device__ __forceinline__ WorldRow world_row(const WorldMapArgs& a, const RowIn& in, const double* X) {
  WorldRow w;
  w.c            = in.c;
  w.n_opt        = in.n_opt;
  const bool inl = in.inlier != 0;
  const double x = (double) w.c.x, y = (double) w.c.y, z = (double) w.c.z;
  w.wx           = (float) (((X[0] * x + X[1] * y) + X[2] * z) + X[3]);
  w.wy           = (float) (((X[4] * x + X[5] * y) + X[6] * z) + X[7]);
  w.wz           = (float) (((X[8] * x + X[9] * y) + X[10] * z) + X[11]);
  w.finite       = finite_bits(w.wx) && finite_bits(w.wy) && finite_bits(w.wz);
  w.passes       = w.n_opt >= a.p.min_n_opt && (!a.p.require_inlier || inl);
  return w;
}

// ---- count: blockIdx.x = (b * maps + m) * chunks + c --------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void world_map_count_kernel(const WorldMapArgs a) {
  __shared__ int s_node;
  __shared__ int s_kept[kWaves], s_bad[kWaves];
  const int tid     = threadIdx.x;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), m = (int) ((id / (uint32_t) a.chunks) % (uint32_t) a.maps);
  const int b = (int) (id / ((uint32_t) a.chunks * (uint32_t) a.maps));
  // everything up to the row loop is the same in every thread of the workgroup.  A sequence the scan will refuse may count what
  // it likes: this kernel only has to stay inside the arrays, the scan sets its maps aside
  const int nn = a.n_nodes[b], cur = a.cur_node[b];
  const bool live = m == a.slot_stride;
  bool ok         = nn >= 1 && nn <= a.node_stride && cur >= 0 && cur < nn && (!live || a.p.include_live != 0);
  int np          = 0;
  if (ok) {
    np = live ? a.live_n_points[b] : a.ar_n_points[(size_t) b * a.slot_stride + m];
    ok = np >= 0 && np <= a.capacity;
  }
  if (!ok || c * kChunk >= np) {
    if (tid == 0) {
      a.ws_count[id]     = 0;
      a.ws_nonfinite[id] = 0;
    }
    return;
  }
  // the row does not depend on the node: its loads are in flight while the node is looked for
  const MapRows rows = map_rows(a, b, m);
  const int r        = c * kChunk + tid;
  RowIn in           = {};
  if (r < np) {
    in = row_in(rows, r);
  }
  // the node whose map this is: the current node for the live map, else the node that names the slot (the slot-to-node inversion;
  // the lowest such node, two of them make the scan refuse the sequence)
  int node = cur;
  if (!live) {
    if (tid == 0) {
      s_node = 0x7fffffff;
    }
    __syncthreads();
    const int32_t* son = a.slot_of_node + (size_t) b * a.node_stride;
    for (int n = tid; n < nn; n += kThreads) {
      if (son[n] == m && !(a.p.include_live != 0 && n == cur)) {
        atomicMin(&s_node, n);  // LDS; a minimum does not depend on the order
      }
    }
    __syncthreads();
    node = s_node;
  }
  node = __builtin_amdgcn_readfirstlane(node);
  if (node == 0x7fffffff) {
    if (tid == 0) {
      a.ws_count[id]     = 0;
      a.ws_nonfinite[id] = 0;
    }
    return;
  }
  const double* X = a.graph_X + ((size_t) b * a.node_stride + node) * 16;
  bool keep = false, bad = false;
  if (r < np) {
    const WorldRow w = world_row(a, in, X);
    keep             = w.passes && w.finite;
    bad              = w.passes && !w.finite;
  }
  const int kept_wave = __popcll(__ballot(keep)), bad_wave = __popcll(__ballot(bad));
  if ((tid & (PRS_WAVE - 1)) == 0) {
    s_kept[tid >> 6] = kept_wave;
    s_bad[tid >> 6]  = bad_wave;
  }
  __syncthreads();
  if (tid == 0) {
    int k = 0, n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      k += s_kept[w];
      n += s_bad[w];
    }
    a.ws_count[id]     = k;
    a.ws_nonfinite[id] = n;
  }
}

// ---- scan: one workgroup per sequence, of 64 .. kWideThreads threads as node_stride asks ------------------------------------------
__global__ __launch_bounds__(kWideThreads) void world_map_scan_kernel(const WorldMapArgs a) {
  __shared__ uint64_t s_scan[17];
  const int tid = threadIdx.x, threads = blockDim.x, b = blockIdx.x;
  const int M = a.maps, C = a.chunks, S = a.slot_stride;
  int32_t* node_of = a.ws_node + (size_t) b * M;
  const int nn = a.n_nodes[b], cur = a.cur_node[b];
  const bool use_live = a.p.include_live != 0;
  int bad             = nn < 1 || nn > a.node_stride || cur < 0 || cur >= nn;
  if (!bad && use_live) {
    const int lp = a.live_n_points[b];
    bad          = lp < 0 || lp > a.capacity;
  }
  for (int m = tid; m < M; m += threads) {
    node_of[m] = -1;
  }
  __syncthreads();
  const int32_t* son = a.slot_of_node + (size_t) b * a.node_stride;
  if (!bad) {
    // every used node claims its slot; a slot claimed twice refuses the sequence (its rows would be written twice by refresh_state).
    // The exchange only decides WHETHER two nodes met, never which value is used: with no collision every slot has one claimant
    for (int n = tid; n < nn; n += threads) {
      if (use_live && n == cur) {
        node_of[S] = n;
        continue;
      }
      const int s = son[n];
      if (s < 0) {
        continue;
      }
      if (s >= S) {
        bad = 1;
        continue;
      }
      const int sp = a.ar_n_points[(size_t) b * S + s];
      if (sp < 0 || sp > a.capacity || atomicCAS(&node_of[s], -1, n) != -1) {
        bad = 1;
      }
    }
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    for (int m = tid; m < M; m += threads) {
      node_of[m] = -1;
    }
    if (tid == 0) {
      a.o.status[b]      = PRS_ERR_RANGE;
      a.o.n_out[b]       = 0;
      a.o.n_total[b]     = 0;
      a.o.n_nonfinite[b] = 0;
    }
    return;
  }
  // node order: every thread one node of a tile of `threads` nodes, the sum of its map's chunk counts scanned over the tile and carried
  // from tile to tile; the map's chunks then take consecutive bases
  uint64_t carry = 0, bad_rows = 0;
  for (int n0 = 0; n0 < nn; n0 += threads) {
    const int n = n0 + tid;
    int m       = -1;
    if (n < nn) {
      const int s = son[n];
      m           = (use_live && n == cur) ? S : (s >= 0 ? s : -1);
    }
    int32_t* cnt = a.ws_count + ((size_t) b * M + (m >= 0 ? m : 0)) * C;
    uint64_t sum = 0;
    if (m >= 0) {
      const int32_t* nf = a.ws_nonfinite + ((size_t) b * M + m) * C;
      for (int c0 = 0; c0 < C; c0 += kBatch) {
        int32_t k[kBatch], f[kBatch];
        load_counts(cnt, c0, C, k);
        load_counts(nf, c0, C, f);
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
          sum += (uint64_t) k[j];
          bad_rows += (uint64_t) f[j];
        }
      }
    }
    uint64_t tile = 0;
    uint64_t at   = carry + block_exclusive_scan_u64(sum, s_scan, tile);
    if (m >= 0) {
      for (int c0 = 0; c0 < C; c0 += kBatch) {
        int32_t k[kBatch];
        load_counts(cnt, c0, C, k);
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
          if (c0 + j < C) {
            cnt[c0 + j] = (int32_t) at;
          }
          at += (uint64_t) k[j];
        }
      }
    }
    carry += tile;
  }
  uint64_t all_bad = 0;
  (void) block_exclusive_scan_u64(bad_rows, s_scan, all_bad);
  if (tid == 0) {
    const int32_t total = (int32_t) carry;  // <= maps * capacity, which the launcher holds below 2^31
    a.o.n_total[b]      = total;
    a.o.n_nonfinite[b]  = (int32_t) all_bad;
    a.o.n_out[b]        = a.write_out ? (total < a.o.out_stride ? total : a.o.out_stride) : 0;
    a.o.status[b]       = (a.write_out && total > a.o.out_stride) ? PRS_ERR_CAPACITY : PRS_OK;
  }
}

// ---- scatter: blockIdx.x = (b * maps + m) * chunks + c ------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void world_map_scatter_kernel(const WorldMapArgs a) {
  __shared__ int s_kept[kWaves];
  __shared__ float s_lo[kWaves][3], s_hi[kWaves][3];
  const int tid     = threadIdx.x;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), m = (int) ((id / (uint32_t) a.chunks) % (uint32_t) a.maps);
  const int b = (int) (id / ((uint32_t) a.chunks * (uint32_t) a.maps));
  const int node = __builtin_amdgcn_readfirstlane(a.ws_node[(size_t) b * a.maps + m]);
  if (node < 0) {
    return;  // not chosen, or the sequence is refused: the bounds pass skips the entry too
  }
  const bool want_bounds = a.write_out && a.o.bounds != nullptr;
  // the scan has held n_points inside [0, capacity]
  const int np = m == a.slot_stride ? a.live_n_points[b] : a.ar_n_points[(size_t) b * a.slot_stride + m];
  if (c * kChunk >= np) {
    if (want_bounds && tid < 6) {
      a.ws_bounds[(size_t) id * 6 + tid] = tid < 3 ? INFINITY : -INFINITY;
    }
    return;
  }
  const MapRows rows = map_rows(a, b, m);
  const double* X    = a.graph_X + ((size_t) b * a.node_stride + node) * 16;
  const int r        = c * kChunk + tid;
  const int lane = tid & (PRS_WAVE - 1), wave = tid >> 6;
  bool keep = false;
  WorldRow w = {};
  if (r < np) {
    w    = world_row(a, row_in(rows, r), X);
    keep = w.passes && w.finite;
    if (a.p.refresh_state && w.finite) {
      float4 st     = rows.state[r];
      st.x          = w.wx;
      st.y          = w.wy;
      st.z          = w.wz;
      rows.state[r] = st;
    }
  }
  if (!a.write_out) {
    return;
  }
  const int pos      = chunk_position(__ballot(keep), s_kept, a.ws_count + id);
  const bool written = keep && pos < a.o.out_stride;
  if (written) {
    const size_t at                                = (size_t) b * a.o.out_stride + pos;
    reinterpret_cast<float4*>(a.o.xyz)[at]         = make_float4(w.wx, w.wy, w.wz, w.c.w);
    if (a.o.desc) {
      const uint4 d0 = rows.desc[2 * (size_t) r], d1 = rows.desc[2 * (size_t) r + 1];
      uint4* od      = reinterpret_cast<uint4*>(a.o.desc) + 2 * at;
      od[0]          = d0;
      od[1]          = d1;
    }
    if (a.o.node) {
      a.o.node[at] = node;
    }
    if (a.o.row) {
      a.o.row[at] = r;
    }
    if (a.o.n_opt) {
      a.o.n_opt[at] = w.n_opt;
    }
  }
  if (!want_bounds) {
    return;
  }
  // + 0.0f turns -0 into +0: min and max then have one answer whatever the order of the reduction
  float lo[3], hi[3];
  const float v[3] = {w.wx + 0.0f, w.wy + 0.0f, w.wz + 0.0f};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    lo[i] = written ? v[i] : INFINITY;
    hi[i] = written ? v[i] : -INFINITY;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      lo[i] = fminf(lo[i], __shfl_xor(lo[i], d, PRS_WAVE));
      hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], d, PRS_WAVE));
    }
    if (lane == 0) {
      s_lo[wave][i] = lo[i];
      s_hi[wave][i] = hi[i];
    }
  }
  __syncthreads();
  if (tid < 6) {
    const int i = tid % 3;
    float r6    = tid < 3 ? s_lo[0][i] : s_hi[0][i];
#pragma unroll
    for (int v2 = 1; v2 < kWaves; ++v2) {
      r6 = tid < 3 ? fminf(r6, s_lo[v2][i]) : fmaxf(r6, s_hi[v2][i]);
    }
    a.ws_bounds[(size_t) id * 6 + tid] = r6;
  }
}

// ---- bounds: one workgroup per sequence, of 64 .. kWideThreads threads as maps * chunks asks ---------------------------------------
__global__ __launch_bounds__(kWideThreads) void world_map_bounds_kernel(const WorldMapArgs a) {
  __shared__ float s_lo[kWideThreads / PRS_WAVE][3], s_hi[kWideThreads / PRS_WAVE][3];
  const int tid = threadIdx.x, threads = blockDim.x, b = blockIdx.x;
  if (a.o.status[b] == PRS_ERR_RANGE) {
    return;  // a refused sequence writes its status and counts only
  }
  const int M = a.maps, C = a.chunks;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int e = tid; e < M * C; e += threads) {
    // 24 bytes at a multiple of 24: three 8-byte loads, issued with the node's before any of them is looked at.  A chunk of a map
    // that was not chosen holds whatever the workspace held: read, then set aside
    const int node  = a.ws_node[(size_t) b * M + e / C];
    const float2* q = reinterpret_cast<const float2*>(a.ws_bounds + ((size_t) b * M * C + e) * 6);
    const float2 q0 = q[0], q1 = q[1], q2 = q[2];
    if (node >= 0) {
      lo[0] = fminf(lo[0], q0.x), lo[1] = fminf(lo[1], q0.y), lo[2] = fminf(lo[2], q1.x);
      hi[0] = fmaxf(hi[0], q1.y), hi[1] = fmaxf(hi[1], q2.x), hi[2] = fmaxf(hi[2], q2.y);
    }
  }
  const int lane = tid & (PRS_WAVE - 1), wave = tid >> 6, waves = threads >> 6;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      lo[i] = fminf(lo[i], __shfl_xor(lo[i], d, PRS_WAVE));
      hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], d, PRS_WAVE));
    }
    if (lane == 0) {
      s_lo[wave][i] = lo[i];
      s_hi[wave][i] = hi[i];
    }
  }
  __syncthreads();
  if (tid < 6) {
    const int i = tid % 3;
    float r6    = tid < 3 ? s_lo[0][i] : s_hi[0][i];
    for (int v = 1; v < waves; ++v) {
      r6 = tid < 3 ? fminf(r6, s_lo[v][i]) : fmaxf(r6, s_hi[v][i]);
    }
    a.o.bounds[(size_t) b * 6 + tid] = r6;
  }
}

// entries of 4 bytes in the workspace, 0 when the shape is not one the launcher takes
uint64_t workspace_words(const int64_t batch, const int64_t slot_stride, const int64_t capacity) {
  if (batch < 1 || slot_stride < 1 || capacity < 1) {
    return 0;
  }
  const uint64_t maps = (uint64_t) slot_stride + 1, chunks = ((uint64_t) capacity + kChunk - 1) / kChunk;
  return (uint64_t) batch * maps * (chunks * 8 + 1);
}

}  // namespace

int world_map_launch(prs_context* ctx, const prs_world_map_params* params, const prs_session_batch* session, const prs_merge_batch* maps,
                     const prs_map_archive* archive, const prs_world_map_batch* out) {
  const std::string who = "prs_world_map_batch_run";
  if (!params || !session || !maps || !archive || !out) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_session_batch& s = *session;
  const prs_map_archive& ar  = *archive;
  const prs_world_map_batch& o = *out;
  const bool refresh = params->refresh_state != 0;
  if (!s.coords || !s.desc || !s.n_points || !s.graph_X || !s.n_nodes || !s.cur_node || !maps->n_opt || !maps->inlier || !ar.coords ||
      !ar.desc || !ar.n_opt || !ar.inlier || !ar.n_points || !ar.slot_of_node || !o.n_out || !o.n_total || !o.n_nonfinite || !o.status ||
      !o.workspace || (refresh && (!ar.state || !maps->state))) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": an input array, a count, the status or the workspace not set (state too, with refresh_state)").c_str());
  }
  if (s.batch < 1 || s.capacity < 1 || s.node_stride < 1 || ar.slot_stride < 1 || ar.batch != s.batch || maps->batch != s.batch ||
      ar.capacity != s.capacity || maps->capacity != s.capacity || ar.node_stride != s.node_stride || o.out_stride < 0 ||
      (o.xyz && o.out_stride < 1)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": batch, capacity or node_stride differ between the structs or are below 1, slot_stride below 1, or out_stride below 1 with xyz set").c_str());
  }
  if (!aligned_to(o.xyz, 16) || !aligned_to(o.desc, 16) || !aligned_to(o.workspace, 16) || !aligned_to(s.coords, 16) || !aligned_to(s.desc, 16) ||
      !aligned_to(ar.coords, 16) || !aligned_to(ar.desc, 16) || (refresh && (!aligned_to(ar.state, 16) || !aligned_to(maps->state, 16))) ||
      !aligned_to(s.graph_X, 8) || !aligned_to(s.n_points, 4) || !aligned_to(s.n_nodes, 4) || !aligned_to(s.cur_node, 4) ||
      !aligned_to(maps->n_opt, 4) || !aligned_to(ar.n_opt, 4) || !aligned_to(ar.n_points, 4) || !aligned_to(ar.slot_of_node, 4) ||
      !aligned_to(o.node, 4) || !aligned_to(o.row, 4) || !aligned_to(o.n_opt, 4) || !aligned_to(o.n_out, 4) || !aligned_to(o.n_total, 4) ||
      !aligned_to(o.n_nonfinite, 4) || !aligned_to(o.bounds, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": xyz, desc, coords, state and the workspace must be 16-byte aligned, graph_X 8-byte, the other arrays 4-byte").c_str());
  }
  const long long M = (long long) ar.slot_stride + 1, C = ((long long) s.capacity + kChunk - 1) / kChunk;
  const long long blocks = (long long) s.batch * M * C;
  if (M * (long long) s.capacity > 0x7fffffffll) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": a sequence's rows beyond 2^31").c_str());
  }
  const auto wide  = [](long long items) { return (int) std::min<long long>(kWideThreads, (items + PRS_WAVE - 1) / PRS_WAVE * PRS_WAVE); };
  const bool write = o.xyz != nullptr;
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid chunks = on.grid(blocks, kThreads);  // count and scatter: batch * (slot_stride + 1) * chunks
  const Grid scan   = on.grid(s.batch, wide(s.node_stride));
  const Grid bounds = write && o.bounds ? on.grid(s.batch, wide(M * C)) : Grid();
  PRS_TRY(on.check());
  WorldMapArgs a = {};
  a.p = *params;
  a.o = o;
  a.batch = s.batch, a.capacity = s.capacity, a.node_stride = s.node_stride, a.slot_stride = ar.slot_stride;
  a.maps = (int32_t) M, a.chunks = (int32_t) C;
  a.write_out     = write;
  a.live_coords   = s.coords;
  a.live_desc     = s.desc;
  a.live_n_points = s.n_points;
  a.live_n_opt    = maps->n_opt;
  a.live_inlier   = maps->inlier;
  a.live_state    = maps->state;
  a.ar_coords     = ar.coords;
  a.ar_desc       = ar.desc;
  a.ar_n_opt      = ar.n_opt;
  a.ar_inlier     = ar.inlier;
  a.ar_state      = ar.state;
  a.ar_n_points   = ar.n_points;
  a.slot_of_node  = ar.slot_of_node;
  a.graph_X       = s.graph_X;
  a.n_nodes       = s.n_nodes;
  a.cur_node      = s.cur_node;
  int32_t* ws     = static_cast<int32_t*>(o.workspace);
  a.ws_count      = ws;
  a.ws_nonfinite  = ws + blocks;
  a.ws_bounds     = reinterpret_cast<float*>(ws + 2 * blocks);
  a.ws_node       = ws + 8 * blocks;
  on.launch(world_map_count_kernel, chunks, 0, a);
  on.launch(world_map_scan_kernel, scan, 0, a);
  if (write || refresh) {
    on.launch(world_map_scatter_kernel, chunks, 0, a);
  }
  if (bounds) {
    on.launch(world_map_bounds_kernel, bounds, 0, a);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_world_map_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_world_map_params);
  sizes2[1] = sizeof(prs_world_map_batch);
}

uint64_t prs_world_map_workspace_bytes(int32_t batch, int32_t slot_stride, int32_t capacity) {
  return (workspace_words(batch, slot_stride, capacity) * 4 + 15) & ~(uint64_t) 15;
}

int prs_world_map_batch_run(prs_context* ctx, const prs_world_map_params* params, const prs_session_batch* session,
                            const prs_merge_batch* maps, const prs_map_archive* archive, const prs_world_map_batch* out) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return world_map_launch(ctx, params, session, maps, archive, out);
}

}  // extern "C"
