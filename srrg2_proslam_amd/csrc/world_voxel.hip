// world_voxel.hip -- the voxel-grid filter of a world-frame landmark cloud on the device: the rows of one cubic voxel are fused into
// one row, the voxel's representative (prs_world_voxel_batch_run; the rule is stated in include/proslam_hip.h, BUILD-DEFINED, and
// restated in tests/world_voxel_ref.py).  A hash table per sequence in the caller's workspace, then the stable stream compaction of
// world_map.hip over the representatives:
//   clear    the tables: keys empty, ranks all ones, counts and sums zero; the per-sequence drop counters
//   insert   one thread per row: voxel key, linear probing with compare-and-swap, then min on the rank, add on the count and, MEAN
//            only, on the three integer sums; the row's slot goes to the workspace
//   flag     one workgroup per chunk: a row is its voxel's representative when the slot's rank names it; the chunk's count
//   scan     one workgroup per sequence: validation, table overflow, chunk bases (an exclusive scan), the per-sequence outputs
//   scatter  one workgroup per chunk: positions from wave ballots and the scanned base; writes the voxels
// The atomics are integer min, add and compare-and-swap: each result is the same whatever the order they arrive in.  WHICH slot a
// voxel lands in may differ from run to run, no output byte does: positions come from the input order alone.
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
constexpr int kChunk   = kThreads;  // rows (insert, flag, scatter) or slots (clear) per workgroup
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kWideThreads = 1024;  // the scan at one long sequence
constexpr unsigned long long kEmpty = ~0ull;
constexpr double kHalfGrid = 1048576.0;     // 2^20 voxels either side of the origin
constexpr double kFraction = 1073741824.0;  // 2^30 steps inside a voxel

// one slot of a table: 48 bytes, three 16-byte stores to clear
struct Slot {
  unsigned long long key;   // kEmpty, or the voxel key (< 2^63)
  unsigned long long rank;  // min over the voxel's rows of (~n_opt << 32) | i
  long long sum[3];         // MEAN: the sums of q_a
  int32_t count;            // rows of the voxel
  int32_t pad;
};
static_assert(sizeof(Slot) == 48, "three 16-byte stores clear a slot");

// per-sequence counters of the insert kernel
struct Drops {
  int32_t nonfinite, outside, failed, pad;
};

struct WorldVoxelArgs {
  prs_world_voxel_params p;
  prs_world_voxel_batch o;
  int32_t chunks;        // chunks of rows per sequence
  int32_t table_chunks;  // chunks of slots per sequence
  int32_t write_out;
  Slot* table;        // [batch][table_stride]
  Drops* drops;       // [batch]
  int32_t* ws_slot;   // [batch][in_stride] slot of the row, -1 = dropped, -2 = the table is full of other voxels
  int32_t* ws_count;  // [batch][chunks] representatives of the chunk; after the scan: the chunk's first output row, -1 = keep out
};

// the voxel of a row: k_a as float64 (integers), the key, and why a row has none
struct Voxel {
  double k[3];
  unsigned long long key;
  bool finite, inside;
};

__device__ __forceinline__ Voxel voxel_of(const float4 c, const double s) {
  Voxel v;
  v.finite = finite_bits(c.x) && finite_bits(c.y) && finite_bits(c.z);
  v.k[0]   = floor((double) c.x / s);
  v.k[1]   = floor((double) c.y / s);
  v.k[2]   = floor((double) c.z / s);
  v.inside = v.finite;
  v.key    = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v.inside = v.inside && v.k[a] >= -kHalfGrid && v.k[a] < kHalfGrid;
  }
  if (v.inside) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v.key = (v.key << 21) | (unsigned long long) ((long long) v.k[a] + 1048576ll);
    }
  }
  return v;
}

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// ---- clear: blockIdx.x = b * table_chunks + c; the 768 16-byte words of 256 slots, thread t the words t, t + 256, t + 512 ----------
__global__ __launch_bounds__(kThreads) void world_voxel_clear_kernel(const WorldVoxelArgs a) {
  const int tid     = threadIdx.x;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.table_chunks), b = (int) (id / (uint32_t) a.table_chunks);
  const int T       = a.o.table_stride;
  const int slots   = min(kChunk, T - c * kChunk);
  uint4* words      = reinterpret_cast<uint4*>(a.table + (size_t) b * T + (size_t) c * kChunk);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int w = tid + j * kThreads;
    if (w < 3 * slots) {
      const uint32_t v = (w % 3 == 0) ? ~0u : 0u;  // word 0 of a slot: key and rank
      words[w]         = make_uint4(v, v, v, v);
    }
  }
  if (c == 0 && tid == 0) {
    *reinterpret_cast<uint4*>(a.drops + b) = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---- insert: blockIdx.x = b * chunks + c --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void world_voxel_insert_kernel(const WorldVoxelArgs a) {
  const int tid     = threadIdx.x;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), b = (int) (id / (uint32_t) a.chunks);
  const int N = a.o.in_stride, T = a.o.table_stride;
  const int n = a.o.in_n[b];
  if (n < 0 || n > N || c * kChunk >= n) {
    return;  // a refused sequence, or a chunk behind the rows: the scan keeps the later kernels away from what is not written here
  }
  const int i = c * kChunk + tid;
  bool nonfinite = false, outside = false, failed = false;
  if (i < n) {
    const size_t at      = (size_t) b * N + i;
    const float4 x       = reinterpret_cast<const float4*>(a.o.in_xyz)[at];
    const uint32_t n_opt = a.o.in_n_opt ? a.o.in_n_opt[at] : 0u;
    const double s       = (double) a.p.voxel_size;
    const Voxel v        = voxel_of(x, s);
    nonfinite            = !v.finite;
    outside              = v.finite && !v.inside;
    int slot             = -1;
    if (v.inside) {
      Slot* table   = a.table + (size_t) b * T;
      uint32_t at_s = (uint32_t) mix64(v.key) & (uint32_t) (T - 1);
      slot          = -2;
      // every slot is visited once: the insertion fails only when all T slots hold other keys
      for (int probe = 0; probe < T; ++probe) {
        const unsigned long long was = atomicCAS(&table[at_s].key, kEmpty, v.key);
        if (was == kEmpty || was == v.key) {
          slot = (int) at_s;
          break;
        }
        at_s = (at_s + 1u) & (uint32_t) (T - 1);
      }
      failed = slot < 0;
      if (!failed) {
        Slot* t = table + slot;
        atomicMin(&t->rank, ((unsigned long long) ~n_opt << 32) | (unsigned long long) (uint32_t) i);
        atomicAdd(&t->count, 1);
        if (a.p.position == PRS_VOXEL_MEAN) {
          const float xa[3] = {x.x, x.y, x.z};
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) {
            const double f    = (double) xa[ax] - v.k[ax] * s;
            const long long q = (long long) rint((f / s) * kFraction);
            atomicAdd(reinterpret_cast<unsigned long long*>(&t->sum[ax]), (unsigned long long) q);  // two's complement: the signed sum
          }
        }
      }
    }
    a.ws_slot[at] = slot;
  }
  // one add per wave and counter, and none for a wave that dropped nothing
  const int wave_nonfinite = __popcll(__ballot(nonfinite)), wave_outside = __popcll(__ballot(outside)), wave_failed = __popcll(__ballot(failed));
  if ((tid & (PRS_WAVE - 1)) == 0) {
    Drops* d = a.drops + b;
    if (wave_nonfinite) {
      atomicAdd(&d->nonfinite, wave_nonfinite);
    }
    if (wave_outside) {
      atomicAdd(&d->outside, wave_outside);
    }
    if (wave_failed) {
      atomicAdd(&d->failed, wave_failed);
    }
  }
}

// row i of sequence b is the representative of its voxel
__device__ __forceinline__ bool is_representative(const WorldVoxelArgs& a, const int b, const int i, int& slot) {
  slot = a.ws_slot[(size_t) b * a.o.in_stride + i];
  return slot >= 0 && (uint32_t) a.table[(size_t) b * a.o.table_stride + slot].rank == (uint32_t) i;
}

// ---- flag and count: blockIdx.x = b * chunks + c ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void world_voxel_flag_kernel(const WorldVoxelArgs a) {
  __shared__ int s_wave[kWaves];
  const int tid     = threadIdx.x;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), b = (int) (id / (uint32_t) a.chunks);
  const int n = a.o.in_n[b];
  if (n < 0 || n > a.o.in_stride || c * kChunk >= n) {
    if (tid == 0) {
      a.ws_count[id] = 0;
    }
    return;
  }
  const int i = c * kChunk + tid;
  int slot;
  const bool rep  = i < n && is_representative(a, b, i, slot);
  const int reps  = __popcll(__ballot(rep));
  if ((tid & (PRS_WAVE - 1)) == 0) {
    s_wave[tid >> 6] = reps;
  }
  __syncthreads();
  if (tid == 0) {
    int k = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      k += s_wave[w];
    }
    a.ws_count[id] = k;
  }
}

// ---- scan: one workgroup per sequence, of 64 .. kWideThreads threads as the chunks ask ---------------------------------------------
__global__ __launch_bounds__(kWideThreads) void world_voxel_scan_kernel(const WorldVoxelArgs a) {
  __shared__ uint64_t s_scan[17];
  const int tid = threadIdx.x, threads = blockDim.x, b = blockIdx.x;
  const int C   = a.chunks;
  int32_t* cnt  = a.ws_count + (size_t) b * C;
  const int n   = a.o.in_n[b];
  const bool refused = n < 0 || n > a.o.in_stride;
  const Drops d      = a.drops[b];
  if (refused || d.failed != 0) {
    for (int c = tid; c < C; c += threads) {
      cnt[c] = -1;
    }
    if (tid == 0) {
      a.o.status[b]      = refused ? PRS_ERR_RANGE : PRS_ERR_CAPACITY;
      a.o.n_out[b]       = 0;
      a.o.n_voxels[b]    = refused ? 0 : -1;
      a.o.n_nonfinite[b] = refused ? 0 : d.nonfinite;
      a.o.n_outside[b]   = refused ? 0 : d.outside;
    }
    return;
  }
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
        cnt[c0 + j] = (int32_t) at;
      }
      at += (uint64_t) k[j];
    }
    carry += tile;
  }
  if (tid == 0) {
    const int32_t total = (int32_t) carry;  // <= in_stride
    a.o.n_voxels[b]     = total;
    a.o.n_nonfinite[b]  = d.nonfinite;
    a.o.n_outside[b]    = d.outside;
    a.o.n_out[b]        = a.write_out ? (total < a.o.out_stride ? total : a.o.out_stride) : 0;
    a.o.status[b]       = (a.write_out && total > a.o.out_stride) ? PRS_ERR_CAPACITY : PRS_OK;
  }
}

// ---- scatter: blockIdx.x = b * chunks + c -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void world_voxel_scatter_kernel(const WorldVoxelArgs a) {
  __shared__ int s_wave[kWaves];
  const int tid     = threadIdx.x;
  const uint32_t id = blockIdx.x;
  const int c = (int) (id % (uint32_t) a.chunks), b = (int) (id / (uint32_t) a.chunks);
  if (__builtin_amdgcn_readfirstlane(a.ws_count[id]) < 0) {
    return;  // the sequence is refused, or its table overflowed
  }
  const int N = a.o.in_stride;
  const int n = a.o.in_n[b];  // the scan has held it inside [0, in_stride]
  if (c * kChunk >= n) {
    return;
  }
  const int i = c * kChunk + tid;
  int slot    = -1;
  const bool rep = i < n && is_representative(a, b, i, slot);
  const int pos  = chunk_position(__ballot(rep), s_wave, a.ws_count + id);
  if (!rep || pos >= a.o.out_stride) {
    return;
  }
  const size_t from = (size_t) b * N + i, at = (size_t) b * a.o.out_stride + pos;
  const Slot* t     = a.table + (size_t) b * a.o.table_stride + slot;
  const int count   = t->count;
  float4 x          = reinterpret_cast<const float4*>(a.o.in_xyz)[from];
  if (a.p.position == PRS_VOXEL_MEAN) {
    const double s = (double) a.p.voxel_size;
    const Voxel v  = voxel_of(x, s);
    float m[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const double mean = (double) t->sum[ax] / (double) count;
      m[ax]             = (float) ((v.k[ax] + mean / kFraction) * s);
    }
    x.x = m[0], x.y = m[1], x.z = m[2];
  }
  reinterpret_cast<float4*>(a.o.xyz)[at] = x;
  if (a.o.index) {
    a.o.index[at] = i;
  }
  if (a.o.count) {
    a.o.count[at] = count;
  }
  if (a.o.desc && a.o.in_desc) {
    const uint4* id4 = reinterpret_cast<const uint4*>(a.o.in_desc) + 2 * from;
    const uint4 d0 = id4[0], d1 = id4[1];
    uint4* od      = reinterpret_cast<uint4*>(a.o.desc) + 2 * at;
    od[0]          = d0;
    od[1]          = d1;
  }
  if (a.o.node && a.o.in_node) {
    a.o.node[at] = a.o.in_node[from];
  }
  if (a.o.row && a.o.in_row) {
    a.o.row[at] = a.o.in_row[from];
  }
  if (a.o.n_opt && a.o.in_n_opt) {
    a.o.n_opt[at] = a.o.in_n_opt[from];
  }
}

long long chunks_of(const long long items) {
  return (items + kChunk - 1) / kChunk;
}

// bytes of the workspace's parts, 0 when a size is not one the launcher takes
struct Layout {
  uint64_t table, drops, slots, counts;
};

Layout layout_of(const int64_t batch, const int64_t in_stride, const int64_t table_stride) {
  Layout l = {};
  if (batch < 1 || in_stride < 1 || table_stride < 1) {
    return l;
  }
  l.table  = (uint64_t) batch * (uint64_t) table_stride * sizeof(Slot);
  l.drops  = (uint64_t) batch * sizeof(Drops);
  l.slots  = (uint64_t) batch * (uint64_t) in_stride * 4;
  l.counts = (uint64_t) batch * (uint64_t) chunks_of(in_stride) * 4;
  return l;
}

}  // namespace

int world_voxel_launch(prs_context* ctx, const prs_world_voxel_params* params, const prs_world_voxel_batch* batch) {
  const std::string who = "prs_world_voxel_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_world_voxel_batch& o = *batch;
  if (!o.in_xyz || !o.in_n || !o.n_out || !o.n_voxels || !o.n_nonfinite || !o.n_outside || !o.status || !o.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": in_xyz, in_n, a per-sequence output or the workspace not set").c_str());
  }
  const bool pow2 = o.table_stride >= 1 && (o.table_stride & (o.table_stride - 1)) == 0;
  if (o.batch < 1 || o.in_stride < 1 || !pow2 || !(params->voxel_size > 0.0f) || !std::isfinite(params->voxel_size) ||
      (params->position != PRS_VOXEL_REPRESENTATIVE && params->position != PRS_VOXEL_MEAN) || (o.xyz && o.out_stride < 1)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": batch or in_stride below 1, table_stride not a power of two, voxel_size not finite and positive, an unknown position, or out_stride below 1 with xyz set").c_str());
  }
  if (!aligned_to(o.in_xyz, 16) || !aligned_to(o.in_desc, 16) || !aligned_to(o.xyz, 16) || !aligned_to(o.desc, 16) || !aligned_to(o.workspace, 16) ||
      !aligned_to(o.in_n, 4) || !aligned_to(o.in_n_opt, 4) || !aligned_to(o.in_node, 4) || !aligned_to(o.in_row, 4) || !aligned_to(o.index, 4) ||
      !aligned_to(o.count, 4) || !aligned_to(o.node, 4) || !aligned_to(o.row, 4) || !aligned_to(o.n_opt, 4) || !aligned_to(o.n_out, 4) ||
      !aligned_to(o.n_voxels, 4) || !aligned_to(o.n_nonfinite, 4) || !aligned_to(o.n_outside, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": xyz, desc (in and out) and the workspace must be 16-byte aligned, the other arrays 4-byte").c_str());
  }
  const long long C = chunks_of(o.in_stride), TC = chunks_of(o.table_stride);
  const long long blocks = (long long) o.batch * C, clear_blocks = (long long) o.batch * TC;
  const int wide = (int) std::min<long long>(kWideThreads, ((C + kCompactBatch - 1) / kCompactBatch + PRS_WAVE - 1) / PRS_WAVE * PRS_WAVE);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid clear = on.grid(clear_blocks, kThreads), chunks = on.grid(blocks, kThreads);  // (chunks: insert, flag and scatter)
  const Grid scan  = on.grid(o.batch, wide);
  PRS_TRY(on.check());
  WorldVoxelArgs a = {};
  a.p = *params;
  a.o = o;
  a.chunks = (int32_t) C, a.table_chunks = (int32_t) TC;
  a.write_out    = o.xyz != nullptr;
  const Layout l = layout_of(o.batch, o.in_stride, o.table_stride);
  uint8_t* ws    = static_cast<uint8_t*>(o.workspace);
  a.table        = reinterpret_cast<Slot*>(ws);
  a.drops        = reinterpret_cast<Drops*>(ws + l.table);
  a.ws_slot      = reinterpret_cast<int32_t*>(ws + l.table + l.drops);
  a.ws_count     = reinterpret_cast<int32_t*>(ws + l.table + l.drops + l.slots);
  on.launch(world_voxel_clear_kernel, clear, 0, a);
  on.launch(world_voxel_insert_kernel, chunks, 0, a);
  on.launch(world_voxel_flag_kernel, chunks, 0, a);
  on.launch(world_voxel_scan_kernel, scan, 0, a);
  if (a.write_out) {
    on.launch(world_voxel_scatter_kernel, chunks, 0, a);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_world_voxel_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_world_voxel_params);
  sizes2[1] = sizeof(prs_world_voxel_batch);
}

uint64_t prs_world_voxel_workspace_bytes(int32_t batch, int32_t in_stride, int32_t table_stride) {
  const Layout l = layout_of(batch, in_stride, table_stride);
  return (l.table + l.drops + l.slots + l.counts + 15) & ~(uint64_t) 15;
}

int prs_world_voxel_batch_run(prs_context* ctx, const prs_world_voxel_params* params, const prs_world_voxel_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return world_voxel_launch(ctx, params, batch);
}

}  // extern "C"
