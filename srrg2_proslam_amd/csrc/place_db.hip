// place_db.hip -- the loop detector's candidate search on the device: CorrespondenceFinderHBST_::compute
// (registration/correspondence_finders/correspondence_finder_hbst.cpp:5-91, correspondences :95-127) against a descriptor database of
// every earlier local map (include/proslam_hip.h, prs_place_db_* / prs_place_query_batch).
//
// The database (BUILD-DEFINED substitution for srrg_hbst::BinaryTree256, which is not in the tree) is searched EXHAUSTIVELY: every
// stored descriptor within the threshold counts.  Storage: the stored descriptors of the maps one after another, each map padded to a
// multiple of 16 rows, so that a 16-row tile of the database never spans two maps (tile_map[] names its map, row_pidx[] the point index
// of a row in its map, -1 on a pad row).
//
// One query batch is three launches on the context's stream:
//   place_init_kernel    match counts [batch][maps] <- 0, best keys [batch][rows] <- ~0.
//   place_score_kernel   grid (database slices of 1024 rows, query blocks of 256 rows, batch).  A wave owns 64 query rows (4 A tiles,
//                        expanded once into registers as 0 / 1 bytes), the workgroup walks its database slice in chunks of 64 rows that
//                        all four waves expand into LDS as +1 / -1 bytes; a 16 x 16 tile of distances is prs_hamming_tile.h's four
//                        v_mfma_i32_16x16x64_i8 per A tile.  A pair (q, r) matches iff q is a Valid query point and d < lim.  Per
//                        database row the best (distance, query index) is one packed atomicMin key (distance << 23 | q): integer, so
//                        the result does not depend on the order the waves arrive in.  The match count of a map is summed in a scalar
//                        register from the ballots of its tiles and added with one atomic per (wave, map run).
//   place_select_kernel  one workgroup per query: index_query (the stored index of the query's graph id, else the number of maps), the
//                        age and inlier rules, the candidates in ascending map index (capped at max_candidates), and per candidate the
//                        correspondences: every row of the map with a key, in ascending row = ascending reference point index.
// prs_place_gather_pairs adds a fourth (place_gather_kernel): the pair slots of a loop-closure batch from the candidate lists.
//
// The place bank (prs_place_bank_*) is B such databases in fixed device arenas, one per sequence, whose sizes are device counters.
// Its query is the same three launches (place_bank_init / _score / _select_kernel) over grids sized by capacity; the bodies of the
// score, select and gather kernels are device functions over a per-sequence view, shared by both forms.  place_bank_append_kernel
// stores a finished map from the session's hand-over slot as prs_place_db_add would, one workgroup per sequence.
#include <string.h>

#include <cmath>
#include <unordered_map>
#include <vector>

#include "prs_device.h"
#include "prs_hamming_tile.h"
#include "prs_host.h"

struct prs_place_db {
  prs_context* ctx = nullptr;
  int32_t maps = 0, rows = 0, max_map_rows = 0;
  int32_t map_cap = 0, row_cap = 0;  // device capacities (rows: a multiple of 16)
  uint8_t* desc      = nullptr;      // [row_cap][32]
  float* xyz         = nullptr;      // [row_cap][4]
  int32_t* row_pidx  = nullptr;      // [row_cap]
  int32_t* tile_map  = nullptr;      // [row_cap / 16]
  int32_t* map_off   = nullptr;      // [map_cap] first row
  int32_t* map_rows  = nullptr;      // [map_cap] stored descriptors (pads excluded)
  int64_t* map_gid   = nullptr;      // [map_cap] graph id
  std::unordered_map<int64_t, int32_t> index_of;
};

// B databases in fixed arenas; the sizes live in `counters` on the device (the host knows capacities only)
struct prs_place_bank {
  prs_context* ctx = nullptr;
  int32_t batch = 0, map_stride = 0, row_stride = 0;  // row_stride: a multiple of 16
  int32_t max_query_stride = 0;   // the largest slot an append has been called with: no stored map is larger
  uint8_t* desc      = nullptr;   // [batch][row_stride][32]
  float* xyz         = nullptr;   // [batch][row_stride][4]
  int32_t* row_pidx  = nullptr;   // [batch][row_stride]
  int32_t* tile_map  = nullptr;   // [batch][row_stride / 16]
  int32_t* map_off   = nullptr;   // [batch][map_stride]
  int32_t* map_rows  = nullptr;   // [batch][map_stride]
  int64_t* map_gid   = nullptr;   // [batch][map_stride]
  int32_t* own_nodes = nullptr;   // [batch][map_stride] the bank's node_of_map
  int32_t* node_of_map = nullptr; // own_nodes, or the array prs_place_bank_bind_node_of_map named
  int32_t* counters  = nullptr;   // n_maps [batch] | n_rows [batch] | max_map_rows [batch]
};

namespace prs {

namespace {

constexpr int kPdThreads  = 256;                      // 4 waves
constexpr int kPdRowsWave = 64;                       // query rows per wave (4 A tiles)
constexpr int kPdRowsWg   = kPdRowsWave * (kPdThreads / 64);
constexpr int kPdChunk    = 64;                       // database rows per LDS chunk (4 B tiles)
constexpr int kPdSlice    = 16 * kPdChunk;            // database rows per workgroup
constexpr int kPdPlaneRow = 64 + 16;                  // a row of a plane: four K blocks of 16 B + 16 B pad (bruteforce.hip's bank layout)
constexpr int kPdPlane    = kPdChunk * kPdPlaneRow;
constexpr int kPdMaxQuery = 65536;                    // query rows per slot (the key keeps 23 bits of query index)
constexpr int kPdMaxCorrStride = 1 << 20;
constexpr uint32_t kNoKey = 0xffffffffu;

struct PlaceArgs {
  prs_place_queries q;
  prs_place_params p;
  const uint32_t* desc;  // database rows as 8 words
  const int32_t* row_pidx;
  const int32_t* tile_map;
  const int32_t* map_off;
  const int32_t* map_rows;
  const int64_t* map_gid;
  int32_t maps, rows;
  int lim;               // match iff d < lim  (== (float) d < maximum_descriptor_distance)
};

__global__ __launch_bounds__(kPdThreads) void place_init_kernel(const PlaceArgs a) {
  const size_t b  = blockIdx.y;
  const size_t i0 = (size_t) blockIdx.x * kPdThreads + threadIdx.x;
  const size_t step = (size_t) gridDim.x * kPdThreads;
  for (size_t i = i0; i < (size_t) a.rows; i += step) {
    a.q.best_keys[b * (size_t) a.q.key_stride + i] = kNoKey;
  }
  for (size_t i = i0; i < (size_t) a.maps; i += step) {
    a.q.match_counts[b * (size_t) a.q.count_stride + i] = 0u;
  }
}

__device__ __forceinline__ int clamp_n(const int n, const int stride) {
  return n < 0 ? 0 : (n > stride ? stride : n);
}

// one sequence's database and query as the scoring loop sees them: place_score_kernel fills it from the handle's arrays and host
// sizes, place_bank_score_kernel from arena b and its device counters
struct ScoreView {
  const uint32_t* desc;  // database rows as 8 words
  const int32_t* row_pidx;
  const int32_t* tile_map;
  int rows;
  const uint32_t* qdesc;  // the query's rows as 8 words
  const uint8_t* valid;   // or nullptr
  int nq;                 // clamped to the slot
  uint32_t* keys;
  uint32_t* counts;
  int lim;                // match iff d < lim
};

// the workgroup (blockIdx.x: database slice, blockIdx.y: query block) of one sequence
__device__ __forceinline__ void place_score_body(const ScoreView& a) {
  __shared__ __attribute__((aligned(256))) unsigned char bbuf[4 * kPdPlane];
  static_assert(kPdPlane % 256 == 0, "planes must not shift the banks");
  __shared__ int popm[kPdChunk];
  __shared__ int tmap[kPdChunk / 16];
  __shared__ uint32_t lut_a[16], lut_b[16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nq     = a.nq;
  const int qblock = (int) blockIdx.y * kPdRowsWg;
  const int row_begin = (int) blockIdx.x * kPdSlice;
  const int row_end   = row_begin + kPdSlice < a.rows ? row_begin + kPdSlice : a.rows;
  if (qblock >= nq || row_begin >= a.rows) {
    return;  // (block-uniform, before any barrier: a grid sized by capacity ends here past the live sizes)
  }
  if (tid < 16) {
    uint32_t v01, vpm;
    hamming_lut_entry(tid, v01, vpm);
    lut_a[tid] = v01;
    lut_b[tid] = vpm;
  }
  __syncthreads();
  const uint32_t* __restrict__ gdq = a.qdesc;
  const uint8_t* valid = a.valid;
  // ---- this wave's query rows: A[t][kb] = bits [64 kb + 16 lg, +16) of row q0 + 16 t + li (absent or not Valid: zeros) ----
  const int q0         = qblock + wave_s * kPdRowsWave;
  const bool wave_live = q0 < nq;
  bf_v4i A[4][4];
  uint64_t rowmask[16];  // accumulator (t, r) of lane l is query row q0 + 16 t + 4 (l >> 4) + r: which lanes hold a Valid one
  {
    uint32_t w[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int q  = q0 + 16 * t + (lane & 15);
      const int qr = q < nq ? q : (nq > 0 ? nq - 1 : 0);
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        w[t][kb] = gdq[8 * (size_t) qr + 2 * kb + (lane >> 5)];
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int q     = q0 + 16 * t + (lane & 15);
      const bool live = q < nq && (!valid || valid[q] != 0);
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        A[t][kb] = hamming_expand16(lut_a, live ? (w[t][kb] >> (16 * ((lane >> 4) & 1))) & 0xffffu : 0u);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qr = q0 + 16 * t + 4 * (lane >> 4) + r;
        rowmask[4 * t + r] = __ballot(qr < nq && (!valid || valid[qr] != 0));
      }
    }
  }
  uint32_t* keys   = a.keys;
  uint32_t* counts = a.counts;
  int run_map      = -1;  // the map of the tiles counted in run_count (wave-uniform)
  uint32_t run_count = 0;
  for (int c = row_begin; c < row_end; c += kPdChunk) {
    // ---- stage 64 database rows: two words per thread (row = idx >> 3, word j = idx & 7), pop(row) over its 8 lanes ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int idx = tid + kPdThreads * h, row = idx >> 3, j = idx & 7;
      const int grow   = c + row;
      const uint32_t w = grow < row_end ? a.desc[8 * (size_t) grow + j] : 0u;
      unsigned char* dst = &bbuf[(2 * (j & 1)) * kPdPlane + row * kPdPlaneRow + 16 * (j >> 1)];
      *reinterpret_cast<bf_v4i*>(dst)            = hamming_expand16(lut_b, w & 0xffffu);
      *reinterpret_cast<bf_v4i*>(dst + kPdPlane) = hamming_expand16(lut_b, w >> 16);
      int pop = __popc(w);
      pop += __shfl_xor(pop, 1, 64);
      pop += __shfl_xor(pop, 2, 64);
      pop += __shfl_xor(pop, 4, 64);
      if (j == 0) {
        popm[row] = grow < row_end && a.row_pidx[grow] >= 0 ? pop : (1 << 20);  // a pad row never meets the threshold
      }
    }
    if (tid < kPdChunk / 16) {
      tmap[tid] = c + 16 * tid < row_end ? a.tile_map[(c >> 4) + tid] : -1;
    }
    __syncthreads();
    if (wave_live) {
      const int li = lane & 15, lg = lane >> 4;
#pragma unroll 1
      for (int bt = 0; bt < kPdChunk / 16; ++bt) {
        if (c + 16 * bt >= row_end) {
          break;  // (uniform)
        }
        const int m = __builtin_amdgcn_readfirstlane(tmap[bt]);
        if (m != run_map) {
          if (run_count != 0u && lane == 0) {
            atomicAdd(&counts[run_map], run_count);
          }
          run_map   = m;
          run_count = 0u;
        }
        const unsigned char* brow = &bbuf[lg * kPdPlane + (16 * bt + li) * kPdPlaneRow];
        const int pop_b = popm[16 * bt + li];
        const int thr   = a.lim - pop_b;  // match  <=>  acc < thr
        bf_v4i B[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          B[kb] = *reinterpret_cast<const bf_v4i*>(brow + 16 * kb);
        }
        bf_v4i acc[4];
        hamming_tiles(A, B, acc);
        const int grow = c + 16 * bt + li;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int v[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint64_t hit = __ballot(v[r] < thr) & rowmask[4 * t + r];
            if (hit != 0ull) {  // (uniform)
              run_count += (uint32_t) __popcll(hit);
              if ((hit >> lane) & 1ull) {
                const uint32_t q = (uint32_t) (q0 + 16 * t + 4 * lg + r);
                atomicMin(&keys[grow], ((uint32_t) (v[r] + pop_b) << 23) | q);
              }
            }
          }
        }
      }
    }
    __syncthreads();  // (the chunk is consumed before the next one is staged over it)
  }
  if (run_count != 0u && lane == 0) {
    atomicAdd(&counts[run_map], run_count);
  }
}

__device__ __forceinline__ ScoreView score_view_of_query(const prs_place_queries& q, const size_t b, const int lim) {
  ScoreView v;
  v.qdesc  = reinterpret_cast<const uint32_t*>(q.desc + b * (size_t) q.query_stride * PRS_DESC_BYTES);
  v.valid  = q.valid ? q.valid + b * (size_t) q.query_stride : nullptr;
  v.nq     = clamp_n(q.n_query[b], q.query_stride);
  v.keys   = q.best_keys + b * (size_t) q.key_stride;
  v.counts = q.match_counts + b * (size_t) q.count_stride;
  v.lim    = lim;
  return v;
}

__global__ __launch_bounds__(kPdThreads) void place_score_kernel(const PlaceArgs a) {
  ScoreView v  = score_view_of_query(a.q, blockIdx.z, a.lim);
  v.desc       = a.desc;
  v.row_pidx   = a.row_pidx;
  v.tile_map   = a.tile_map;
  v.rows       = a.rows;
  place_score_body(v);
}

// the query's status word: 0, PRS_WARN_EMPTY_INPUT (the reference's "query descriptor vector is empty", :13-18), or a PRS_ERR_* code
__device__ __forceinline__ int query_status(const prs_place_queries& q, const size_t b) {
  const int n = q.n_query[b];
  if (q.graph_id[b] < 0 || n < 0) {
    return PRS_ERR_RANGE;
  }
  if (n > q.query_stride) {
    return PRS_ERR_CAPACITY;
  }
  return n == 0 ? PRS_WARN_EMPTY_INPUT : 0;
}

// one sequence's maps as the selection sees them, and the bank's optional link outputs (all nullptr for a prs_place_db)
struct SelectView {
  int maps;
  const int64_t* map_gid;
  const int32_t* map_off;
  const int32_t* map_rows;
  const int32_t* row_pidx;
  int32_t* cand_flat;    // [max_candidates] of this query, or nullptr
  int32_t flat_base;     // b * map_stride
  int32_t* query_node;   // this query's word, or nullptr
  int64_t graph_id_base;
};

// kBank: the live sizes are not known at the call, so a candidate map larger than corr_stride is refused here
template <bool kBank>
__device__ __forceinline__ void place_select_body(const prs_place_queries& q, const prs_place_params& p, const SelectView& a, const size_t b) {
  __shared__ int s_index;
  __shared__ int s_ncand;
  __shared__ int s_cand[256];  // candidates of the query (max_candidates <= 256)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int maxc   = p.max_candidates;
  int status       = query_status(q, b);
  // index_query (:47-55): the stored index of the query's graph id, else the number of maps
  if (tid == 0) {
    s_index = a.maps;
  }
  __syncthreads();
  const int64_t gid = q.graph_id[b];
  for (int m = tid; m < a.maps; m += kPdThreads) {
    if (a.map_gid[m] == gid) {
      atomicMin(&s_index, m);
    }
  }
  __syncthreads();
  const uint64_t index_query = (uint64_t) s_index;
  // the candidates in ascending map index (:70-90), by one wave
  if (wave == 0) {
    const uint32_t* counts = q.match_counts + b * (size_t) q.count_stride;
    int total = 0;
    if (status >= 0 && status != PRS_WARN_EMPTY_INPUT) {
      for (int base = 0; base < a.maps; base += 64) {
        const int m = base + lane;
        bool pass   = false;
        if (m < a.maps) {
          const uint64_t ref  = (uint64_t) m;
          const uint64_t diff = index_query - ref;  // uint64_t: wraps when the query is older than the reference
          pass = (double) diff > (double) p.minimum_age_difference_to_candidates && p.relocalize_min_inliers >= 0 &&
                 counts[m] > (uint32_t) p.relocalize_min_inliers;
        }
        const uint64_t mk = __ballot(pass);
        const int pos = total + (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mk, 0u));
        if (pass && pos < maxc) {
          s_cand[pos] = m;
        }
        total += __popcll(mk);
      }
    }
    if (lane == 0) {
      s_ncand = total < maxc ? total : maxc;
      if (total > maxc) {
        status = PRS_ERR_CAPACITY;
      }
      q.n_candidates[b] = total < maxc ? total : maxc;
      q.status[b]       = status;
      if (q.index_query) {
        q.index_query[b] = (int64_t) index_query;
      }
      if (a.query_node) {
        *a.query_node = status >= 0 && total > 0 ? (int32_t) (gid - a.graph_id_base) : -1;
      }
    }
  }
  __syncthreads();
  const int ncand = s_ncand;
  if (tid < maxc) {
    q.candidates[b * (size_t) maxc + tid] = tid < ncand ? s_cand[tid] : -1;
    if (a.cand_flat) {
      a.cand_flat[tid] = tid < ncand ? a.flat_base + s_cand[tid] : -1;
    }
  }
  // per candidate, its correspondences (:95-127): every row with a key, (fixed = query index, moving = point index, distance)
  const uint32_t* keys = q.best_keys + b * (size_t) q.key_stride;
  for (int k = wave; k < maxc; k += kPdThreads / 64) {
    int n = 0;
    if (k < ncand) {
      const int m = s_cand[k], off = a.map_off[m];
      int nr      = a.map_rows[m];
      if (kBank && nr > q.corr_stride) {  // (uniform; written after the barrier that follows the status word above)
        nr = 0;
        if (lane == 0) {
          q.status[b] = PRS_ERR_CAPACITY;
          if (a.query_node) {
            *a.query_node = -1;
          }
        }
      }
      prs_corr* out = q.corr + (b * (size_t) maxc + (size_t) k) * (size_t) q.corr_stride;
      int row = off;  // stored rows of the map: [off, off + nr) (pads follow)
      for (int base = 0; base < nr; base += 64) {
        const int r       = row + base + lane;
        const uint32_t ky = base + lane < nr ? keys[r] : kNoKey;
        const bool hit    = ky != kNoKey;
        const uint64_t mk = __ballot(hit);
        const int pos     = n + (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mk, 0u));
        if (hit) {
          prs_corr cr;
          cr.fixed_idx  = (int32_t) (ky & 0x7fffffu);
          cr.moving_idx = a.row_pidx[r];
          cr.response   = (float) (ky >> 23);
          out[pos]      = cr;
        }
        n += __popcll(mk);
      }
    }
    if (lane == 0) {
      q.n_corr[b * (size_t) maxc + (size_t) k] = n;
    }
  }
}

__global__ __launch_bounds__(kPdThreads) void place_select_kernel(const PlaceArgs a) {
  SelectView v;
  v.maps          = a.maps;
  v.map_gid       = a.map_gid;
  v.map_off       = a.map_off;
  v.map_rows      = a.map_rows;
  v.row_pidx      = a.row_pidx;
  v.cand_flat     = nullptr;
  v.flat_base     = 0;
  v.query_node    = nullptr;
  v.graph_id_base = 0;
  place_select_body<false>(a.q, a.p, v, blockIdx.x);
}

struct GatherArgs {
  prs_place_queries q;
  prs_place_pairs o;
  const uint8_t* desc;
  const float* xyz;
  const int32_t* map_off;
  const int32_t* map_rows;
  int maxc;
};

// one wave per pair slot (query b, candidate k): fixed = the query's Valid points in index order, moving = the candidate map's stored
// points, X = identity; a slot without a candidate gets n = 0 on both sides.  desc / xyz / map_off / map_rows: the database of query b;
// kBank: a map larger than the slot is refused here (n = 0 on both sides), the live sizes are not known at the call
template <bool kBank>
__device__ __forceinline__ void place_gather_slot(const prs_place_queries& q, const prs_place_pairs& o, const int maxc, const size_t slot,
                                                  const size_t b, const int k, const uint8_t* desc, const float* xyz,
                                                  const int32_t* map_off, const int32_t* map_rows) {
  const int lane = threadIdx.x & 63;
  bool use = k < q.n_candidates[b];  // (a query over max_candidates still fills its slots; other errors have none)
  int m = 0;
  if (use) {
    m = q.candidates[b * (size_t) maxc + (size_t) k];
    if (kBank && map_rows[m] > o.moving_stride) {
      use = false;
    }
  }
  int nf = 0, nm = 0;
  if (use) {
    const int nq = clamp_n(q.n_query[b], q.query_stride);
    const uint8_t* valid = q.valid ? q.valid + b * (size_t) q.query_stride : nullptr;
    const uint4* qd = reinterpret_cast<const uint4*>(q.desc + b * (size_t) q.query_stride * PRS_DESC_BYTES);
    const float4* qx = reinterpret_cast<const float4*>(q.xyz + b * (size_t) q.query_stride * 4);
    uint4* fd  = reinterpret_cast<uint4*>(o.fixed_desc + slot * (size_t) o.fixed_stride * PRS_DESC_BYTES);
    float4* fx = reinterpret_cast<float4*>(o.fixed_xyz + slot * (size_t) o.fixed_stride * 4);
    for (int base = 0; base < nq; base += 64) {
      const int i    = base + lane;
      const bool in  = i < nq && (!valid || valid[i] != 0);
      const uint64_t mk = __ballot(in);
      const int pos  = nf + (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mk, 0u));
      if (in) {
        fd[2 * (size_t) pos]     = qd[2 * (size_t) i];
        fd[2 * (size_t) pos + 1] = qd[2 * (size_t) i + 1];
        fx[pos]                  = qx[i];
      }
      nf += __popcll(mk);
    }
    const int off = map_off[m];
    nm = map_rows[m];
    const uint4* dd  = reinterpret_cast<const uint4*>(desc) + 2 * (size_t) off;
    const float4* dx = reinterpret_cast<const float4*>(xyz) + (size_t) off;
    uint4* md  = reinterpret_cast<uint4*>(o.moving_desc + slot * (size_t) o.moving_stride * PRS_DESC_BYTES);
    float4* mx = reinterpret_cast<float4*>(o.moving_xyz + slot * (size_t) o.moving_stride * 4);
    for (int i = lane; i < nm; i += 64) {
      md[2 * (size_t) i]     = dd[2 * (size_t) i];
      md[2 * (size_t) i + 1] = dd[2 * (size_t) i + 1];
      mx[i]                  = dx[i];
    }
  }
  if (lane < 16) {
    o.X[16 * slot + lane] = (lane % 5 == 0) ? 1.0f : 0.0f;
  }
  if (lane == 0) {
    o.n_fixed[slot]  = nf;
    o.n_moving[slot] = nm;
  }
}

__global__ __launch_bounds__(kPdThreads) void place_gather_kernel(const GatherArgs g) {
  const size_t slot = (size_t) blockIdx.x * (kPdThreads / 64) + (threadIdx.x >> 6);
  if (slot >= (size_t) g.q.batch * (size_t) g.maxc) {
    return;
  }
  place_gather_slot<false>(g.q, g.o, g.maxc, slot, slot / (size_t) g.maxc, (int) (slot % (size_t) g.maxc), g.desc, g.xyz, g.map_off,
                           g.map_rows);
}

int lim_of(const float thr) {
  // (float) d < maximum_descriptor_distance for integer d  <=>  d < lim  (lim 257: every distance of 256 bits)
  int lim = 0;
  while (lim <= 256 && (float) lim < thr) {
    ++lim;
  }
  return lim;
}

int check_params(prs_context* ctx, const prs_place_params* p, const char* what) {
  if (!p) {
    return ctx_fail(ctx, PRS_ERR_NULL, what);
  }
  if (std::isnan(p->maximum_descriptor_distance)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_query: maximum_descriptor_distance is NaN");
  }
  if (p->max_candidates < 1 || p->max_candidates > 256) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_query: max_candidates must be in [1, 256]");
  }
  return PRS_OK;
}

PlaceArgs make_args(const prs_place_db* db, const prs_place_params* p, const prs_place_queries* q) {
  PlaceArgs a;
  memset(&a, 0, sizeof(a));
  a.q        = *q;
  a.p        = *p;
  a.desc     = reinterpret_cast<const uint32_t*>(db->desc);
  a.row_pidx = db->row_pidx;
  a.tile_map = db->tile_map;
  a.map_off  = db->map_off;
  a.map_rows = db->map_rows;
  a.map_gid  = db->map_gid;
  a.maps     = db->maps;
  a.rows     = db->rows;
  a.lim      = lim_of(p->maximum_descriptor_distance);
  return a;
}

int place_query_launch(prs_place_db* db, const prs_place_params* p, const prs_place_queries* q) {
  prs_context* ctx = db->ctx;
  int rc = check_params(ctx, p, "prs_place_query_batch: parameters not set");
  if (rc != PRS_OK) {
    return rc;
  }
  if (!q) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_query_batch: queries not set");
  }
  if (q->batch <= 0) {
    return PRS_OK;
  }
  if (!q->desc || !q->n_query || !q->graph_id || !q->match_counts || !q->best_keys || !q->candidates || !q->n_candidates || !q->corr ||
      !q->n_corr || !q->status) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_query_batch: input or output buffer not set");
  }
  if (q->batch > 65535) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_query_batch: more than 65535 queries");
  }
  if (q->query_stride < 1 || q->query_stride > kPdMaxQuery) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_query_batch: query_stride must be in [1, 65536]");
  }
  if (q->count_stride < db->maps || q->key_stride < db->rows || q->corr_stride < db->max_map_rows || q->corr_stride > kPdMaxCorrStride) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_place_query_batch: count_stride, key_stride or corr_stride below the database's size");
  }
  if (!aligned_to(q->desc, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_query_batch: descriptor rows must be 4-byte aligned");
  }
  const PlaceArgs a = make_args(db, p, q);
  Launches on(ctx, "prs_place_query_batch", ctx_stream(ctx));
  const int64_t big = db->rows > db->maps ? db->rows : db->maps, init_x = (big + kPdThreads - 1) / kPdThreads;
  const Grid init   = big > 0 ? on.grid(init_x < 1024 ? init_x : 1024, q->batch, kPdThreads) : Grid();
  const Grid score  = db->rows > 0 ? on.grid(((int64_t) db->rows + kPdSlice - 1) / kPdSlice,
                                             ((int64_t) q->query_stride + kPdRowsWg - 1) / kPdRowsWg, q->batch, kPdThreads)
                                   : Grid();
  const Grid select = on.grid(q->batch, kPdThreads);
  PRS_TRY(on.check());
  if (init) {
    on.launch(place_init_kernel, init, 0, a);
  }
  if (score) {
    on.launch(place_score_kernel, score, 0, a);
  }
  on.launch(place_select_kernel, select, 0, a);
  return on.finish();
}

template <typename T>
int grow(prs_context* ctx, const char* name, T*& ptr, const size_t old_n, const size_t new_n) {
  // (the database's arrays carry its rows from call to call: guard mode paints them here, and the zeroing below follows)
  T* p = nullptr;
  if (owned_alloc(ctx, name, &p, new_n * sizeof(T) > 0 ? new_n * sizeof(T) : sizeof(T)) != hipSuccess) {
    return ctx_fail(ctx, PRS_ERR_HIP, "prs_place_db: device allocation failed");
  }
  hipError_t e = hipMemsetAsync(p, 0, new_n * sizeof(T), ctx->stream);
  if (e == hipSuccess && ptr && old_n > 0) {
    e = hipMemcpyAsync(p, ptr, old_n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
  }
  if (e == hipSuccess) {
    e = hipStreamSynchronize(ctx->stream);
  }
  if (e != hipSuccess) {
    owned_free(ctx, p);
    return ctx_fail_hip(ctx, e, "prs_place_db: growth copy");
  }
  owned_free(ctx, ptr);
  ptr = p;
  return PRS_OK;
}

int db_reserve(prs_place_db* db, int64_t maps, int64_t rows) {
  prs_context* ctx = db->ctx;
  rows = (rows + 15) / 16 * 16;
  if (maps > INT32_MAX || rows > INT32_MAX - 16) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_db_reserve: above 2^31 maps or rows");
  }
  (void) hipSetDevice(ctx->device);
  if (maps > db->map_cap) {
    const size_t o = (size_t) db->maps, n = (size_t) maps;
    int rc = grow(ctx, "place_db.map_off", db->map_off, o, n);
    rc     = rc == PRS_OK ? grow(ctx, "place_db.map_rows", db->map_rows, o, n) : rc;
    rc     = rc == PRS_OK ? grow(ctx, "place_db.map_gid", db->map_gid, o, n) : rc;
    if (rc != PRS_OK) {
      return rc;
    }
    db->map_cap = (int32_t) maps;
  }
  if (rows > db->row_cap) {
    const size_t o = (size_t) db->rows, n = (size_t) rows;
    int rc = grow(ctx, "place_db.desc", db->desc, o * PRS_DESC_BYTES, n * PRS_DESC_BYTES);
    rc     = rc == PRS_OK ? grow(ctx, "place_db.xyz", db->xyz, o * 4, n * 4) : rc;
    rc     = rc == PRS_OK ? grow(ctx, "place_db.row_pidx", db->row_pidx, o, n) : rc;
    rc     = rc == PRS_OK ? grow(ctx, "place_db.tile_map", db->tile_map, o / 16, n / 16) : rc;
    if (rc != PRS_OK) {
      return rc;
    }
    db->row_cap = (int32_t) rows;
  }
  return PRS_OK;
}

// ---- place bank: the same three launches over per-sequence arenas whose sizes are device counters, and the append kernel ----
struct BankDev {
  uint8_t* desc;
  float* xyz;
  int32_t* row_pidx;
  int32_t* tile_map;
  int32_t* map_off;
  int32_t* map_rows;
  int64_t* map_gid;
  int32_t* node_of_map;
  int32_t* n_maps;
  int32_t* n_rows;
  int32_t* max_map_rows;
  int32_t batch, map_stride, row_stride;
};

struct BankArgs {
  prs_place_queries q;
  prs_place_params p;
  BankDev d;
  prs_place_bank_links links;  // all nullptr without links
  int lim;
};

// live sizes of arena b, clamped to the capacities (the counters have one writer, the append kernel, which keeps them inside)
__device__ __forceinline__ int bank_rows(const BankDev& d, const size_t b) {
  return clamp_n(d.n_rows[b], d.row_stride);
}
__device__ __forceinline__ int bank_maps(const BankDev& d, const size_t b) {
  return clamp_n(d.n_maps[b], d.map_stride);
}

__global__ __launch_bounds__(kPdThreads) void place_bank_init_kernel(const BankArgs a) {
  const size_t b  = blockIdx.y;
  const size_t i0 = (size_t) blockIdx.x * kPdThreads + threadIdx.x;
  const size_t step = (size_t) gridDim.x * kPdThreads;
  const size_t rows = (size_t) bank_rows(a.d, b), maps = (size_t) bank_maps(a.d, b);
  for (size_t i = i0; i < rows; i += step) {
    a.q.best_keys[b * (size_t) a.q.key_stride + i] = kNoKey;
  }
  for (size_t i = i0; i < maps; i += step) {
    a.q.match_counts[b * (size_t) a.q.count_stride + i] = 0u;
  }
}

__global__ __launch_bounds__(kPdThreads) void place_bank_score_kernel(const BankArgs a) {
  const size_t b = blockIdx.z;
  ScoreView v    = score_view_of_query(a.q, b, a.lim);
  v.desc         = reinterpret_cast<const uint32_t*>(a.d.desc) + b * (size_t) a.d.row_stride * 8;
  v.row_pidx     = a.d.row_pidx + b * (size_t) a.d.row_stride;
  v.tile_map     = a.d.tile_map + b * (size_t) (a.d.row_stride / 16);
  v.rows         = bank_rows(a.d, b);
  place_score_body(v);
}

__global__ __launch_bounds__(kPdThreads) void place_bank_select_kernel(const BankArgs a) {
  const size_t b = blockIdx.x;
  SelectView v;
  v.maps          = bank_maps(a.d, b);
  v.map_gid       = a.d.map_gid + b * (size_t) a.d.map_stride;
  v.map_off       = a.d.map_off + b * (size_t) a.d.map_stride;
  v.map_rows      = a.d.map_rows + b * (size_t) a.d.map_stride;
  v.row_pidx      = a.d.row_pidx + b * (size_t) a.d.row_stride;
  v.cand_flat     = a.links.candidates_flat ? a.links.candidates_flat + b * (size_t) a.p.max_candidates : nullptr;
  v.flat_base     = (int32_t) b * a.d.map_stride;
  v.query_node    = a.links.query_node ? a.links.query_node + b : nullptr;
  v.graph_id_base = a.links.graph_id_base ? a.links.graph_id_base[b] : 0;
  place_select_body<true>(a.q, a.p, v, b);
}

struct BankGatherArgs {
  prs_place_queries q;
  prs_place_pairs o;
  BankDev d;
  int maxc;
};

__global__ __launch_bounds__(kPdThreads) void place_bank_gather_kernel(const BankGatherArgs g) {
  const size_t slot = (size_t) blockIdx.x * (kPdThreads / 64) + (threadIdx.x >> 6);
  if (slot >= (size_t) g.q.batch * (size_t) g.maxc) {
    return;
  }
  const size_t b = slot / (size_t) g.maxc;
  place_gather_slot<true>(g.q, g.o, g.maxc, slot, b, (int) (slot % (size_t) g.maxc), g.d.desc + b * (size_t) g.d.row_stride * PRS_DESC_BYTES,
                          g.d.xyz + b * (size_t) g.d.row_stride * 4, g.d.map_off + b * (size_t) g.d.map_stride,
                          g.d.map_rows + b * (size_t) g.d.map_stride);
}

__global__ __launch_bounds__(kPdThreads) void place_bank_clear_kernel(const BankDev d) {
  const size_t i = (size_t) blockIdx.x * kPdThreads + threadIdx.x;
  if (i < (size_t) d.batch * (size_t) d.map_stride) {
    d.node_of_map[i] = -1;
  }
  if (i < (size_t) d.batch) {
    d.n_maps[i]       = 0;
    d.n_rows[i]       = 0;
    d.max_map_rows[i] = 0;
  }
}

struct AppendArgs {
  prs_place_bank_append in;
  BankDev d;
};

// prs_place_db_add on the device, one workgroup per sequence: checks, count of the Valid rows, compaction in point order onto the
// arena's tail (ballot + mbcnt prefix per wave, the waves' counts through LDS, a running offset across chunks of 256 rows), pad rows,
// tile and map entries, and last of all the counters, by one thread.  Every early return is block-uniform.
__global__ __launch_bounds__(kPdThreads) void place_bank_append_kernel(const AppendArgs a) {
  __shared__ int s_wave[kPdThreads / 64];
  __shared__ int s_dup;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t b    = blockIdx.x;
  const int n       = a.in.n_query[b];
  const int64_t gid = a.in.graph_id[b];
  const int maps    = bank_maps(a.d, b), rows = bank_rows(a.d, b);
  int status        = PRS_OK;
  if (n == 0) {
    status = PRS_WARN_EMPTY_INPUT;
  } else if (n < 0 || gid < 0) {
    status = PRS_ERR_RANGE;
  } else if (n > a.in.query_stride) {
    status = PRS_ERR_CAPACITY;
  }
  if (status != PRS_OK) {
    if (tid == 0) {
      a.in.status[b] = status;
    }
    return;
  }
  if (tid == 0) {
    s_dup = 0;
  }
  __syncthreads();
  const int64_t* map_gid = a.d.map_gid + b * (size_t) a.d.map_stride;
  for (int m = tid; m < maps; m += kPdThreads) {
    if (map_gid[m] == gid) {
      s_dup = 1;
    }
  }
  // the Valid rows of the slot
  const uint8_t* valid = a.in.valid ? a.in.valid + b * (size_t) a.in.query_stride : nullptr;
  int mine = 0;
  for (int base = 0; base < n; base += kPdThreads) {
    const int i = base + tid;
    mine += (int) __popcll(__ballot(i < n && (!valid || valid[i] != 0)));  // (per wave: every lane holds its wave's count)
  }
  if (lane == 0) {
    s_wave[wave] = mine;
  }
  __syncthreads();
  int nk = 0;
#pragma unroll
  for (int w = 0; w < kPdThreads / 64; ++w) {
    nk += s_wave[w];
  }
  const int padded = (nk + 15) / 16 * 16;
  if (s_dup != 0) {
    status = PRS_ERR_RANGE;
  } else if (maps >= a.d.map_stride || padded > a.d.row_stride - rows) {
    status = PRS_ERR_CAPACITY;
  }
  if (status != PRS_OK) {
    if (tid == 0) {
      a.in.status[b] = status;
    }
    return;
  }
  const uint4* src_d  = reinterpret_cast<const uint4*>(a.in.desc + b * (size_t) a.in.query_stride * PRS_DESC_BYTES);
  const float4* src_x = a.in.xyz ? reinterpret_cast<const float4*>(a.in.xyz + b * (size_t) a.in.query_stride * 4) : nullptr;
  const size_t r0     = b * (size_t) a.d.row_stride + (size_t) rows;  // the first new row, counted over the whole bank
  uint4* dst_d        = reinterpret_cast<uint4*>(a.d.desc) + 2 * r0;
  float4* dst_x       = reinterpret_cast<float4*>(a.d.xyz) + r0;
  int32_t* dst_p      = a.d.row_pidx + r0;
  int done = 0;  // rows stored by the chunks before this one
  for (int base = 0; base < n; base += kPdThreads) {
    __syncthreads();  // (s_wave of the chunk before, or of the count, has been read)
    const int i       = base + tid;
    const bool in     = i < n && (!valid || valid[i] != 0);
    const uint64_t mk = __ballot(in);
    if (lane == 0) {
      s_wave[wave] = (int) __popcll(mk);
    }
    __syncthreads();
    int before = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < kPdThreads / 64; ++w) {
      before += w < wave ? s_wave[w] : 0;
      chunk += s_wave[w];
    }
    if (in) {
      const int pos = done + before + (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mk, 0u));
      if (pos < padded) {  // (always: pos < nk; keeps a sequence inside its arena whatever the inputs do between the two passes)
        dst_d[2 * (size_t) pos]     = src_d[2 * (size_t) i];
        dst_d[2 * (size_t) pos + 1] = src_d[2 * (size_t) i + 1];
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (src_x) {
          x   = src_x[i];
          x.w = 0.0f;
        }
        dst_x[pos] = x;
        dst_p[pos] = i;
      }
    }
    done += chunk;
  }
  // pad rows, the tiles of the map, the map's entry
  for (int r = (done < nk ? done : nk) + tid; r < padded; r += kPdThreads) {
    dst_d[2 * (size_t) r]     = make_uint4(0u, 0u, 0u, 0u);
    dst_d[2 * (size_t) r + 1] = make_uint4(0u, 0u, 0u, 0u);
    dst_x[r]                  = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    dst_p[r]                  = -1;
  }
  int32_t* tiles = a.d.tile_map + b * (size_t) (a.d.row_stride / 16) + (size_t) (rows / 16);
  for (int t = tid; t < padded / 16; t += kPdThreads) {
    tiles[t] = maps;
  }
  __syncthreads();
  if (tid == 0) {
    const size_t m = b * (size_t) a.d.map_stride + (size_t) maps;
    a.d.map_off[m]     = rows;
    a.d.map_rows[m]    = nk;
    a.d.map_gid[m]     = gid;
    a.d.node_of_map[m] = (int32_t) (gid - (a.in.graph_id_base ? a.in.graph_id_base[b] : 0));
    a.d.n_maps[b]      = maps + 1;
    a.d.n_rows[b]      = rows + padded;
    if (nk > a.d.max_map_rows[b]) {
      a.d.max_map_rows[b] = nk;
    }
    a.in.status[b] = PRS_OK;
  }
}

BankDev bank_dev(const prs_place_bank* k) {
  BankDev d;
  d.desc         = k->desc;
  d.xyz          = k->xyz;
  d.row_pidx     = k->row_pidx;
  d.tile_map     = k->tile_map;
  d.map_off      = k->map_off;
  d.map_rows     = k->map_rows;
  d.map_gid      = k->map_gid;
  d.node_of_map  = k->node_of_map;
  d.n_maps       = k->counters;
  d.n_rows       = k->counters + k->batch;
  d.max_map_rows = k->counters + 2 * (size_t) k->batch;
  d.batch        = k->batch;
  d.map_stride   = k->map_stride;
  d.row_stride   = k->row_stride;
  return d;
}

// the smallest slot that holds every map the bank can hold
int32_t bank_largest_map(const prs_place_bank* k) {
  return k->row_stride < k->max_query_stride ? k->row_stride : k->max_query_stride;
}

}  // namespace

}  // namespace prs

using namespace prs;

extern "C" {

int prs_place_db_create(prs_context* ctx, prs_place_db** db) {
  if (!ctx || !db) {
    return PRS_ERR_NULL;
  }
  *db = new prs_place_db();
  (*db)->ctx = ctx;
  return PRS_OK;
}

int prs_place_db_destroy(prs_place_db* db) {
  if (!db) {
    return PRS_OK;
  }
  (void) hipSetDevice(db->ctx->device);
  (void) hipStreamSynchronize(db->ctx->stream);
  void* ptrs[] = {db->desc, db->xyz, db->row_pidx, db->tile_map, db->map_off, db->map_rows, db->map_gid};
  for (void* p : ptrs) {
    owned_free(db->ctx, p);
  }
  delete db;
  return PRS_OK;
}

int prs_place_db_clear(prs_place_db* db) {
  if (!db) {
    return PRS_ERR_NULL;
  }
  db->maps = db->rows = db->max_map_rows = 0;
  db->index_of.clear();
  return PRS_OK;
}

int prs_place_db_reserve(prs_place_db* db, int64_t maps, int64_t rows) {
  if (!db) {
    return PRS_ERR_NULL;
  }
  if (maps < 0 || rows < 0) {
    return ctx_fail(db->ctx, PRS_ERR_RANGE, "prs_place_db_reserve: negative size");
  }
  return db_reserve(db, maps, rows);
}

int prs_place_db_size(const prs_place_db* db, int32_t* maps, int32_t* rows, int32_t* max_map_rows) {
  if (!db) {
    return PRS_ERR_NULL;
  }
  if (maps) {
    *maps = db->maps;
  }
  if (rows) {
    *rows = db->rows;
  }
  if (max_map_rows) {
    *max_map_rows = db->max_map_rows;
  }
  return PRS_OK;
}

int prs_place_db_add(prs_place_db* db, int64_t graph_id, const float* xyz, const uint8_t* desc, const uint8_t* valid, int32_t n) {
  if (!db) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = db->ctx;
  if (n < 0 || graph_id < 0) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_db_add: negative size or graph id");
  }
  if (n > 0 && !desc) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_db_add: descriptors not set");
  }
  if (db->index_of.count(graph_id)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_db_add: graph id already stored");
  }
  std::vector<int32_t> keep;
  keep.reserve((size_t) n);
  for (int32_t i = 0; i < n; ++i) {
    if (!valid || valid[i] != 0) {
      keep.push_back(i);
    }
  }
  const int32_t nk = (int32_t) keep.size(), padded = (nk + 15) / 16 * 16;
  if ((int64_t) db->rows + padded > INT32_MAX - 16) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_db_add: above 2^31 rows");
  }
  if (db->maps + 1 > db->map_cap || db->rows + padded > db->row_cap) {
    const int64_t want_maps = db->maps + 1 > db->map_cap ? 2 * (int64_t) db->map_cap + 16 : db->map_cap;
    const int64_t want_rows = db->rows + padded > db->row_cap ? 2 * (int64_t) db->row_cap + padded + 1024 : db->row_cap;
    const int rc = db_reserve(db, want_maps, want_rows > INT32_MAX - 16 ? (int64_t) db->rows + padded : want_rows);
    if (rc != PRS_OK) {
      return rc;
    }
  }
  (void) hipSetDevice(ctx->device);
  const size_t tiles = (size_t) padded / 16;
  const size_t o_xyz = (size_t) padded * PRS_DESC_BYTES, o_pidx = o_xyz + (size_t) padded * 16, o_tile = o_pidx + (size_t) padded * 4;
  const size_t o_map = o_tile + tiles * 4, total = o_map + 16;
  unsigned char* h = static_cast<unsigned char*>(ctx_arena(ctx, ARENA_PINNED, total));
  if (!h) {
    return ctx_fail(ctx, PRS_ERR_HIP, "prs_place_db_add: staging allocation failed");
  }
  memset(h, 0, total);
  float* hx    = reinterpret_cast<float*>(h + o_xyz);
  int32_t* hp  = reinterpret_cast<int32_t*>(h + o_pidx);
  int32_t* ht  = reinterpret_cast<int32_t*>(h + o_tile);
  for (int32_t r = 0; r < padded; ++r) {
    hp[r] = -1;
  }
  for (int32_t r = 0; r < nk; ++r) {
    const int32_t i = keep[(size_t) r];
    memcpy(h + (size_t) r * PRS_DESC_BYTES, desc + (size_t) i * PRS_DESC_BYTES, PRS_DESC_BYTES);
    if (xyz) {
      hx[4 * (size_t) r]     = xyz[3 * (size_t) i];
      hx[4 * (size_t) r + 1] = xyz[3 * (size_t) i + 1];
      hx[4 * (size_t) r + 2] = xyz[3 * (size_t) i + 2];
    }
    hp[r] = i;
  }
  const int32_t m = db->maps;
  for (size_t t = 0; t < tiles; ++t) {
    ht[t] = m;
  }
  int32_t* hm = reinterpret_cast<int32_t*>(h + o_map);
  hm[0] = db->rows;
  hm[1] = nk;
  memcpy(h + o_map + 8, &graph_id, 8);
  hipStream_t s = ctx->stream;
  const size_t r0 = (size_t) db->rows;
  hipError_t e = hipSuccess;
  if (padded > 0) {
    e = hipMemcpyAsync(db->desc + r0 * PRS_DESC_BYTES, h, (size_t) padded * PRS_DESC_BYTES, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      e = hipMemcpyAsync(db->xyz + r0 * 4, hx, (size_t) padded * 16, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) {
      e = hipMemcpyAsync(db->row_pidx + r0, hp, (size_t) padded * 4, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) {
      e = hipMemcpyAsync(db->tile_map + r0 / 16, ht, tiles * 4, hipMemcpyHostToDevice, s);
    }
  }
  if (e == hipSuccess) {
    e = hipMemcpyAsync(db->map_off + m, hm, 4, hipMemcpyHostToDevice, s);
  }
  if (e == hipSuccess) {
    e = hipMemcpyAsync(db->map_rows + m, hm + 1, 4, hipMemcpyHostToDevice, s);
  }
  if (e == hipSuccess) {
    e = hipMemcpyAsync(db->map_gid + m, h + o_map + 8, 8, hipMemcpyHostToDevice, s);
  }
  if (e == hipSuccess) {
    e = hipStreamSynchronize(s);  // (the pinned staging is reused by the next call)
  }
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_place_db_add upload");
  }
  db->index_of[graph_id] = m;
  db->maps += 1;
  db->rows += padded;
  db->max_map_rows = nk > db->max_map_rows ? nk : db->max_map_rows;
  return PRS_OK;
}

int prs_place_query_batch(prs_place_db* db, const prs_place_params* params, const prs_place_queries* queries) {
  if (!db) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(db->ctx->device);
  return place_query_launch(db, params, queries);
}

int prs_place_query(prs_place_db* db, const prs_place_params* params, int64_t graph_id, const uint8_t* desc, const uint8_t* valid,
                    int32_t n, int32_t* candidates, int32_t* n_candidates, prs_corr* corr, int32_t corr_stride, int32_t* n_corr,
                    uint32_t* match_counts) {
  if (!db) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = db->ctx;
  PRS_TRY(check_params(ctx, params, "prs_place_query: parameters not set"));
  if (!candidates || !n_candidates || !corr || !n_corr || (n > 0 && !desc)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_query: input or output buffer not set");
  }
  if (n > kPdMaxQuery) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_query: more than 65536 query points");
  }
  if (corr_stride < db->max_map_rows || corr_stride < 1) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_place_query: corr_stride below the largest stored map");
  }
  (void) hipSetDevice(ctx->device);
  const size_t maxc = (size_t) params->max_candidates;
  const size_t nq = (size_t) (n > 0 ? n : 1), maps = (size_t) (db->maps > 0 ? db->maps : 1), rows = (size_t) (db->rows > 0 ? db->rows : 1);
  struct In {
    int32_t n_query;
    int64_t graph_id;
  };
  struct Out {
    int32_t status, n_candidates;
  };
  // descriptors | valid | n, graph id (uploaded) | status | counts | candidates | n_corr (downloaded) | corr | keys (device only:
  // the rows of the candidates go straight into the caller's buffer below)
  Staging st(ctx, "prs_place_query");
  auto qdesc  = st.up<uint8_t>(nq * PRS_DESC_BYTES);
  auto qvalid = st.up<uint8_t>(nq);
  auto in     = st.up<In>(1);
  auto out    = st.down<Out>(1);
  auto counts = st.down<uint32_t>(maps);
  auto cand   = st.down<int32_t>(maxc);
  auto ncorr  = st.down<int32_t>(maxc);
  auto dcorr  = st.device<prs_corr>(maxc * (size_t) corr_stride);
  auto keys   = st.device<uint32_t>(rows);
  PRS_TRY(st.commit());
  if (n > 0) {
    memcpy(qdesc.h(), desc, (size_t) n * PRS_DESC_BYTES);
    if (valid) {
      memcpy(qvalid.h(), valid, (size_t) n);
    }
  }
  in.h()->n_query  = n;
  in.h()->graph_id = graph_id;
  PRS_TRY(st.upload());
  prs_place_queries q;
  memset(&q, 0, sizeof(q));
  q.batch        = 1;
  q.query_stride = (int32_t) nq;
  q.desc         = qdesc.d();
  q.valid        = valid ? qvalid.d() : nullptr;
  q.n_query      = &in.d()->n_query;
  q.graph_id     = &in.d()->graph_id;
  q.count_stride = (int32_t) maps;
  q.match_counts = counts.d();
  q.key_stride   = (int32_t) rows;
  q.best_keys    = keys.d();
  q.corr_stride  = corr_stride;
  q.candidates   = cand.d();
  q.n_candidates = &out.d()->n_candidates;
  q.corr         = dcorr.d();
  q.n_corr       = ncorr.d();
  q.status       = &out.d()->status;
  PRS_TRY(place_query_launch(db, params, &q));
  PRS_TRY(st.download());
  const int32_t nc  = out.h()->n_candidates;
  const int32_t* hn = ncorr.h();
  memcpy(candidates, cand.h(), maxc * 4);
  memcpy(n_corr, hn, maxc * 4);
  *n_candidates = nc;
  // the correspondences of the candidates only (candidate k's rows start at k * corr_stride)
  hipStream_t s = ctx->stream;
  hipError_t e  = hipSuccess;
  for (int32_t k = 0; k < nc; ++k) {
    if (hn[k] > 0) {
      e = hipMemcpyAsync(corr + (size_t) k * (size_t) corr_stride, dcorr.d() + (size_t) k * (size_t) corr_stride,
                         (size_t) hn[k] * sizeof(prs_corr), hipMemcpyDeviceToHost, s);
      if (e != hipSuccess) {
        break;
      }
    }
  }
  if (e == hipSuccess && match_counts && db->maps > 0) {
    e = hipMemcpyAsync(match_counts, counts.d(), (size_t) db->maps * 4, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) {
    e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_place_query download");
  }
  if (out.h()->status < 0) {
    return ctx_fail(ctx, out.h()->status, "prs_place_query: query rejected (graph id, size or candidate capacity)");
  }
  return out.h()->status;
}

int prs_place_gather_pairs(prs_place_db* db, const prs_place_params* params, const prs_place_queries* queries, const prs_place_pairs* pairs) {
  if (!db) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = db->ctx;
  int rc = check_params(ctx, params, "prs_place_gather_pairs: parameters not set");
  if (rc != PRS_OK) {
    return rc;
  }
  if (!queries || !pairs) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_gather_pairs: queries or pairs not set");
  }
  if (queries->batch <= 0) {
    return PRS_OK;
  }
  if (!queries->desc || !queries->xyz || !queries->n_query || !queries->candidates || !queries->n_candidates || !queries->status ||
      !pairs->fixed_xyz || !pairs->fixed_desc || !pairs->n_fixed || !pairs->moving_xyz || !pairs->moving_desc || !pairs->n_moving ||
      !pairs->X) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_gather_pairs: input or output buffer not set");
  }
  if (pairs->fixed_stride < queries->query_stride || pairs->moving_stride < db->max_map_rows) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_place_gather_pairs: a pair slot is smaller than the query or the largest stored map");
  }
  if (!aligned_to(queries->desc, 16) || !aligned_to(queries->xyz, 16) || !aligned_to(pairs->fixed_xyz, 16) || !aligned_to(pairs->fixed_desc, 16) ||
      !aligned_to(pairs->moving_xyz, 16) || !aligned_to(pairs->moving_desc, 16)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_gather_pairs: rows must be 16-byte aligned");
  }
  (void) hipSetDevice(ctx->device);
  GatherArgs g;
  memset(&g, 0, sizeof(g));
  g.q        = *queries;
  g.o        = *pairs;
  g.desc     = db->desc;
  g.xyz      = db->xyz;
  g.map_off  = db->map_off;
  g.map_rows = db->map_rows;
  g.maxc     = params->max_candidates;
  const int64_t slots = (int64_t) queries->batch * params->max_candidates;
  return Launches(ctx, "prs_place_gather_pairs", ctx_stream(ctx)).one((slots + 3) / 4, kPdThreads, place_gather_kernel, 0, g);
}

int prs_place_bank_create(prs_context* ctx, int32_t batch, int32_t map_stride, int32_t row_stride, prs_place_bank** bank) {
  if (!ctx || !bank) {
    return PRS_ERR_NULL;
  }
  *bank = nullptr;
  if (batch < 1 || batch > 65535 || map_stride < 1 || row_stride < 1 || row_stride > (1 << 20)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_bank_create: batch in [1, 65535], map_stride >= 1, row_stride in [1, 2^20]");
  }
  if ((int64_t) batch * map_stride > INT32_MAX) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_bank_create: batch * map_stride above 2^31 (the flat candidate index is int32)");
  }
  (void) hipSetDevice(ctx->device);
  prs_place_bank* k = new prs_place_bank();
  k->ctx        = ctx;
  k->batch      = batch;
  k->map_stride = map_stride;
  k->row_stride = (row_stride + 15) / 16 * 16;
  const size_t rows = (size_t) batch * (size_t) k->row_stride, maps = (size_t) batch * (size_t) map_stride;
  // (the bank's arrays carry its rows from call to call: guard mode paints them here and never again)
  bool ok = owned_alloc(ctx, "place_bank.desc", &k->desc, rows * PRS_DESC_BYTES) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.xyz", &k->xyz, rows * 16) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.row_pidx", &k->row_pidx, rows * 4) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.tile_map", &k->tile_map, rows / 16 * 4) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.map_off", &k->map_off, maps * 4) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.map_rows", &k->map_rows, maps * 4) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.map_gid", &k->map_gid, maps * 8) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.own_nodes", &k->own_nodes, maps * 4) == hipSuccess;
  ok      = ok && owned_alloc(ctx, "place_bank.counters", &k->counters, (size_t) batch * 3 * 4) == hipSuccess;
  k->node_of_map = k->own_nodes;
  if (!ok || prs_place_bank_clear(k) != PRS_OK) {
    (void) hipGetLastError();
    (void) prs_place_bank_destroy(k);
    return ctx_fail(ctx, PRS_ERR_HIP, "prs_place_bank_create: device allocation failed");
  }
  *bank = k;
  return PRS_OK;
}

int prs_place_bank_destroy(prs_place_bank* bank) {
  if (!bank) {
    return PRS_OK;
  }
  (void) hipSetDevice(bank->ctx->device);
  (void) hipStreamSynchronize(bank->ctx->stream);
  void* ptrs[] = {bank->desc, bank->xyz, bank->row_pidx, bank->tile_map, bank->map_off, bank->map_rows, bank->map_gid, bank->own_nodes,
                  bank->counters};
  for (void* p : ptrs) {
    owned_free(bank->ctx, p);
  }
  delete bank;
  return PRS_OK;
}

int prs_place_bank_clear(prs_place_bank* bank) {
  if (!bank) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = bank->ctx;
  (void) hipSetDevice(ctx->device);
  const int64_t n = (int64_t) bank->batch * bank->map_stride;  // >= batch
  return Launches(ctx, "prs_place_bank_clear", ctx_stream(ctx)).one((n + kPdThreads - 1) / kPdThreads, kPdThreads, place_bank_clear_kernel,
                                                                    0, bank_dev(bank));
}

int prs_place_bank_sizes(prs_place_bank* bank, int32_t* maps, int32_t* rows, int32_t* max_map_rows) {
  if (!bank) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = bank->ctx;
  (void) hipSetDevice(ctx->device);
  const size_t B = (size_t) bank->batch;
  std::vector<int32_t> h(3 * B);
  hipError_t e = hipMemcpyAsync(h.data(), bank->counters, 3 * B * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) {
    e = hipStreamSynchronize(ctx->stream);
  }
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_place_bank_sizes download");
  }
  int32_t* out[3] = {maps, rows, max_map_rows};
  for (int i = 0; i < 3; ++i) {
    if (out[i]) {
      memcpy(out[i], h.data() + (size_t) i * B, B * 4);
    }
  }
  return PRS_OK;
}

void prs_place_bank_struct_sizes(uint64_t* sizes2) {
  if (sizes2) {
    sizes2[0] = sizeof(prs_place_bank_append);
    sizes2[1] = sizeof(prs_place_bank_links);
  }
}

int prs_place_bank_bind_node_of_map(prs_place_bank* bank, int32_t* node_of_map) {
  if (!bank) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = bank->ctx;
  int32_t* to      = node_of_map ? node_of_map : bank->own_nodes;
  if (to != bank->node_of_map) {
    (void) hipSetDevice(ctx->device);
    const hipError_t e = hipMemcpyAsync(to, bank->node_of_map, (size_t) bank->batch * (size_t) bank->map_stride * 4, hipMemcpyDeviceToDevice,
                                        ctx->stream);
    if (e != hipSuccess) {
      return ctx_fail_hip(ctx, e, "prs_place_bank_bind_node_of_map copy");
    }
    bank->node_of_map = to;
  }
  return PRS_OK;
}

int prs_place_bank_append_batch(prs_place_bank* bank, const prs_place_bank_append* in) {
  if (!bank) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = bank->ctx;
  if (!in) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_bank_append_batch: input not set");
  }
  if (!in->desc || !in->n_query || !in->graph_id || !in->status) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_bank_append_batch: input or output buffer not set");
  }
  if (in->batch != bank->batch) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_bank_append_batch: batch differs from the bank's");
  }
  if (in->query_stride < 1 || in->query_stride > kPdMaxQuery) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_bank_append_batch: query_stride must be in [1, 65536]");
  }
  if (!aligned_to(in->desc, 16) || !aligned_to(in->xyz, 16)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_bank_append_batch: rows must be 16-byte aligned");
  }
  (void) hipSetDevice(ctx->device);
  AppendArgs a;
  memset(&a, 0, sizeof(a));
  a.in = *in;
  a.d  = bank_dev(bank);
  Launches on(ctx, "prs_place_bank_append_batch", ctx_stream(ctx));
  const Grid grid = on.grid(bank->batch, kPdThreads);
  PRS_TRY(on.check());
  on.launch(place_bank_append_kernel, grid, 0, a);
  PRS_TRY(on.finish());
  bank->max_query_stride = in->query_stride > bank->max_query_stride ? in->query_stride : bank->max_query_stride;
  return PRS_OK;
}

int prs_place_bank_query_batch(prs_place_bank* bank, const prs_place_params* params, const prs_place_queries* q,
                               const prs_place_bank_links* links) {
  if (!bank) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = bank->ctx;
  PRS_TRY(check_params(ctx, params, "prs_place_bank_query_batch: parameters not set"));
  if (!q) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_bank_query_batch: queries not set");
  }
  if (!q->desc || !q->n_query || !q->graph_id || !q->match_counts || !q->best_keys || !q->candidates || !q->n_candidates || !q->corr ||
      !q->n_corr || !q->status || (links && (!links->candidates_flat || !links->query_node))) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_bank_query_batch: input or output buffer not set");
  }
  if (q->batch != bank->batch) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_bank_query_batch: batch differs from the bank's");
  }
  if (q->query_stride < 1 || q->query_stride > kPdMaxQuery) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_bank_query_batch: query_stride must be in [1, 65536]");
  }
  if (q->count_stride < bank->map_stride || q->key_stride < bank->row_stride || q->corr_stride < bank_largest_map(bank) ||
      q->corr_stride < 1 || q->corr_stride > kPdMaxCorrStride) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_place_bank_query_batch: count_stride, key_stride or corr_stride below the bank's capacity");
  }
  if (!aligned_to(q->desc, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_bank_query_batch: descriptor rows must be 4-byte aligned");
  }
  (void) hipSetDevice(ctx->device);
  BankArgs a;
  memset(&a, 0, sizeof(a));
  a.q   = *q;
  a.p   = *params;
  a.d   = bank_dev(bank);
  a.lim = lim_of(params->maximum_descriptor_distance);
  if (links) {
    a.links = *links;
  }
  Launches on(ctx, "prs_place_bank_query_batch", ctx_stream(ctx));
  const int64_t big = bank->row_stride > bank->map_stride ? bank->row_stride : bank->map_stride, init_x = (big + kPdThreads - 1) / kPdThreads;
  const Grid init   = on.grid(init_x < 1024 ? init_x : 1024, q->batch, kPdThreads);
  const Grid score  = on.grid(((int64_t) bank->row_stride + kPdSlice - 1) / kPdSlice, ((int64_t) q->query_stride + kPdRowsWg - 1) / kPdRowsWg,
                              q->batch, kPdThreads);
  const Grid select = on.grid(q->batch, kPdThreads);
  PRS_TRY(on.check());
  on.launch(place_bank_init_kernel, init, 0, a);
  on.launch(place_bank_score_kernel, score, 0, a);
  on.launch(place_bank_select_kernel, select, 0, a);
  return on.finish();
}

int prs_place_bank_gather_pairs(prs_place_bank* bank, const prs_place_params* params, const prs_place_queries* queries,
                                const prs_place_pairs* pairs) {
  if (!bank) {
    return PRS_ERR_NULL;
  }
  prs_context* ctx = bank->ctx;
  PRS_TRY(check_params(ctx, params, "prs_place_bank_gather_pairs: parameters not set"));
  if (!queries || !pairs) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_bank_gather_pairs: queries or pairs not set");
  }
  if (!queries->desc || !queries->xyz || !queries->n_query || !queries->candidates || !queries->n_candidates || !queries->status ||
      !pairs->fixed_xyz || !pairs->fixed_desc || !pairs->n_fixed || !pairs->moving_xyz || !pairs->moving_desc || !pairs->n_moving ||
      !pairs->X) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_place_bank_gather_pairs: input or output buffer not set");
  }
  if (queries->batch != bank->batch) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_place_bank_gather_pairs: batch differs from the bank's");
  }
  if (queries->query_stride < 1 || queries->query_stride > kPdMaxQuery) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_bank_gather_pairs: query_stride must be in [1, 65536]");
  }
  if (pairs->fixed_stride < queries->query_stride || pairs->moving_stride < bank_largest_map(bank) || pairs->moving_stride < 1) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_place_bank_gather_pairs: a pair slot is smaller than the query or the largest map the bank holds");
  }
  if (!aligned_to(queries->desc, 16) || !aligned_to(queries->xyz, 16) || !aligned_to(pairs->fixed_xyz, 16) || !aligned_to(pairs->fixed_desc, 16) ||
      !aligned_to(pairs->moving_xyz, 16) || !aligned_to(pairs->moving_desc, 16)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_place_bank_gather_pairs: rows must be 16-byte aligned");
  }
  (void) hipSetDevice(ctx->device);
  BankGatherArgs g;
  memset(&g, 0, sizeof(g));
  g.q    = *queries;
  g.o    = *pairs;
  g.d    = bank_dev(bank);
  g.maxc = params->max_candidates;
  const int64_t slots = (int64_t) queries->batch * params->max_candidates;
  return Launches(ctx, "prs_place_bank_gather_pairs", ctx_stream(ctx)).one((slots + 3) / 4, kPdThreads, place_bank_gather_kernel, 0, g);
}

}  // extern "C"
