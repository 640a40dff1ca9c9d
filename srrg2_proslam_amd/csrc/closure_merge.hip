// closure_merge.hip -- the closure merger on the device: folds the landmarks of the map being left (the measurement cloud) into
// the reloaded map (the scene) after an accepted loop closure.
//
// Reference: MergerCorrespondencePointIntensityDescriptor3f, the `closure_merger` of every shipped tracker slice
// (kitti.conf:446-460, euroc.conf:519, icl.conf:773, tum.conf:437, malaga.conf:536), and MergerCorrespondenceProjectiveDepth3D
// (mapping/mergers/merger_correspondence_projective_depth_3d.cpp:7-33), the same merger behind an unprojection.  Their compute
// (MergerCorrespondence_::compute, srrg2_slam_interfaces) is not in the tree: the rule is BUILD-DEFINED, stated in
// include/proslam_hip.h and restated in numpy by tests/closure_merge_ref.py, which this kernel equals bit for bit.
//
// One 256-thread workgroup per (scene, measurement) pair.  LDS: a scene bitmap (duplicate test), four measurement bitmaps
// (merged, candidate, pass-1 winner, chosen), a word-prefix table per compaction and the bin table.  Correspondences name
// distinct landmarks, so each one is merged by its own lane; integer counts are the only things lanes add up.  Which
// measurements are appended, and where, follows from bitmaps alone: a bin's winner is one 64-bit LDS atomic-min on (depth bits,
// index), "the first k set bits" is a prefix count over the bitmap's words, and a chosen measurement's row is the number of
// chosen bits below it -- measurement order by construction, nothing depends on arrival order.
#include <string.h>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kClosureThreads    = 256;
constexpr int kClosureMaxWords   = kClosureThreads;  // one 64-bit bitmap word per thread: measurement_stride <= 16384
constexpr uint32_t kClosureLds   = 64u * 1024u;
constexpr unsigned long long kBinEmpty   = ~0ull;
constexpr unsigned long long kBinBlocked = 0ull;  // below every key: the depth of a binned candidate is > 0

struct ClosureArgs {
  prs_closure_merger_params p;
  prs_closure_merge_batch b;
  float row_w, col_w;  // bin widths in pixels (merger_projective_impl.cpp:30-33)
  int nbr, nbc;        // bin table extent
  int n_words;         // 64-bit words of a measurement bitmap
  uint32_t off_seen, off_merged, off_cand, off_pass1, off_chosen, off_prefix, off_bins, off_sh, off_scan;
};

struct ClosureShared {
  float measurement_in_scene[16];
  float scene_in_world[16];
  int error;
  int fault;
  int gated_off;
  int n_merged;
};

// the measurement in its own frame; false: never merged or added
__device__ __forceinline__ bool closure_point(const prs_closure_merger_params& P, const float4 z, float* p) {
  if (P.measurement_kind == PRS_CLOSURE_UVD) {
    const float d = z.z;
    p[0]          = (z.x - P.cx) / P.fx * d;  // the expression of PRS_MERGER_DEPTH_EKF (mapping.hip; one function for both changes that kernel's code)
    p[1]          = (z.y - P.cy) / P.fy * d;
    p[2]          = d;
    return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]) && d > 0.0f;
  }
  p[0] = z.x;
  p[1] = z.y;
  p[2] = z.z;
  return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]);
}

// bin of a measurement, -1: unbinned (behind the camera or off the canvas)
__device__ __forceinline__ int closure_bin(const ClosureArgs& a, const float4 z, const float* p) {
  const prs_closure_merger_params& P = a.p;
  float u, v;
  if (P.measurement_kind == PRS_CLOSURE_UVD) {
    u = z.x;
    v = z.y;
  } else {
    if (!(p[2] > 0.0f)) {
      return -1;
    }
    u = P.fx * p[0] / p[2] + P.cx;
    v = P.fy * p[1] / p[2] + P.cy;
  }
  if (!(u >= 0.0f && u < (float) P.canvas_cols && v >= 0.0f && v < (float) P.canvas_rows)) {
    return -1;
  }
  const int br = (int) roundf(v / a.row_w), bc = (int) roundf(u / a.col_w);  // merger_projective_impl.cpp:84-85
  if (br >= a.nbr || bc >= a.nbc) {
    return -1;
  }
  return br * a.nbc + bc;
}

__device__ __forceinline__ unsigned long long closure_key(float depth, int index) {
  return ((unsigned long long) __float_as_uint(depth) << 32) | (unsigned long long) (uint32_t) index;  // positive floats order as integers
}

// the lowest k set bits of `word`, which has `before` set bits in the words below it
__device__ __forceinline__ unsigned long long take_first(unsigned long long word, int before, int k) {
  int room = k - before;
  if (room <= 0) {
    return 0ull;
  }
  while (__popcll(word) > room) {
    word &= ~(1ull << (63 - __clzll((long long) word)));
  }
  return word;
}

__device__ __forceinline__ bool bit_of(const unsigned long long* bits, int i) {
  return (bits[i >> 6] >> (i & 63)) & 1ull;
}

__global__ __launch_bounds__(kClosureThreads) void closure_merge_kernel(const ClosureArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* seen             = reinterpret_cast<uint32_t*>(smem + a.off_seen);  // scene indices already named
  uint32_t* merged32         = reinterpret_cast<uint32_t*>(smem + a.off_merged);
  unsigned long long* merged = reinterpret_cast<unsigned long long*>(smem + a.off_merged);  // measurements merged
  unsigned long long* cand   = reinterpret_cast<unsigned long long*>(smem + a.off_cand);    // valid and not merged
  unsigned long long* pass1  = reinterpret_cast<unsigned long long*>(smem + a.off_pass1);   // bin winners
  unsigned long long* chosen = reinterpret_cast<unsigned long long*>(smem + a.off_chosen);  // to append
  int* prefix                = reinterpret_cast<int*>(smem + a.off_prefix);                 // chosen bits below each word
  unsigned long long* bins   = reinterpret_cast<unsigned long long*>(smem + a.off_bins);
  ClosureShared& sh          = *reinterpret_cast<ClosureShared*>(smem + a.off_sh);
  uint64_t* scan             = reinterpret_cast<uint64_t*>(smem + a.off_scan);
  const int tid              = threadIdx.x;
  const int lane             = tid & 63;
  const int pair             = blockIdx.x;
  const prs_closure_merge_batch& B   = a.b;
  const prs_closure_merger_params& P = a.p;
  const int nbins    = a.nbr * a.nbc;
  const int n_points = B.n_points[pair];
  // counts as the caller gave them; the clamped values only keep the loops of a refused pair inside the rows
  const int n_meas_in = B.n_measured[pair];
  const int n_corr_in = B.n_corr ? B.n_corr[pair] : 0;
  const int n_meas    = n_meas_in < 0 ? 0 : (n_meas_in > B.measurement_stride ? B.measurement_stride : n_meas_in);
  const int n_corr    = n_corr_in < 0 ? 0 : (n_corr_in > B.corr_stride ? B.corr_stride : n_corr_in);
  const size_t row0   = (size_t) pair * (size_t) B.capacity;
  const float4* __restrict__ zs     = reinterpret_cast<const float4*>(B.measurement) + (size_t) pair * B.measurement_stride;
  const uint8_t* __restrict__ zdesc = B.measurement_desc + (size_t) pair * B.measurement_stride * 32;
  const prs_corr* __restrict__ corr = B.corr ? B.corr + (size_t) pair * B.corr_stride : nullptr;
  float4* coords = reinterpret_cast<float4*>(B.coords) + row0;
  float4* state  = B.state ? reinterpret_cast<float4*>(B.state) + row0 : nullptr;

  if (tid == 0) {
    float T[16];
    for (int i = 0; i < 16; ++i) {
      T[i] = B.transform[(size_t) pair * 16 + i];
    }
    if (B.transform_is_scene_in_measurement) {
      se3_inverse(T, sh.measurement_in_scene);
    } else {
      for (int i = 0; i < 16; ++i) {
        sh.measurement_in_scene[i] = T[i];
      }
    }
    for (int i = 0; i < 16; ++i) {
      sh.scene_in_world[i] = B.scene_in_world ? B.scene_in_world[(size_t) pair * 16 + i] : (i % 5 == 0 ? 1.0f : 0.0f);
    }
    sh.gated_off = B.gate && B.gate[pair].accepted == 0;
    sh.error     = (n_points < 0 || n_points > B.capacity || n_meas_in < 0 || n_corr_in < 0) ? PRS_ERR_RANGE : 0;
    if (!sh.error && (n_meas_in > B.measurement_stride || n_corr_in > B.corr_stride)) {
      sh.error = PRS_ERR_CAPACITY;
    }
    sh.fault    = 0;
    sh.n_merged = 0;
  }
  for (int i = tid; i < nbins; i += kClosureThreads) {
    bins[i] = kBinEmpty;
  }
  for (int i = tid; i < (B.capacity + 31) / 32; i += kClosureThreads) {
    seen[i] = 0u;
  }
  for (int i = tid; i < a.n_words; i += kClosureThreads) {
    merged[i] = 0ull;
    cand[i]   = 0ull;
    pass1[i]  = 0ull;
    chosen[i] = 0ull;
  }
  __syncthreads();
  if (sh.gated_off || sh.error) {  // (block-uniform)
    if (tid == 0) {
      B.result[pair].n_merged = 0;
      B.result[pair].n_added  = 0;
      B.result[pair].status   = sh.gated_off ? PRS_OK : sh.error;
    }
    return;
  }

  // ---- the correspondence vector: refused whole before anything is written -----------------------------------
  for (int c = tid; c < n_corr; c += kClosureThreads) {
    const prs_corr cr = corr[c];
    const int s       = B.corr_from_aligner ? cr.moving_idx : cr.fixed_idx;
    const int m       = B.corr_from_aligner ? cr.fixed_idx : cr.moving_idx;
    // a fault only raises a flag here (which of two entries naming one landmark meets the other's bit is arbitrary); the
    // code reported is settled below, in vector order
    if (s < 0 || s >= n_points || m < 0 || m >= n_meas) {
      sh.fault = 1;
    } else if (atomicOr(&seen[s >> 5], 1u << (s & 31)) & (1u << (s & 31))) {
      sh.fault = 1;
    }
  }
  __syncthreads();
  if (sh.fault) {
    // rare, and the pair is refused: the FIRST fault in vector order, as a sequential walk meets it, on a cleared bitmap
    for (int i = tid; i < (B.capacity + 31) / 32; i += kClosureThreads) {
      seen[i] = 0u;
    }
    __syncthreads();
    if (tid == 0) {
      int code = 0;
      for (int c = 0; c < n_corr && !code; ++c) {
        const prs_corr cr = corr[c];
        const int s       = B.corr_from_aligner ? cr.moving_idx : cr.fixed_idx;
        const int m       = B.corr_from_aligner ? cr.fixed_idx : cr.moving_idx;
        if (s < 0 || s >= n_points || m < 0 || m >= n_meas) {
          code = PRS_ERR_RANGE;
        } else if (seen[s >> 5] & (1u << (s & 31))) {
          code = PRS_ERR_DUPLICATE;
        } else {
          seen[s >> 5] |= 1u << (s & 31);
        }
      }
      B.result[pair].n_merged = 0;
      B.result[pair].n_added  = 0;
      B.result[pair].status   = code;
    }
    return;
  }

  // ---- merge: one correspondence per lane ---------------------------------------------------------------------------
  for (int c0 = 0; c0 < n_corr; c0 += kClosureThreads) {
    const int c = c0 + tid;
    bool ok     = false;
    if (c < n_corr) {
      const prs_corr cr = corr[c];
      const int s       = B.corr_from_aligner ? cr.moving_idx : cr.fixed_idx;
      const int m       = B.corr_from_aligner ? cr.fixed_idx : cr.moving_idx;
      float p[3], q[3] = {0.0f, 0.0f, 0.0f};
      const bool valid = closure_point(P, zs[m], p);
      float4 l         = coords[s];
      if (valid && !(cr.response >= P.maximum_response)) {
        se3_apply(sh.measurement_in_scene, p, q);
        const float dx = l.x - q[0], dy = l.y - q[1], dz = l.z - q[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        ok             = d2 < P.maximum_distance_geometry_squared;
      }
      if (ok) {
        l.x       = 0.5f * (l.x + q[0]);
        l.y       = 0.5f * (l.y + q[1]);
        l.z       = 0.5f * (l.z + q[2]);
        coords[s] = l;
        const uint4* src = reinterpret_cast<const uint4*>(zdesc + 32 * (size_t) m);  // merger_projective_impl.cpp:186
        uint4* dst       = reinterpret_cast<uint4*>(B.desc + 32 * (row0 + (size_t) s));
        dst[0]           = src[0];
        dst[1]           = src[1];
        atomicOr(&merged32[m >> 5], 1u << (m & 31));
        if (B.n_opt) {
          B.n_opt[row0 + s] += 1u;
        }
        if (state) {
          const float lp[3] = {l.x, l.y, l.z};
          float w[3];
          se3_apply(sh.scene_in_world, lp, w);
          state[s] = make_float4(w[0], w[1], w[2], 0.0f);
        }
      }
      if (B.inlier) {
        B.inlier[row0 + s] = ok ? 1 : 0;  // :66
      }
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0 && bal) {
      atomicAdd(&sh.n_merged, __popcll(bal));
    }
  }
  __syncthreads();
  const int n_merged = sh.n_merged;
  int n_to_add       = 0;  // merger_projective_impl.cpp:158-163
  if ((uint32_t) n_merged < P.target_number_of_merges) {
    const long long by_target = (long long) P.target_number_of_merges - n_merged, by_size = (long long) n_meas - n_merged;
    const long long least     = by_target < by_size ? by_target : by_size;
    n_to_add                  = least < 0 ? 0 : (int) least;
  }

  // ---- candidates (valid, not merged); bins that hold a merged measurement are blocked --------------------------------
  for (int i0 = 0; i0 < n_meas; i0 += kClosureThreads) {  // (a wave covers one bitmap word per round)
    const int i    = i0 + tid;
    bool candidate = false;
    if (i < n_meas) {
      const float4 z = zs[i];
      float p[3];
      const bool valid  = closure_point(P, z, p);
      const bool is_merged = bit_of(merged, i);
      candidate         = valid && !is_merged;
      if (P.enable_binning && is_merged) {
        const int bin = closure_bin(a, z, p);
        if (bin >= 0) {
          bins[bin] = kBinBlocked;
        }
      }
    }
    const unsigned long long bal = __ballot(candidate);
    if (lane == 0 && i < n_meas) {
      cand[i >> 6] = bal;
    }
  }
  __syncthreads();
  uint64_t total = 0;
  const unsigned long long my_cand = tid < a.n_words ? cand[tid] : 0ull;
  (void) block_exclusive_scan_u64((uint64_t) __popcll(my_cand), scan, total);
  const int n_cand  = (int) total;
  const int n_added = n_cand < n_to_add ? n_cand : n_to_add;

  // ---- pass 1, only when the cap bites: per free bin the candidate with the smallest depth (lowest index on ties) ------
  if (P.enable_binning && n_cand > n_to_add) {  // (block-uniform)
    for (int i = tid; i < n_meas; i += kClosureThreads) {
      if (bit_of(cand, i)) {
        const float4 z = zs[i];
        float p[3];
        (void) closure_point(P, z, p);
        const int bin = closure_bin(a, z, p);
        if (bin >= 0) {
          atomicMin(&bins[bin], closure_key(p[2], i));  // a blocked bin stays 0
        }
      }
    }
    __syncthreads();
    for (int i0 = 0; i0 < n_meas; i0 += kClosureThreads) {
      const int i = i0 + tid;
      bool winner = false;
      if (i < n_meas && bit_of(cand, i)) {
        const float4 z = zs[i];
        float p[3];
        (void) closure_point(P, z, p);
        const int bin = closure_bin(a, z, p);
        winner        = bin >= 0 && bins[bin] == closure_key(p[2], i);
      }
      const unsigned long long bal = __ballot(winner);
      if (lane == 0 && i < n_meas) {
        pass1[i >> 6] = bal;
      }
    }
    __syncthreads();
  }
  // pass 1 keeps its lowest n_to_add indices; pass 2 fills what is left from the other candidates in measurement order
  const unsigned long long my_p1 = tid < a.n_words ? pass1[tid] : 0ull;
  const int before_p1   = (int) block_exclusive_scan_u64((uint64_t) __popcll(my_p1), scan, total);
  const int n_pass1     = (int) total < n_to_add ? (int) total : n_to_add;
  const unsigned long long my_rest = my_cand & ~my_p1;
  const int before_rest = (int) block_exclusive_scan_u64((uint64_t) __popcll(my_rest), scan, total);
  const unsigned long long my_chosen = take_first(my_p1, before_p1, n_to_add) | take_first(my_rest, before_rest, n_to_add - n_pass1);
  const int before_chosen = (int) block_exclusive_scan_u64((uint64_t) __popcll(my_chosen), scan, total);
  if (tid < a.n_words) {
    chosen[tid] = my_chosen;
    prefix[tid] = before_chosen;
  }
  __syncthreads();

  if (n_points + n_added > B.capacity) {  // decided before anything is appended
    if (tid == 0) {
      B.result[pair].n_merged = n_merged;
      B.result[pair].n_added  = 0;
      B.result[pair].status   = PRS_ERR_SCENE_FULL;
    }
    return;
  }

  // ---- append in ascending measurement index ---------------------------------------------------------------------------------
  for (int i = tid; i < n_meas; i += kClosureThreads) {
    const unsigned long long word = chosen[i >> 6];
    if (!((word >> (i & 63)) & 1ull)) {
      continue;
    }
    const int r = n_points + prefix[i >> 6] + __popcll(word & ((1ull << (i & 63)) - 1ull));
    float p[3], q[3];
    (void) closure_point(P, zs[i], p);
    se3_apply(sh.measurement_in_scene, p, q);
    coords[r]        = make_float4(q[0], q[1], q[2], 0.0f);
    const uint4* src = reinterpret_cast<const uint4*>(zdesc + 32 * (size_t) i);
    uint4* dst       = reinterpret_cast<uint4*>(B.desc + 32 * (row0 + (size_t) r));
    dst[0]           = src[0];
    dst[1]           = src[1];
    if (state) {  // merger_projective_impl.cpp:317-320
      float w[3];
      se3_apply(sh.scene_in_world, q, w);
      state[r] = make_float4(w[0], w[1], w[2], 0.0f);
    }
    if (B.covariance) {
      float* cov = B.covariance + 9 * (row0 + (size_t) r);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        cov[k] = (k % 4 == 0) ? 1.0f : 0.0f;
      }
    }
    if (B.n_opt) {
      B.n_opt[row0 + r] = 0u;
    }
    if (B.inlier) {
      B.inlier[row0 + r] = 1;
    }
    if (B.n_meas) {
      B.n_meas[row0 + r] = 0u;
    }
  }
  if (tid == 0) {
    B.n_points[pair]        = n_points + n_added;
    B.result[pair].n_merged = n_merged;
    B.result[pair].n_added  = n_added;
    B.result[pair].status   = PRS_OK;
  }
}

uint32_t cm_align16(uint32_t v) {
  return (v + 15u) & ~15u;
}

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

}  // namespace

int closure_merge_launch(prs_context* ctx, const prs_closure_merger_params* params, const prs_closure_merge_batch* batch) {
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_closure_merge_batch_run: parameters not set");
  }
  const prs_closure_merge_batch& b = *batch;
  if (!b.coords || !b.desc || !b.n_points) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_closure_merge_batch_run: scene not set");
  }
  if (!b.measurement || !b.measurement_desc || !b.n_measured || !b.transform || !b.result || (b.corr_stride > 0 && (!b.corr || !b.n_corr))) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_closure_merge_batch_run: measurement, correspondences or transform not set");
  }
  if (b.state && !b.scene_in_world) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_closure_merge_batch_run: a map that keeps `state` needs scene_in_world");
  }
  if (b.batch <= 0) {
    return PRS_OK;
  }
  const prs_closure_merger_params& p = *params;
  if ((p.measurement_kind != PRS_CLOSURE_XYZ && p.measurement_kind != PRS_CLOSURE_UVD) || b.capacity <= 0 || b.measurement_stride <= 0 ||
      b.corr_stride < 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_closure_merge_batch_run: unknown measurement kind or empty strides");
  }
  if (!aligned16(b.coords) || !aligned16(b.desc) || !aligned16(b.measurement) || !aligned16(b.measurement_desc) || !aligned16(b.state)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_closure_merge_batch_run: coordinate and descriptor rows must be 16-byte aligned");
  }
  ClosureArgs a;
  a.p     = p;
  a.b     = b;
  a.row_w = a.col_w = 1.0f;
  a.nbr = a.nbc = 0;
  if (p.enable_binning) {
    if (p.number_of_row_bins == 0 || p.number_of_col_bins == 0 || p.number_of_row_bins > 4096 || p.number_of_col_bins > 4096 || p.canvas_rows <= 0 ||
        p.canvas_cols <= 0) {
      return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_closure_merge_batch_run: binning needs a canvas and 1 .. 4096 bins a side");
    }
    a.row_w = (float) p.canvas_rows / (float) p.number_of_row_bins;  // merger_projective_impl.cpp:30-33
    a.col_w = (float) p.canvas_cols / (float) p.number_of_col_bins;
    a.nbr   = (int) p.number_of_row_bins + 2;
    a.nbc   = (int) p.number_of_col_bins + 2;
  }
  if (b.measurement_stride > kClosureMaxWords * 64) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_closure_merge_batch_run: measurement_stride above 16384");
  }
  a.n_words = (b.measurement_stride + 63) / 64;
  const uint64_t nbins = (uint64_t) a.nbr * (uint64_t) a.nbc;
  const uint64_t need  = ((uint64_t) b.capacity + 31) / 32 * 4 + (uint64_t) a.n_words * (4 * 8 + 4) + nbins * 8 + sizeof(ClosureShared) + 17 * 8 + 10 * 16;
  if (need > kClosureLds) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_closure_merge_batch_run: scene bitmap + measurement bitmaps + bin table do not fit 64 KiB of LDS");
  }
  uint32_t off = 0;
  a.off_bins   = off; off = cm_align16(off + (uint32_t) nbins * 8);
  a.off_merged = off; off = cm_align16(off + (uint32_t) a.n_words * 8);
  a.off_cand   = off; off = cm_align16(off + (uint32_t) a.n_words * 8);
  a.off_pass1  = off; off = cm_align16(off + (uint32_t) a.n_words * 8);
  a.off_chosen = off; off = cm_align16(off + (uint32_t) a.n_words * 8);
  a.off_scan   = off; off = cm_align16(off + 17 * 8);
  a.off_prefix = off; off = cm_align16(off + (uint32_t) a.n_words * 4);
  a.off_seen   = off; off = cm_align16(off + ((uint32_t) b.capacity + 31) / 32 * 4);
  a.off_sh     = off; off = cm_align16(off + (uint32_t) sizeof(ClosureShared));
  return Launches(ctx, "prs_closure_merge_batch_run", ctx_stream(ctx)).one(b.batch, kClosureThreads, closure_merge_kernel, off, a);
}

}  // namespace prs

extern "C" {

int prs_closure_merge_batch_run(prs_context* ctx, const prs_closure_merger_params* params, const prs_closure_merge_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  return prs::closure_merge_launch(ctx, params, batch);
}

void prs_closure_merge_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_closure_merger_params);
  sizes2[1] = sizeof(prs_closure_merge_batch);
}

// host pointers, one pair: everything staged in ONE block (prs::Staging), one upload, one launch, one download
int prs_closure_merge(prs_context* ctx, const prs_closure_merger_params* params, int32_t capacity, int32_t* n_points, float* coords4,
                      uint8_t* desc, float* state4, float* covariance9, uint32_t* n_opt, uint8_t* inlier, uint32_t* n_meas,
                      const float* scene_in_world16, const float* measurement4, const uint8_t* measurement_desc, int32_t n_measured,
                      const prs_corr* corr, int32_t n_corr, int32_t corr_from_aligner, const float* transform16,
                      int32_t transform_is_scene_in_measurement, prs_merge_result* result) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (!params || !n_points || !coords4 || !desc || !transform16 || !result || (state4 && !scene_in_world16)) {
    return prs::ctx_fail(ctx, PRS_ERR_NULL, "prs_closure_merge: parameters, scene, transform or result not set");
  }
  if (capacity <= 0 || n_measured < 0 || n_corr < 0) {
    return prs::ctx_fail(ctx, PRS_ERR_RANGE, "prs_closure_merge: capacity must be positive, counts not negative");
  }
  if ((n_measured > 0 && (!measurement4 || !measurement_desc)) || (n_corr > 0 && !corr)) {
    return prs::ctx_fail(ctx, PRS_ERR_NULL, "prs_closure_merge: measurement or correspondences not set");
  }
  (void) hipSetDevice(ctx->device);
  const size_t cap = (size_t) capacity, nm = (size_t) (n_measured > 0 ? n_measured : 1), nc = (size_t) (n_corr > 0 ? n_corr : 1);
  // the scene travels both ways as ONE section (rows of 16 + 32 + 16 + 36 + 4 + 4 + 1 bytes, array after array), the frame up
  struct Head {
    int32_t n_points, n_measured, n_corr, pad;
    prs_merge_result result;
    int32_t pad2;
    float transform[16];
    float scene_in_world[16];
  };
  const size_t o_coords = 0, o_desc = o_coords + prs::align256(cap * 16), o_state = o_desc + prs::align256(cap * 32),
               o_cov = o_state + prs::align256(cap * 16), o_nopt = o_cov + prs::align256(cap * 36), o_nmeas = o_nopt + prs::align256(cap * 4),
               o_inl = o_nmeas + prs::align256(cap * 4), scene_bytes = o_inl + prs::align256(cap);
  prs::Staging st(ctx, "prs_closure_merge");
  auto s_z     = st.up<float>(nm * 4);
  auto s_zdesc = st.up<uint8_t>(nm * 32);
  auto s_corr  = st.up<prs_corr>(nc);
  auto s_head  = st.both<Head>(1);
  auto s_scene = st.both<unsigned char>(scene_bytes);
  PRS_TRY(st.commit());
  if (n_measured > 0) {
    memcpy(s_z.h(), measurement4, (size_t) n_measured * 16);
    memcpy(s_zdesc.h(), measurement_desc, (size_t) n_measured * 32);
  }
  if (n_corr > 0) {
    memcpy(s_corr.h(), corr, (size_t) n_corr * sizeof(prs_corr));
  }
  Head* hd = s_head.h();
  memset(hd, 0, sizeof(Head));
  hd->n_points   = *n_points;
  hd->n_measured = n_measured;
  hd->n_corr     = n_corr;
  memcpy(hd->transform, transform16, 64);
  if (scene_in_world16) {
    memcpy(hd->scene_in_world, scene_in_world16, 64);
  }
  unsigned char* hs = s_scene.h();
  memcpy(hs + o_coords, coords4, cap * 16);
  memcpy(hs + o_desc, desc, cap * 32);
  if (state4) memcpy(hs + o_state, state4, cap * 16);
  if (covariance9) memcpy(hs + o_cov, covariance9, cap * 36);
  if (n_opt) memcpy(hs + o_nopt, n_opt, cap * 4);
  if (n_meas) memcpy(hs + o_nmeas, n_meas, cap * 4);
  if (inlier) memcpy(hs + o_inl, inlier, cap);
  PRS_TRY(st.upload());
  unsigned char* ds = s_scene.d();
  Head* dh          = s_head.d();
  prs_closure_merge_batch b;
  memset(&b, 0, sizeof(b));
  b.batch = 1;
  b.capacity = capacity;
  b.coords = reinterpret_cast<float*>(ds + o_coords);
  b.desc = ds + o_desc;
  b.n_points = &dh->n_points;
  b.state = state4 ? reinterpret_cast<float*>(ds + o_state) : nullptr;
  b.covariance = covariance9 ? reinterpret_cast<float*>(ds + o_cov) : nullptr;
  b.n_opt = n_opt ? reinterpret_cast<uint32_t*>(ds + o_nopt) : nullptr;
  b.n_meas = n_meas ? reinterpret_cast<uint32_t*>(ds + o_nmeas) : nullptr;
  b.inlier = inlier ? ds + o_inl : nullptr;
  b.scene_in_world = state4 ? dh->scene_in_world : nullptr;
  b.measurement_stride = (int32_t) nm;
  b.measurement = s_z.d();
  b.measurement_desc = s_zdesc.d();
  b.n_measured = &dh->n_measured;
  b.corr_stride = (int32_t) nc;
  b.corr = s_corr.d();
  b.n_corr = &dh->n_corr;
  b.corr_from_aligner = corr_from_aligner ? 1 : 0;
  b.transform = dh->transform;
  b.transform_is_scene_in_measurement = transform_is_scene_in_measurement ? 1 : 0;
  b.result = &dh->result;
  PRS_TRY(prs::closure_merge_launch(ctx, params, &b));
  PRS_TRY(st.download());
  *result   = hd->result;
  *n_points = hd->n_points;
  memcpy(coords4, hs + o_coords, cap * 16);
  memcpy(desc, hs + o_desc, cap * 32);
  if (state4) memcpy(state4, hs + o_state, cap * 16);
  if (covariance9) memcpy(covariance9, hs + o_cov, cap * 36);
  if (n_opt) memcpy(n_opt, hs + o_nopt, cap * 4);
  if (n_meas) memcpy(n_meas, hs + o_nmeas, cap * 4);
  if (inlier) memcpy(inlier, hs + o_inl, cap);
  return hd->result.status;
}

}  // extern "C"
