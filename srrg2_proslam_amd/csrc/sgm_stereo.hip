// sgm_stereo.hip -- semi-global dense stereo on the device: a rectified pair to a disparity and a depth image by path-aggregated
// census costs (prs_sgm_stereo_batch_run; the rule is stated in include/proslam_hip.h, BUILD-DEFINED, and restated in
// tests/sgm_stereo_ref.py).  Every decision is integer arithmetic; the only rounded operations are one float32 division and one
// addition (sub-pixel) and one division (depth) a pixel.  The census and the finish kernel are dense stereo's (dense_stereo.hip),
// launched once for all images; the images are worked through in chunks of images_in_flight, which share one volume S
// [chunk][rows][cols][n_disparities] uint16, indexed with 64-bit offsets.
//   path     one launch a direction of travel (dy, dx); a wave owns a line and walks it, so nothing is handed from wave to wave.  For
//            dy = 0 the line is a row.  Otherwise it starts at column x0 of the first row in the direction of travel and visits
//            (y, (x0 + t * dx) mod cols); where it wraps, the predecessor lies outside the image and the path restarts with L = C.
//            Lane l holds the K neighbouring disparities l * K .. l * K + K - 1 (K = 1, 2, 4 for up to 64, 128, 256), so i - 1 and
//            i + 1 are the neighbouring register, and one shuffle up and one down a step serve the lane borders whatever K is; m is
//            one DPP reduction.  Disparities at or beyond n_disparities carry kBig, which stays above every real cost after + P1 and
//            never wraps 32 bits.  C comes from the census words by 64-bit popcounts and is never stored.  The first direction
//            stores S, the later ones read, add and store: the launches are ordered on the stream, so there are no atomics.  The
//            census words and S values of the next four steps (two at K = 4) are loaded before this step's arithmetic.  When K divides n_disparities a lane
//            moves its K values of S as one 4- or 8-byte word (VEC).  (dy, dx) are launch arguments, not template parameters: they
//            only steer scalar address arithmetic a step, and K x VEC already makes five instantiations.
//   winner   a wave a pixel at a time, kWinnerRun pixels a wave, lane l the disparities l, l + 64, ..: the left winner as a packed
//            (S << 16) | i minimum, A2, the uniqueness test and the sub-pixel rule (the winner's neighbours by shuffles from the lanes
//            that hold them) into dense stereo's records, which the lanes keep and store once a run
//   right    with the left-right check: the right winners from the diagonals S(y, x + d_i, i), a workgroup 128 right pixels of a
//            row, the row's slice of the volume staged in LDS 64 disparities at a time (see the kernel)
// Plain launches: no persistent workgroup, no spinning, no workgroup waits for another.
#include <stddef.h>

#include <string>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"

namespace prs {

namespace {

constexpr int kThreads   = 256;
constexpr int kWaves     = kThreads / PRS_WAVE;
constexpr int kWinnerRun = 16;  // pixels a winner wave takes, one after another
constexpr int kRightTile  = 128;                     // right pixels of a right-winner workgroup, two threads each
constexpr int kRightRows  = kRightTile + PRS_WAVE;   // the pixels it stages for 64 disparities (kRightTile + 63 are reached)
constexpr int kRightPitch = PRS_WAVE + 2;            // halfwords of a staged pixel: 33 words
constexpr uint32_t kBig    = 1u << 20;       // a path cost that is not there: above 4157 + 4095, and far from wrapping

struct SgmArgs {
  prs_sgm_stereo_params p;
  int32_t frames, rows, cols;
  const int32_t* n_images;
  int32_t image0;   // the first image of the chunk
  int32_t n_chunk;  // its images
  int32_t runs;     // ceil(rows * cols / kWinnerRun): the winner waves of an image
  int32_t rtiles;   // ceil(cols / kRightTile): the right-winner workgroups of a row
  const uint64_t* census_l;  // [images][rows][cols]
  const uint64_t* census_r;
  uint16_t* vol;             // [n_chunk][rows][cols][n_disparities]
  uint2* rec_l;              // [images][rows][cols] dense stereo's records
  int16_t* win_r;            // [images][rows][cols] i* of the right pixel or -1 (lr_max_diff >= 0 only)
};

// whether image `image` of the batch is one the call works on (its sequence is in range and long enough)
__device__ __forceinline__ bool served(const SgmArgs& a, const uint32_t image) {
  const int f = (int) (image % (uint32_t) a.frames), b = (int) (image / (uint32_t) a.frames);
  const int n = a.n_images ? a.n_images[b] : a.frames;
  return n >= 0 && n <= a.frames && f < n;
}

template <int K>
struct Step {
  uint64_t cl;
  uint64_t cr[K];
  uint32_t s[K];
};

// ---- path: wave blockIdx.x * kWaves + w = slot * lines + line ----------------------------------------------------------------------
template <int K, bool VEC>
__global__ __launch_bounds__(kThreads) void sgm_path_kernel(const SgmArgs a, const int dy, const int dx, const int first) {
  const int lane  = threadIdx.x & (PRS_WAVE - 1);
  const int64_t g = (int64_t) blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int rows = a.rows, cols = a.cols, n = a.p.n_disparities, d0 = a.p.min_disparity;
  const int lines = dy == 0 ? rows : cols;
  const int slot  = (int) (g / lines), line = (int) (g - (int64_t) slot * lines);
  if (slot >= a.n_chunk) {
    return;
  }
  const uint32_t image = (uint32_t) (a.image0 + slot);
  if (!served(a, image)) {
    return;
  }
  const size_t image_px = (size_t) rows * (size_t) cols;
  const uint64_t* cl    = a.census_l + (size_t) image * image_px;
  const uint64_t* cr    = a.census_r + (size_t) image * image_px;
  uint16_t* vol         = a.vol + (size_t) slot * image_px * (size_t) n;
  const uint32_t P1 = (uint32_t) a.p.p1, P2 = (uint32_t) a.p.p2;
  const int i0 = lane * K;  // the lane's disparities i0 .. i0 + K - 1

  const auto load = [&](const int y, const int x, Step<K>& t) {
    const size_t px = (size_t) y * (size_t) cols + (size_t) x;
    t.cl            = cl[px];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      t.cr[k] = cr[px - (size_t) min(d0 + i0 + k, x)];  // column max(x - d_i, 0): inside the row for every lane
    }
    if (!first) {
      const uint16_t* s = vol + px * (size_t) n + i0;
      if (VEC) {  // K divides n: the lane's K values are all there or all beyond n, and aligned to their 2 K bytes
        if (i0 < n) {
          if constexpr (K == 1) {
            t.s[0] = s[0];
          } else if constexpr (K == 2) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(s);
            t.s[0] = v & 0xffffu, t.s[1] = v >> 16;
          } else {
            const uint2 v = *reinterpret_cast<const uint2*>(s);
            t.s[0] = v.x & 0xffffu, t.s[1] = v.x >> 16, t.s[2] = v.y & 0xffffu, t.s[3] = v.y >> 16;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if (i0 + k < n) {
            t.s[k] = s[k];
          }
        }
      }
    }
  };

  // two cursors on the line: `at` is the pixel being computed, `ahead` the pixel whose words are being loaded, kDepth steps on
  struct Cursor {
    int y, x;
    bool restart;  // the predecessor lies outside the image: the path starts again with L = C
  };
  const auto advance = [&](Cursor& c) {
    c.y += dy, c.x += dx, c.restart = false;
    if (dy != 0) {
      if (c.x < 0) {
        c.x = cols - 1, c.restart = true;
      } else if (c.x >= cols) {
        c.x = 0, c.restart = true;
      }
    }
  };
  constexpr int kDepth = K == 4 ? 2 : 4;  // steps loaded ahead: one was not enough to keep the memory pipes full
  const int steps = dy == 0 ? cols : rows;
  Cursor at = {dy == 0 ? line : (dy > 0 ? 0 : rows - 1), dy == 0 ? (dx > 0 ? 0 : cols - 1) : line, true}, ahead = at;
  int loaded = 0;
  uint32_t L[K];
  Step<K> ring[kDepth];
#pragma unroll
  for (int d = 0; d < kDepth; ++d) {
    ring[d] = {};
    if (loaded < steps) {
      load(ahead.y, ahead.x, ring[d]);
      advance(ahead);
      ++loaded;
    }
  }
  for (int t = 0; t < steps; t += kDepth) {
#pragma unroll
    for (int d = 0; d < kDepth; ++d) {
      if (t + d >= steps) {
        break;
      }
      const Step<K> cur = ring[d];
      if (loaded < steps) {
        load(ahead.y, ahead.x, ring[d]);
        advance(ahead);
        ++loaded;
      }
      const int y = at.y, x = at.x;
      const bool restart = at.restart;
      uint32_t c[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        c[k] = (uint32_t) __popcll(cur.cl ^ cur.cr[k]);
      }
      if (restart) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          L[k] = i0 + k < n ? c[k] : kBig;
        }
      } else {
        uint32_t m = L[0];
#pragma unroll
        for (int k = 1; k < K; ++k) {
          m = min(m, L[k]);
        }
        m = wave_min_u32(m);
        uint32_t below = (uint32_t) __shfl_up((int) L[K - 1], 1, PRS_WAVE), above = (uint32_t) __shfl_down((int) L[0], 1, PRS_WAVE);
        below = lane == 0 ? kBig : below;
        above = lane == PRS_WAVE - 1 ? kBig : above;
        uint32_t Ln[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const uint32_t lo = k == 0 ? below : L[k == 0 ? 0 : k - 1], hi = k == K - 1 ? above : L[k == K - 1 ? k : k + 1];
          const uint32_t v  = min(min(L[k], m + P2), min(lo, hi) + P1);
          Ln[k] = i0 + k < n ? c[k] + v - m : kBig;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
          L[k] = Ln[k];
        }
      }
      uint16_t* s = vol + ((size_t) y * (size_t) cols + (size_t) x) * (size_t) n + i0;
      uint32_t out[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        out[k] = first ? L[k] : cur.s[k] + L[k];
      }
      if (VEC) {
        if (i0 < n) {
          if constexpr (K == 1) {
            s[0] = (uint16_t) out[0];
          } else if constexpr (K == 2) {
            *reinterpret_cast<uint32_t*>(s) = out[0] | (out[1] << 16);
          } else {
            *reinterpret_cast<uint2*>(s) = make_uint2(out[0] | (out[1] << 16), out[2] | (out[3] << 16));
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if (i0 + k < n) {
            s[k] = (uint16_t) out[k];
          }
        }
      }
      advance(at);
    }
  }
}

// ---- winner: wave blockIdx.x * kWaves + w = slot * runs + run, a run kWinnerRun pixels of an image in raster order ------------------
template <int K>
__global__ __launch_bounds__(kThreads) void sgm_winner_kernel(const SgmArgs a) {
  const int lane  = threadIdx.x & (PRS_WAVE - 1);
  const int64_t g = (int64_t) blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  const int slot  = (int) (g / a.runs), run = (int) (g - (int64_t) slot * a.runs);
  if (slot >= a.n_chunk) {
    return;
  }
  const uint32_t image = (uint32_t) (a.image0 + slot);
  if (!served(a, image)) {
    return;
  }
  const int rows = a.rows, cols = a.cols, n = a.p.n_disparities, d0 = a.p.min_disparity, q = a.p.uniqueness_percent;
  const size_t image_px = (size_t) rows * (size_t) cols;
  const uint16_t* vol   = a.vol + (size_t) slot * image_px * (size_t) n;
  const int64_t px0 = (int64_t) run * kWinnerRun, px1 = min(px0 + kWinnerRun, (int64_t) image_px);
  uint2 rec = make_uint2(0u, 0u);  // lane j keeps the record of the run's pixel j: the run is stored once
  for (int64_t px = px0; px < px1; ++px) {
    const int x     = (int) (px % cols);
    const int i_end = min(n, x - d0 + 1);  // admissible disparity indices of the left pixel: i < i_end
    uint32_t v[K];
    uint32_t best = kStereoNoBest;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * PRS_WAVE + lane;
      v[k]        = i < n ? (uint32_t) vol[(size_t) px * (size_t) n + (size_t) i] : kStereoNoCost;
      if (i < i_end) {
        best = min(best, (v[k] << 16) | (uint32_t) i);
      }
    }
    best = wave_min_u32(best);
    const int istar = (int) (best & 0xffffu);
    uint32_t a2 = kStereoNoCost;  // the least cost two or more disparities away from the winner
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * PRS_WAVE + lane;
      if (i < i_end && abs(i - istar) >= 2) {
        a2 = min(a2, v[k]);
      }
    }
    a2 = wave_min_u32(a2);
    int Am = 0, Ap = 0;  // the winner's neighbours, from the lanes that hold them (read only where both exist)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int tm = __shfl((int) v[k], (istar - 1) & (PRS_WAVE - 1), PRS_WAVE), tp = __shfl((int) v[k], (istar + 1) & (PRS_WAVE - 1), PRS_WAVE);
      Am = ((istar - 1) >> 6) == k ? tm : Am;
      Ap = ((istar + 1) >> 6) == k ? tp : Ap;
    }
    const uint2 r = stereo_winner_record(best, a2, Am, Ap, i_end, d0, q);  // every operand is the same in every lane
    if (lane == (int) (px - px0)) {
      rec = r;
    }
  }
  if (lane < (int) (px1 - px0)) {
    a.rec_l[(size_t) image * image_px + (size_t) px0 + (size_t) lane] = rec;
  }
}

// ---- right winner: blockIdx.x = (slot * rows + y) * rtiles + tile, a tile kRightTile right pixels of a row --------------------------
// S_R(y, x, i) = S(y, x + d_i, i), admissible iff x + d_i <= cols - 1: a diagonal of the row's slice of the volume.  Read from global
// memory every lane of a wave touched a cache line of its own (a wave a pixel, built first: 18 ms of a 65 ms call for 64 KITTI
// pairs).  So the slice is staged in LDS 64 disparities at a time, with coalesced loads: for the disparities c0 .. c0 + 63 the
// pixels x0 + d0 + c0 .. + kRightTile + 62 are all the tile's right pixels reach.  A staged pixel takes 33 words, so the threads of
// neighbouring right pixels, which read the same disparity of neighbouring staged pixels, hit different banks.  Two threads share a
// right pixel, 32 disparities of the 64 each; each keeps min((S << 16) | i), so the lowest disparity wins a tie, and LDS joins them.
// V = 1, 2 or 4 disparities a lane and load of the staging, the largest that divides n_disparities (their 2 V bytes are aligned then):
// 64 / V lanes a pixel, V pixels a wave instruction.
template <int V>
__global__ __launch_bounds__(kThreads) void sgm_right_kernel(const SgmArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_cost[kRightRows * kRightPitch];
  __shared__ uint32_t s_best[kThreads];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), w = tid >> 6;
  uint32_t id    = blockIdx.x;
  const int tile = (int) (id % (uint32_t) a.rtiles);
  id /= (uint32_t) a.rtiles;
  const int y = (int) (id % (uint32_t) a.rows), slot = (int) (id / (uint32_t) a.rows);
  const uint32_t image = (uint32_t) (a.image0 + slot);
  if (slot >= a.n_chunk || !served(a, image)) {  // the same for every thread of the workgroup
    return;
  }
  const int cols = a.cols, n = a.p.n_disparities, d0 = a.p.min_disparity;
  const size_t image_px = (size_t) a.rows * (size_t) cols;
  const uint16_t* row   = a.vol + ((size_t) slot * image_px + (size_t) y * (size_t) cols) * (size_t) n;  // S(y, ., .)
  const int x0 = tile * kRightTile, r = tid & (kRightTile - 1), half = tid / kRightTile;
  const int64_t x = (int64_t) x0 + r;  // the thread's right pixel
  uint32_t best = kStereoNoBest;
  for (int c0 = 0; c0 < n; c0 += PRS_WAVE) {
    const int64_t p0 = (int64_t) x0 + d0 + c0;  // the first staged pixel
    __syncthreads();  // the readers of the last 64 disparities are through
    const int il0 = (lane % (PRS_WAVE / V)) * V;  // the lane's first disparity of the 64
    for (int j = w * V + lane / (PRS_WAVE / V); j < kRightRows; j += kWaves * V) {
      const int64_t p = p0 + j;
      if (p < cols && c0 + il0 < n) {  // V divides n and c0: all V are there
        const uint16_t* from = row + (size_t) p * (size_t) n + (size_t) (c0 + il0);
        uint16_t* to         = s_cost + j * kRightPitch + il0;  // 4-byte aligned when V is 2 or 4: the pitch and il0 are even
        if constexpr (V == 1) {
          to[0] = from[0];
        } else if constexpr (V == 2) {
          *reinterpret_cast<uint32_t*>(to) = *reinterpret_cast<const uint32_t*>(from);
        } else {
          const uint2 v = *reinterpret_cast<const uint2*>(from);
          reinterpret_cast<uint32_t*>(to)[0] = v.x, reinterpret_cast<uint32_t*>(to)[1] = v.y;
        }
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int il = half * (PRS_WAVE / 2); il < (half + 1) * (PRS_WAVE / 2); ++il) {
      const int i = c0 + il;
      if (i < n && x + d0 + i <= cols - 1) {  // staged: pixel x + d0 + i is row r + il of the stage
        best = min(best, ((uint32_t) s_cost[(r + il) * kRightPitch + il] << 16) | (uint32_t) i);
      }
    }
  }
  s_best[tid] = best;
  __syncthreads();
  if (tid < kRightTile && x < cols) {
    best = min(s_best[tid], s_best[tid + kRightTile]);
    a.win_r[(size_t) image * image_px + (size_t) y * (size_t) cols + (size_t) x] = best != kStereoNoBest ? (int16_t) (best & 0xffffu) : (int16_t) -1;
  }
}

using PathKernel   = void (*)(SgmArgs, int, int, int);
using WinnerKernel = void (*)(SgmArgs);

// the parts of the workspace, in bytes: dense stereo's and behind them the volume; pixels 0 when a size is not one the launcher takes
struct Layout {
  DenseLayout dense;
  uint64_t in_flight, volume, total;
};

Layout layout_of(const int64_t batch, const int64_t frames, const int64_t rows, const int64_t cols, const int64_t n_disparities, const bool lr,
                 const int64_t images_in_flight) {
  Layout l = {};
  if (images_in_flight < 1) {
    return l;
  }
  l.dense = dense_layout_of(batch, frames, rows, cols, n_disparities, lr);
  if (l.dense.pixels < 1) {
    return l;
  }
  l.in_flight = (uint64_t) (images_in_flight < batch * frames ? images_in_flight : batch * frames);
  l.volume    = up16(2 * l.in_flight * (uint64_t) (rows * cols) * (uint64_t) n_disparities);  // below 2^31 * 2^8 * 2
  l.total     = l.dense.total + l.volume;
  return l;
}

}  // namespace

int sgm_stereo_launch(prs_context* ctx, const prs_sgm_stereo_params* params, const prs_sgm_stereo_batch* batch) {
  const std::string who = "prs_sgm_stereo_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_sgm_stereo_params& p = *params;
  const prs_sgm_stereo_batch& o  = *batch;
  // the stages this one shares its checks and its census and finish kernels with read these two
  prs_dense_stereo_params dp = {};
  dp.n_disparities = p.n_disparities, dp.min_disparity = p.min_disparity, dp.uniqueness_percent = p.uniqueness_percent;
  dp.lr_max_diff = p.lr_max_diff, dp.bf = p.bf;
  prs_dense_stereo_batch db = {};
  db.batch = o.batch, db.frames = o.frames, db.rows = o.rows, db.cols = o.cols;
  db.left_pitch = o.left_pitch, db.right_pitch = o.right_pitch, db.out_pitch = o.out_pitch;
  db.left = o.left, db.right = o.right, db.n_images = o.n_images, db.disparity = o.disparity, db.depth = o.depth;
  db.n_valid = o.n_valid, db.status = o.status, db.workspace = o.workspace;
  PRS_TRY(stereo_call_check(ctx, who, dp, db, (p.n_paths == 4 || p.n_paths == 8) && p.p1 >= 0 && p.p2 >= p.p1 && p.p2 <= 4095,
                            "n_paths not 4 or 8, p1 below 0, p2 below p1 or above 4095", o.images_in_flight, " or images_in_flight"));
  const bool lr  = p.lr_max_diff >= 0;
  const Layout l = layout_of(o.batch, o.frames, o.rows, o.cols, p.n_disparities, lr, o.images_in_flight);

  SgmArgs a = {};
  a.p = p;
  a.frames = o.frames, a.rows = o.rows, a.cols = o.cols;
  a.n_images = o.n_images;
  const int64_t image_px = (int64_t) o.rows * o.cols, images = (int64_t) o.batch * o.frames, in_flight = (int64_t) l.in_flight;
  a.runs   = (int32_t) ((image_px + kWinnerRun - 1) / kWinnerRun);
  a.rtiles = (int32_t) (((int64_t) o.cols + kRightTile - 1) / kRightTile);
  uint8_t* ws = static_cast<uint8_t*>(o.workspace);
  a.census_l  = reinterpret_cast<uint64_t*>(ws);
  a.census_r  = reinterpret_cast<uint64_t*>(ws + l.dense.census);
  a.rec_l     = reinterpret_cast<uint2*>(ws + 2 * l.dense.census);
  a.win_r     = lr ? reinterpret_cast<int16_t*>(ws + 2 * l.dense.census + l.dense.rec) : nullptr;
  a.vol       = reinterpret_cast<uint16_t*>(ws + l.dense.total);
  // the grids of the call, before anything is launched (each factor is below 2^31): census and finish over every image, the rest
  // over the images in flight -- every group of them but the last is full
  static_assert(kThreads == kDenseThreads, "the shared launches' workgroup");
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid census = on.grid(dense_census_blocks(db), kThreads), finish = on.grid(dense_finish_blocks(db), kThreads);
  struct GroupGrids {
    Grid path_along_rows, path_along_cols, winner, right;  // a wave per image row or column (path), per run of pixels (winner)
  };
  const auto group_grids = [&](const int64_t n_chunk) {
    GroupGrids g;
    g.path_along_rows = on.grid((n_chunk * o.rows + kWaves - 1) / kWaves, kThreads);
    g.path_along_cols = on.grid((n_chunk * o.cols + kWaves - 1) / kWaves, kThreads);
    g.winner          = on.grid((n_chunk * a.runs + kWaves - 1) / kWaves, kThreads);
    g.right           = lr ? on.grid(n_chunk * o.rows * a.rtiles, kThreads) : Grid();
    return g;
  };
  const GroupGrids full = group_grids(in_flight), last = images % in_flight ? group_grids(images % in_flight) : full;
  PRS_TRY(on.check());
  const int n = p.n_disparities;
  const PathKernel path = n <= 64    ? sgm_path_kernel<1, true>
                          : n <= 128 ? (n % 2 == 0 ? sgm_path_kernel<2, true> : sgm_path_kernel<2, false>)
                                     : (n % 4 == 0 ? sgm_path_kernel<4, true> : sgm_path_kernel<4, false>);
  const WinnerKernel winner = n <= 64 ? sgm_winner_kernel<1> : n <= 128 ? sgm_winner_kernel<2> : sgm_winner_kernel<4>;
  const WinnerKernel right = n % 4 == 0 ? sgm_right_kernel<4> : n % 2 == 0 ? sgm_right_kernel<2> : sgm_right_kernel<1>;
  static const int kDirections[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};  // (dy, dx)

  dense_census_enqueue(on, census, db, const_cast<uint64_t*>(a.census_l), const_cast<uint64_t*>(a.census_r));
  for (int64_t image0 = 0; image0 < images; image0 += in_flight) {
    const GroupGrids& g = images - image0 < in_flight ? last : full;
    a.image0  = (int32_t) image0;
    a.n_chunk = (int32_t) (images - image0 < in_flight ? images - image0 : in_flight);
    for (int r = 0; r < p.n_paths; ++r) {
      const int dy = kDirections[r][0], dx = kDirections[r][1];
      on.launch(path, dy == 0 ? g.path_along_rows : g.path_along_cols, 0, a, dy, dx, r == 0 ? 1 : 0);
    }
    on.launch(winner, g.winner, 0, a);
    if (lr) {
      on.launch(right, g.right, 0, a);
    }
  }
  dense_finish_enqueue(on, finish, dp, db, a.rec_l, a.win_r);
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_sgm_stereo_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_sgm_stereo_params);
  sizes2[1] = sizeof(prs_sgm_stereo_batch);
}

uint64_t prs_sgm_stereo_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols, int32_t n_disparities, int32_t lr_check,
                                        int32_t images_in_flight) {
  return layout_of(batch, frames, rows, cols, n_disparities, lr_check != 0, images_in_flight).total;
}

int prs_sgm_stereo_batch_run(prs_context* ctx, const prs_sgm_stereo_params* params, const prs_sgm_stereo_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return sgm_stereo_launch(ctx, params, batch);
}

}  // extern "C"
