// dense_stereo.hip -- dense stereo on the device: a rectified pair to a disparity and a depth image (prs_dense_stereo_batch_run; the
// rule is stated in include/proslam_hip.h, BUILD-DEFINED, and restated in tests/dense_stereo_ref.py).  Every decision is integer
// arithmetic; the only rounded operations are one float32 division and one addition (sub-pixel) and one division (depth) a pixel.
//   census   one workgroup per 64 x 16 tile of one image (left or right): the tile with its 4 / 3 pixel halo, at clamped
//            coordinates, in LDS once; a lane four pixels, 62 byte compares each; the words go to the workspace
//   match    instantiated for the left and the right reference.  A workgroup of four waves owns 64 - 2r output columns of a band of
//            32 rows of one image and walks down the band.  Lane x of every wave stands for the extended column t0 - r + x
//            (clamped), so the 2r halo columns of the box sum are lanes of the same wave; wave w takes the disparity pairs w, w + 4,
//            ..  Two disparities share a 32-bit word as 16-bit halves (no sum passes 62 * 15 * 15 = 13950, so a plain 32-bit add or
//            subtract is the packed one).  Per row: the entering and the leaving census row of the other image, the
//            64 + n_disparities columns the tile can reach, are staged in LDS; V[pair][x], the vertical running sums, get the
//            entering row's costs added and the leaving row's subtracted, both recomputed by 64-bit popcounts; the box sum of a
//            pair is 2r + 1 LDS reads of V; each lane keeps min((cost << 16) | i) over its wave's admissible disparities, so the
//            lowest disparity wins a tie, and LDS joins the four waves.  The left pass keeps the aggregated row A[pair][x] in LDS
//            for a second walk (the runner-up two or more away) and for the winner's neighbours, applies the uniqueness test and
//            the sub-pixel rule, and writes (s or 0, i*) per pixel; the right pass writes i* alone.  The cost volume never leaves
//            the chip.  The first row of a band costs 2r + 1 row additions.  r is a template parameter (the reads of a box sum are
//            issued together; a loop over a run-time radius waited for each) and a wave takes four pairs between two wave syncs
//   finish   a workgroup 8 rows of an image, a lane a pixel at a time: the left-right check against the right pass's winners,
//            disparity, depth = bf / s, and n_valid by wave ballots and one integer atomic add a workgroup (an integer sum does not
//            depend on the order; one add a wave, built first, made this launch wait on 7000 adds to one address an image)
// Plain launches: no persistent workgroup, no spinning, nothing handed from workgroup to workgroup but through the launch order.
#include <math.h>
#include <stddef.h>

#include <string>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"

namespace prs {

namespace {

constexpr int kThreads    = 256;
constexpr int kWaves      = kThreads / PRS_WAVE;
constexpr int kBandRows   = 32;  // rows a match workgroup walks
constexpr int kGroup      = 4;   // disparity pairs a wave takes between two wave syncs
constexpr int kFinishRows = 8;   // rows of a finish workgroup
constexpr int kCensusRows = 16;  // the census tile is PRS_WAVE x kCensusRows
constexpr int kHaloX = 4, kHaloY = 3;

struct DenseStereoArgs {
  prs_dense_stereo_params p;
  prs_dense_stereo_batch o;
  int32_t npairs;       // ceil(n_disparities / 2)
  int32_t tile;         // PRS_WAVE - 2 r: the output columns of a match workgroup
  int32_t tiles;        // ceil(cols / tile)
  int32_t bands;        // ceil(rows / kBandRows)
  int32_t ctiles_x, ctiles_y;  // the census tiles of an image
  int32_t fblocks;             // ceil(rows / kFinishRows): the finish workgroups of an image
  uint64_t* census_l;   // [images][rows][cols]
  uint64_t* census_r;
  uint2* rec_l;         // [images][rows][cols] (the bits of s, or of 0.0f when the uniqueness test drops the pixel; i* or -1)
  int16_t* win_r;       // [images][rows][cols] i* of the right pixel or -1 (lr_max_diff >= 0 only)
};

// ---- census: blockIdx.x = ((image * 2 + side) * ctiles_y + ty) * ctiles_x + tx ----------------------------------------------------
__global__ __launch_bounds__(kThreads) void dense_census_kernel(const DenseStereoArgs a) {
  constexpr int W = PRS_WAVE + 2 * kHaloX, H = kCensusRows + 2 * kHaloY;
  __shared__ uint8_t s_px[H][W];
  const int tid = threadIdx.x;
  uint32_t id   = blockIdx.x;
  const int tx  = (int) (id % (uint32_t) a.ctiles_x);
  id /= (uint32_t) a.ctiles_x;
  const int ty = (int) (id % (uint32_t) a.ctiles_y);
  id /= (uint32_t) a.ctiles_y;
  const int side       = (int) (id & 1u);
  const uint32_t image = id >> 1;
  const int f = frame_of(image, a.o.frames), b = sequence_of(image, a.o.frames);
  const int n_img  = images_of(a.o, b);
  const bool first = side == 0 && tx == 0 && ty == 0 && tid == 0;
  if (first && f == 0) {
    a.o.status[b] = n_img < 0 ? PRS_ERR_RANGE : PRS_OK;
  }
  if (f >= n_img) {
    return;
  }
  if (first && a.o.n_valid) {
    a.o.n_valid[image] = 0;  // the finish launch adds to it
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const size_t pitch = (size_t) (side ? a.o.right_pitch : a.o.left_pitch);
  const uint8_t* img = (side ? a.o.right : a.o.left) + (size_t) image * (size_t) rows * pitch;
  const int x0 = tx * PRS_WAVE, y0 = ty * kCensusRows;
  for (int i = tid; i < H * W; i += kThreads) {
    const int yy = i / W, xx = i - yy * W;
    s_px[yy][xx] = img[(size_t) clampi(y0 - kHaloY + yy, 0, rows - 1) * pitch + clampi(x0 - kHaloX + xx, 0, cols - 1)];
  }
  __syncthreads();
  uint64_t* out = (side ? a.census_r : a.census_l) + (size_t) image * (size_t) rows * (size_t) cols;
  const int lx = tid & (PRS_WAVE - 1), x = x0 + lx;
  for (int ly = tid >> 6; ly < kCensusRows; ly += kWaves) {
    const int y = y0 + ly;
    if (x < cols && y < rows) {
      const uint8_t c = s_px[ly + kHaloY][lx + kHaloX];
      uint32_t lo = 0, hi = 0;  // bits 0 .. 30 and 31 .. 61, in the window's raster order
      int bit = 0;
#pragma unroll
      for (int dy = -kHaloY; dy <= kHaloY; ++dy) {
#pragma unroll
        for (int dx = -kHaloX; dx <= kHaloX; ++dx) {
          if (dy != 0 || dx != 0) {
            const uint32_t less = s_px[ly + kHaloY + dy][lx + kHaloX + dx] < c ? 1u : 0u;
            if (bit < 31) {
              lo |= less << bit;
            } else {
              hi |= less << (bit - 31);
            }
            ++bit;
          }
        }
      }
      out[(size_t) y * (size_t) cols + x] = ((uint64_t) hi << 31) | lo;
    }
  }
}

// the dynamic LDS of a match workgroup: the two staged census rows, V, A (left pass), and the four waves' minima twice
__host__ __device__ inline int seg_words(const int npairs) {
  return PRS_WAVE + 2 * npairs;  // the columns a tile's extended lanes reach over the padded disparity range, rounded up
}
inline size_t match_lds(const int npairs, const bool right) {
  return (size_t) 2 * seg_words(npairs) * 8 + (size_t) (right ? 1 : 2) * npairs * PRS_WAVE * 4 + (size_t) 2 * kThreads * 4;
}

// ---- match: blockIdx.x = (image * bands + band) * tiles + tile --------------------------------------------------------------------
// R = aggregation_radius is a template parameter so that the 2 R + 1 LDS reads of a box sum are issued together (with a loop over a
// run-time radius every read was waited for before the next was issued)
template <bool RIGHT, int R>
__global__ __launch_bounds__(kThreads) void dense_match_kernel(const DenseStereoArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int r = R, tile_w = PRS_WAVE - 2 * R;
  const int npairs = a.npairs, n = a.p.n_disparities, n2 = 2 * npairs, d0 = a.p.min_disparity;
  const int L      = seg_words(npairs);
  uint64_t* s_seg  = reinterpret_cast<uint64_t*>(smem);                 // [2][L] the entering and the leaving row of the other image
  uint32_t* s_best = reinterpret_cast<uint32_t*>(s_seg + 2 * L);        // [kWaves][64]
  uint32_t* s_a2   = s_best + kThreads;                                 // [kWaves][64]
  uint32_t* s_V    = s_a2 + kThreads;                                   // [npairs][64] vertical sums of disparities 2 p | 2 p + 1
  uint32_t* s_A    = s_V + (size_t) npairs * PRS_WAVE;                  // [npairs][64] their box sums (left pass)
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), w = tid >> 6;
  uint32_t id    = blockIdx.x;
  const int tile = (int) (id % (uint32_t) a.tiles);
  id /= (uint32_t) a.tiles;
  const int band       = (int) (id % (uint32_t) a.bands);
  const uint32_t image = id / (uint32_t) a.bands;
  if (!image_served(a.o, image)) {
    return;
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const int t0 = tile * tile_w, v0 = band * kBandRows, v1 = min(v0 + kBandRows, rows);
  const size_t at_image = (size_t) image * (size_t) rows * (size_t) cols;
  const uint64_t* ref   = (RIGHT ? a.census_r : a.census_l) + at_image;
  const uint64_t* other = (RIGHT ? a.census_l : a.census_r) + at_image;
  // the lane's extended column, and where it sits in the staged segment: disparity index i of it is word xo + i (right
  // reference: column + d) or xo + n2 - 1 - i (left reference: column - d) of a segment that starts at column seg0
  const int xc   = clampi(t0 - r + lane, 0, cols - 1);
  const int xo   = xc - (t0 - r);  // 0 .. 63
  const int seg0 = RIGHT ? t0 - r + d0 : t0 - r - (d0 + n2 - 1);
  const int u    = t0 + lane;      // the lane's output column
  const bool out = lane < tile_w && u < cols;
  // admissible disparity indices of the output column: i < i_end
  const int i_end = out ? min(n, RIGHT ? cols - u - d0 : u - d0 + 1) : 0;

  for (int i = tid; i < npairs * PRS_WAVE; i += kThreads) {
    s_V[i] = 0;
  }
  for (int t = -2 * r; t < v1 - v0; ++t) {
    const int enter  = clampi(v0 + t + r, 0, rows - 1);
    const bool leave = t > 0, emit = t >= 0;
    const int leaving = clampi(v0 + t - r - 1, 0, rows - 1);
    __syncthreads();  // the last row's readers of the segments and of the waves' minima are through; V is zeroed
    for (int k = tid; k < L; k += kThreads) {
      const int c = clampi(seg0 + k, 0, cols - 1);
      s_seg[k]    = other[(size_t) enter * (size_t) cols + c];
      if (leave) {
        s_seg[L + k] = other[(size_t) leaving * (size_t) cols + c];
      }
    }
    const uint64_t ref_e = ref[(size_t) enter * (size_t) cols + xc];
    const uint64_t ref_l = leave ? ref[(size_t) leaving * (size_t) cols + xc] : 0;
    __syncthreads();
    uint32_t best = kStereoNoBest;
    // kGroup pairs between two wave syncs: their LDS round trips overlap
    for (int dp0 = w; dp0 < npairs; dp0 += kWaves * kGroup) {
#pragma unroll
      for (int g = 0; g < kGroup; ++g) {
        const int dp = dp0 + g * kWaves;
        if (dp < npairs) {
          const int i  = 2 * dp;
          const int k  = RIGHT ? xo + i : xo + (n2 - 1 - i);
          const int k1 = RIGHT ? k + 1 : k - 1;
          uint32_t V   = s_V[dp * PRS_WAVE + lane];
          V += (uint32_t) __popcll(ref_e ^ s_seg[k]) | ((uint32_t) __popcll(ref_e ^ s_seg[k1]) << 16);
          if (leave) {
            V -= (uint32_t) __popcll(ref_l ^ s_seg[L + k]) | ((uint32_t) __popcll(ref_l ^ s_seg[L + k1]) << 16);
          }
          s_V[dp * PRS_WAVE + lane] = V;
        }
      }
      if (emit) {
        wave_sync();
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
          const int dp = dp0 + g * kWaves;
          if (dp < npairs) {
            const int i = 2 * dp;
            uint32_t A  = 0;
            if (lane < tile_w) {
#pragma unroll
              for (int j = 0; j <= 2 * r; ++j) {
                A += s_V[dp * PRS_WAVE + lane + j];
              }
            }
            if (!RIGHT) {
              s_A[dp * PRS_WAVE + lane] = A;
            }
            if (i < i_end) {
              best = min(best, ((A & 0xffffu) << 16) | (uint32_t) i);
            }
            if (i + 1 < i_end) {
              best = min(best, (A & 0xffff0000u) | (uint32_t) (i + 1));
            }
          }
        }
      }
    }
    if (!emit) {
      continue;
    }
    s_best[tid] = best;
    __syncthreads();
    best = min(min(s_best[lane], s_best[PRS_WAVE + lane]), min(s_best[2 * PRS_WAVE + lane], s_best[3 * PRS_WAVE + lane]));
    const int istar = (int) (best & 0xffffu);
    const size_t px = at_image + (size_t) (v0 + t) * (size_t) cols + (size_t) u;
    if (RIGHT) {
      if (w == 0 && out) {
        a.win_r[px] = best != kStereoNoBest ? (int16_t) istar : (int16_t) -1;
      }
      continue;
    }
    // the least cost two or more disparities away from the winner
    uint32_t a2 = kStereoNoCost;
    for (int dp = w; dp < npairs; dp += kWaves) {
      const uint32_t A = s_A[dp * PRS_WAVE + lane];
      const int i      = 2 * dp;
      if (i < i_end && abs(i - istar) >= 2) {
        a2 = min(a2, A & 0xffffu);
      }
      if (i + 1 < i_end && abs(i + 1 - istar) >= 2) {
        a2 = min(a2, A >> 16);
      }
    }
    s_a2[tid] = a2;
    __syncthreads();
    if (w == 0 && out) {
      a2 = min(min(s_a2[lane], s_a2[PRS_WAVE + lane]), min(s_a2[2 * PRS_WAVE + lane], s_a2[3 * PRS_WAVE + lane]));
      int Am = 0, Ap = 0;  // the winner's neighbours, read where both are in the range and admissible
      if (istar >= 1 && istar + 1 < i_end) {
        const uint32_t wm = s_A[((istar - 1) >> 1) * PRS_WAVE + lane], wp = s_A[((istar + 1) >> 1) * PRS_WAVE + lane];
        Am = (int) (((istar - 1) & 1) ? wm >> 16 : wm & 0xffffu);
        Ap = (int) (((istar + 1) & 1) ? wp >> 16 : wp & 0xffffu);
      }
      a.rec_l[px] = stereo_winner_record(best, a2, Am, Ap, i_end, d0, a.p.uniqueness_percent);
    }
  }
}

using MatchKernel = void (*)(DenseStereoArgs);
#define PRS_MATCH_ROW(right) \
  {dense_match_kernel<right, 0>, dense_match_kernel<right, 1>, dense_match_kernel<right, 2>, dense_match_kernel<right, 3>, \
   dense_match_kernel<right, 4>, dense_match_kernel<right, 5>, dense_match_kernel<right, 6>, dense_match_kernel<right, 7>}
const MatchKernel kMatchKernels[2][8] = {PRS_MATCH_ROW(false), PRS_MATCH_ROW(true)};  // [right reference][aggregation_radius]
#undef PRS_MATCH_ROW

// ---- finish: blockIdx.x = image * fblocks + block, a block kFinishRows rows --------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dense_finish_kernel(const DenseStereoArgs a) {
  __shared__ int s_count[kWaves];
  const int tid        = threadIdx.x;
  const int block      = (int) (blockIdx.x % (uint32_t) a.fblocks);
  const uint32_t image = blockIdx.x / (uint32_t) a.fblocks;
  if (!image_served(a.o, image)) {
    return;
  }
  const int cols = a.o.cols, v0 = block * kFinishRows;
  const int total     = (min(v0 + kFinishRows, a.o.rows) - v0) * cols;  // the block's pixels, row after row
  const size_t first  = ((size_t) image * (size_t) a.o.rows + (size_t) v0) * (size_t) cols;
  const size_t out0   = ((size_t) image * (size_t) a.o.rows + (size_t) v0) * (size_t) (a.o.out_pitch >> 2);
  int count = 0;  // the wave's valid pixels
  for (int base = 0; base < total; base += kThreads) {
    const int at = base + tid;
    bool valid   = false;
    if (at < total) {
      const int dv = at / cols, u = at - dv * cols;
      const uint2 rec = a.rec_l[first + at];
      const float s   = __uint_as_float(rec.x);
      const int istar = (int) rec.y;
      valid = istar >= 0 && s > 0.0f;
      if (valid && a.p.lr_max_diff >= 0) {
        const int ir = a.win_r[first + at - (a.p.min_disparity + istar)];  // the winner is admissible: the column is inside the row
        valid = ir >= 0 && abs(ir - istar) <= a.p.lr_max_diff;
      }
      const size_t to = out0 + (size_t) dv * (size_t) (a.o.out_pitch >> 2) + (size_t) u;
      if (a.o.disparity) {
        a.o.disparity[to] = valid ? s : 0.0f;
      }
      if (a.o.depth) {
        a.o.depth[to] = valid ? a.p.bf / s : 0.0f;
      }
    }
    count += (int) __popcll(__ballot(valid));
  }
  if (a.o.n_valid) {  // one integer atomic add a workgroup: the sum does not depend on the order
    if ((tid & (PRS_WAVE - 1)) == 0) {
      s_count[tid >> 6] = count;
    }
    __syncthreads();
    if (tid == 0) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        sum += s_count[w];
      }
      if (sum != 0) {
        atomicAdd(a.o.n_valid + image, sum);
      }
    }
  }
}

}  // namespace

DenseLayout dense_layout_of(const int64_t batch, const int64_t frames, const int64_t rows, const int64_t cols, const int64_t n_disparities, const bool lr) {
  DenseLayout l = {};
  if (n_disparities < 1 || n_disparities > 256) {
    return l;
  }
  l.pixels = image_pixels(batch, frames, rows, cols);
  l.census = up16(8 * l.pixels);
  l.rec    = up16(8 * l.pixels);
  l.right  = lr ? up16(2 * l.pixels) : 0;
  l.total  = 2 * l.census + l.rec + l.right;
  return l;
}

int stereo_call_check(prs_context* ctx, const std::string& who, const prs_dense_stereo_params& p, const prs_dense_stereo_batch& o,
                      const bool stage_ok, const char* stage_rule, const int64_t stage_size, const char* stage_size_name) {
  if (!o.left || !o.right || !o.status || !o.workspace || (!o.disparity && !o.depth)) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": left, right, status or the workspace not set, or neither disparity nor depth").c_str());
  }
  if (p.n_disparities < 1 || p.n_disparities > 256 || p.min_disparity < 0 || p.min_disparity + p.n_disparities > 4096 || !stage_ok ||
      p.uniqueness_percent < 0 || p.uniqueness_percent > 99 || p.lr_max_diff < -1 || p.lr_max_diff > 255 || !std::isfinite(p.bf) || !(p.bf > 0.0f)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": n_disparities outside 1..256, min_disparity below 0 or min_disparity + n_disparities above 4096, " + stage_rule + ", uniqueness_percent outside 0..99, lr_max_diff outside -1..255, or bf not finite and positive").c_str());
  }
  if (o.batch < 1 || o.frames < 1 || o.rows < 1 || o.cols < 1 || stage_size < 1 || o.left_pitch < o.cols || o.right_pitch < o.cols ||
      !pitch_ok(o.out_pitch, o.cols, 4)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size" + stage_size_name + " below 1, an image pitch below cols, or out_pitch below cols floats or not a multiple of 4").c_str());
  }
  if (!aligned_to(o.disparity, 4) || !aligned_to(o.depth, 4) || !aligned_to(o.workspace, 16) || !aligned_to(o.n_images, 4) ||
      !aligned_to(o.n_valid, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": the workspace must be 16-byte aligned, the other arrays but the images 4-byte").c_str());
  }
  if (image_pixels(o.batch, o.frames, o.rows, o.cols) < 1) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": batch * frames * rows * cols beyond 2^31 - 1").c_str());
  }
  return PRS_OK;
}

// the census and the finish launch for the stages that share them (sgm_stereo.hip): the caller has checked the batch, declared
// *_blocks workgroups of kDenseThreads among its launches and checked those
static_assert(kThreads == kDenseThreads, "the shared launches' workgroup");
static int census_tiles_x(const prs_dense_stereo_batch& o) {
  return (o.cols + PRS_WAVE - 1) / PRS_WAVE;
}
static int census_tiles_y(const prs_dense_stereo_batch& o) {
  return (o.rows + kCensusRows - 1) / kCensusRows;
}
static int finish_blocks_per_image(const prs_dense_stereo_batch& o) {
  return (o.rows + kFinishRows - 1) / kFinishRows;
}
int64_t dense_census_blocks(const prs_dense_stereo_batch& o) {  // (each factor is below 2^31 and batch * frames * rows * cols is)
  return (int64_t) o.batch * o.frames * 2 * census_tiles_x(o) * census_tiles_y(o);
}
int64_t dense_finish_blocks(const prs_dense_stereo_batch& o) {
  return (int64_t) o.batch * o.frames * finish_blocks_per_image(o);
}

void dense_census_enqueue(const Launches& on, const Grid& grid, const prs_dense_stereo_batch& o, uint64_t* census_l, uint64_t* census_r) {
  DenseStereoArgs a = {};
  a.o        = o;
  a.ctiles_x = census_tiles_x(o);
  a.ctiles_y = census_tiles_y(o);
  a.census_l = census_l;
  a.census_r = census_r;
  on.launch(dense_census_kernel, grid, 0, a);
}

void dense_finish_enqueue(const Launches& on, const Grid& grid, const prs_dense_stereo_params& p, const prs_dense_stereo_batch& o, uint2* rec_l,
                          int16_t* win_r) {
  DenseStereoArgs a = {};
  a.p       = p;
  a.o       = o;
  a.fblocks = finish_blocks_per_image(o);
  a.rec_l   = rec_l;
  a.win_r   = win_r;
  on.launch(dense_finish_kernel, grid, 0, a);
}

int dense_stereo_launch(prs_context* ctx, const prs_dense_stereo_params* params, const prs_dense_stereo_batch* batch) {
  const std::string who = "prs_dense_stereo_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_dense_stereo_params& p = *params;
  const prs_dense_stereo_batch& o  = *batch;
  PRS_TRY(stereo_call_check(ctx, who, p, o, p.aggregation_radius >= 0 && p.aggregation_radius <= 7, "aggregation_radius outside 0..7"));
  const bool lr       = p.lr_max_diff >= 0;
  const DenseLayout l = dense_layout_of(o.batch, o.frames, o.rows, o.cols, p.n_disparities, lr);
  DenseStereoArgs a = {};
  a.p = p;
  a.o = o;
  a.npairs   = (p.n_disparities + 1) / 2;
  a.tile     = PRS_WAVE - 2 * p.aggregation_radius;
  a.tiles    = (o.cols + a.tile - 1) / a.tile;
  a.bands    = (o.rows + kBandRows - 1) / kBandRows;
  a.ctiles_x = census_tiles_x(o);
  a.ctiles_y = census_tiles_y(o);
  a.fblocks  = finish_blocks_per_image(o);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid census = on.grid(dense_census_blocks(o), kThreads), match = on.grid((int64_t) o.batch * o.frames * a.bands * a.tiles, kThreads),
             finish = on.grid(dense_finish_blocks(o), kThreads);
  PRS_TRY(on.check());
  uint8_t* ws = static_cast<uint8_t*>(o.workspace);
  a.census_l  = reinterpret_cast<uint64_t*>(ws);
  a.census_r  = reinterpret_cast<uint64_t*>(ws + l.census);
  a.rec_l     = reinterpret_cast<uint2*>(ws + 2 * l.census);
  a.win_r     = lr ? reinterpret_cast<int16_t*>(ws + 2 * l.census + l.rec) : nullptr;
  const size_t lds_l = match_lds(a.npairs, false), lds_r = match_lds(a.npairs, true);
  const MatchKernel match_l = kMatchKernels[0][p.aggregation_radius], match_r = kMatchKernels[1][p.aggregation_radius];
  hipError_t e = allow_lds(match_l, lds_l);
  if (e == hipSuccess) {
    e = allow_lds(match_r, lds_r);
  }
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_dense_stereo_batch_run LDS request");
  }
  on.launch(dense_census_kernel, census, 0, a);
  on.launch(match_l, match, lds_l, a);
  if (lr) {
    on.launch(match_r, match, lds_r, a);
  }
  on.launch(dense_finish_kernel, finish, 0, a);
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_dense_stereo_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_dense_stereo_params);
  sizes2[1] = sizeof(prs_dense_stereo_batch);
}

uint64_t prs_dense_stereo_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols, int32_t n_disparities, int32_t lr_check) {
  return dense_layout_of(batch, frames, rows, cols, n_disparities, lr_check != 0).total;
}

int prs_dense_stereo_batch_run(prs_context* ctx, const prs_dense_stereo_params* params, const prs_dense_stereo_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return dense_stereo_launch(ctx, params, batch);
}

}  // extern "C"
