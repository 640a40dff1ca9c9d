// selective.hip -- the selective intensity feature extractor on the device:
// IntensityFeatureExtractorSelective_::computeKeypoints + compute (sensor_processing/feature_extractors/
// intensity_feature_extractor_selective.cpp:45-203, intensity_feature_extractor_base.cpp:56-85) around cv::GFTTDetector,
// restated from OpenCV's goodFeaturesToTrack (include/proslam_hip.h).  Every image runs one or two GFTT "runs": run 0 with the
// tracking mask (projections given) or the seeding mask (external or everything), run 1 with the complement of the tracking
// mask when enable_seeding_when_tracking is set.  Both runs share the corner response; each has its own maximum, threshold,
// candidates and maxCorners budget.
//
// Six launches per batch of images:
//   mask_raster_kernel  one workgroup per 8 rows of an image: the union of the projections' rectangles as a row-wise difference
//                       array in LDS (two atomics per rectangle and row), a prefix sum per row, one bit per pixel out
//   response_kernel<0>  one 64x16 tile per workgroup: image (3-px halo) -> Sobel -> products -> 3x3 box sums -> minimum
//                       eigenvalue in LDS, all in float in the checker's operation order; the maximum of each run's mask
//                       (order-preserving uint form of the float, one atomic per workgroup and run)
//   response_kernel<1>  the same tile again (instead of a float map of every image, 1.9 MB per KITTI frame written and read back;
//                       the two were not measured against each other), threshold, 3x3 dilation, mask test; candidate keys
//                       (response << 32 | pixel) appended with one atomic per workgroup and run
//   select_kernel       one workgroup per image and run: bitonic sort of the keys in LDS (response desc, pixel desc), then one
//                       wave runs the greedy min-distance filter over chunks of 64 candidates: each lane tests its candidate
//                       against the accepted set (linked lists per grid cell in LDS), the conflicts inside the chunk are a
//                       per-lane mask of later lanes, resolved in order with scalar bit operations; at most maxCorners
//                       accepted, then the 31-px border filter (cv::ORB::compute), order kept
//   finalize_kernel     one workgroup per image: run 0's keypoints, then run 1's, status
//   blur_kernel + describe_kernel of features.hip (describe_selected_launch): the ORB descriptors
#include <string.h>

#include "prs_device.h"
#include "prs_host.h"

namespace prs {

namespace {

constexpr int kRespW = 64, kRespH = 16, kRespThreads = 256;
constexpr int kEigW = kRespW + 2, kEigH = kRespH + 2;    // eigenvalues of the tile and its 1-px ring (dilation)
constexpr int kProdW = kRespW + 4, kProdH = kRespH + 4;  // gradient products (+1 ring: box sums)
constexpr int kImgW = kRespW + 6, kImgH = kRespH + 6;    // image (+1 ring: Sobel)
constexpr int kMaskRows = 8, kMaskThreads = 256, kMaxWordsPerRow = 128;
constexpr int kSelThreads = 512;
constexpr int kBorder = 31;                       // cv::ORB edgeThreshold
constexpr int kBaseRadius = 10;                   // selective.cpp:67
constexpr int kDefaultCandidates = 8192, kMaxCandidates = 16384, kMaxCorners = 8192, kMaxSide = 4096;
constexpr size_t kMaxLds = 160 * 1024;

struct SelArgs {
  prs_selective_extractor_params p;
  prs_selective_extract_batch b;
  int wpr;                   // mask words per image row
  uint32_t* mask;            // [batch][rows][wpr]: bit set = pixel belongs to run 0's mask (run 1 uses the complement)
  uint32_t* maxima;          // [batch][2] largest response of each run's mask, order-preserving uint form (0 = empty mask)
  uint32_t* n_cand;          // [batch][2] candidates appended (may exceed cap: the run fails)
  int32_t* bad;              // [batch] set when a projection or radius is outside the supported domain
  unsigned long long* cand;  // [batch][2][cap]
  int cap, sort_n;           // candidate capacity, its power of two (LDS keys of select_kernel)
  uint32_t* sel;             // [batch][2][maxc] accepted keypoints inside the ORB border, per run
  int32_t* n_sel;            // [batch][2] (-1 = more candidates than cap)
  uint32_t* kept;            // [batch][stride] final keypoint pixel indices (describe_kernel)
  int maxc, md, cell, gw, gh;
};

__device__ __forceinline__ int reflect_clamp(int v, const int n) {  // BORDER_REFLECT_101 for the 3 px around the image
  v = v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v);
  return v < 0 ? 0 : (v >= n ? n - 1 : v);
}
__device__ __forceinline__ bool run_active(const SelArgs& a, const int img, const int run) {
  const bool tracking = a.b.projections && a.b.n_projections[img] > 0;
  return run == 0 || (tracking && a.p.enable_seeding_when_tracking);
}
__device__ __forceinline__ float run_threshold(const SelArgs& a, const int img, const int run) {
  const uint32_t m = a.maxima[2 * img + run];
  const float max_val = m ? from_ordered(m) : 0.0f;  // minMaxLoc over an empty mask: 0
  return (float) ((double) max_val * 0.01);           // cv::threshold(eig, eig, maxVal * qualityLevel, 0, THRESH_TOZERO)
}

// ---- detection masks: tracking rectangles as a row-wise difference array, or the external seeding mask ----
__global__ __launch_bounds__(kMaskThreads) void mask_raster_kernel(const SelArgs a) {
  extern __shared__ int diff[];  // [kMaskRows][cols + 1]
  __shared__ int word_base[kMaskRows][kMaxWordsPerRow];
  const int img = blockIdx.y, y0 = blockIdx.x * kMaskRows, tid = threadIdx.x;
  const int rows = a.b.rows, cols = a.b.cols, wpr = a.wpr, nr = min(kMaskRows, rows - y0);
  uint32_t* __restrict__ out = a.mask + ((size_t) img * rows + y0) * wpr;
  int n = a.b.projections ? a.b.n_projections[img] : 0;
  if (n < 0 || n > a.b.projection_stride) {
    if (tid == 0 && blockIdx.x == 0) {
      a.bad[img] = 1;
    }
    n = 0;
  }
  if (n == 0) {  // seeding mode: the external mask, or every pixel
    const uint8_t* __restrict__ m = a.b.seeding_mask ? a.b.seeding_mask + (size_t) img * rows * a.b.pitch : nullptr;
    for (int i = tid; i < nr * wpr; i += kMaskThreads) {
      const int r = i / wpr, w = i - r * wpr;
      uint32_t bits = 0;
      for (int j = 0; j < 32; ++j) {
        const int x = 32 * w + j;
        if (x < cols && (!m || m[(size_t) (y0 + r) * a.b.pitch + x] != 0)) {
          bits |= 1u << j;
        }
      }
      out[i] = bits;
    }
    return;
  }
  const int width = cols + 1;
  for (int i = tid; i < kMaskRows * width; i += kMaskThreads) {
    diff[i] = 0;
  }
  __syncthreads();
  const int radius = a.b.detection_radius ? a.b.detection_radius[img] : 0;
  const int r = radius + kBaseRadius;
  const bool left = a.p.enable_full_distance_to_left != 0, right = a.p.enable_full_distance_to_right != 0;
  const prs_kp2* __restrict__ proj = a.b.projections + (size_t) img * a.b.projection_stride;
  for (int i = tid; i < n; i += kMaskThreads) {
    const prs_kp2 uv = proj[i];
    if (!(uv.u >= 0.0f && uv.u < (float) cols && uv.v >= 0.0f && uv.v < (float) rows) || radius < 0 || radius > kMaxSide) {
      if (blockIdx.x == 0) {
        a.bad[img] = 1;  // the reference asserts (selective.cpp:84-87); the image fails with PRS_ERR_RANGE
      }
      continue;
    }
    const int col = (int) roundf(uv.u), row = (int) roundf(uv.v);  // std::round: half away from zero
    const int tl_row = max(row - r, 0);
    const int r0 = tl_row, r1 = tl_row + min(2 * r, rows - tl_row);
    int c0, c1;
    if (left && right) {
      c0 = 0, c1 = cols;
    } else if (left) {
      c0 = 0, c1 = col;
    } else if (right) {
      c0 = col, c1 = cols;
    } else {
      c0 = max(col - r, 0);
      c1 = c0 + min(2 * r, cols - c0);
    }
    c1 = min(c1, cols);
    const int ya = max(r0, y0), yb = min(r1, y0 + nr);
    if (c0 < c1) {
      for (int y = ya; y < yb; ++y) {
        atomicAdd(&diff[(y - y0) * width + c0], 1);
        atomicAdd(&diff[(y - y0) * width + c1], -1);
      }
    }
  }
  __syncthreads();
  // prefix sum per row: word sums, a scan of each row's words, then the bits of every word
  for (int i = tid; i < nr * wpr; i += kMaskThreads) {
    const int rr = i / wpr, w = i - rr * wpr;
    int s = 0;
    for (int j = 0; j < 32 && 32 * w + j < cols; ++j) {
      s += diff[rr * width + 32 * w + j];
    }
    word_base[rr][w] = s;
  }
  __syncthreads();
  if (tid < nr) {
    int s = 0;
    for (int w = 0; w < wpr; ++w) {
      const int t = word_base[tid][w];
      word_base[tid][w] = s;
      s += t;
    }
  }
  __syncthreads();
  for (int i = tid; i < nr * wpr; i += kMaskThreads) {
    const int rr = i / wpr, w = i - rr * wpr;
    int s = word_base[rr][w];
    uint32_t bits = 0;
    for (int j = 0; j < 32 && 32 * w + j < cols; ++j) {
      s += diff[rr * width + 32 * w + j];
      bits |= (s > 0 ? 1u : 0u) << j;
    }
    out[i] = bits;
  }
}

// ---- corner response of a 64x16 tile and its 1-px ring (cornerMinEigenVal, blockSize 3, ksize 3) ----
// PASS 0: the maximum of each run's mask.  PASS 1: the candidates of each run.
template <int PASS>
__global__ __launch_bounds__(kRespThreads) void response_kernel(const SelArgs a) {
  __shared__ uint8_t im[kImgH][kImgW];
  __shared__ float prod[3][kProdH][kProdW];
  __shared__ float hsum[3][kProdH][kEigW];
  __shared__ float eig[kEigH][kEigW];
  __shared__ uint32_t red[2][kRespThreads / 64];
  __shared__ int n_local[2], base[2];
  const int rows = a.b.rows, cols = a.b.cols, pitch = a.b.pitch;
  const int img = blockIdx.z, x0 = blockIdx.x * kRespW, y0 = blockIdx.y * kRespH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t* __restrict__ src = a.b.images + (size_t) img * rows * pitch;
  for (int i = tid; i < kImgH * kImgW; i += kRespThreads) {
    const int iy = i / kImgW, ix = i - iy * kImgW;
    im[iy][ix] = src[(size_t) reflect_clamp(y0 - 3 + iy, rows) * pitch + reflect_clamp(x0 - 3 + ix, cols)];
  }
  if (tid < 2) {
    n_local[tid] = 0;
  }
  __syncthreads();
  // products at image positions (y0 - 2 + py, x0 - 2 + px); outside the image they are those of the reflected position
  // (cv::boxFilter pads the products, not the image).  Sobel as exact integers, then one rounding to float.
  const float scale = (float) (1.0 / (4.0 * 3.0 * 255.0));
  for (int i = tid; i < kProdH * kProdW; i += kRespThreads) {
    const int py = i / kProdW, px = i - py * kProdW;
    const int iy = min(max(reflect_clamp(y0 - 2 + py, rows) - (y0 - 3), 1), kImgH - 2);
    const int ix = min(max(reflect_clamp(x0 - 2 + px, cols) - (x0 - 3), 1), kImgW - 2);
    const int sx = ((int) im[iy - 1][ix + 1] - (int) im[iy - 1][ix - 1]) + 2 * ((int) im[iy][ix + 1] - (int) im[iy][ix - 1]) +
                   ((int) im[iy + 1][ix + 1] - (int) im[iy + 1][ix - 1]);
    const int sy = ((int) im[iy + 1][ix - 1] - (int) im[iy - 1][ix - 1]) + 2 * ((int) im[iy + 1][ix] - (int) im[iy - 1][ix]) +
                   ((int) im[iy + 1][ix + 1] - (int) im[iy - 1][ix + 1]);
    const float dx = (float) sx * scale, dy = (float) sy * scale;
    prod[0][py][px] = dx * dx;
    prod[1][py][px] = dx * dy;
    prod[2][py][px] = dy * dy;
  }
  __syncthreads();
  for (int i = tid; i < 3 * kProdH * kEigW; i += kRespThreads) {
    const int c = i / (kProdH * kEigW), rem = i - c * (kProdH * kEigW), py = rem / kEigW, ex = rem - py * kEigW;
    hsum[c][py][ex] = (prod[c][py][ex] + prod[c][py][ex + 1]) + prod[c][py][ex + 2];
  }
  __syncthreads();
  for (int i = tid; i < kEigH * kEigW; i += kRespThreads) {
    const int ey = i / kEigW, ex = i - ey * kEigW;
    const float sxx = (hsum[0][ey][ex] + hsum[0][ey + 1][ex]) + hsum[0][ey + 2][ex];
    const float sxy = (hsum[1][ey][ex] + hsum[1][ey + 1][ex]) + hsum[1][ey + 2][ex];
    const float syy = (hsum[2][ey][ex] + hsum[2][ey + 1][ex]) + hsum[2][ey + 2][ex];
    const float ca = sxx * 0.5f, cb = sxy, cc = syy * 0.5f, d = ca - cc;
    eig[ey][ex] = (ca + cc) - sqrtf(d * d + cb * cb);  // calcMinEigenVal
  }
  __syncthreads();
  const uint32_t* __restrict__ mask = a.mask + (size_t) img * rows * a.wpr;
  constexpr int kPer = kRespW * kRespH / kRespThreads;  // 4 pixels per thread
  if (PASS == 0) {
    uint32_t m0 = 0, m1 = 0;
    for (int k = 0; k < kPer; ++k) {
      const int i = tid + kRespThreads * k, ly = i / kRespW, lx = i - ly * kRespW, y = y0 + ly, x = x0 + lx;
      if (y < rows && x < cols) {
        const uint32_t o = ordered(eig[ly + 1][lx + 1]);
        if ((mask[(size_t) y * a.wpr + (x >> 5)] >> (x & 31)) & 1u) {
          m0 = max(m0, o);
        } else {
          m1 = max(m1, o);
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      m0 = max(m0, (uint32_t) __shfl_xor((int) m0, off));
      m1 = max(m1, (uint32_t) __shfl_xor((int) m1, off));
    }
    if (lane == 0) {
      red[0][wave] = m0;
      red[1][wave] = m1;
    }
    __syncthreads();
    if (tid < 2) {
      uint32_t m = 0;
      for (int w = 0; w < kRespThreads / 64; ++w) {
        m = max(m, red[tid][w]);
      }
      if (m && run_active(a, img, tid)) {
        atomicMax(&a.maxima[2 * img + tid], m);
      }
    }
    return;
  }
  const bool active1 = run_active(a, img, 1);
  const float thr0 = run_threshold(a, img, 0), thr1 = active1 ? run_threshold(a, img, 1) : 0.0f;
  unsigned long long key[kPer];
  int pos[kPer], run_of[kPer];
  for (int k = 0; k < kPer; ++k) {
    const int i = tid + kRespThreads * k, ly = i / kRespW, lx = i - ly * kRespW, y = y0 + ly, x = x0 + lx;
    run_of[k] = -1;
    if (y >= 1 && y <= rows - 2 && x >= 1 && x <= cols - 2) {
      const int run = ((mask[(size_t) y * a.wpr + (x >> 5)] >> (x & 31)) & 1u) ? 0 : 1;
      if (run == 0 || active1) {
        const float thr = run ? thr1 : thr0;
        const float e = eig[ly + 1][lx + 1];
        if (e > thr && e != 0.0f) {  // thresholded value non-zero
          bool peak = true;
          for (int dy = 0; dy < 3; ++dy) {
            for (int dx = 0; dx < 3; ++dx) {
              const float en = eig[ly + dy][lx + dx];
              peak = peak && (en > thr ? en : 0.0f) <= e;  // e == 3x3 maximum of the thresholded map
            }
          }
          if (peak) {
            run_of[k] = run;
            key[k]    = ((unsigned long long) ordered(e) << 32) | (uint32_t) (y * cols + x);
            pos[k]    = atomicAdd(&n_local[run], 1);
          }
        }
      }
    }
  }
  __syncthreads();
  if (tid < 2) {
    base[tid] = n_local[tid] ? (int) atomicAdd(&a.n_cand[2 * img + tid], (uint32_t) n_local[tid]) : 0;  // one atomic per run
  }
  __syncthreads();
  for (int k = 0; k < kPer; ++k) {
    if (run_of[k] >= 0) {
      const int at = base[run_of[k]] + pos[k];
      if (at < a.cap) {  // beyond: the run fails with PRS_ERR_CAPACITY (select_kernel sees the count)
        a.cand[((size_t) img * 2 + run_of[k]) * a.cap + at] = key[k];
      }
    }
  }
}

// ---- one run of one image: sort, greedy min-distance acceptance, border filter ----
__global__ __launch_bounds__(kSelThreads) void select_kernel(const SelArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];  // [sort_n]; then pixels [n] | cell heads
  const int img = blockIdx.x, run = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int slot = 2 * img + run;
  if (!run_active(a, img, run)) {
    if (tid == 0) {
      a.n_sel[slot] = 0;
    }
    return;
  }
  const int n = (int) a.n_cand[slot];
  if (n > a.cap) {
    if (tid == 0) {
      a.n_sel[slot] = -1;
    }
    return;
  }
  int P = 2;
  while (P < n) {
    P <<= 1;
  }
  const unsigned long long* __restrict__ cand = a.cand + (size_t) slot * a.cap;
  for (int i = tid; i < P; i += kSelThreads) {
    keys[i] = i < n ? cand[i] : 0ull;  // 0 sorts last (no real key is 0: its response would be a NaN)
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {  // bitonic sort, descending
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kSelThreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = keys[i], y = keys[ixj];
          if ((i & k) == 0 ? x < y : x > y) {
            keys[i]   = y;
            keys[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  // the sorted pixel indices into the first half of the keys' bytes (chunks: read, barrier, write)
  uint32_t* pix = reinterpret_cast<uint32_t*>(keys);
  for (int c = 0; c < n; c += kSelThreads) {
    const int i = c + tid;
    const uint32_t v = i < n ? (uint32_t) keys[i] : 0u;
    __syncthreads();
    if (i < n) {
      pix[i] = v;
    }
  }
  int* heads = reinterpret_cast<int*>(pix + a.sort_n);  // [gw * gh] (the second half of the keys' bytes)
  uint32_t* acc_pix = reinterpret_cast<uint32_t*>(keys + a.sort_n);
  int* acc_next = reinterpret_cast<int*>(acc_pix + a.maxc);
  const int md = a.md, cells = a.md > 0 ? a.gw * a.gh : 0;
  for (int i = tid; i < cells; i += kSelThreads) {
    heads[i] = -1;
  }
  __syncthreads();
  if (tid >= 64) {
    return;
  }
  const int rows = a.b.rows, cols = a.b.cols, md2 = md * md, cell = a.cell, maxc = a.maxc;
  uint32_t* __restrict__ out = a.sel + (size_t) slot * maxc;
  int acc = 0, n_out = 0;  // (wave-uniform)
  const uint64_t below = (1ull << lane) - 1ull;
  for (int c = 0; c < n && acc < maxc; c += 64) {
    const int i = c + lane;
    const bool valid = i < n;
    const uint32_t p = valid ? pix[i] : 0u;
    const int y = (int) (p / (uint32_t) cols), x = (int) (p - (uint32_t) y * (uint32_t) cols);
    bool ok = valid;
    uint64_t later = 0;  // lanes after this one whose candidate lies closer than md
    if (md > 0) {
      const int cx = x / cell, cy = y / cell;
      for (int gy = max(cy - 1, 0); ok && gy <= min(cy + 1, a.gh - 1); ++gy) {
        for (int gx = max(cx - 1, 0); ok && gx <= min(cx + 1, a.gw - 1); ++gx) {
          for (int j = valid ? heads[gy * a.gw + gx] : -1; j >= 0; j = acc_next[j]) {
            const uint32_t q = acc_pix[j];
            const int qy = (int) (q / (uint32_t) cols), qx = (int) (q - (uint32_t) qy * (uint32_t) cols);
            if ((x - qx) * (x - qx) + (y - qy) * (y - qy) < md2) {
              ok = false;
              break;
            }
          }
        }
      }
      const int last = min(63, n - 1 - c);
      for (int t = 1; t <= last; ++t) {
        const int xt = __shfl(x, t), yt = __shfl(y, t);
        if (t > lane && (x - xt) * (x - xt) + (y - yt) * (y - yt) < md2) {
          later |= 1ull << t;
        }
      }
    }
    uint64_t alive = __ballot(ok), taken = 0;
    int budget = maxc - acc;
    while (alive && budget > 0) {  // in candidate order: take the first alive one, drop the later ones it conflicts with
      const int j = __builtin_ctzll(alive);
      const uint64_t lj = ((uint64_t) (uint32_t) __shfl((int) (later >> 32), j) << 32) | (uint32_t) __shfl((int) later, j);
      taken |= 1ull << j;
      alive &= ~(1ull << j) & ~lj;
      --budget;
    }
    const bool mine = (taken >> lane) & 1ull;
    if (mine) {
      const int idx = acc + __popcll(taken & below);
      acc_pix[idx] = p;
      if (md > 0) {
        acc_next[idx] = atomicExch(&heads[(y / cell) * a.gw + x / cell], idx);
      }
    }
    acc += __popcll(taken);
    const bool inside = mine && x >= kBorder && x < cols - kBorder && y >= kBorder && y < rows - kBorder;
    const uint64_t m = __ballot(inside);
    if (inside) {
      out[n_out + __popcll(m & below)] = p;
    }
    n_out += __popcll(m);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the accepted set of this chunk is read by the next
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    a.n_sel[slot] = n_out;
  }
}

__global__ __launch_bounds__(256) void finalize_kernel(const SelArgs a) {
  const int img = blockIdx.x, tid = threadIdx.x;
  const int n0 = a.n_sel[2 * img], n1 = a.n_sel[2 * img + 1];
  int status = PRS_OK;
  if (a.bad[img]) {
    status = PRS_ERR_RANGE;
  } else if (n0 < 0 || n1 < 0 || n0 + n1 > a.b.stride) {
    status = PRS_ERR_CAPACITY;
  } else if (n0 + n1 == 0) {
    status = PRS_WARN_NO_MATCHES;
  }
  const int n = status < 0 ? 0 : n0 + n1;
  const uint32_t* __restrict__ s0 = a.sel + (size_t) (2 * img) * a.maxc;
  const uint32_t* __restrict__ s1 = a.sel + (size_t) (2 * img + 1) * a.maxc;
  uint32_t* __restrict__ kept = a.kept + (size_t) img * a.b.stride;
  for (int i = tid; i < n; i += 256) {
    kept[i] = i < n0 ? s0[i] : s1[i - n0];
  }
  if (tid == 0) {
    a.b.n_features[img] = n;
    a.b.status[img]     = status;
  }
}

}  // namespace

int selective_extract_launch(prs_context* ctx, const prs_selective_extractor_params* params, const prs_selective_extract_batch* batch) {
  if (!params || !batch || !batch->images) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_extract_features_selective_batch: image not set");
  }
  if (!batch->keypoints || !batch->descriptors || !batch->n_features || !batch->status) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_extract_features_selective_batch: target feature buffer not set");
  }
  if (batch->projections && (!batch->n_projections || batch->projection_stride <= 0)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_extract_features_selective_batch: projections without n_projections / projection_stride");
  }
  if (!aligned_to(batch->keypoints, 8) || !aligned_to(batch->descriptors, 4) || !aligned_to(batch->projections, 8)) {
    // mask_raster_kernel loads a projection, describe_kernel stores a keypoint as one piece and a descriptor in words
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_extract_features_selective_batch: keypoints and projections must be 8-byte aligned, descriptors 4-byte");
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  if (params->detector_type != PRS_DETECTOR_GFTT) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_extract_features_selective_batch: only the GFTT detector is built");
  }
  if (params->descriptor_type != PRS_DESCRIPTOR_ORB_256 && params->descriptor_type != PRS_DESCRIPTOR_BRIEF_256) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_extract_features_selective_batch: unknown descriptor_type");
  }
  const int cap = params->max_candidates > 0 ? params->max_candidates : kDefaultCandidates;
  if (batch->rows < 8 || batch->cols < 8 || batch->rows > kMaxSide || batch->cols > kMaxSide || batch->pitch < batch->cols || batch->stride <= 0 ||
      params->target_number_of_keypoints < 1 || params->target_number_of_keypoints > kMaxCorners || params->target_bin_width_pixels < 0 ||
      params->target_bin_width_pixels > kMaxSide || params->max_candidates < 0 || cap > kMaxCandidates) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED,
                    "prs_extract_features_selective_batch: image side outside [8, 4096], target_number_of_keypoints outside [1, 8192], "
                    "target_bin_width_pixels outside [0, 4096] or max_candidates above 16384");
  }
  SelArgs a;
  memset(&a, 0, sizeof(a));
  a.p      = *params;
  a.b      = *batch;
  a.cap    = cap;
  a.maxc   = params->target_number_of_keypoints;
  a.sort_n = 2;
  while (a.sort_n < cap) {
    a.sort_n <<= 1;
  }
  a.md   = params->target_bin_width_pixels;
  a.cell = a.md > 0 ? a.md : 1;  // cells of at least minDistance: the 3x3 cells around a candidate hold every conflict
  a.gw = (batch->cols + a.cell - 1) / a.cell;
  a.gh = (batch->rows + a.cell - 1) / a.cell;
  while (a.md > 0 && (size_t) a.gw * a.gh > (size_t) a.sort_n) {  // the heads live in the half of the keys' LDS the pixels leave free
    a.cell *= 2;
    a.gw = (batch->cols + a.cell - 1) / a.cell;
    a.gh = (batch->rows + a.cell - 1) / a.cell;
  }
  const size_t lds_sel = (size_t) a.sort_n * 8 + (size_t) a.maxc * 8;
  if (lds_sel > kMaxLds) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_extract_features_selective_batch: max_candidates and target_number_of_keypoints exceed the LDS");
  }
  prs_extract_batch eb;
  eb.batch       = batch->batch;
  eb.rows        = batch->rows;
  eb.cols        = batch->cols;
  eb.pitch       = batch->pitch;
  eb.images      = batch->images;
  eb.stride      = batch->stride;
  eb.keypoints   = batch->keypoints;
  eb.intensity   = batch->intensity;
  eb.descriptors = batch->descriptors;
  eb.n_features  = batch->n_features;
  eb.status      = batch->status;
  hipStream_t stream = ctx_stream(ctx);
  Launches on(ctx, "prs_extract_features_selective_batch", stream);  // its own launches and the describe stage's
  const Grid mask     = on.grid(((int64_t) batch->rows + kMaskRows - 1) / kMaskRows, batch->batch, kMaskThreads);
  const Grid tiles    = on.grid(((int64_t) batch->cols + kRespW - 1) / kRespW, ((int64_t) batch->rows + kRespH - 1) / kRespH, batch->batch, kRespThreads);
  const Grid select   = on.grid(batch->batch, 2, kSelThreads);
  const Grid finalize = on.grid(batch->batch, 256);
  const DescribeGrids describe = describe_selected_grids(on, eb);
  PRS_TRY(on.check());
  const size_t B = (size_t) batch->batch;
  a.wpr = (batch->cols + 31) / 32;
  const size_t b_mask = align256(B * batch->rows * a.wpr * 4), b_small = align256(B * 5 * 4), b_cand = align256(B * 2 * cap * 8);
  const size_t b_sel = align256(B * 2 * a.maxc * 4), b_nsel = align256(B * 2 * 4), b_kept = align256(B * batch->stride * 4);
  unsigned char* d = static_cast<unsigned char*>(ctx_arena(ctx, ARENA_WORK_3, b_mask + b_small + b_cand + b_sel + b_nsel + b_kept));
  if (!d) {
    return ctx_fail(ctx, PRS_ERR_HIP, "prs_extract_features_selective_batch: scratch allocation failed");
  }
  a.mask   = reinterpret_cast<uint32_t*>(d);
  a.maxima = reinterpret_cast<uint32_t*>(d + b_mask);  // maxima [2B] | n_cand [2B] | bad [B]: zeroed together
  a.n_cand = a.maxima + 2 * B;
  a.bad    = reinterpret_cast<int32_t*>(a.n_cand + 2 * B);
  a.cand   = reinterpret_cast<unsigned long long*>(d + b_mask + b_small);
  a.sel    = reinterpret_cast<uint32_t*>(d + b_mask + b_small + b_cand);
  a.n_sel  = reinterpret_cast<int32_t*>(d + b_mask + b_small + b_cand + b_sel);
  a.kept   = reinterpret_cast<uint32_t*>(d + b_mask + b_small + b_cand + b_sel + b_nsel);
  hipError_t e = hipMemsetAsync(a.maxima, 0, B * 5 * 4, stream);
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_extract_features_selective_batch: counters");
  }
  const size_t lds_mask = (size_t) kMaskRows * (batch->cols + 1) * sizeof(int);
  e = allow_lds(mask_raster_kernel, lds_mask, true);
  if (e == hipSuccess) {
    e = allow_lds(select_kernel, lds_sel, true);
  }
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_extract_features_selective_batch: LDS of the mask / selection kernels");
  }
  on.launch(mask_raster_kernel, mask, lds_mask, a);
  on.launch(response_kernel<0>, tiles, 0, a);
  on.launch(response_kernel<1>, tiles, 0, a);
  on.launch(select_kernel, select, lds_sel, a);
  on.launch(finalize_kernel, finalize, 0, a);
  PRS_TRY(on.finish());
  return describe_selected_launch(ctx, on, describe, &eb, a.kept);
}

}  // namespace prs
