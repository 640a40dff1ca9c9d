// dense_align.hip -- the dense frame-to-model aligner on the device (prs_dense_align_batch_run; the rule is stated in
// include/proslam_hip_dense_align.h, BUILD-DEFINED, and restated in tests/dense_align_ref.py).
//   head       a thread a pair: whether the twelve top-row entries of X[b] are finite, as a flag into the workspace.  The flag is the
//              INPUT's: the estimate the steps write is judged by the rule alone
//   linearise  one workgroup of 256 threads per chunk of 256 * P samples of one pair, consecutive lanes on consecutive samples, a
//              thread on its P samples in ascending order.  X[b] is a workgroup-uniform read; the live depth is a coalesced load, the
//              model a gather of 4 + 16 bytes.  The 29 running sums and the class counts stay in registers, are combined by the
//              butterfly of wave_sum and through four LDS rows in the order ((W0 + W1) + W2) + W3: one barrier and one 128-byte store
//              (29 sums, the four counts packed two a word) a chunk
//   solve      one wave per pair, four pairs a workgroup, the waves never meet: chunk c on lane c mod 64 in ascending c, the butterfly,
//              the camera-frame system, Rt^T Hc Rt and Rt^T bc in the plain multiply-add form (point_align.hip, assemble_system),
//              prs::gn_step; lane 0 writes X and the result
// No float atomic: the shape of the reduction is fixed, so the same inputs give the same bits for every batch size and position.
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <string>

#include "../../include/proslam_hip_dense_align.h"
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
constexpr int kP       = PRS_DENSE_ALIGN_SAMPLES_PER_THREAD;
constexpr int kChunk   = kThreads * kP;  // samples of a chunk
constexpr int kSums    = 29;             // 21 of g g^T, 6 of g r, chi of the inliers, chi or the threshold of all weighted
constexpr int kWords   = 32;             // words of a chunk's record: the sums, inliers | outliers << 16, rejected | invalid << 16, 0
constexpr int kPairsPerBlock = kThreads / PRS_WAVE;
constexpr int kUnmatched = 0, kInlier = 1, kOutlier = 2, kRejected = 3, kInvalid = 4;
static_assert(kChunk < 65536, "a chunk's counts are packed into 16 bits");

struct DenseAlignArgs {
  prs_dense_align_params p;
  prs_dense_align_batch o;
  int32_t cols_s;    // samples of a row
  int32_t n;         // samples of a pair
  int32_t chunks;    // chunks of a pair
  int32_t it;        // the linearisation this launch belongs to
  int32_t last;      // it is the last one: the mask is written
  int32_t* flag;     // [batch] 1: X[b] was not finite when the call began
  uint32_t* sums;    // [batch][chunks][kWords]
};

// ---- head: thread = b ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dense_align_head_kernel(const DenseAlignArgs a) {
  const int64_t b = (int64_t) blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.o.batch) {
    return;
  }
  const float* X = a.o.X + (size_t) b * 16;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    finite = finite && finite_bits(X[i]);
  }
  a.flag[b] = finite ? 0 : 1;
}

// ---- linearise: blockIdx.x = the chunk, blockIdx.y = b ------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(kThreads) void dense_align_linearise_kernel(const DenseAlignArgs a) {
  __shared__ uint32_t s_row[kWaves][kWords];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), wave = tid >> 6;
  const size_t b       = blockIdx.y;
  const uint32_t chunk = blockIdx.x;
  const uint32_t n     = (uint32_t) a.n;
  const uint32_t q0    = chunk * (uint32_t) kChunk + (uint32_t) tid;  // n < 2^31: no sample index of the grid wraps
  uint8_t* mask = (a.last && a.o.mask) ? a.o.mask + b * (size_t) n : nullptr;
  if (a.flag[b] != 0) {  // uniform over the workgroup
    if (mask) {
#pragma unroll
      for (int j = 0; j < kP; ++j) {
        const uint32_t q = q0 + (uint32_t) (j * kThreads);
        if (q < n) {
          mask[q] = kUnmatched;
        }
      }
    }
    return;
  }
  const prs_dense_align_params& P = a.p;
  const float* Xb = a.o.X + b * 16;
  float X[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    X[i] = Xb[i];
  }
  const int rows = a.o.rows, cols = a.o.cols, step = a.o.step;
  const float frows = (float) rows, fcols = (float) cols;
  const uint32_t cols_s = (uint32_t) a.cols_s;
  const float max_d2    = P.max_distance * P.max_distance;
  const float tau       = P.chi_threshold;
  const bool saturated  = P.robustifier == PRS_ROBUSTIFIER_SATURATED;
  const uint8_t* live   = static_cast<const uint8_t*>(a.o.live_depth);
  const uint8_t* mdepth = reinterpret_cast<const uint8_t*>(a.o.model_depth);
  const float4* mnormal = reinterpret_cast<const float4*>(a.o.model_normal);
  const float4* lnormal = reinterpret_cast<const float4*>(a.o.live_normal);

  float s[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    s[i] = 0.0f;
  }
  int n_io = 0, n_ri = 0;  // inliers | outliers << 16, rejected | invalid << 16
  for (int j = 0; j < kP; ++j) {
    const uint32_t q = q0 + (uint32_t) (j * kThreads);
    if (q >= n) {
      break;  // the thread's later samples lie further on
    }
    const uint32_t vs = q / cols_s, us = q - vs * cols_s;
    const int v = (int) vs * step, u = (int) us * step;
    const size_t line = b * (size_t) rows + (size_t) v;
    const float raw   = (float) reinterpret_cast<const E*>(live + line * (size_t) a.o.live_pitch)[u];
    int cls = kUnmatched;
    float d;
    if (depth_valid(raw, P.depth_scaling_factor_to_meters, P.range_min, P.range_max, d)) {
      float p[3];
      depth_point(u, v, d, P.fx, P.fy, P.cx, P.cy, p);
      const float y0 = (X[0] * p[0] + X[1] * p[1]) + X[2] * p[2];
      const float y1 = (X[4] * p[0] + X[5] * p[1]) + X[6] * p[2];
      const float y2 = (X[8] * p[0] + X[9] * p[1]) + X[10] * p[2];
      const float m0 = y0 + X[3], m1 = y1 + X[7], m2 = y2 + X[11];
      if (m2 > 0.0f) {
        const float uf = floorf((m0 / m2 * P.fx + P.cx) + 0.5f);
        const float vf = floorf((m1 / m2 * P.fy + P.cy) + 0.5f);
        if (uf >= 0.0f && uf < fcols && vf >= 0.0f && vf < frows) {
          const int um = (int) uf, vm = (int) vf;  // below 2^31: uf < (float) cols
          if (um < cols && vm < rows) {            // false only where (float) cols rounds up, beyond 2^24 pixels along an axis
            const size_t mline = b * (size_t) rows + (size_t) vm;
            const float dm     = reinterpret_cast<const float*>(mdepth + mline * (size_t) a.o.model_pitch)[um];
            if (dm > 0.0f) {
              const float4 nr = mnormal[mline * (size_t) cols + (size_t) um];
              if (nr.w > 0.0f) {
                float f[3];
                depth_point(um, vm, dm, P.fx, P.fy, P.cx, P.cy, f);
                const float e0 = m0 - f[0], e1 = m1 - f[1], e2 = m2 - f[2];
                const float dist2 = (e0 * e0 + e1 * e1) + e2 * e2;
                const float r     = (nr.x * e0 + nr.y * e1) + nr.z * e2;
                const float chi   = r * r;
                if (!finite_bits(dist2) || !finite_bits(chi)) {
                  cls = kInvalid;
                } else {
                  bool pass = dist2 <= max_d2;
                  if (pass && lnormal) {
                    const float4 l = lnormal[line * (size_t) cols + (size_t) u];
                    const float k0 = (X[0] * l.x + X[1] * l.y) + X[2] * l.z;
                    const float k1 = (X[4] * l.x + X[5] * l.y) + X[6] * l.z;
                    const float k2 = (X[8] * l.x + X[9] * l.y) + X[10] * l.z;
                    pass = l.w > 0.0f && (k0 * nr.x + k1 * nr.y) + k2 * nr.z >= P.min_normal_cos;
                  }
                  if (!pass) {
                    cls = kRejected;
                  } else {
                    const bool inlier = chi <= tau;
                    cls = inlier ? kInlier : kOutlier;
                    if (inlier) {
                      s[27] = s[27] + chi;
                      s[28] = s[28] + chi;
                    } else {
                      s[28] = s[28] + tau;
                    }
                    if (inlier || saturated) {
                      const float w = inlier ? 1.0f : 1.0f / chi;
                      const float g[6] = {nr.x, nr.y, nr.z, y1 * nr.z - y2 * nr.y, y2 * nr.x - y0 * nr.z, y0 * nr.y - y1 * nr.x};
                      int k = 0;
#pragma unroll
                      for (int i = 0; i < 6; ++i) {
#pragma unroll
                        for (int jj = i; jj < 6; ++jj) {
                          s[k] = s[k] + w * (g[i] * g[jj]);
                          ++k;
                        }
                      }
#pragma unroll
                      for (int i = 0; i < 6; ++i) {
                        s[21 + i] = s[21 + i] + w * (g[i] * r);
                      }
                    }
                  }
                }
              }
            }
          }
        }
      }
    }
    n_io += cls == kInlier ? 1 : (cls == kOutlier ? 0x10000 : 0);
    n_ri += cls == kRejected ? 1 : (cls == kInvalid ? 0x10000 : 0);
    if (mask) {
      mask[q] = (uint8_t) cls;
    }
  }
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    s[i] = wave_sum(s[i]);
  }
  n_io = wave_sum(n_io);
  n_ri = wave_sum(n_ri);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
      s_row[wave][i] = __float_as_uint(s[i]);
    }
    s_row[wave][29] = (uint32_t) n_io;
    s_row[wave][30] = (uint32_t) n_ri;
    s_row[wave][31] = 0u;
  }
  __syncthreads();
  if (tid < kWords) {
    uint32_t word;
    if (tid < kSums) {
      const float t = ((__uint_as_float(s_row[0][tid]) + __uint_as_float(s_row[1][tid])) + __uint_as_float(s_row[2][tid])) +
                      __uint_as_float(s_row[3][tid]);
      word = __float_as_uint(t);
    } else {
      word = ((s_row[0][tid] + s_row[1][tid]) + s_row[2][tid]) + s_row[3][tid];
    }
    a.sums[(b * (size_t) a.chunks + (size_t) chunk) * kWords + (size_t) tid] = word;
  }
}

// ---- solve: wave = b ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dense_align_solve_kernel(const DenseAlignArgs a) {
  const int lane     = threadIdx.x & (PRS_WAVE - 1);
  const int64_t pair = (int64_t) blockIdx.x * kPairsPerBlock + (threadIdx.x >> 6);
  if (pair >= a.o.batch) {
    return;  // whole wave: nothing below waits for it
  }
  const prs_dense_align_params& P = a.p;
  const size_t b = (size_t) pair;
  prs_dense_align_result* res = a.o.result + b;
  if (a.flag[b] != 0) {  // uniform over the wave
    if (lane == 0 && a.it == 0) {
      prs_dense_align_result zero = {};
      zero.num_samples = a.n;
      zero.warnings    = PRS_ERR_RANGE;
      *res = zero;
    }
    return;
  }
  float s[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    s[i] = 0.0f;
  }
  int n_in = 0, n_out = 0, n_rej = 0, n_inv = 0;
  for (int c = lane; c < a.chunks; c += PRS_WAVE) {
    const uint4* rec = reinterpret_cast<const uint4*>(a.sums + (b * (size_t) a.chunks + (size_t) c) * kWords);
    uint32_t w[kWords];
#pragma unroll
    for (int i = 0; i < kWords / 4; ++i) {
      const uint4 t = rec[i];
      w[4 * i] = t.x, w[4 * i + 1] = t.y, w[4 * i + 2] = t.z, w[4 * i + 3] = t.w;
    }
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
      s[i] = s[i] + __uint_as_float(w[i]);
    }
    n_in += (int) (w[29] & 0xffffu);
    n_out += (int) (w[29] >> 16);
    n_rej += (int) (w[30] & 0xffffu);
    n_inv += (int) (w[30] >> 16);
  }
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    s[i] = wave_sum(s[i]);
  }
  n_in  = wave_sum(n_in);
  n_out = wave_sum(n_out);
  n_rej = wave_sum(n_rej);
  n_inv = wave_sum(n_inv);

  float X[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    X[i] = a.o.X[b * 16 + i];
  }
  // the camera-frame system: Hc = scale scale^T o S, bc = scale o S_r, scale = (1, 1, 1, 2, 2, 2)
  float Hc[36], bc[6];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) {
        const float scale = (i >= 3 ? 2.0f : 1.0f) * (j >= 3 ? 2.0f : 1.0f);
        const float h     = scale * s[k];
        Hc[6 * i + j] = h;
        Hc[6 * j + i] = h;
        ++k;
      }
      bc[i] = (i >= 3 ? 2.0f : 1.0f) * s[21 + i];
    }
  }
  // Rt^T Hc Rt, Rt^T bc: the plain multiply-add form of prs_se3.h rotate_normal_equations (point_align.hip, assemble_system)
  float Hn[36], H[36], bb[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int blk = r >= 3 ? 1 : 0;
    const int i   = r - 3 * blk;
    const float Ri0 = X[i], Ri1 = X[4 + i], Ri2 = X[8 + i];
    const float* Y = Hc + 18 * blk;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[c] = (Ri0 * Y[3 * cb + c] + Ri1 * Y[6 + 3 * cb + c]) + Ri2 * Y[12 + 3 * cb + c];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Hn[6 * r + 3 * cb + j] = (v[0] * X[j] + v[1] * X[4 + j]) + v[2] * X[8 + j];
      }
    }
    bb[r] = (Ri0 * bc[3 * blk] + Ri1 * bc[3 * blk + 1]) + Ri2 * bc[3 * blk + 2];
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      H[6 * r + c] = Hn[6 * r + c];
      H[6 * c + r] = Hn[6 * r + c];
    }
  }
  const int status = n_in >= P.min_num_inliers ? 1 : 0;
  bool stepped = false;
  if (status && !P.linearize_only) {  // uniform over the wave: every lane runs the same solve
    stepped = gn_step(H, bb, P.damping, X);
  }
  if (lane != 0) {
    return;
  }
  const int steps_before = a.it > 0 ? res->steps_taken : 0;
  if (stepped) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      a.o.X[b * 16 + i] = X[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) {
    res->H[i] = H[i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    res->b[i] = bb[i];
  }
  res->chi_inliers   = s[27];
  res->chi_total     = s[28];
  res->num_inliers   = n_in;
  res->num_outliers  = n_out;
  res->num_rejected  = n_rej;
  res->num_invalid   = n_inv;
  res->num_unmatched = a.n - (((n_in + n_out) + n_rej) + n_inv);
  res->num_samples   = a.n;
  res->status        = status;
  res->iterations    = a.it + 1;
  res->steps_taken   = steps_before + (stepped ? 1 : 0);
  res->warnings      = 0;
  res->reserved[0]   = 0;
  res->reserved[1]   = 0;
}

// samples and chunks of a pair, 0 chunks for sizes the call refuses
struct DenseAlignShape {
  int64_t cols_s, n, chunks;
};
DenseAlignShape dense_align_shape(const int64_t batch, const int64_t rows, const int64_t cols, const int64_t step) {
  DenseAlignShape sh = {0, 0, 0};
  if (batch < 1 || rows < 1 || cols < 1 || step < 1 || rows * cols > 0x7fffffffll) {
    return sh;
  }
  sh.cols_s = (cols + step - 1) / step;
  sh.n      = ((rows + step - 1) / step) * sh.cols_s;
  const int64_t chunks = (sh.n + kChunk - 1) / kChunk;
  sh.chunks = batch * chunks > 0x7fffffffll ? 0 : chunks;
  return sh;
}
uint64_t flag_bytes(const int64_t batch) {
  return up16((uint64_t) batch * sizeof(int32_t));
}

}  // namespace

int dense_align_launch(prs_context* ctx, const prs_dense_align_params* params, const prs_dense_align_batch* batch) {
  const std::string who = "prs_dense_align_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_dense_align_params& p = *params;
  const prs_dense_align_batch& o  = *batch;
  if (!o.model_depth || !o.model_normal || !o.live_depth || !o.X || !o.result || !o.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": model_depth, model_normal, live_depth, X, result or the workspace not set").c_str());
  }
  const int64_t elem = depth_bytes(p.depth_type);
  const bool finite  = std::isfinite(p.depth_scaling_factor_to_meters) && std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) &&
                      std::isfinite(p.cy) && std::isfinite(p.range_min) && std::isfinite(p.range_max) && std::isfinite(p.max_distance) &&
                      std::isfinite(p.min_normal_cos) && std::isfinite(p.chi_threshold) && std::isfinite(p.damping);
  if (o.batch < 1 || o.rows < 1 || o.cols < 1 || o.step < 1 || p.max_iterations < 0 || (p.max_iterations < 1 && !p.linearize_only) ||
      !pitch_ok(o.model_pitch, o.cols, 4) || (elem != 0 && !pitch_ok(o.live_pitch, o.cols, elem)) || !finite ||
      !(p.depth_scaling_factor_to_meters > 0.0f) || p.range_min < 0.0f || p.range_min > p.range_max || !(p.max_distance > 0.0f) ||
      p.chi_threshold < 0.0f || p.damping < 0.0f || p.min_normal_cos < -1.0f || p.min_normal_cos > 1.0f ||
      (p.robustifier != PRS_ROBUSTIFIER_CLAMP && p.robustifier != PRS_ROBUSTIFIER_SATURATED)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size or step below 1, max_iterations negative or 0 without linearize_only, a pitch below its row or not a multiple of its element, a parameter not finite, a scale or max_distance not positive, range_min negative or above range_max, chi_threshold or damping negative, min_normal_cos outside [-1, 1], or an unknown robustifier").c_str());
  }
  if (elem == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": unknown depth type").c_str());
  }
  if (!aligned_to(o.model_normal, 16) || !aligned_to(o.live_normal, 16) || !aligned_to(o.X, 16) || !aligned_to(o.workspace, 16) ||
      !aligned_to(o.model_depth, 4) || !aligned_to(o.live_depth, (uintptr_t) elem) || !aligned_to(o.result, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": the normals, X and the workspace must be 16-byte aligned, a depth image aligned to its element, result 4-byte").c_str());
  }
  const DenseAlignShape sh = dense_align_shape(o.batch, o.rows, o.cols, o.step);
  if (sh.chunks == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": rows * cols or batch * chunks beyond 2^31 - 1").c_str());
  }
  DenseAlignArgs a;
  memset(&a, 0, sizeof(a));
  a.p      = p;
  a.o      = o;
  a.cols_s = (int32_t) sh.cols_s;
  a.n      = (int32_t) sh.n;
  a.chunks = (int32_t) sh.chunks;
  a.flag   = static_cast<int32_t*>(o.workspace);
  a.sums   = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(o.workspace) + flag_bytes(o.batch));
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid head      = on.grid(((int64_t) o.batch + kThreads - 1) / kThreads, kThreads);
  const Grid linearise = on.grid(sh.chunks, o.batch, kThreads);
  const Grid solve     = on.grid(((int64_t) o.batch + kPairsPerBlock - 1) / kPairsPerBlock, kThreads);
  PRS_TRY(on.check());
  on.launch(dense_align_head_kernel, head, 0, a);
  const int iterations = p.linearize_only ? 1 : p.max_iterations;
  for (int it = 0; it < iterations; ++it) {
    a.it   = it;
    a.last = it + 1 == iterations ? 1 : 0;
    if (p.depth_type == PRS_DEPTH_U16) {
      on.launch(dense_align_linearise_kernel<uint16_t>, linearise, 0, a);
    } else {
      on.launch(dense_align_linearise_kernel<float>, linearise, 0, a);
    }
    on.launch(dense_align_solve_kernel, solve, 0, a);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_dense_align_struct_sizes(uint64_t* sizes3) {
  sizes3[0] = sizeof(prs_dense_align_params);
  sizes3[1] = sizeof(prs_dense_align_batch);
  sizes3[2] = sizeof(prs_dense_align_result);
}

uint64_t prs_dense_align_workspace_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t step) {
  const DenseAlignShape sh = dense_align_shape(batch, rows, cols, step);
  if (sh.chunks == 0) {
    return 0;
  }
  return flag_bytes(batch) + (uint64_t) batch * (uint64_t) sh.chunks * kWords * sizeof(uint32_t);
}

int prs_dense_align_batch_run(prs_context* ctx, const prs_dense_align_params* params, const prs_dense_align_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return dense_align_launch(ctx, params, batch);
}

}  // extern "C"
