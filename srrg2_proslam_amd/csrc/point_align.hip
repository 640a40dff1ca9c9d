// point_align.hip -- the loop aligner on the device: MultiAligner3DQR "loop_aligner" with one AlignerSliceProcessor3D
// (registration/aligner_slice_processor_3d.hpp:7-22: SE3Point2PointErrorFactor, information I3; registration/instances.cpp:28,52),
// run on the correspondences the brute-force matcher emits (include/proslam_hip.h, prs_point_align_batch).
//
// One launch per batch:
//   point_align_kernel<K>  one wave per cloud pair, four pairs per workgroup of 256 threads.  The waves never meet: there is no
//                          workgroup barrier and no LDS.  A wave first checks its pair (status passed through, counts against
//                          the strides, every index against n_fixed / n_moving) and parks the matched points of its first K
//                          correspondences per lane in registers (correspondence k = lane + 64 j, j < K); the rest are streamed
//                          from memory in every iteration.  Then max_iterations times: linearise at X, Gauss-Newton step.
//
// Linearisation (BUILD-DEFINED, the header states the arithmetic).  With y = R p, e = y + t - f and J = [I | -2 [y]x] Rt
// (Rt = blockdiag(R, R)), the terms of J^T J and J^T e before the rotation are
//   sum w,  sum w y,  sum w [y]x^T [y]x  (six entries, accumulated as w (y1 y1 + y2 y2), ..., w (y0 y1), ... -- never as
//   |y|^2 I - y y^T, which cancels at KITTI depths),  sum w e,  sum w (y x e)
// plus the two chi sums: 18 running float sums per lane.  Each lane adds the terms of its correspondences in ascending k; the
// lanes are then combined by a butterfly v <- v + v[lane ^ m] for m = 32, 16, 8, 4, 2, 1 (float addition is commutative, so every
// lane ends with the same bits and runs the same uniform solve: no broadcast).  The 6 x 6 camera-frame system is assembled from
// the sums with exact scalings (x 2, x 4, negation) and rotated once, Rt^T H Rt and Rt^T b, by the plain multiply-add form of
// prs_se3.h rotate_normal_equations (no fused operations here: the library builds with -ffp-contract=off).  prs::gn_step solves.
// The shape is the same for every batch size, position in the batch, instantiation K and entry point.
#include <string.h>

#include <cmath>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kThreads = 256, kPairsPerBlock = kThreads / 64;
constexpr int kMaxCorrStride = 8192;
constexpr int kSums = 18;  // w, w y (3), w [y]x^T[y]x (6), w e (3), w y x e (3), chi_inliers, chi_total

struct PointAlignArgs {
  prs_point_align_pairs b;
  prs_point_align_params p;
};

// terms of one correspondence, added to the lane's running sums; returns 1 inlier, 0 outlier, -1 invalid
__device__ __forceinline__ int accumulate(const float* X, const float tau, const bool saturated, const float px, const float py,
                                          const float pz, const float fx, const float fy, const float fz, float* s) {
  const float y0 = (X[0] * px + X[1] * py) + X[2] * pz;
  const float y1 = (X[4] * px + X[5] * py) + X[6] * pz;
  const float y2 = (X[8] * px + X[9] * py) + X[10] * pz;
  const float e0 = (y0 + X[3]) - fx;
  const float e1 = (y1 + X[7]) - fy;
  const float e2 = (y2 + X[11]) - fz;
  const float chi = (e0 * e0 + e1 * e1) + e2 * e2;
  if (!__builtin_isfinite(chi)) {
    return -1;
  }
  const bool inlier = chi <= tau;
  if (inlier) {
    s[16] = s[16] + chi;
    s[17] = s[17] + chi;
  } else {
    s[17] = s[17] + tau;
  }
  if (inlier || saturated) {
    const float w = inlier ? 1.0f : 1.0f / chi;
    s[0]  = s[0] + w;
    s[1]  = s[1] + w * y0;
    s[2]  = s[2] + w * y1;
    s[3]  = s[3] + w * y2;
    s[4]  = s[4] + w * (y1 * y1 + y2 * y2);
    s[5]  = s[5] + w * (y0 * y0 + y2 * y2);
    s[6]  = s[6] + w * (y0 * y0 + y1 * y1);
    s[7]  = s[7] + w * (y0 * y1);
    s[8]  = s[8] + w * (y0 * y2);
    s[9]  = s[9] + w * (y1 * y2);
    s[10] = s[10] + w * e0;
    s[11] = s[11] + w * e1;
    s[12] = s[12] + w * e2;
    s[13] = s[13] + w * (y1 * e2 - y2 * e1);
    s[14] = s[14] + w * (y2 * e0 - y0 * e2);
    s[15] = s[15] + w * (y0 * e1 - y1 * e0);
  }
  return inlier ? 1 : 0;
}

// the summed system -> H (row-major 6 x 6, symmetric), b: camera-frame assembly, then Rt^T H Rt, Rt^T b
__device__ __forceinline__ void assemble_system(const float* X, const float* s, float* H, float* b) {
  float Hc[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) {
    Hc[i] = 0.0f;
  }
  Hc[0] = s[0];
  Hc[7] = s[0];
  Hc[14] = s[0];
  const float u0 = 2.0f * s[1], u1 = 2.0f * s[2], u2 = 2.0f * s[3];
  // -2 [sum w y]x (rows 0-2, columns 3-5) and its transpose
  Hc[6 * 0 + 4] = u2;
  Hc[6 * 0 + 5] = -u1;
  Hc[6 * 1 + 3] = -u2;
  Hc[6 * 1 + 5] = u0;
  Hc[6 * 2 + 3] = u1;
  Hc[6 * 2 + 4] = -u0;
  Hc[6 * 4 + 0] = u2;
  Hc[6 * 5 + 0] = -u1;
  Hc[6 * 3 + 1] = -u2;
  Hc[6 * 5 + 1] = u0;
  Hc[6 * 3 + 2] = u1;
  Hc[6 * 4 + 2] = -u0;
  // 4 sum w [y]x^T [y]x
  Hc[6 * 3 + 3] = 4.0f * s[4];
  Hc[6 * 4 + 4] = 4.0f * s[5];
  Hc[6 * 5 + 5] = 4.0f * s[6];
  const float d10 = -(4.0f * s[7]), d20 = -(4.0f * s[8]), d21 = -(4.0f * s[9]);
  Hc[6 * 4 + 3] = d10;
  Hc[6 * 3 + 4] = d10;
  Hc[6 * 5 + 3] = d20;
  Hc[6 * 3 + 5] = d20;
  Hc[6 * 5 + 4] = d21;
  Hc[6 * 4 + 5] = d21;
  const float bc[6] = {s[10], s[11], s[12], 2.0f * s[13], 2.0f * s[14], 2.0f * s[15]};
  float Hn[36];
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
    b[r] = (Ri0 * bc[3 * blk] + Ri1 * bc[3 * blk + 1]) + Ri2 * bc[3 * blk + 2];
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      H[6 * r + c] = Hn[6 * r + c];
      H[6 * c + r] = Hn[6 * r + c];
    }
  }
}

__device__ __forceinline__ void load_pair(const prs_point_align_pairs& B, const size_t pair, const int k, int& fi, int& mi) {
  const prs_corr c = B.corr[pair * (size_t) B.corr_stride + (size_t) k];
  fi = c.fixed_idx;
  mi = c.moving_idx;
}

template <int K>
__global__ __launch_bounds__(kThreads) void point_align_kernel(const PointAlignArgs a) {
  const prs_point_align_pairs& B = a.b;
  const prs_point_align_params& P = a.p;
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * kPairsPerBlock + (threadIdx.x >> 6);
  if (pair >= B.batch) {
    return;  // whole wave: nothing below waits for it
  }
  prs_point_align_result* res = B.result + pair;
  const int n  = B.n_corr[pair];
  const int nf = B.n_fixed[pair], nm = B.n_moving[pair];
  int warn     = 0;
  if (B.match_status && B.match_status[pair] < 0) {
    warn = B.match_status[pair];
  } else if (n < 0 || nf < 0 || nm < 0) {
    warn = PRS_ERR_RANGE;
  } else if (n > B.corr_stride || nf > B.fixed_stride || nm > B.moving_stride) {
    warn = PRS_ERR_CAPACITY;
  }
  const size_t p = (size_t) pair;
  const float4* fixed  = reinterpret_cast<const float4*>(B.fixed) + p * (size_t) B.fixed_stride;
  const float4* moving = reinterpret_cast<const float4*>(B.moving) + p * (size_t) B.moving_stride;
  // checks and parking: correspondence k = lane + 64 j
  float pk[K][6];
  bool bad = false;
  if (warn == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int k = lane + 64 * j;
      pk[j][0] = pk[j][1] = pk[j][2] = pk[j][3] = pk[j][4] = pk[j][5] = 0.0f;
      if (k < n) {
        int fi, mi;
        load_pair(B, p, k, fi, mi);
        if (fi < 0 || fi >= nf || mi < 0 || mi >= nm) {
          bad = true;
        } else {
          const float4 f = fixed[fi], m = moving[mi];
          pk[j][0] = m.x;
          pk[j][1] = m.y;
          pk[j][2] = m.z;
          pk[j][3] = f.x;
          pk[j][4] = f.y;
          pk[j][5] = f.z;
        }
      }
    }
    for (int k = 64 * K + lane; k < n; k += 64) {
      int fi, mi;
      load_pair(B, p, k, fi, mi);
      bad = bad || fi < 0 || fi >= nf || mi < 0 || mi >= nm;
    }
    if (__ballot(bad) != 0ull) {
      warn = PRS_ERR_RANGE;
    }
  }
  float X[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    X[i] = B.X[16 * p + i];
    asm volatile("" : "+v"(X[i]));  // the estimate lives in vector registers (the solve writes it there): no scalar copy to spill
  }
  const bool run      = warn >= 0 && n > 0 && n >= P.min_num_correspondences;
  const int iters     = !run ? 0 : (P.linearize_only ? 1 : P.max_iterations);
  const bool saturated = P.robustifier == PRS_ROBUSTIFIER_SATURATED;
  const float tau     = P.chi_threshold;
  float H[36], b[6], s[kSums];
#pragma unroll
  for (int i = 0; i < 36; ++i) {
    H[i] = 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    b[i] = 0.0f;
  }
  int n_in = 0, n_out = 0, n_inv = 0;
  float chi_in = 0.0f, chi_tot = 0.0f;
  for (int it = 0; it < iters; ++it) {
    const bool last = it + 1 == iters;
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
      s[i] = 0.0f;
    }
    n_in = n_out = n_inv = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int k  = lane + 64 * j;
      const bool act = k < n;
      int c = 0;
      if (act) {
        c = accumulate(X, tau, saturated, pk[j][0], pk[j][1], pk[j][2], pk[j][3], pk[j][4], pk[j][5], s);
        if (last && B.inlier_mask) {
          B.inlier_mask[p * (size_t) B.corr_stride + (size_t) k] = c > 0 ? 1 : 0;
        }
      }
      n_in += __popcll(__ballot(act && c > 0));
      n_out += __popcll(__ballot(act && c == 0));
      n_inv += __popcll(__ballot(act && c < 0));
    }
    for (int base = 64 * K; base < n; base += 64) {
      const int k  = base + lane;
      const bool act = k < n;
      int c = 0;
      if (act) {
        int fi, mi;
        load_pair(B, p, k, fi, mi);
        const float4 f = fixed[fi], m = moving[mi];
        c = accumulate(X, tau, saturated, m.x, m.y, m.z, f.x, f.y, f.z, s);
        if (last && B.inlier_mask) {
          B.inlier_mask[p * (size_t) B.corr_stride + (size_t) k] = c > 0 ? 1 : 0;
        }
      }
      n_in += __popcll(__ballot(act && c > 0));
      n_out += __popcll(__ballot(act && c == 0));
      n_inv += __popcll(__ballot(act && c < 0));
    }
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
      s[i] = wave_sum(s[i]);
    }
    assemble_system(X, s, H, b);
    chi_in  = s[16];
    chi_tot = s[17];
    if (!P.linearize_only) {
      gn_step(H, b, P.damping, X);
    }
  }
  if (warn >= 0 && iters == 0 && B.inlier_mask) {
    for (int k = lane; k < n; k += 64) {
      B.inlier_mask[p * (size_t) B.corr_stride + (size_t) k] = 0;
    }
  }
  if (lane != 0) {
    return;
  }
  if (warn >= 0 && n == 0) {
    warn |= PRS_WARN_NO_MATCHES;
  }
  const int status = iters > 0 && n_in >= P.min_num_inliers ? 1 : 0;
  const bool accepted = status && n_in >= P.relocalize_min_inliers && (float) n_in / (float) n >= P.relocalize_min_inliers_ratio &&
                        chi_in / (float) n_in <= P.relocalize_max_chi_inliers;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    B.X[16 * p + i] = X[i];
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) {
    res->H[i] = H[i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    res->b[i] = b[i];
  }
  res->chi_inliers         = chi_in;
  res->chi_total           = chi_tot;
  res->num_inliers         = n_in;
  res->num_outliers        = n_out;
  res->num_invalid         = n_inv;
  res->num_correspondences = n;
  res->status              = status;
  res->accepted            = accepted ? 1 : 0;
  res->iterations          = iters;
  res->warnings            = warn;
}

}  // namespace

// instantiation by corr_stride: every correspondence parked up to 64 per pair (K = 1) and 256 (K = 4); beyond, 384 parked and the
// rest streamed (K = 6: 188 VGPRs; K = 8 spills scalar registers).  params->parked_per_lane selects one for tests and A-B runs (same results).
int point_align_launch(prs_context* ctx, const prs_point_align_params* params, const prs_point_align_pairs* batch) {
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_point_align_batch: parameters not set");
  }
  if (params->robustifier != PRS_ROBUSTIFIER_CLAMP && params->robustifier != PRS_ROBUSTIFIER_SATURATED) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_point_align_batch: unknown robustifier");
  }
  if (!std::isfinite(params->chi_threshold) || !std::isfinite(params->damping) || params->max_iterations < 0) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_point_align_batch: non-finite chi_threshold or damping, or negative max_iterations");
  }
  const int K = params->parked_per_lane;
  if (K != 0 && K != 1 && K != 4 && K != 6) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_point_align_batch: parked_per_lane must be 0, 1, 4 or 6");
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  if (!batch->fixed || !batch->n_fixed || !batch->moving || !batch->n_moving || !batch->corr || !batch->n_corr || !batch->X ||
      !batch->result) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_point_align_batch: input or output buffer not set");
  }
  if (batch->fixed_stride < 1 || batch->moving_stride < 1 || batch->corr_stride < 1) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_point_align_batch: stride below 1");
  }
  if (batch->corr_stride > kMaxCorrStride) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_point_align_batch: corr_stride above 8192");
  }
  if (!aligned_to(batch->fixed, 16) || !aligned_to(batch->moving, 16) || !aligned_to(batch->corr, 4) || !aligned_to(batch->X, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_point_align_batch: point rows must be 16-byte aligned");
  }
  PointAlignArgs a;
  memset(&a, 0, sizeof(a));
  a.b = *batch;
  a.p = *params;
  const int k = K != 0 ? K : (batch->corr_stride <= 64 ? 1 : (batch->corr_stride <= 256 ? 4 : 6));
  Launches on(ctx, "prs_point_align_batch", ctx_stream(ctx));
  const Grid grid = on.grid(((int64_t) batch->batch + kPairsPerBlock - 1) / kPairsPerBlock, kThreads);
  PRS_TRY(on.check());
  if (k == 1) {
    on.launch(point_align_kernel<1>, grid, 0, a);
  } else if (k == 4) {
    on.launch(point_align_kernel<4>, grid, 0, a);
  } else {
    on.launch(point_align_kernel<6>, grid, 0, a);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

int prs_point_align_batch(prs_context* ctx, const prs_point_align_params* params, const prs_point_align_pairs* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return point_align_launch(ctx, params, batch);
}

int prs_point_align(prs_context* ctx, const prs_point_align_params* params, const float* fixed_xyz, int32_t n_fixed,
                    const float* moving_xyz, int32_t n_moving, const prs_corr* corr, int32_t n_corr, float* X16,
                    prs_point_align_result* result, uint8_t* inlier_mask) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (!params || !X16 || !result || (n_fixed > 0 && !fixed_xyz) || (n_moving > 0 && !moving_xyz) || (n_corr > 0 && !corr)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_point_align: input or output buffer not set");
  }
  if (n_fixed < 0 || n_moving < 0 || n_corr < 0) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_point_align: negative size");
  }
  if (n_corr > kMaxCorrStride) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_point_align: more than 8192 correspondences");
  }
  (void) hipSetDevice(ctx->device);
  const size_t nf = (size_t) (n_fixed > 0 ? n_fixed : 1), nm = (size_t) (n_moving > 0 ? n_moving : 1);
  const size_t nc = (size_t) (n_corr > 0 ? n_corr : 1);
  struct Meta {
    int32_t n_fixed, n_moving, n_corr, pad;
    float X[16];
  };
  // fixed rows | moving rows | correspondences | sizes, X (uploaded) | result | mask (downloaded)
  Staging st(ctx, "prs_point_align");
  auto fixed  = st.up<float>(nf * 4);
  auto moving = st.up<float>(nm * 4);
  auto pairs  = st.up<prs_corr>(nc);
  auto meta   = st.both<Meta>(1);
  auto res    = st.down<prs_point_align_result>(1);
  auto mask   = st.down<uint8_t>(nc);
  PRS_TRY(st.commit());
  float* hf = fixed.h();
  float* hm = moving.h();
  for (int32_t i = 0; i < n_fixed; ++i) {
    hf[4 * (size_t) i]     = fixed_xyz[3 * (size_t) i];
    hf[4 * (size_t) i + 1] = fixed_xyz[3 * (size_t) i + 1];
    hf[4 * (size_t) i + 2] = fixed_xyz[3 * (size_t) i + 2];
    hf[4 * (size_t) i + 3] = 0.0f;
  }
  for (int32_t i = 0; i < n_moving; ++i) {
    hm[4 * (size_t) i]     = moving_xyz[3 * (size_t) i];
    hm[4 * (size_t) i + 1] = moving_xyz[3 * (size_t) i + 1];
    hm[4 * (size_t) i + 2] = moving_xyz[3 * (size_t) i + 2];
    hm[4 * (size_t) i + 3] = 0.0f;
  }
  if (n_corr > 0) {
    memcpy(pairs.h(), corr, (size_t) n_corr * sizeof(prs_corr));
  }
  Meta& m = *meta.h();
  m.n_fixed = n_fixed, m.n_moving = n_moving, m.n_corr = n_corr, m.pad = 0;
  memcpy(m.X, X16, sizeof(m.X));
  PRS_TRY(st.upload());
  prs_point_align_pairs b;
  memset(&b, 0, sizeof(b));
  b.batch         = 1;
  b.fixed_stride  = (int32_t) nf;
  b.moving_stride = (int32_t) nm;
  b.corr_stride   = (int32_t) nc;
  b.fixed         = fixed.d();
  b.moving        = moving.d();
  b.corr          = pairs.d();
  b.n_fixed       = &meta.d()->n_fixed;
  b.n_moving      = &meta.d()->n_moving;
  b.n_corr        = &meta.d()->n_corr;
  b.X             = meta.d()->X;
  b.result        = res.d();
  b.inlier_mask   = inlier_mask ? mask.d() : nullptr;
  PRS_TRY(point_align_launch(ctx, params, &b));
  PRS_TRY(st.download());
  memcpy(result, res.h(), sizeof(prs_point_align_result));
  memcpy(X16, m.X, sizeof(m.X));
  if (inlier_mask && n_corr > 0) {
    memcpy(inlier_mask, mask.h(), (size_t) n_corr);
  }
  if (result->warnings < 0) {
    return ctx_fail(ctx, result->warnings, "prs_point_align: a correspondence index lies outside its cloud");
  }
  return result->warnings;
}

}  // extern "C"
