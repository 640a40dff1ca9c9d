/* proslam_hip_dense_align.h -- the dense frame-to-model aligner on the device (gfx950): the fifth public header of
 * libproslam_hip.so.
 *
 * include/proslam_hip.h is pinned to the layout of PRS_ABI_VERSION 104; what this header declares joins it, as it stands here, at
 * the next layout bump, and this file then only includes the main header.  Until then: the entry points below are exported from
 * the same library, use PRS_API, the status codes, prs_context, PRS_DEPTH_* and PRS_ROBUSTIFIER_* of the main header, and have
 * their own size query (prs_dense_align_struct_sizes) in the place of prs_abi_check.  Every struct ends in reserved words: memset
 * it to 0 before filling it in.
 */
#ifndef PROSLAM_HIP_DENSE_ALIGN_H
#define PROSLAM_HIP_DENSE_ALIGN_H

#include "proslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* samples a thread of the linearisation adds before the lanes are combined: part of the rule (the reduction's shape), fixed at 4
 * after both 4 and 16 were timed (profiles/dense_align/README.md) */
#define PRS_DENSE_ALIGN_SAMPLES_PER_THREAD 4

/* ================================================================================================
 * Dense align: projective data association of a live depth image against a rendered model view (depth and normal of
 * prs_tsdf_raycast_batch_run, include/proslam_hip_tsdf_raycast.h) and a point-to-plane Gauss-Newton on SE(3): the step
 * raycast -> align -> integrate of a dense tracker (KinectFusion's frame-to-model ICP).  X is the live camera in the model
 * camera's frame (liveInModel: the point aligner's movingInFixed); world poses are the caller's: camera_live = camera_model * X.
 *
 * BUILD-DEFINED, like the other dense stages: the reference has no dense tracker.  tests/dense_align_ref.py restates the rule in
 * numpy and the kernels equal that byte for byte.  All arithmetic is explicit two-operand float32 in the order written,
 * -ffp-contract=off, division and sqrtf correctly rounded, denormals kept; depth_valid and depth_point are those of csrc/prs_depth.h
 * (d = scale * raw, valid iff raw > 0 && d >= range_min && d <= range_max; point = (((float) u - cx) / fx * d,
 * ((float) v - cy) / fy * d, d)), gn_step that of csrc/prs_se3.h.
 *
 * ---- prs_dense_align_batch_run: X (in/out), result, mask (out) <- model_depth, model_normal, live_depth, live_normal (in) ----
 * One batch element b is one independent pair of a model view and a live image; one camera matrix fx, fy, cx, cy for both.
 *   samples  rows_s = (rows + step - 1) / step, cols_s likewise, N = rows_s * cols_s.  Sample q = vs * cols_s + us is the live pixel
 *            (v, u) = (vs * step, us * step).  The model is always looked up at full resolution: a coarse-to-fine schedule is
 *            calls with step 4, 2, 1 on the same X.
 * Per sample, at the current X = [R | t]:
 *   live     the raw element of live_depth(v, u) through depth_valid gives d, depth_point(u, v, d) gives p.  Not valid: UNMATCHED.
 *   move     y_i = (R_i0 * p0 + R_i1 * p1) + R_i2 * p2, m_i = y_i + t_i.  Go on iff m2 > 0 (which drops NaN).
 *   project  uf = floorf((m0 / m2 * fx + cx) + 0.5f), vf the same with m1, fy, cy.  Go on iff uf >= 0 && uf < (float) cols &&
 *            vf >= 0 && vf < (float) rows, and then, with um = (int) uf, vm = (int) vf, iff um < cols && vm < rows (the last says
 *            nothing new up to 2^24 pixels along an axis, where the float is exact).
 *   model    dm = model_depth(vm, um): go on iff dm > 0.  (n0, n1, n2, nw) = model_normal(vm, um): go on iff nw > 0.  A sample
 *            that stops in move, project or model is UNMATCHED.
 *   error    f = depth_point(um, vm, dm), e_i = m_i - f_i, dist2 = (e0 * e0 + e1 * e1) + e2 * e2, r = (n0 * e0 + n1 * e1) + n2 * e2,
 *            chi = r * r.  INVALID when dist2 or chi is not finite.
 *   gates    REJECTED unless dist2 <= max_distance * max_distance (the product formed once) and, only when live_normal is given,
 *            with (l0, l1, l2, lw) = live_normal(v, u): lw > 0 && (q0 * n0 + q1 * n1) + q2 * n2 >= min_normal_cos, q = R l in the
 *            form of `move`.
 *   weight   INLIER iff chi <= chi_threshold, weight 1; otherwise OUTLIER, weight 0 (PRS_ROBUSTIFIER_CLAMP) or 1.0f / chi
 *            (PRS_ROBUSTIFIER_SATURATED).
 *   terms    c = y x n: c0 = y1 * n2 - y2 * n1, c1 = y2 * n0 - y0 * n2, c2 = y0 * n1 - y1 * n0 (y, not m: with the right
 *            perturbation X <- X exp(dx) of VariableSE3QuaternionRight, n^T J = [n^T, 2 (y x n)^T] Rt, Rt = blockdiag(R, R)).  With
 *            g = (n0, n1, n2, c0, c1, c2) the 29 sums S are: w * (g_i * g_j) for i <= j in row-major order of the upper triangle
 *            (21), w * (g_i * r) (6), chi of the inliers, and chi of the inliers plus chi_threshold for every outlier.  An outlier
 *            of weight 0 adds nothing to the first 27.
 * Reduction (fixed shape, part of the rule; P = PRS_DENSE_ALIGN_SAMPLES_PER_THREAD): sample q belongs to chunk q / (256 * P);
 * inside the chunk the local index k goes to thread k mod 256 of a workgroup (lane k mod 64 of wave (k / 64) mod 4).  A thread adds
 * the terms of its up to P samples in ascending q, starting from +0.0f; a sample that contributes no term to a sum is skipped, not
 * added as a zero.  The 64 lanes of a wave are combined by the butterfly v <- v + v[lane ^ m], m = 32, 16, 8, 4, 2, 1, the four
 * wave totals as ((W0 + W1) + W2) + W3.  Per pair, chunk c goes to lane c mod 64 of one wave, which adds its chunks in ascending c
 * from +0.0f; the butterfly again.  The counts are integers.  The same inputs give the same bits for every batch size and every
 * position in the batch.
 * System: with scale_i = 1 for i < 3 and 2 for i >= 3, Hc[i][j] = Hc[j][i] = (scale_i * scale_j) * S_ij and bc_i = scale_i * S_ir
 * (exact powers of two); H = Rt^T Hc Rt and b = Rt^T bc in the plain multiply-add form of prs_se3.h rotate_normal_equations, as
 * the point aligner forms them: row r = 3 * blk + i of the result is v = (column i of R)^T Y, out = v R for the two 3 x 3 blocks Y of
 * block row blk of Hc, every three-term sum as (a + b) + c; the lower triangle is mirrored into the upper one.
 * Step: iff num_inliers >= min_num_inliers, prs::gn_step(H, b, damping, X), the diagonal damping form, X <- X exp(dx); a pivot that
 * is not positive leaves X its bits, as do too few inliers.
 * Loop: max_iterations times (linearise, step), no termination test; linearize_only = 1: one linearisation, no step.  The result
 * holds the LAST linearisation: H, b, chi_inliers, chi_total, the five class counts (they add up to num_samples = N), status =
 * (num_inliers >= min_num_inliers), iterations = the linearisations made, steps_taken = the steps that changed X, warnings.
 * mask (optional) [batch][N]: the class of every sample at the last linearisation, 0 unmatched, 1 inlier, 2 outlier, 3 rejected,
 * 4 invalid.
 * Per pair: when one of the twelve top-row entries of X[b] is not finite, warnings = PRS_ERR_RANGE, nothing is iterated, X[b] is
 * untouched, the mask is written as 0 and the result is all zero but num_samples and warnings.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, model_depth, model_normal, live_depth, X,
 * result or workspace unset); PRS_ERR_RANGE (batch, rows, cols or step < 1; max_iterations < 0, or < 1 without linearize_only; a
 * pitch below its row or not a multiple of its element; a parameter that is not finite; depth_scaling_factor_to_meters <= 0;
 * range_min < 0 or range_min > range_max; max_distance <= 0; chi_threshold < 0; damping < 0; min_normal_cos outside [-1, 1]; an
 * unknown robustifier); PRS_ERR_UNSUPPORTED (an unknown depth type; model_normal, live_normal, X or workspace not 16-byte aligned,
 * a depth image not aligned to its element, result not 4-byte aligned; rows * cols or batch * chunks beyond 2^31 - 1, chunks =
 * (N + 256 * P - 1) / (256 * P); a launch beyond 2^32 - 1 work-items: prs_launch_fits).
 * 1 + 2 * iterations plain launches on the context's stream.  head (a thread a pair): the X check into the workspace.  linearise
 * (a workgroup of 256 threads per chunk of one pair, consecutive lanes on consecutive samples): X[b] is a workgroup-uniform read, the
 * live depth a coalesced load, the model a gather of 4 + 16 bytes; the 29 sums stay in registers, are combined by the butterfly and
 * four LDS rows, one barrier and one 128-byte store a chunk.  solve (a wave a pair, four pairs a workgroup): sums the chunk totals,
 * assembles, rotates, steps, writes X and the result.  All indexing into the images is 64-bit.  No float atomic, no allocation, no
 * synchronisation, no host read: graph-capturable.
 *
 * Left out: a colour / photometric term; an image pyramid (the model is read at full resolution at every step); bilateral
 * pre-filtering of the live depth; a termination criterion; a host-pointer variant and a C++ adapter in plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t depth_type;                    /* PRS_DEPTH_U16 or PRS_DEPTH_F32: the live image's element */
  float depth_scaling_factor_to_meters;  /* finite, > 0: metres per unit of the live image */
  float fx, fy, cx, cy;                  /* the camera matrix of both images */
  float range_min, range_max;            /* metres of live depth, finite, 0 <= range_min <= range_max */
  float max_distance;                    /* metres, finite, > 0: the distance gate */
  float min_normal_cos;                  /* in [-1, 1]: the normal gate (read only with live_normal) */
  int32_t robustifier;                   /* PRS_ROBUSTIFIER_* */
  float chi_threshold;                   /* square metres, finite, >= 0 */
  float damping;                         /* finite, >= 0 */
  int32_t max_iterations;
  int32_t min_num_inliers;
  int32_t linearize_only;                /* 1: one linearisation, no step */
  int32_t reserved[4];
} prs_dense_align_params;

typedef struct {
  float H[36];                 /* row-major 6 x 6, symmetric */
  float b[6];
  float chi_inliers, chi_total;
  int32_t num_inliers, num_outliers, num_rejected, num_invalid, num_unmatched;
  int32_t num_samples;         /* N */
  int32_t status;              /* 1: num_inliers >= min_num_inliers at the last linearisation */
  int32_t iterations;          /* linearisations made */
  int32_t steps_taken;
  int32_t warnings;            /* 0, or PRS_ERR_RANGE: X was not finite */
  int32_t reserved[2];
} prs_dense_align_result;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t rows, cols;
  int32_t step;                 /* every step-th pixel of every step-th row of the live image is a sample */
  int32_t model_pitch;          /* bytes of a row of model_depth: a multiple of 4, at least 4 * cols */
  int32_t live_pitch;           /* bytes of a row of live_depth: a multiple of its element, at least cols of them */
  int32_t reserved0[2];
  const float* model_depth;     /* in [batch][rows][model_pitch] metres of z depth, 0 = no surface */
  const float* model_normal;    /* in [batch][rows][cols][4] in the model camera's frame, fourth float > 0 = present; 16-byte aligned */
  const void* live_depth;       /* in [batch][rows][live_pitch] */
  const float* live_normal;     /* in [batch][rows][cols][4] in the live camera's frame (NULL allowed: no normal gate); 16-byte aligned */
  float* X;                     /* in/out [batch][16] row-major, 16-byte aligned */
  prs_dense_align_result* result; /* out [batch] */
  uint8_t* mask;                /* out [batch][N] (NULL allowed) */
  void* workspace;              /* prs_dense_align_workspace_bytes(batch, rows, cols, step), 16-byte aligned */
  void* reserved[2];
} prs_dense_align_batch;

/* device pointers, asynchronous on the context's stream */
PRS_API int prs_dense_align_batch_run(prs_context* ctx, const prs_dense_align_params* params, const prs_dense_align_batch* batch);
/* bytes of the workspace, 0 for sizes the call refuses */
PRS_API uint64_t prs_dense_align_workspace_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t step);
/* sizeof prs_dense_align_params, prs_dense_align_batch, prs_dense_align_result as the library was compiled (bindings check) */
PRS_API void prs_dense_align_struct_sizes(uint64_t* sizes3);

#ifdef __cplusplus
}
#endif

#endif /* PROSLAM_HIP_DENSE_ALIGN_H */
