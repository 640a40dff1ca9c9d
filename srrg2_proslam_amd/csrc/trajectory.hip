// trajectory.hip -- trajectory evaluator on the device: Horn-aligned absolute trajectory error (ATE), fixed-delta relative pose error
// (RPE) with a per-axis block, and the KITTI devkit's subsequence errors, for B sequences in the layout prs_session_unroll_batch writes.
// The definitions are stated in include/proslam_hip.h (BUILD-DEFINED) and restated in tests/trajectory_ref.py.  All arithmetic is
// float64 on the float32 inputs.  One workgroup per sequence; every sum is a fixed-order reduction (per-thread strided partials, wave
// shuffles, a tree over the waves' partials in LDS), so a sequence's result depends neither on the batch around it nor on the run.
#include <math.h>
#include <stddef.h>

#include <cmath>

#include "prs_device.h"
#include "prs_host.h"

namespace prs {

namespace {

constexpr int kThreads = 512;
constexpr int kWaves   = kThreads / PRS_WAVE;
// LDS stage, at most this many bytes: the translations of both clouds, 24 bytes a row (4541 rows: 109 KB), and beside them, while
// they fit too, the cumulative distances of the KITTI block, 8 bytes a row (4541 rows: 145 KB in all).  A longer frame_stride reads
// the distances, then also the translations, from global memory (same arithmetic, same bits)
constexpr size_t kStageLimit = 150u * 1024u;
constexpr int kJacobiSweeps  = 12;
constexpr double kRadToDeg   = 57.295779513082320876798154814105;

#define PRS_HD __host__ __device__ __forceinline__

// the top three rows of a rigid transform, float64
struct Pose {
  double r[9];
  double t[3];
};

PRS_HD void pose_load(const float* m, Pose& T) {
  const float4* q = reinterpret_cast<const float4*>(m);
  const float4 a = q[0], b = q[1], c = q[2];
  T.r[0] = a.x, T.r[1] = a.y, T.r[2] = a.z, T.t[0] = a.w;
  T.r[3] = b.x, T.r[4] = b.y, T.r[5] = b.z, T.t[1] = b.w;
  T.r[6] = c.x, T.r[7] = c.y, T.r[8] = c.z, T.t[2] = c.w;
}

// C = A^-1 B with the rigid inverse: R = Ra^T Rb, t = Ra^T (tb - ta)
PRS_HD void pose_rel(const Pose& A, const Pose& B, Pose& C) {
  const double d0 = B.t[0] - A.t[0], d1 = B.t[1] - A.t[1], d2 = B.t[2] - A.t[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      C.r[3 * i + j] = (A.r[0 + i] * B.r[0 + j] + A.r[3 + i] * B.r[3 + j]) + A.r[6 + i] * B.r[6 + j];
    }
    C.t[i] = (A.r[0 + i] * d0 + A.r[3 + i] * d1) + A.r[6 + i] * d2;
  }
}

// C = A B^-1 with the rigid inverse: R = Ra Rb^T, t = ta - R tb
PRS_HD void pose_mul_inv(const Pose& A, const Pose& B, Pose& C) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      C.r[3 * i + j] = (A.r[3 * i + 0] * B.r[3 * j + 0] + A.r[3 * i + 1] * B.r[3 * j + 1]) + A.r[3 * i + 2] * B.r[3 * j + 2];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    C.t[i] = A.t[i] - ((C.r[3 * i + 0] * B.t[0] + C.r[3 * i + 1] * B.t[1]) + C.r[3 * i + 2] * B.t[2]);
  }
}

// the relative-pose error between rows i and j: E = (G_i^-1 G_j)^-1 (P_i^-1 P_j)
PRS_HD void pair_error(const float* Pi, const float* Pj, const float* Gi, const float* Gj, Pose& E) {
  Pose a, b, dG, dP;
  pose_load(Gi, a);
  pose_load(Gj, b);
  pose_rel(a, b, dG);
  pose_load(Pi, a);
  pose_load(Pj, b);
  pose_rel(a, b, dP);
  pose_rel(dG, dP, E);
}

// theta = atan2(|v| / 2, (tr R - 1) / 2) with v the vee of R - R^T (|v| = 2 sin theta); rv = theta v / |v|, 0 when |v| = 0
PRS_HD double rotation_error(const double* r, double* rv) {
  const double vx = r[7] - r[5], vy = r[2] - r[6], vz = r[3] - r[1];
  const double nv = sqrt((vx * vx + vy * vy) + vz * vz);
  const double tr = (r[0] + r[4]) + r[8];
  const double th = atan2(0.5 * nv, 0.5 * (tr - 1.0));
  const double s  = nv > 0.0 ? th / nv : 0.0;
  rv[0] = s * vx, rv[1] = s * vy, rv[2] = s * vz;
  return th;
}

PRS_HD double norm3(const double* v) {
  return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// one Jacobi rotation of the symmetric 4x4 a in the (P, Q) plane, accumulated in the columns of v (indices are compile-time
// constants: the matrices stay in registers)
template <int P, int Q>
PRS_HD void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) {
    return;
  }
  const double app = a[P][P], aqq = a[Q][Q];
  const double g = 100.0 * fabs(apq);
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {  // nothing left of it beside the diagonal
    a[P][Q] = 0.0;
    a[Q][P] = 0.0;
    return;
  }
  const double h = aqq - app;
  double t;
  if (fabs(h) + g == fabs(h)) {
    t = apq / h;
  } else {
    const double theta = 0.5 * h / apq;
    t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
    if (theta < 0.0) {
      t = -t;
    }
  }
  const double c = 1.0 / sqrt(1.0 + t * t);
  const double s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // a <- a J
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq;
    a[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // a <- J^T a
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk;
    a[Q][k] = s * apk + c * aqk;
  }
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
}

// Horn's closed form: the proper rotation R (det = +1) that maximises tr(R M) for M[3 a + b] = sum p'_a g'_b of the centred clouds,
// i.e. minimises sum |g' - R p'|^2 over rotations: the unit quaternion is the eigenvector of the largest eigenvalue of the symmetric
// 4x4 N(M), found by cyclic Jacobi with a fixed number of sweeps.  A quaternion always gives a proper rotation, also where the
// unconstrained optimum is a reflection.
PRS_HD void horn_rotation(const double* M, double* R) {
  const double Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
  double a[4][4], v[4][4];
  a[0][0] = (Sxx + Syy) + Szz;
  a[1][1] = (Sxx - Syy) - Szz;
  a[2][2] = (Syy - Sxx) - Szz;
  a[3][3] = (Szz - Sxx) - Syy;
  a[0][1] = a[1][0] = Syz - Szy;
  a[0][2] = a[2][0] = Szx - Sxz;
  a[0][3] = a[3][0] = Sxy - Syx;
  a[1][2] = a[2][1] = Sxy + Syx;
  a[1][3] = a[3][1] = Szx + Sxz;
  a[2][3] = a[3][2] = Syz + Szy;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  }
#pragma unroll 1
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<0, 3>(a, v);
    jacobi_rotate<1, 2>(a, v);
    jacobi_rotate<1, 3>(a, v);
    jacobi_rotate<2, 3>(a, v);
  }
  double best = a[0][0];
  double q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    if (a[j][j] > best) {
      best = a[j][j];
      q0 = v[0][j], q1 = v[1][j], q2 = v[2][j], q3 = v[3][j];
    }
  }
  const double n = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
  const double w = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// running mean and sum of squared deviations of the six axis quantities (Welford), merged pairwise (Chan): no cancellation where the
// deviation is small beside the mean
struct AxisStats {
  double n;
  double mean[6];
  double m2[6];
};

PRS_HD void axis_init(AxisStats& s) {
  s.n = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    s.mean[i] = 0.0;
    s.m2[i]   = 0.0;
  }
}

PRS_HD void axis_add(AxisStats& s, const double* x) {
  s.n += 1.0;
  const double inv = 1.0 / s.n;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double d = x[i] - s.mean[i];
    s.mean[i] += d * inv;
    s.m2[i] += d * (x[i] - s.mean[i]);
  }
}

// a <- a merged with b (b after a)
PRS_HD void axis_merge(AxisStats& a, const double bn, const double* bmean, const double* bm2) {
  const double n = a.n + bn;
  if (n > 0.0) {
    const double fb = bn / n;
    const double fab = a.n * fb;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double d = bmean[i] - a.mean[i];
      a.mean[i] += d * fb;
      a.m2[i] = (a.m2[i] + bm2[i]) + (d * d) * fab;
    }
    a.n = n;
  }
}

struct TrajArgs {
  prs_trajectory_params p;
  prs_trajectory_batch t;
  int stage_clouds;  // the translations fit the LDS
  int stage_dist;    // and the cumulative distances beside them
};

struct SumOp {
  __device__ __forceinline__ double operator()(const double a, const double b) const { return a + b; }
};
struct MaxOp {
  __device__ __forceinline__ double operator()(const double a, const double b) const { return a > b ? a : b; }
};
struct MinOp {
  __device__ __forceinline__ double operator()(const double a, const double b) const { return a < b ? a : b; }
};

// v[i] over the workgroup, in every thread: butterfly over the lanes of each wave, then the tree ((w0 w1)(w2 w3))((w4 w5)(w6 w7)) over
// the waves' results in LDS.  scratch: kWaves * N doubles.  Two barriers.
template <int N, class Op>
__device__ __forceinline__ void block_reduce(double (&v)[N], double* scratch, const Op op) {
  const int lane = threadIdx.x & (PRS_WAVE - 1);
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      v[i] = op(v[i], __shfl_xor(v[i], m, PRS_WAVE));
    }
  }
  __syncthreads();  // the scratch's last readers are done
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      scratch[wave * N + i] = v[i];
    }
  }
  __syncthreads();
  static_assert(kWaves == 8, "the tree below is written for eight waves");
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double a = op(op(scratch[0 * N + i], scratch[1 * N + i]), op(scratch[2 * N + i], scratch[3 * N + i]));
    const double b = op(op(scratch[4 * N + i], scratch[5 * N + i]), op(scratch[6 * N + i], scratch[7 * N + i]));
    v[i] = op(a, b);
  }
}

constexpr int kScratchDoubles = kWaves * 24;  // the KITTI block's sums: 8 lengths x 3 per wave

// the translations of row k of both clouds, from the LDS stage or from global memory
struct Clouds {
  const float* est;
  const float* gt;
  const float* sp;  // nullptr: not staged
  const float* sg;
  const uint8_t* valid;
  __device__ __forceinline__ bool ok(const int k) const { return !valid || valid[k] != 0; }
  __device__ __forceinline__ void p(const int k, double* out) const {
    if (sp) {
      out[0] = sp[3 * k + 0], out[1] = sp[3 * k + 1], out[2] = sp[3 * k + 2];
    } else {
      const float* m = est + (size_t) k * 16;
      out[0] = m[3], out[1] = m[7], out[2] = m[11];
    }
  }
  __device__ __forceinline__ void g(const int k, double* out) const {
    if (sg) {
      out[0] = sg[3 * k + 0], out[1] = sg[3 * k + 1], out[2] = sg[3 * k + 2];
    } else {
      const float* m = gt + (size_t) k * 16;
      out[0] = m[3], out[1] = m[7], out[2] = m[11];
    }
  }
  // |t(G_k) - t(G_{k-1})|, k >= 1
  __device__ __forceinline__ double step(const int k) const {
    double a[3], b[3];
    g(k - 1, a);
    g(k, b);
    const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    return norm3(d);
  }
};

__device__ __forceinline__ void write_identity(double* S) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    S[i] = (i % 5 == 0) ? 1.0 : 0.0;
  }
}

// every field but status, n_valid and S
__device__ __forceinline__ void zero_metrics(prs_trajectory_result* r) {
  r->n_rpe = 0, r->n_kitti = 0;
  r->path_length = 0.0;
  r->ate_rmse = r->ate_mean = r->ate_max = 0.0;
  r->rpe_t_rmse = r->rpe_t_mean = r->rpe_t_max = 0.0;
  r->rpe_r_rmse = r->rpe_r_mean = r->rpe_r_max = 0.0;
  for (int i = 0; i < 3; ++i) {
    r->axis_t_mean[i] = r->axis_t_std[i] = r->axis_r_mean[i] = r->axis_r_std[i] = 0.0;
  }
  r->kitti_t = r->kitti_r = 0.0;
  for (int i = 0; i < 8; ++i) {
    r->kitti_t_len[i] = r->kitti_r_len[i] = 0.0;
    r->kitti_n_len[i] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void trajectory_eval_kernel(const TrajArgs a) {
  extern __shared__ __attribute__((aligned(16))) float stage[];  // both clouds' translations, then the distances (doubles)
  __shared__ double scratch[kScratchDoubles];
  __shared__ double sS[12];  // the alignment: R (9), t (3)

  const prs_trajectory_batch& t = a.t;
  const int b      = blockIdx.x;
  const int tid    = threadIdx.x;
  const int lane   = tid & (PRS_WAVE - 1);
  const int wave   = tid >> 6;
  const int stride = t.frame_stride;
  const size_t row0 = (size_t) b * stride;
  prs_trajectory_result* res = t.result + b;
  float* ferr = t.frame_error ? t.frame_error + row0 : nullptr;

  int status = PRS_OK;
  int n      = t.n_frames[b];
  if (n < 0) {
    status = PRS_ERR_RANGE;
    n      = 0;
  }
  n = n < stride ? n : stride;

  Clouds c;
  c.est   = t.estimate + row0 * 16;
  c.gt    = t.ground_truth + row0 * 16;
  c.valid = t.valid ? t.valid + row0 : nullptr;
  c.sp    = a.stage_clouds ? stage : nullptr;
  c.sg    = a.stage_clouds ? stage + 3 * (size_t) stride : nullptr;

  // ---- stage the translations; count the valid rows and find the first
  double cnt = 0.0, first = (double) n;
  for (int k = tid; k < n; k += kThreads) {
    if (a.stage_clouds) {
      const float* pe = c.est + (size_t) k * 16;
      const float* pg = c.gt + (size_t) k * 16;
      stage[3 * k + 0] = pe[3], stage[3 * k + 1] = pe[7], stage[3 * k + 2] = pe[11];
      float* sg = stage + 3 * (size_t) stride;
      sg[3 * k + 0] = pg[3], sg[3 * k + 1] = pg[7], sg[3 * k + 2] = pg[11];
    }
    if (c.ok(k)) {
      cnt += 1.0;
      first = first < (double) k ? first : (double) k;
    }
  }
  {
    double v[1] = {cnt};
    block_reduce(v, scratch, SumOp());  // (its barriers also publish the stage)
    cnt = v[0];
    v[0] = first;
    block_reduce(v, scratch, MinOp());
    first = v[0];
  }
  const int n_valid = (int) cnt;
  const int f       = (int) first;

  if (status == PRS_OK && ((a.p.align == PRS_TRAJ_ALIGN_RIGID && n_valid < 3) || (a.p.align == PRS_TRAJ_ALIGN_FIRST && n_valid < 1))) {
    status = PRS_ERR_RANGE;
  }
  if (status != PRS_OK) {
    if (tid == 0) {
      res->status  = status;
      res->n_valid = n_valid;
      write_identity(res->S);
      zero_metrics(res);
    }
    if (ferr) {
      for (int k = tid; k < stride; k += kThreads) {
        ferr[k] = -1.0f;
      }
    }
    return;
  }

  // ---- centroids of the valid rows and the ground truth's path length (steps between adjacent valid rows)
  double s7[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = tid; k < n; k += kThreads) {
    if (c.ok(k)) {
      double p[3], g[3];
      c.p(k, p);
      c.g(k, g);
      s7[0] += p[0], s7[1] += p[1], s7[2] += p[2];
      s7[3] += g[0], s7[4] += g[1], s7[5] += g[2];
      if (k > 0 && c.ok(k - 1)) {
        s7[6] += c.step(k);
      }
    }
  }
  block_reduce(s7, scratch, SumOp());
  if (tid == 0) {
    res->status      = PRS_OK;
    res->n_valid     = n_valid;
    res->path_length = s7[6];
  }

  // ---- the alignment S
  if (a.p.align == PRS_TRAJ_ALIGN_RIGID) {
    const double inv_n = 1.0 / (double) n_valid;
    const double cp[3] = {s7[0] * inv_n, s7[1] * inv_n, s7[2] * inv_n};
    const double cg[3] = {s7[3] * inv_n, s7[4] * inv_n, s7[5] * inv_n};
    double M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < n; k += kThreads) {
      if (c.ok(k)) {
        double p[3], g[3];
        c.p(k, p);
        c.g(k, g);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          p[i] -= cp[i];
          g[i] -= cg[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            M[3 * i + j] += p[i] * g[j];
          }
        }
      }
    }
    block_reduce(M, scratch, SumOp());
    if (tid == 0) {
      double R[9];
      horn_rotation(M, R);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        sS[i] = R[i];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        sS[9 + i] = cg[i] - ((R[3 * i + 0] * cp[0] + R[3 * i + 1] * cp[1]) + R[3 * i + 2] * cp[2]);
      }
    }
  } else if (tid == 0) {
    if (a.p.align == PRS_TRAJ_ALIGN_FIRST) {
      Pose G, P, S;
      pose_load(c.gt + (size_t) f * 16, G);
      pose_load(c.est + (size_t) f * 16, P);
      pose_mul_inv(G, P, S);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        sS[i] = S.r[i];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        sS[9 + i] = S.t[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        sS[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      res->S[4 * i + 0] = sS[3 * i + 0];
      res->S[4 * i + 1] = sS[3 * i + 1];
      res->S[4 * i + 2] = sS[3 * i + 2];
      res->S[4 * i + 3] = sS[9 + i];
    }
    res->S[12] = 0.0, res->S[13] = 0.0, res->S[14] = 0.0, res->S[15] = 1.0;
  }

  // ---- ATE
  const double inv_valid = n_valid > 0 ? 1.0 / (double) n_valid : 0.0;
  double ate[2] = {0.0, 0.0};
  double ate_max[1] = {0.0};
  double S[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    S[i] = sS[i];
  }
  for (int k = tid; k < stride; k += kThreads) {
    float fe = -1.0f;
    if (k < n && c.ok(k)) {
      double p[3], g[3], d[3];
      c.p(k, p);
      c.g(k, g);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        d[i] = g[i] - (((S[3 * i + 0] * p[0] + S[3 * i + 1] * p[1]) + S[3 * i + 2] * p[2]) + S[9 + i]);
      }
      const double e = norm3(d);
      ate[0] += e * e;
      ate[1] += e;
      ate_max[0] = e > ate_max[0] ? e : ate_max[0];
      fe = (float) e;
    }
    if (ferr) {
      ferr[k] = fe;
    }
  }
  block_reduce(ate, scratch, SumOp());
  block_reduce(ate_max, scratch, MaxOp());
  if (tid == 0) {
    res->ate_rmse = sqrt(ate[0] * inv_valid);
    res->ate_mean = ate[1] * inv_valid;
    res->ate_max  = ate_max[0];
  }

  // ---- RPE and its per-axis block
  double rpe[4]     = {0.0, 0.0, 0.0, 0.0};  // sum t^2, t, theta^2, theta
  double rpe_max[2] = {0.0, 0.0};
  AxisStats ax;
  axis_init(ax);
  const int delta = a.p.rpe_delta;
  const int pairs = delta < n ? n - delta : 0;  // rows k with k + delta < n
  for (int k = tid; k < pairs; k += kThreads) {
    if (c.ok(k) && c.ok(k + delta)) {
      Pose E;
      pair_error(c.est + (size_t) k * 16, c.est + (size_t) (k + delta) * 16, c.gt + (size_t) k * 16, c.gt + (size_t) (k + delta) * 16, E);
      double rv[3];
      const double th = rotation_error(E.r, rv);
      const double te = norm3(E.t);
      rpe[0] += te * te;
      rpe[1] += te;
      rpe[2] += th * th;
      rpe[3] += th;
      rpe_max[0] = te > rpe_max[0] ? te : rpe_max[0];
      rpe_max[1] = th > rpe_max[1] ? th : rpe_max[1];
      const double x[6] = {fabs(E.t[0]), fabs(E.t[1]), fabs(E.t[2]), fabs(rv[0]) * kRadToDeg, fabs(rv[1]) * kRadToDeg, fabs(rv[2]) * kRadToDeg};
      axis_add(ax, x);
    }
  }
  block_reduce(rpe, scratch, SumOp());
  block_reduce(rpe_max, scratch, MaxOp());
  // the axis statistics: lane l takes lane l + m's for m = 32 .. 1, lane 0 of each wave leaves the wave's in LDS, and the waves' are
  // merged there in the tree's order: 1 into 0, 3 into 2, 5 into 4, 7 into 6; 2 into 0, 6 into 4; 4 into 0
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double on = __shfl_down(ax.n, m, PRS_WAVE);
    double om[6], o2[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      om[i] = __shfl_down(ax.mean[i], m, PRS_WAVE);
      o2[i] = __shfl_down(ax.m2[i], m, PRS_WAVE);
    }
    if (lane < m) {
      axis_merge(ax, on, om, o2);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int m = 1; m < kWaves; m <<= 1) {
    if (lane == 0 && (wave & (2 * m - 1)) == m) {
      scratch[wave * 13] = ax.n;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        scratch[wave * 13 + 1 + i] = ax.mean[i];
        scratch[wave * 13 + 7 + i] = ax.m2[i];
      }
    }
    __syncthreads();
    if (lane == 0 && (wave & (2 * m - 1)) == 0) {
      const double* o = scratch + (wave + m) * 13;
      axis_merge(ax, o[0], o + 1, o + 7);
    }
  }
  if (tid == 0) {
    const int n_rpe = (int) ax.n;
    const double ir = n_rpe > 0 ? 1.0 / (double) n_rpe : 0.0;
    res->n_rpe      = n_rpe;
    res->rpe_t_rmse = sqrt(rpe[0] * ir);
    res->rpe_t_mean = rpe[1] * ir;
    res->rpe_t_max  = rpe_max[0];
    res->rpe_r_rmse = sqrt(rpe[2] * ir);
    res->rpe_r_mean = rpe[3] * ir;
    res->rpe_r_max  = rpe_max[1];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      res->axis_t_mean[i] = ax.mean[i];
      res->axis_t_std[i]  = sqrt(ax.m2[i] * ir);
      res->axis_r_mean[i] = ax.mean[3 + i];
      res->axis_r_std[i]  = sqrt(ax.m2[3 + i] * ir);
    }
  }

  // ---- the KITTI devkit's subsequence errors
  const bool kitti = a.p.kitti_step > 0 && n > 0 && n_valid == n;
  double kt = 0.0, kr = 0.0, kn = 0.0;  // thread 0's totals, by length in order
  if (kitti) {
    double* dist = t.workspace + row0;
    // the copy the subsequence search reads: in LDS behind the clouds where it fits (24 * stride is a multiple of 8)
    double* sdist = a.stage_dist ? reinterpret_cast<double*>(stage + 6 * (size_t) stride) : dist;
    // dist[k] = sum of the steps up to row k: every thread sums a run of consecutive rows, the runs' totals are scanned over the
    // workgroup (shuffles in the wave, the waves' totals in sequence), then every thread walks its run again
    const int run = (n + kThreads - 1) / kThreads;
    const int lo  = (long long) tid * run < n ? tid * run : n;
    const int hi  = run < n - lo ? lo + run : n;
    double local = 0.0;
    for (int k = lo > 1 ? lo : 1; k < hi; ++k) {
      local += c.step(k);
    }
    double incl = local;
#pragma unroll
    for (int d = 1; d < PRS_WAVE; d <<= 1) {
      const double o = __shfl_up(incl, d, PRS_WAVE);
      if (lane >= d) {
        incl += o;
      }
    }
    __syncthreads();
    if (lane == PRS_WAVE - 1) {
      scratch[wave] = incl;
    }
    __syncthreads();
    double base = 0.0;
    for (int w = 0; w < wave; ++w) {
      base += scratch[w];
    }
    double running = base + (incl - local);
    for (int k = lo; k < hi; ++k) {
      if (k > 0) {
        running += c.step(k);
      }
      dist[k] = running;
      if (a.stage_dist) {
        sdist[k] = running;
      }
    }
    __syncthreads();  // the distances are read across the workgroup below

    // per length: every thread takes subsequence starts kThreads apart; the sums are reduced over the wave by shuffles and left in
    // LDS by wave and length, with no barrier between the lengths; thread 0 adds the waves' in the tree's order at the end
    const long long kstep = a.p.kitti_step;
    for (int li = 0; li < a.p.n_lengths; ++li) {
      const double L = (double) a.p.lengths[li];
      double s3[3] = {0.0, 0.0, 0.0};  // sum t_err, sum r_err, subsequences
      for (long long fi = tid; fi * kstep < (long long) n; fi += kThreads) {
        const int first_row = (int) (fi * kstep);
        const double limit  = sdist[first_row] + L;
        // the first index with dist > limit (the devkit's scan; dist does not decrease)
        int lo_i = first_row, hi_i = n;  // dist[lo_i] <= limit; hi_i = n or dist[hi_i] > limit
        while (hi_i - lo_i > 1) {
          const int mid = lo_i + ((hi_i - lo_i) >> 1);
          if (sdist[mid] > limit) {
            hi_i = mid;
          } else {
            lo_i = mid;
          }
        }
        if (hi_i < n) {
          Pose E;
          pair_error(c.est + (size_t) first_row * 16, c.est + (size_t) hi_i * 16, c.gt + (size_t) first_row * 16, c.gt + (size_t) hi_i * 16, E);
          double rv[3];
          const double th = rotation_error(E.r, rv);
          s3[0] += norm3(E.t) / L;
          s3[1] += th / L;
          s3[2] += 1.0;
        }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        s3[i] = wave_sum(s3[i]);
        if (lane == 0) {
          scratch[(wave * 8 + li) * 3 + i] = s3[i];
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      for (int li = 0; li < a.p.n_lengths; ++li) {
        double s3[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double* w = scratch + li * 3 + i;  // wave v's partial at w[24 v]
          s3[i] = ((w[0] + w[24]) + (w[48] + w[72])) + ((w[96] + w[120]) + (w[144] + w[168]));
        }
        const double il = s3[2] > 0.0 ? 1.0 / s3[2] : 0.0;
        res->kitti_t_len[li] = s3[0] * il;
        res->kitti_r_len[li] = s3[1] * il;
        res->kitti_n_len[li] = (int) s3[2];
        kt += s3[0];
        kr += s3[1];
        kn += s3[2];
      }
    }
  }
  if (tid == 0) {
    const double ik = kn > 0.0 ? 1.0 / kn : 0.0;
    res->n_kitti = (int) kn;
    res->kitti_t = kt * ik;
    res->kitti_r = kr * ik;
    for (int li = kitti ? a.p.n_lengths : 0; li < 8; ++li) {
      res->kitti_t_len[li] = 0.0;
      res->kitti_r_len[li] = 0.0;
      res->kitti_n_len[li] = 0;
    }
  }
}

}  // namespace

int trajectory_eval_launch(prs_context* ctx, const prs_trajectory_params* params, const prs_trajectory_batch* batch) {
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_trajectory_eval_batch: params or batch not set");
  }
  const prs_trajectory_params& p = *params;
  const prs_trajectory_batch& t  = *batch;
  if (!t.estimate || !t.ground_truth || !t.n_frames || !t.result) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_trajectory_eval_batch: estimate, ground_truth, n_frames or result not set");
  }
  if (p.kitti_step > 0 && !t.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_trajectory_eval_batch: kitti_step > 0 needs the workspace");
  }
  if (t.batch < 1 || t.frame_stride < 1) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_trajectory_eval_batch: batch or frame_stride below 1");
  }
  if (p.rpe_delta < 1 || p.kitti_step < 0 || p.n_lengths < 0 || p.n_lengths > 8) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_trajectory_eval_batch: rpe_delta < 1, kitti_step < 0 or n_lengths outside 0..8");
  }
  for (int i = 0; i < p.n_lengths; ++i) {
    if (!std::isfinite(p.lengths[i]) || !(p.lengths[i] > 0.0f) || (i > 0 && !(p.lengths[i] > p.lengths[i - 1]))) {
      return ctx_fail(ctx, PRS_ERR_RANGE, "prs_trajectory_eval_batch: a length that is not finite, not positive or not ascending");
    }
  }
  if (p.align != PRS_TRAJ_ALIGN_NONE && p.align != PRS_TRAJ_ALIGN_FIRST && p.align != PRS_TRAJ_ALIGN_RIGID) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_trajectory_eval_batch: unknown align");
  }
  if ((reinterpret_cast<uintptr_t>(t.estimate) & 15) || (reinterpret_cast<uintptr_t>(t.ground_truth) & 15)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_trajectory_eval_batch: estimate or ground_truth not 16-byte aligned");
  }
  if ((reinterpret_cast<uintptr_t>(t.result) & 7) || (reinterpret_cast<uintptr_t>(t.workspace) & 7)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_trajectory_eval_batch: result or workspace not 8-byte aligned");
  }
  TrajArgs a;
  a.p = p;
  a.t = t;
  const size_t clouds = (size_t) t.frame_stride * 24, dist = (size_t) t.frame_stride * 8;
  a.stage_clouds      = clouds <= kStageLimit;
  a.stage_dist        = p.kitti_step > 0 && clouds + dist <= kStageLimit;
  const size_t lds    = a.stage_clouds ? clouds + (a.stage_dist ? dist : 0) : 0;
  Launches on(ctx, "prs_trajectory_eval_batch", ctx_stream(ctx));
  const Grid grid = on.grid(t.batch, kThreads);
  PRS_TRY(on.check());
  const hipError_t e = allow_lds(trajectory_eval_kernel, lds);
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_trajectory_eval_batch: LDS request");
  }
  on.launch(trajectory_eval_kernel, grid, lds, a);
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_trajectory_struct_sizes(uint64_t* sizes3) {
  sizes3[0] = sizeof(prs_trajectory_params);
  sizes3[1] = sizeof(prs_trajectory_result);
  sizes3[2] = sizeof(prs_trajectory_batch);
}

int prs_trajectory_eval_batch(prs_context* ctx, const prs_trajectory_params* params, const prs_trajectory_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return trajectory_eval_launch(ctx, params, batch);
}

}  // extern "C"
