// pose_graph.hip -- the global solver on the device: Gauss-Newton over SE(3) pose graphs with loop closures, the consumer of the
// loop detector's accepted closures (include/proslam_hip.h, prs_pose_graph_optimize_batch).  Stands in for the `global_solver` every
// shipped .conf wires into MultiGraphSLAM3D (kitti.conf:895-936 -> Solver :420-444, IterationAlgorithmGN :826-832,
// SimpleTerminationCriteria :884-889, SparseBlockLinearSolverCholeskyCholmod); the arithmetic lives in srrg2_solver, not in the tree:
// BUILD-DEFINED, stated in the header.
//
// One launch per batch:
//   pose_graph_kernel   one workgroup per graph, and a workgroup is ONE wave: the factorisation is a dependency chain of about
//                       6 * (sum of the block rows' scalar widths) steps, each a handful of multiply-subtracts per lane, so a second
//                       wave would buy a hardware barrier per step and nothing else.  With 64 threads every __syncthreads() below
//                       is a wait on the wave's own memory counters (the compiler drops the barrier instruction), i.e. there is no
//                       workgroup barrier inside a row or anywhere else; B graphs fill the device, not the threads of one graph.
//   Memory              float64 throughout.  LDS (dynamic, sized by node_stride): 1 / d per scalar row and the right-hand side
//                       (b, then y, then dx) at 6 doubles per node each, first() and the envelope's block-row offsets at one int
//                       per node each, and the CURRENT BLOCK ROW of the factor (six scalar rows), at most what is left of 160 KiB.
//                       Global (the caller's workspace): the row envelope of H / the factor, 36 doubles per block.  A block row
//                       wider than the LDS buffer is factorised in place in the workspace by the same code (same bits, slower).
//                       At node_stride 1024 the fixed part is 105 KiB and the row buffer 54 KiB (194 blocks); that is the limit
//                       the call accepts (kMaxNodeStride).
//   Sums                no atomics on floating-point data.  Edges are linearised one after the other, ascending, the 36 + 36 + 36
//                       + 6 + 6 sums of an edge spread over the lanes; every element of the factor is one chain in ascending column
//                       (right-looking inside the block row: step m applies subtraction m to every element of the six rows that
//                       has one, which is the order of the left-looking definition).
//   pose_graph_lm_kernel  the Levenberg-Marquardt form (prs_pose_graph_optimize_lm_batch; IterationAlgorithmLM of icl.conf:665-685 and
//                       tum.conf:174-194, BUILD-DEFINED like the rest: Nielsen's gain-ratio schedule, stated in the header).  The same
//                       mapping and the same device functions: a round is a Gauss-Newton iteration inside a loop of trials that
//                       damp with lambda, solve, try the step from X0 and accept or reject it by the gain ratio.  d = diag(H), g = -b
//                       and X0 of the round (28 doubles per node) live in the workspace behind the envelope -- LDS is full at
//                       node_stride 1024 -- and a trial after a rejection linearises again at X0 instead of keeping a second envelope.
//   append_closures_kernel  one wave per graph scans the detector's slots in ascending order and appends the accepted ones by a
//                       prefix count (ballot + popcount): the order is the slot order, whatever the hardware does.
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kThreads        = 64;
constexpr int kMaxNodeStride  = 1024;
constexpr size_t kLdsBytes    = 160 * 1024;
constexpr int kMaxIterations  = PRS_POSE_GRAPH_MAX_ITERATIONS;

struct PoseGraphArgs {
  prs_pose_graphs g;
  prs_pose_graph_params p;
  long long capacity_blocks;  // envelope blocks of workspace per graph
  int rb_cols;                // scalar columns of the LDS block-row buffer
};

// what one graph's workgroup keeps in LDS
struct Lds {
  double* invd;   // [6 n] 1 / d_r
  double* y;      // [6 n] b, then y, then z / dx
  double* row;    // [6][rb_cols] the current block row
  double* edge;   // [4 * 36 + 6] Jf, Jt, Omega Jf, Omega Jt, Omega e of the current edge
  int* first;     // [n]
  int* off;       // [n + 1] exclusive prefix of the block rows' widths, in blocks
};

constexpr int kEdgeScratch = 4 * 36 + 6;

__host__ __device__ inline size_t lds_fixed_bytes(const int node_stride) {
  return (size_t) node_stride * (12 * sizeof(double) + 2 * sizeof(int)) + kEdgeScratch * sizeof(double) + 2 * sizeof(int) + 16;
}

struct Graph {
  int n, n_edges;
  double* X;
  const uint8_t* fixed;
  const int32_t *from, *to;
  const float *Z, *omega;
  double* env;
};

// the first scalar of block row j's storage, and the address of block (j, lo)'s row a
__device__ __forceinline__ size_t row_base(const Lds& s, const int j) {
  return (size_t) 36 * (size_t) s.off[j];
}
__device__ __forceinline__ int row_width(const Lds& s, const int j) {
  return 6 * (j - s.first[j] + 1);
}

// Linearises edge k at the current poses: chi_k (returned, uniform); with kSystem the edge's terms go to the envelope and to b.
// All lanes evaluate the error and the Jacobians (uniform), lane 0 parks the Jacobians in LDS, lanes 0-35 own one entry (a, b) of
// Omega J and then of the three blocks, lanes 36-41 one entry of Omega e and of b_from, lanes 42-47 one of b_to.
template <bool kSystem>
__device__ __forceinline__ double linearize_edge(const Graph& G, const Lds& s, const int k, const int lane) {
  const int f = G.from[k], t = G.to[k];
  double Z[12], Xf[12], Xt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    Z[i]  = (double) G.Z[16 * (size_t) k + i];
    Xf[i] = G.X[16 * (size_t) f + i];
    Xt[i] = G.X[16 * (size_t) t + i];
  }
  double Zi[12], Xfi[12], A[12], E[12], e[6];
  se3_inverse<false>(Z, Zi);
  se3_inverse<false>(Xf, Xfi);
  se3_mul<false>(Xfi, Xt, A);
  se3_mul<false>(Zi, A, E);
  const double w = t2tnq(E, e);
  double* sJf  = s.edge;
  double* sJt  = s.edge + 36;
  double* sOJf = s.edge + 72;
  double* sOJt = s.edge + 108;
  double* sOe  = s.edge + 144;
  if (kSystem && lane == 0) {
    const double v0 = e[3], v1 = e[4], v2 = e[5];
    const double a0 = A[3], a1 = A[7], a2 = A[11];
#pragma unroll
    for (int i = 0; i < 36; ++i) {
      sJf[i] = 0.0;
      sJt[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        sJt[6 * i + j] = E[4 * i + j];
        sJf[6 * i + j] = -Z[4 * j + i];
      }
      sJf[6 * i + 3] = 2.0 * (Z[4 + i] * a2 - Z[8 + i] * a1);
      sJf[6 * i + 4] = 2.0 * (Z[8 + i] * a0 - Z[i] * a2);
      sJf[6 * i + 5] = 2.0 * (Z[i] * a1 - Z[4 + i] * a0);
    }
    sJt[21] = w, sJt[22] = -v2, sJt[23] = v1;
    sJt[27] = v2, sJt[28] = w, sJt[29] = -v0;
    sJt[33] = -v1, sJt[34] = v0, sJt[35] = w;
    const double M[3][3] = {{w, v2, -v1}, {-v2, w, v0}, {v1, -v0, w}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        sJf[6 * (3 + i) + 3 + j] = -((M[i][0] * Z[4 * j] + M[i][1] * Z[4 * j + 1]) + M[i][2] * Z[4 * j + 2]);
      }
    }
  }
  __syncthreads();
  // Omega e (every lane: chi is uniform) and Omega J
  double Oe[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
      const double o = G.omega ? (double) G.omega[36 * (size_t) k + 6 * r + l] : (r == l ? 1.0 : 0.0);
      acc = l == 0 ? o * e[l] : acc + o * e[l];
    }
    Oe[r] = acc;
  }
  double chi = e[0] * Oe[0];
#pragma unroll
  for (int r = 1; r < 6; ++r) {
    chi = chi + e[r] * Oe[r];
  }
  if (!kSystem) {
    return chi;
  }
  const int a = lane / 6, b = lane - 6 * a;  // lanes 0-35: entry (a, b)
  if (lane < 36) {
    double accf = 0.0, acct = 0.0;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
      const double o = G.omega ? (double) G.omega[36 * (size_t) k + 6 * a + l] : (a == l ? 1.0 : 0.0);
      accf = l == 0 ? o * sJf[6 * l + b] : accf + o * sJf[6 * l + b];
      acct = l == 0 ? o * sJt[6 * l + b] : acct + o * sJt[6 * l + b];
    }
    sOJf[lane] = accf;
    sOJt[lane] = acct;
  } else if (lane < 42) {
    // (Oe is in registers; park it for the b lanes, whose row index is not a compile-time constant)
    double v = Oe[0];
#pragma unroll
    for (int r = 1; r < 6; ++r) {
      v = lane - 36 == r ? Oe[r] : v;
    }
    sOe[lane - 36] = v;
  }
  __syncthreads();
  const bool ff = G.fixed[f] != 0, ft = G.fixed[t] != 0;
  if (lane < 36) {
    double hff = 0.0, htt = 0.0, htf = 0.0;
    const bool up = t > f;  // block (t, f) as it is; from > to: block (f, t), transposed
    const int x = up ? a : b, yy = up ? b : a;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double pf = sJf[6 * r + a] * sOJf[6 * r + b];
      const double pt = sJt[6 * r + a] * sOJt[6 * r + b];
      const double pc = sJt[6 * r + x] * sOJf[6 * r + yy];
      hff = r == 0 ? pf : hff + pf;
      htt = r == 0 ? pt : htt + pt;
      htf = r == 0 ? pc : htf + pc;
    }
    if (!ff) {
      double* p = G.env + row_base(s, f) + (size_t) a * row_width(s, f) + 6 * (f - s.first[f]) + b;
      *p = *p + hff;
    }
    if (!ft) {
      double* p = G.env + row_base(s, t) + (size_t) a * row_width(s, t) + 6 * (t - s.first[t]) + b;
      *p = *p + htt;
    }
    if (!ff && !ft) {
      const int hi = up ? t : f, lo = up ? f : t;
      double* p = G.env + row_base(s, hi) + (size_t) a * row_width(s, hi) + 6 * (lo - s.first[hi]) + b;
      *p = *p + htf;
    }
  } else if (lane < 48) {
    const bool to_side = lane >= 42;
    const int c        = lane - (to_side ? 42 : 36);
    const double* J    = to_side ? sJt : sJf;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double p = J[6 * r + c] * sOe[r];
      acc = r == 0 ? p : acc + p;
    }
    const int node = to_side ? t : f;
    if (!(to_side ? ft : ff)) {
      s.y[6 * node + c] = s.y[6 * node + c] + acc;
    }
  }
  __syncthreads();
  return chi;
}

template <bool kSystem>
__device__ __forceinline__ double linearize(const Graph& G, const Lds& s, const int lane) {
  double chi = 0.0;
  for (int k = 0; k < G.n_edges; ++k) {
    chi = chi + linearize_edge<kSystem>(G, s, k, lane);
  }
  return chi;
}

// One block row of the factorisation, forward substitution included.  `row` holds the six scalar rows (width W each, first column
// c0), in LDS or in the envelope itself.  Returns false at a pivot that is not positive and finite.
__device__ __forceinline__ bool factor_block_row(const Graph& G, const Lds& s, double* row, const int j, const int lane) {
  const int c0 = 6 * s.first[j], d0 = 6 * j, W = d0 + 6 - c0;
  for (int m = c0; m < d0; ++m) {
    const double inv = s.invd[m], ym = s.y[m];
    double l[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      l[a] = row[a * W + (m - c0)] * inv;
    }
    for (int c = m + 1 + lane; c < d0; c += kThreads) {
      const int jc = c / 6, cc0 = 6 * s.first[jc];
      if (cc0 <= m) {
        const double u = G.env[row_base(s, jc) + (size_t) (c - 6 * jc) * (6 * jc + 6 - cc0) + (m - cc0)];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          row[a * W + (c - c0)] = row[a * W + (c - c0)] - l[a] * u;
        }
      }
    }
    if (lane < 36) {
      const int a = lane / 6, a2 = lane - 6 * a;
      if (a2 <= a) {
        double la = l[0];
#pragma unroll
        for (int q = 1; q < 6; ++q) {
          la = a == q ? l[q] : la;
        }
        row[a * W + (d0 + a2 - c0)] = row[a * W + (d0 + a2 - c0)] - la * row[a2 * W + (m - c0)];
      }
    } else if (lane < 42) {
      const int a = lane - 36;
      double la = l[0];
#pragma unroll
      for (int q = 1; q < 6; ++q) {
        la = a == q ? l[q] : la;
      }
      s.y[d0 + a] = s.y[d0 + a] - la * ym;
    }
    __syncthreads();
  }
  for (int p = 0; p < 6; ++p) {
    const int m    = d0 + p;
    const double d = row[p * W + (m - c0)];
    if (!(d > 0.0) || !__builtin_isfinite(d)) {
      return false;
    }
    const double inv = 1.0 / d;
    if (lane == 0) {
      s.invd[m] = inv;
    }
    if (lane < 36) {
      const int a = lane / 6, cc = lane - 6 * a;
      if (a > p && cc > p && cc <= a) {
        const double la = row[a * W + (m - c0)] * inv;
        row[a * W + (d0 + cc - c0)] = row[a * W + (d0 + cc - c0)] - la * row[cc * W + (m - c0)];
      }
    } else if (lane < 42) {
      const int a = lane - 36;
      if (a > p) {
        const double la = row[a * W + (m - c0)] * inv;
        s.y[d0 + a]     = s.y[d0 + a] - la * s.y[m];
      }
    }
    __syncthreads();
  }
  return true;
}

__device__ __forceinline__ void carve_lds(Lds& s, unsigned char* smem, const int N, const int rb_cols) {
  s.invd  = reinterpret_cast<double*>(smem);
  s.y     = s.invd + 6 * (size_t) N;
  s.row   = s.y + 6 * (size_t) N;
  s.edge  = s.row + 6 * (size_t) rb_cols;
  s.first = reinterpret_cast<int*>(s.edge + kEdgeScratch);
  s.off   = s.first + N;
}

// graph g of the batch; its envelope starts at `env`
__device__ __forceinline__ void graph_of(Graph& G, const prs_pose_graphs& B, const int g, double* env) {
  const int N = B.node_stride;
  G.n       = B.n_nodes[g];
  G.n_edges = B.n_edges[g];
  G.X       = B.X + (size_t) g * N * 16;
  G.fixed   = B.fixed + (size_t) g * N;
  G.from    = B.from + (size_t) g * B.edge_stride;
  G.to      = B.to + (size_t) g * B.edge_stride;
  G.Z       = B.Z + (size_t) g * B.edge_stride * 16;
  G.omega   = B.omega ? B.omega + (size_t) g * B.edge_stride * 36 : nullptr;
  G.env     = env;
}

// The checks of the header's table, then first() and the envelope's offsets -> the graph's status; `blocks` and `any_free` are set
// where the status is PRS_OK (blocks also where the envelope does not fit).
__device__ __forceinline__ int check_graph(const Graph& G, const Lds& s, const prs_pose_graphs& B, const long long capacity_blocks,
                                           const int lane, int& blocks, bool& any_free) {
  const int n = G.n, E = G.n_edges, N = B.node_stride;
  int status = PRS_OK;
  blocks   = 0;
  any_free = false;
  if (n < 0 || E < 0) {
    status = PRS_ERR_RANGE;
  } else if (n > N || E > B.edge_stride) {
    status = PRS_ERR_CAPACITY;
  } else if (n == 0) {
    status = PRS_WARN_EMPTY_INPUT;
  } else {
    for (int i = lane; i < n; i += kThreads) {
      s.first[i] = i;
    }
    __syncthreads();
    bool bad = false, free_node = false;
    for (int k = lane; k < E; k += kThreads) {
      const int f = G.from[k], t = G.to[k];
      if (f < 0 || f >= n || t < 0 || t >= n || f == t) {
        bad = true;
      } else {
        atomicMin(&s.first[f > t ? f : t], f > t ? t : f);
      }
    }
    for (int i = lane; i < n; i += kThreads) {
      free_node = free_node || G.fixed[i] == 0;
    }
    any_free = __ballot(free_node) != 0ull;
    __syncthreads();
    if (__ballot(bad) != 0ull) {
      status = PRS_ERR_RANGE;
    } else {
      // exclusive prefix of the widths j - first(j) + 1, 64 block rows at a time
      int base = 0;
      for (int j0 = 0; j0 < n; j0 += kThreads) {
        const int j = j0 + lane;
        const int w = j < n ? j - s.first[j] + 1 : 0;
        int incl    = w;
#pragma unroll
        for (int d = 1; d < kThreads; d <<= 1) {
          const int o = __shfl_up(incl, d, kThreads);
          if (lane >= d) {
            incl += o;
          }
        }
        if (j < n) {
          s.off[j] = base + incl - w;
        }
        base += __shfl(incl, kThreads - 1, kThreads);
      }
      if (lane == 0) {
        s.off[n] = base;
      }
      blocks = base;
      __syncthreads();
      if ((long long) blocks > capacity_blocks) {
        status = PRS_ERR_CAPACITY;
      }
    }
  }
  return status;
}

// H <- 0, b <- 0
__device__ __forceinline__ void clear_system(const Graph& G, const Lds& s, const int blocks, const int lane) {
  for (size_t i = lane; i < (size_t) blocks * 36; i += kThreads) {
    G.env[i] = 0.0;
  }
  for (int i = lane; i < 6 * G.n; i += kThreads) {
    s.y[i] = 0.0;
  }
  __syncthreads();
}

// fixed nodes, damping, right-hand side -b
__device__ __forceinline__ void damp_system(const Graph& G, const Lds& s, const double lambda, const int damping_form, const int lane) {
  for (int r = lane; r < 6 * G.n; r += kThreads) {
    const int j = r / 6, a = r - 6 * j;
    double* d = G.env + row_base(s, j) + (size_t) a * row_width(s, j) + 6 * (j - s.first[j]) + a;
    if (G.fixed[j]) {
      *d = 1.0;
    } else if (damping_form == PRS_DAMPING_IDENTITY) {
      *d = *d + lambda;
    } else {
      *d = *d + lambda * *d;
    }
    s.y[r] = -s.y[r];
  }
  __syncthreads();
}

// Factorisation and both substitutions: dx is left in s.y.  Returns false at a pivot that is not positive and finite.
__device__ __forceinline__ bool solve_system(const Graph& G, const Lds& s, const int rb_cols, const int lane) {
  const int n = G.n;
  bool ok = true;
  for (int j = 0; j < n && ok; ++j) {
    const int W    = row_width(s, j);
    double* in_env = G.env + row_base(s, j);
    if (W <= rb_cols) {
      for (int i = lane; i < 6 * W; i += kThreads) {
        s.row[i] = in_env[i];
      }
      __syncthreads();
      ok = factor_block_row(G, s, s.row, j, lane);
      for (int i = lane; i < 6 * W; i += kThreads) {
        in_env[i] = s.row[i];
      }
      __syncthreads();
    } else {
      ok = factor_block_row(G, s, in_env, j, lane);
    }
  }
  if (!ok) {
    return false;
  }
  // z = y / d, then column-oriented back substitution: dx_r = z_r is final, z_m -= l_rm dx_r for every m of row r
  for (int r = lane; r < 6 * n; r += kThreads) {
    s.y[r] = s.y[r] * s.invd[r];
  }
  __syncthreads();
  for (int r = 6 * n - 1; r > 0; --r) {
    const int j = r / 6, a = r - 6 * j, c0 = 6 * s.first[j];
    const double dxr  = s.y[r];
    const double* urow = G.env + row_base(s, j) + (size_t) a * row_width(s, j);
    for (int m = c0 + lane; m < r; m += kThreads) {
      s.y[m] = s.y[m] - (urow[m - c0] * s.invd[m]) * dxr;
    }
    __syncthreads();
  }
  return true;
}

// X <- X0 tnq2t(dx) for every free node (X0 [n][16]; Gauss-Newton passes the poses themselves)
__device__ __forceinline__ void update_poses(const Graph& G, const Lds& s, const double* X0, const int lane) {
  for (int i = lane; i < G.n; i += kThreads) {
    if (G.fixed[i] == 0) {
      double dx[6], D[12], X[12], Xn[12];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        dx[q] = s.y[6 * i + q];
      }
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        X[q] = X0[16 * (size_t) i + q];
      }
      tnq2t<false>(dx, D);
      se3_mul<false>(X, D, Xn);
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        G.X[16 * (size_t) i + q] = Xn[q];
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void pose_graph_kernel(const PoseGraphArgs args) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const prs_pose_graphs& B      = args.g;
  const prs_pose_graph_params& P = args.p;
  const int lane = threadIdx.x, g = blockIdx.x;
  Lds s;
  carve_lds(s, smem, B.node_stride, args.rb_cols);
  Graph G;
  graph_of(G, B, g, reinterpret_cast<double*>(B.workspace) + (size_t) g * (size_t) args.capacity_blocks * 36);
  const int E = G.n_edges;
  prs_pose_graph_result* res = B.result + g;

  int blocks = 0;
  bool any_free = false;
  int status = check_graph(G, s, B, args.capacity_blocks, lane, blocks, any_free);

  int iterations = 0, n_chi = 0;
  double chi_prev = 0.0, chi_final = 0.0;
  if (status == PRS_OK && E > 0 && any_free) {
    const double lambda = (double) P.damping, eps = (double) P.epsilon;
    for (int it = 0; it < P.max_iterations; ++it) {
      clear_system(G, s, blocks, lane);
      const double chi = linearize<true>(G, s, lane);
      if (lane == 0) {
        res->chi[it] = chi;
      }
      n_chi = it + 1;
      if (eps > 0.0 && it > 0 && chi_prev - chi < eps * chi_prev) {
        break;
      }
      chi_prev = chi;
      damp_system(G, s, lambda, P.damping_form, lane);
      if (!solve_system(G, s, args.rb_cols, lane)) {
        status = PRS_ERR_NOT_POSITIVE_DEFINITE;
        break;
      }
      update_poses(G, s, G.X, lane);
      iterations = it + 1;
    }
  }
  if ((status == PRS_OK || status == PRS_ERR_NOT_POSITIVE_DEFINITE) && E > 0) {
    chi_final = linearize<false>(G, s, lane);
  }
  if (lane == 0) {
    for (int i = n_chi; i < kMaxIterations; ++i) {
      res->chi[i] = 0.0;
    }
    res->chi_final       = chi_final;
    res->linearizations  = n_chi;
    res->iterations      = iterations;
    res->envelope_blocks = blocks;
    res->status          = status;
  }
}

// ---- Levenberg-Marquardt: the same linearisation, solve and update inside Nielsen's gain-ratio schedule (the header states it) ----
struct PoseGraphLmArgs {
  prs_pose_graphs g;
  prs_pose_graph_lm_params p;
  prs_pose_graph_lm_result* result;
  long long graph_doubles;    // doubles of workspace per graph: the envelope, then d, g (6 per node each) and X0 (16 per node)
  long long capacity_blocks;  // envelope blocks of workspace per graph
  int rb_cols;
};

constexpr int kLmNodeDoubles = 28;

__global__ __launch_bounds__(kThreads) void pose_graph_lm_kernel(const PoseGraphLmArgs args) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const prs_pose_graphs& B          = args.g;
  const prs_pose_graph_lm_params& P = args.p;
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = B.node_stride;
  Lds s;
  carve_lds(s, smem, N, args.rb_cols);
  Graph G;
  double* ws = reinterpret_cast<double*>(B.workspace) + (size_t) g * (size_t) args.graph_doubles;
  graph_of(G, B, g, ws);
  double* sd  = ws + (size_t) args.capacity_blocks * 36;  // d_r = h_rr, undamped
  double* sg  = sd + 6 * (size_t) N;                       // g_r = -b_r
  double* sX0 = sg + 6 * (size_t) N;                       // the poses the round started from
  const int n = G.n, E = G.n_edges;
  prs_pose_graph_lm_result* res = args.result + g;

  int blocks = 0;
  bool any_free = false;
  int status = check_graph(G, s, B, args.capacity_blocks, lane, blocks, any_free);

  int iterations = 0, n_chi = 0, rounds = 0, trials_total = 0, rejected_npd = 0, stalled = 0;
  double chi_final = 0.0;
  if (status == PRS_OK && E > 0 && any_free) {
    const double eps = (double) P.epsilon, user = (double) P.user_lambda_init, tau = (double) P.tau;
    const double step_high = (double) P.step_high, step_low = (double) P.step_low;
    const bool variable = P.variable_damping != 0;
    const int form      = variable ? PRS_DAMPING_DIAG : PRS_DAMPING_IDENTITY;
    double lambda = 0.0, nu = 2.0, chi_prev = 0.0;
    for (int it = 0; it < P.max_iterations; ++it) {
      clear_system(G, s, blocks, lane);
      const double chi = linearize<true>(G, s, lane);
      if (lane == 0) {
        res->chi[it] = chi;
      }
      n_chi = it + 1;
      if (eps > 0.0 && it > 0 && chi_prev - chi < eps * chi_prev) {
        break;
      }
      chi_prev = chi;
      // d, g and X0 of this round; the largest h_rr of a free node (a maximum has no order)
      double hmax = 0.0;
      bool odd = false;  // a diagonal entry that is not finite
      for (int r = lane; r < 6 * n; r += kThreads) {
        const int j = r / 6, a = r - 6 * j;
        const double h = G.env[row_base(s, j) + (size_t) a * row_width(s, j) + 6 * (j - s.first[j]) + a];
        sd[r] = h;
        sg[r] = -s.y[r];
        if (G.fixed[j] == 0) {
          odd  = odd || !__builtin_isfinite(h);
          hmax = h > hmax ? h : hmax;
        }
      }
      for (int i = lane; i < 16 * n; i += kThreads) {
        sX0[i] = G.X[i];
      }
      if (it == 0) {
        nu = 2.0;
        if (user > 0.0) {
          lambda = user;
        } else {
#pragma unroll
          for (int d = kThreads / 2; d > 0; d >>= 1) {
            const double o = __shfl_xor(hmax, d, kThreads);
            hmax = o > hmax ? o : hmax;
          }
          if (__ballot(odd) != 0ull || !(hmax > 0.0)) {
            status = PRS_ERR_NOT_POSITIVE_DEFINITE;
            break;
          }
          lambda = tau * hmax;
        }
      }
      __syncthreads();
      bool accepted = false, pivot_failed = false;
      double lambda_used = lambda;
      int t = 0;
      for (t = 1; t <= P.lm_iterations_max; ++t) {
        if (t > 1) {
          // the undamped system again: X is X0, so these are the bits of the round's linearisation
          clear_system(G, s, blocks, lane);
          (void) linearize<true>(G, s, lane);
        }
        lambda_used = lambda;
        damp_system(G, s, lambda, form, lane);
        pivot_failed = !solve_system(G, s, args.rb_cols, lane);
        accepted     = false;
        if (pivot_failed) {
          ++rejected_npd;
        } else {
          update_poses(G, s, sX0, lane);
          const double chi_t = linearize<false>(G, s, lane);
          // scale: the terms dx_r ((lambda D_r) dx_r + g_r) side by side (1 / d is no longer needed: they go where it was), then
          // one chain over the rows in ascending order from +0, which every lane runs (uniform)
          for (int r = lane; r < 6 * n; r += kThreads) {
            const double dx = s.y[r], D = variable ? sd[r] : 1.0;
            s.invd[r] = G.fixed[r / 6] ? 0.0 : dx * ((lambda * D) * dx + sg[r]);
          }
          __syncthreads();
          double scale = 0.0;
          for (int r = 0; r < 6 * n; ++r) {
            scale = scale + s.invd[r];
          }
          scale = scale + 1e-3;
          __syncthreads();
          const double rho = (chi - chi_t) / scale;
          accepted         = rho > 0.0 && __builtin_isfinite(chi_t);
          if (accepted) {
            const double u = 2.0 * rho - 1.0;
            const double alpha = 1.0 - (u * u) * u;
            const double m = alpha < step_high ? alpha : step_high;
            lambda = lambda * (m > step_low ? m : step_low);
            nu     = 2.0;
            break;
          }
          for (int i = lane; i < 16 * n; i += kThreads) {
            G.X[i] = sX0[i];
          }
          __syncthreads();
        }
        lambda = lambda * nu;
        nu     = 2.0 * nu;
        if (!__builtin_isfinite(lambda)) {
          break;
        }
      }
      t = t > P.lm_iterations_max ? P.lm_iterations_max : t;
      if (lane == 0) {
        res->lambda[it] = lambda_used;
        res->trials[it] = t;
      }
      trials_total += t;
      rounds = it + 1;
      if (!accepted) {
        if (pivot_failed) {
          status = PRS_ERR_NOT_POSITIVE_DEFINITE;
        } else {
          stalled = 1;
        }
        break;
      }
      iterations = it + 1;
    }
  }
  if ((status == PRS_OK || status == PRS_ERR_NOT_POSITIVE_DEFINITE) && E > 0) {
    chi_final = linearize<false>(G, s, lane);
  }
  if (lane == 0) {
    for (int i = n_chi; i < kMaxIterations; ++i) {
      res->chi[i] = 0.0;
    }
    for (int i = rounds; i < kMaxIterations; ++i) {  // rounds that ran no trial: lambda 0, 0 trials
      res->lambda[i] = 0.0;
      res->trials[i] = 0;
    }
    res->chi_final                      = chi_final;
    res->linearizations                 = n_chi;
    res->iterations                     = iterations;
    res->envelope_blocks                = blocks;
    res->status                         = status;
    res->trials_total                   = trials_total;
    res->rejected_not_positive_definite = rejected_npd;
    res->stalled                        = stalled;
  }
}

struct AppendArgs {
  prs_pose_graphs g;
  prs_pose_graph_closures c;
  float information;
};

__device__ __forceinline__ bool closure_for(const AppendArgs& a, const int slot, const int g, int& from, int& to) {
  const prs_pose_graph_closures& C = a.c;
  const int q = slot / C.max_candidates;
  if (C.result[slot].accepted == 0 || C.graph_of_query[q] != g) {
    return false;
  }
  const int map = C.candidates[slot];
  if (map < 0 || map >= C.n_maps) {
    return false;
  }
  from = C.node_of_query[q];
  to   = C.node_of_map[map];
  return from >= 0 && to >= 0;
}

__global__ __launch_bounds__(kThreads) void append_closures_kernel(const AppendArgs a) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int slots = a.c.n_queries * a.c.max_candidates;
  int total = 0;
  for (int s0 = 0; s0 < slots; s0 += kThreads) {
    int from, to;
    const bool take = s0 + lane < slots && closure_for(a, s0 + lane, g, from, to);
    total += __popcll(__ballot(take));
  }
  const int have = a.g.n_edges[g];
  int status = PRS_OK;
  if (have < 0) {
    status = PRS_ERR_RANGE;
  } else if ((long long) have + total > a.g.edge_stride) {
    status = PRS_ERR_CAPACITY;
  }
  if (status == PRS_OK && total > 0) {
    int at = have;
    for (int s0 = 0; s0 < slots; s0 += kThreads) {
      const int slot = s0 + lane;
      int from = 0, to = 0;
      const bool take = slot < slots && closure_for(a, slot, g, from, to);
      const unsigned long long m = __ballot(take);
      if (take) {
        const size_t k = (size_t) g * a.g.edge_stride + (size_t) (at + __popcll(m & ((1ull << lane) - 1ull)));
        a.g.from[k] = from;
        a.g.to[k]   = to;
        for (int i = 0; i < 16; ++i) {
          a.g.Z[16 * k + i] = a.c.X[16 * (size_t) slot + i];
        }
        if (a.g.omega) {
          for (int i = 0; i < 36; ++i) {
            a.g.omega[36 * k + i] = i % 7 == 0 ? a.information : 0.0f;
          }
        }
      }
      at += __popcll(m);
    }
  }
  if (lane == 0) {
    if (status == PRS_OK) {
      a.g.n_edges[g] = have + total;
    }
    a.c.status[g] = status;
    if (a.c.n_appended) {
      a.c.n_appended[g] = status == PRS_OK ? total : 0;
    }
  }
}

int pose_graph_rb_cols(const int node_stride) {
  const size_t left = kLdsBytes - lds_fixed_bytes(node_stride);
  const size_t cols = left / (6 * sizeof(double));
  const size_t want = 6 * (size_t) node_stride;
  return (int) (cols < want ? cols : want);
}

}  // namespace

namespace {

// the call-level checks both algorithms share (`who`: the entry point, for the message)
int check_batch(prs_context* ctx, const std::string& who, const prs_pose_graphs* graphs, const void* result) {
  if (!graphs->X || !graphs->fixed || !graphs->n_nodes || !graphs->from || !graphs->to || !graphs->Z || !graphs->n_edges ||
      !graphs->workspace || !result) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": input or output buffer not set").c_str());
  }
  if (graphs->node_stride < 1 || graphs->edge_stride < 1) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": stride below 1").c_str());
  }
  if (graphs->node_stride > kMaxNodeStride) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, (who + ": node_stride above 1024 (LDS holds 104 bytes per node)").c_str());
  }
  if ((reinterpret_cast<uintptr_t>(graphs->X) | reinterpret_cast<uintptr_t>(graphs->workspace) | reinterpret_cast<uintptr_t>(result)) & 7) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": X, workspace and result must be 8-byte aligned").c_str());
  }
  return PRS_OK;
}

template <class Kernel, class Args>
int launch_one_wave_per_graph(prs_context* ctx, const std::string& who, Kernel kernel, const Args& a, const int batch, const int node_stride) {
  const size_t lds = lds_fixed_bytes(node_stride) + (size_t) a.rb_cols * 6 * sizeof(double);
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid grid = on.grid(batch, kThreads);
  PRS_TRY(on.check());
  const hipError_t e = allow_lds(kernel, lds);
  if (e == hipSuccess) {
    on.launch(kernel, grid, lds, a);
  }
  return on.finish(e);
}

}  // namespace

int pose_graph_launch(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs) {
  if (!params || !graphs) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_pose_graph_optimize_batch: parameters not set");
  }
  if (params->damping_form != PRS_DAMPING_DIAG && params->damping_form != PRS_DAMPING_IDENTITY) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_pose_graph_optimize_batch: unknown damping form");
  }
  if (!std::isfinite(params->damping) || params->damping < 0.0f || !std::isfinite(params->epsilon) || params->max_iterations < 0 ||
      params->max_iterations > kMaxIterations) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_pose_graph_optimize_batch: damping or epsilon not finite, or max_iterations outside [0, 32]");
  }
  if (graphs->batch <= 0) {
    return PRS_OK;
  }
  PRS_TRY(check_batch(ctx, "prs_pose_graph_optimize_batch", graphs, graphs->result));
  PoseGraphArgs a;
  memset(&a, 0, sizeof(a));
  a.g               = *graphs;
  a.p               = *params;
  a.capacity_blocks = (long long) (graphs->workspace_bytes / (uint64_t) graphs->batch / (36 * sizeof(double)));
  a.rb_cols         = pose_graph_rb_cols(graphs->node_stride);
  return launch_one_wave_per_graph(ctx, "prs_pose_graph_optimize_batch", pose_graph_kernel, a, graphs->batch, graphs->node_stride);
}

int pose_graph_lm_launch(prs_context* ctx, const prs_pose_graph_lm_params* params, const prs_pose_graphs* graphs,
                         prs_pose_graph_lm_result* result) {
  if (!params || !graphs) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_pose_graph_optimize_lm_batch: parameters not set");
  }
  if (!std::isfinite(params->user_lambda_init) || !std::isfinite(params->tau) || params->tau < 0.0f || !std::isfinite(params->step_high) ||
      !std::isfinite(params->step_low) || !std::isfinite(params->epsilon) || params->max_iterations < 0 ||
      params->max_iterations > kMaxIterations) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_pose_graph_optimize_lm_batch: a parameter is not finite, tau is negative, or max_iterations outside [0, 32]");
  }
  if (params->lm_iterations_max < 1 || params->step_low > params->step_high) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_pose_graph_optimize_lm_batch: lm_iterations_max below 1 or step_low above step_high");
  }
  if (graphs->batch <= 0) {
    return PRS_OK;
  }
  PRS_TRY(check_batch(ctx, "prs_pose_graph_optimize_lm_batch", graphs, result));
  PoseGraphLmArgs a;
  memset(&a, 0, sizeof(a));
  a.g             = *graphs;
  a.p             = *params;
  a.result        = result;
  a.graph_doubles = (long long) (graphs->workspace_bytes / (uint64_t) graphs->batch / sizeof(double));
  // what d, g and X0 leave of a graph's share is its envelope (a share below them: no room for any graph, PRS_ERR_CAPACITY each)
  const long long left = a.graph_doubles - (long long) kLmNodeDoubles * graphs->node_stride;
  a.capacity_blocks    = left > 0 ? left / 36 : 0;
  a.rb_cols            = pose_graph_rb_cols(graphs->node_stride);
  return launch_one_wave_per_graph(ctx, "prs_pose_graph_optimize_lm_batch", pose_graph_lm_kernel, a, graphs->batch, graphs->node_stride);
}

int pose_graph_append_launch(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs,
                             const prs_pose_graph_closures* closures) {
  if (!params || !graphs || !closures) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_pose_graph_append_closures: parameters not set");
  }
  if (graphs->batch <= 0) {
    return PRS_OK;
  }
  if (!graphs->from || !graphs->to || !graphs->Z || !graphs->n_edges || !closures->status ||
      (closures->n_queries > 0 && (!closures->candidates || !closures->result || !closures->X || !closures->graph_of_query ||
                                   !closures->node_of_query || !closures->node_of_map))) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_pose_graph_append_closures: input or output buffer not set");
  }
  if (closures->n_queries < 0 || closures->max_candidates < 1 || closures->n_maps < 0 || graphs->edge_stride < 1 ||
      !std::isfinite(params->closure_information)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_pose_graph_append_closures: negative count, max_candidates below 1 or information not finite");
  }
  if (!graphs->omega && params->closure_information != 1.0f) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_pose_graph_append_closures: graphs without omega hold identity information only");
  }
  AppendArgs a;
  memset(&a, 0, sizeof(a));
  a.g           = *graphs;
  a.c           = *closures;
  a.information = params->closure_information;
  return Launches(ctx, "prs_pose_graph_append_closures", ctx_stream(ctx)).one(graphs->batch, kThreads, append_closures_kernel, 0, a);
}

// The host-pointer entry of either algorithm: sizes the envelope, stages, runs `launch(descriptor, device result)`, downloads.
// node_doubles: doubles of workspace per node behind the envelope.
template <class Params, class Result, class Launch>
int optimize_on_host(prs_context* ctx, const char* entry, const Params* params, int32_t n_nodes, double* X16, const uint8_t* fixed,
                     int32_t n_edges, const int32_t* from, const int32_t* to, const float* Z16, const float* omega36, Result* result,
                     const int node_doubles, Launch launch) {
  const std::string who(entry);
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (!params || !result || (n_nodes > 0 && (!X16 || !fixed)) || (n_edges > 0 && (!from || !to || !Z16))) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": input or output buffer not set").c_str());
  }
  if (n_nodes < 0 || n_edges < 0) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": negative size").c_str());
  }
  if (n_nodes > kMaxNodeStride) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, (who + ": more than 1024 nodes").c_str());
  }
  (void) hipSetDevice(ctx->device);
  const size_t nn = (size_t) (n_nodes > 0 ? n_nodes : 1), ne = (size_t) (n_edges > 0 ? n_edges : 1);
  // the envelope of this graph (an endpoint out of range is the kernel's to report: it takes no part here)
  size_t blocks = 0;
  {
    std::vector<int32_t> first(nn);
    for (int32_t i = 0; i < n_nodes; ++i) {
      first[i] = i;
    }
    for (int32_t k = 0; k < n_edges; ++k) {
      const int32_t f = from[k], t = to[k];
      if (f >= 0 && f < n_nodes && t >= 0 && t < n_nodes && f != t) {
        const int32_t hi = f > t ? f : t, lo = f > t ? t : f;
        first[hi] = lo < first[hi] ? lo : first[hi];
      }
    }
    for (int32_t i = 0; i < n_nodes; ++i) {
      blocks += (size_t) (i - first[i] + 1);
    }
  }
  blocks = blocks > 0 ? blocks : 1;
  struct Meta {
    int32_t n_nodes, n_edges;
  };
  // fixed | sizes | from | to | Z | omega (uploaded) | X (both) | result (downloaded) | envelope (device only)
  Staging st(ctx, entry, ARENA_STAGE_POSE_GRAPH);
  auto s_fixed = st.up<uint8_t>(nn);
  auto s_meta  = st.up<Meta>(1);
  auto s_from  = st.up<int32_t>(ne);
  auto s_to    = st.up<int32_t>(ne);
  auto s_Z     = st.up<float>(ne * 16);
  auto s_omega = st.up<float>(omega36 ? ne * 36 : 0);
  auto s_X     = st.both<double>(nn * 16);
  auto s_res   = st.down<Result>(1);
  const size_t ws_doubles = blocks * 36 + (size_t) node_doubles * nn;
  auto s_env   = st.device<double>(ws_doubles);
  PRS_TRY(st.commit());
  if (n_nodes > 0) {
    memcpy(s_fixed.h(), fixed, (size_t) n_nodes);
    memcpy(s_X.h(), X16, (size_t) n_nodes * 16 * sizeof(double));
  }
  s_meta.h()->n_nodes = n_nodes;
  s_meta.h()->n_edges = n_edges;
  if (n_edges > 0) {
    memcpy(s_from.h(), from, (size_t) n_edges * sizeof(int32_t));
    memcpy(s_to.h(), to, (size_t) n_edges * sizeof(int32_t));
    memcpy(s_Z.h(), Z16, (size_t) n_edges * 16 * sizeof(float));
    if (omega36) {
      memcpy(s_omega.h(), omega36, (size_t) n_edges * 36 * sizeof(float));
    }
  }
  PRS_TRY(st.upload());
  prs_pose_graphs b;
  memset(&b, 0, sizeof(b));
  b.batch           = 1;
  b.node_stride     = (int32_t) nn;
  b.edge_stride     = (int32_t) ne;
  b.X               = s_X.d();
  b.fixed           = s_fixed.d();
  b.n_nodes         = &s_meta.d()->n_nodes;
  b.from            = s_from.d();
  b.to              = s_to.d();
  b.Z               = s_Z.d();
  b.omega           = omega36 ? s_omega.d() : nullptr;
  b.n_edges         = &s_meta.d()->n_edges;
  b.workspace       = s_env.d();
  b.workspace_bytes = ws_doubles * sizeof(double);
  PRS_TRY(launch(&b, s_res.d()));
  PRS_TRY(st.download());
  memcpy(result, s_res.h(), sizeof(Result));
  if (n_nodes > 0) {
    memcpy(X16, s_X.h(), (size_t) n_nodes * 16 * sizeof(double));
  }
  if (result->status < 0) {
    return ctx_fail(ctx, result->status, (who + ": the graph was refused or its system is not positive definite").c_str());
  }
  return result->status;
}

}  // namespace prs

using namespace prs;

extern "C" {

uint64_t prs_pose_graph_workspace_bytes(int32_t batch, int32_t node_stride, int64_t envelope_blocks_per_graph) {
  (void) node_stride;  // (the envelope is the only part of a graph's state that does not fit LDS)
  if (batch <= 0 || envelope_blocks_per_graph <= 0) {
    return 0;
  }
  return (uint64_t) batch * (uint64_t) envelope_blocks_per_graph * 36u * sizeof(double);
}

void prs_pose_graph_struct_sizes(uint64_t* sizes4) {
  sizes4[0] = sizeof(prs_pose_graph_params);
  sizes4[1] = sizeof(prs_pose_graph_result);
  sizes4[2] = sizeof(prs_pose_graphs);
  sizes4[3] = sizeof(prs_pose_graph_closures);
}

int prs_pose_graph_optimize_batch(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return pose_graph_launch(ctx, params, graphs);
}

int prs_pose_graph_append_closures(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs,
                                   const prs_pose_graph_closures* closures) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return pose_graph_append_launch(ctx, params, graphs, closures);
}

int prs_pose_graph_optimize(prs_context* ctx, const prs_pose_graph_params* params, int32_t n_nodes, double* X16, const uint8_t* fixed,
                            int32_t n_edges, const int32_t* from, const int32_t* to, const float* Z16, const float* omega36,
                            prs_pose_graph_result* result) {
  return optimize_on_host(ctx, "prs_pose_graph_optimize", params, n_nodes, X16, fixed, n_edges, from, to, Z16, omega36, result, 0,
                          [&](prs_pose_graphs* b, prs_pose_graph_result* d_result) {
                            b->result = d_result;
                            return pose_graph_launch(ctx, params, b);
                          });
}

uint64_t prs_pose_graph_lm_workspace_bytes(int32_t batch, int32_t node_stride, int64_t envelope_blocks_per_graph) {
  if (batch <= 0 || node_stride <= 0 || envelope_blocks_per_graph <= 0) {
    return 0;
  }
  return (uint64_t) batch * ((uint64_t) envelope_blocks_per_graph * 36u + (uint64_t) kLmNodeDoubles * (uint64_t) node_stride) * sizeof(double);
}

void prs_pose_graph_lm_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_pose_graph_lm_params);
  sizes2[1] = sizeof(prs_pose_graph_lm_result);
}

int prs_pose_graph_optimize_lm_batch(prs_context* ctx, const prs_pose_graph_lm_params* params, const prs_pose_graphs* graphs,
                                     prs_pose_graph_lm_result* result) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return pose_graph_lm_launch(ctx, params, graphs, result);
}

int prs_pose_graph_optimize_lm(prs_context* ctx, const prs_pose_graph_lm_params* params, int32_t n_nodes, double* X16,
                               const uint8_t* fixed, int32_t n_edges, const int32_t* from, const int32_t* to, const float* Z16,
                               const float* omega36, prs_pose_graph_lm_result* result) {
  return optimize_on_host(ctx, "prs_pose_graph_optimize_lm", params, n_nodes, X16, fixed, n_edges, from, to, Z16, omega36, result,
                          kLmNodeDoubles, [&](prs_pose_graphs* b, prs_pose_graph_lm_result* d_result) {
                            return pose_graph_lm_launch(ctx, params, b, d_result);
                          });
}

}  // extern "C"
