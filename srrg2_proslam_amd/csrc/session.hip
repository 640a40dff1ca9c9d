// session.hip -- local-map manager on the device: the per-frame step between the aligner and the merger (pose update, trajectory
// log, splitting criterion, growth of the pose graph, hand-over and reset of the finished map, next prediction) and the unrolling
// of the logged trajectories through the graph.  The rule is stated in include/proslam_hip.h (BUILD-DEFINED) and restated in
// tests/session_ref.py; every float expression is an explicit two-operand operation in a fixed order (prs_se3.h).
#include <math.h>
#include <string.h>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_se3.h"

namespace prs {

namespace {

constexpr int kThreads = 256;

struct StepArgs {
  prs_session_batch s;
  float d2;          // local_map_distance^2, formed in float on the host
  float cos_a;       // (float) cos((double) angle); -inf for an angle >= pi
  float info_split;  // makeNewMap(1)
  float info_lost;   // makeNewMap(0.1)
};

// what the first wave loads, what thread 0 decides and the matrices the workgroup stores
struct StepShared {
  float in_pred[16], in_X[16], in_pose[16];
  int in_i[16];  // n_frames, slot, cur_node, n_nodes, n_edges, n_points, n_corr, result.status, result.warnings
  float pose[16], prev[16], pred[16], logged[16];
  double node_X[16];
  int run;        // 0: a counter is out of range, nothing but the status is written
  int write_log;  // the log has room for this frame
  int reason;     // PRS_SESSION_*: the split performed
  int n_points;   // of the map as the frame found it
  int frame_row;  // n_frames[b] as the frame found it
  int node;       // the new node (split)
  int edge;       // the new edge (split)
};

// one workgroup per sequence: the first wave loads, thread 0 does the pose arithmetic and publishes the decision through LDS, the
// workgroup stores the matrices and, on a split (block-uniform), copies the finished map out and clears its measurement counts
__global__ __launch_bounds__(kThreads) void session_step_kernel(const StepArgs a) {
  __shared__ StepShared sh;
  const prs_session_batch& s = a.s;
  const int b   = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < 16) {
    sh.in_pred[tid] = s.prediction[(size_t) b * 16 + tid];
  } else if (tid < 32) {
    sh.in_X[tid - 16] = s.X[(size_t) b * 16 + (tid - 16)];
  } else if (tid < 48) {
    sh.in_pose[tid - 32] = s.pose[(size_t) b * 16 + (tid - 32)];
  } else if (tid < 57) {
    const int32_t* src = tid == 48   ? s.n_frames + b
                         : tid == 49 ? s.slot + b
                         : tid == 50 ? s.cur_node + b
                         : tid == 51 ? s.n_nodes + b
                         : tid == 52 ? s.n_edges + b
                         : tid == 53 ? s.n_points + b
                         : tid == 54 ? s.n_corr + b
                         : tid == 55 ? &s.result[b].status
                                     : &s.result[b].warnings;
    sh.in_i[tid - 48] = *src;
  }
  __syncthreads();
  if (tid == 0) {
    const int k = sh.in_i[0], slot = sh.in_i[1], cur = sh.in_i[2], nn = sh.in_i[3], ne = sh.in_i[4], np = sh.in_i[5];
    int status = PRS_OK, reason = PRS_SESSION_NO_SPLIT, n_query = 0;
    const bool bad = k < 0 || slot < 0 || cur < 0 || nn < 0 || ne < 0 || np < 0 || cur >= nn || nn > s.node_stride ||
                     ne > s.edge_stride || np > s.capacity;
    sh.run = bad ? 0 : 1;
    if (bad) {
      status = PRS_ERR_RANGE;
    } else {
      float pose_new[16], prev_new[16];
      int want = PRS_SESSION_NO_SPLIT;
      if (k == 0) {
        se3_identity(pose_new);
        se3_identity(prev_new);
      } else {
        float pred[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          pred[i]     = sh.in_pred[i];
          prev_new[i] = sh.in_pose[i];
        }
        const bool lost = sh.in_i[7] != 1 || sh.in_i[8] < 0;
        if (lost) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            pose_new[i] = pred[i];
          }
        } else {
          float Xm[16], Xi[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            Xm[i] = sh.in_X[i];
          }
          se3_inverse(Xm, Xi);
          se3_mul(pred, Xi, pose_new);
        }
        const float t2 = (pose_new[3] * pose_new[3] + pose_new[7] * pose_new[7]) + pose_new[11] * pose_new[11];
        const float c  = (((pose_new[0] + pose_new[5]) + pose_new[10]) - 1.0f) * 0.5f;
        want = lost ? PRS_SESSION_SPLIT_LOST : ((t2 > a.d2 || c < a.cos_a) ? PRS_SESSION_SPLIT_VIEWPOINT : PRS_SESSION_NO_SPLIT);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        sh.logged[i] = pose_new[i];
      }
      sh.write_log = k < s.frame_stride ? 1 : 0;
      sh.frame_row = k;
      sh.n_points  = np;
      if (k >= s.frame_stride) {
        status = PRS_ERR_CAPACITY;
      }
      if (want != PRS_SESSION_NO_SPLIT && (nn >= s.node_stride || ne >= s.edge_stride)) {
        status = PRS_ERR_CAPACITY;
        want   = PRS_SESSION_NO_SPLIT;
      }
      float pose_out[16], prev_out[16], pred_out[16];
      int frame, n_corr_merge;
      if (want != PRS_SESSION_NO_SPLIT) {
        double Xc[16], Pd[16], Xn[16];
        const double* gx = s.graph_X + ((size_t) b * s.node_stride + cur) * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          Xc[i] = gx[i];
          Pd[i] = (double) pose_new[i];
        }
        se3_mul(Xc, Pd, Xn);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          sh.node_X[i] = Xn[i];
        }
        float Pi[16];
        se3_inverse(pose_new, Pi);
        se3_mul(Pi, prev_new, prev_out);
        se3_identity(pose_out);
        frame        = 0;
        n_corr_merge = 0;
        sh.node      = nn;
        sh.edge      = ne;
        s.fixed[(size_t) b * s.node_stride + nn] = 0;
        s.from[(size_t) b * s.edge_stride + ne]  = cur;
        s.to[(size_t) b * s.edge_stride + ne]    = nn;
        s.n_nodes[b]  = nn + 1;
        s.n_edges[b]  = ne + 1;
        s.cur_node[b] = nn;
        s.n_points[b] = 0;
        n_query       = np;
        if (s.handover_desc) {
          s.handover_graph_id[b] = (s.graph_id_base ? s.graph_id_base[b] : 0) + (int64_t) cur;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          pose_out[i] = pose_new[i];
          prev_out[i] = prev_new[i];
        }
        frame        = k == 0 ? 0 : slot;
        n_corr_merge = k == 0 ? 0 : sh.in_i[6];
      }
      reason = want;
      motion_predict(prev_out, pose_out, pred_out);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        sh.pose[i] = pose_out[i];
        sh.prev[i] = prev_out[i];
        sh.pred[i] = pred_out[i];
      }
      s.frame[b]        = frame;
      s.n_corr_merge[b] = n_corr_merge;
      s.slot[b]         = frame + 1;
      s.n_frames[b]     = k + 1;
    }
    sh.reason   = reason;
    s.status[b] = status;
    s.reason[b] = reason;
    if (s.handover_desc) {
      s.handover_n_query[b] = n_query;
    }
  }
  __syncthreads();
  if (!sh.run) {
    return;
  }
  const bool split = sh.reason != PRS_SESSION_NO_SPLIT;  // block-uniform
  if (tid < 16) {
    const float v = sh.pose[tid];
    s.pose[(size_t) b * 16 + tid]                 = v;
    s.measurement_in_world[(size_t) b * 16 + tid] = v;
    s.measurement_in_scene[(size_t) b * 16 + tid] = v;
  } else if (tid < 32) {
    s.prev[(size_t) b * 16 + (tid - 16)] = sh.prev[tid - 16];
  } else if (tid < 48) {
    s.prediction[(size_t) b * 16 + (tid - 32)] = sh.pred[tid - 32];
  } else if (tid < 64) {
    if (sh.write_log) {
      const size_t row = (size_t) b * s.frame_stride + sh.frame_row;
      s.frame_pose[row * 16 + (tid - 48)] = sh.logged[tid - 48];
      if (tid == 48) {
        s.frame_node[row] = sh.in_i[2];
      }
    }
  } else if (split) {
    const size_t erow = (size_t) b * s.edge_stride + sh.edge;
    if (tid < 80) {
      s.Z[erow * 16 + (tid - 64)] = sh.logged[tid - 64];
    } else if (tid < 96) {
      s.graph_X[((size_t) b * s.node_stride + sh.node) * 16 + (tid - 80)] = sh.node_X[tid - 80];
    } else if (tid < 132 && s.omega) {
      const int j    = tid - 96;
      const float in = sh.reason == PRS_SESSION_SPLIT_LOST ? a.info_lost : a.info_split;
      s.omega[erow * 36 + j] = (j % 7 == 0) ? in : 0.0f;
    }
  }
  if (!split) {
    return;
  }
  const int np = sh.n_points;
  if (s.handover_desc) {
    // 16 bytes per access: one per row of coords, two per row of desc
    const uint4* cs = reinterpret_cast<const uint4*>(s.coords) + (size_t) b * s.capacity;
    uint4* cd       = reinterpret_cast<uint4*>(s.handover_xyz) + (size_t) b * s.handover_stride;
    for (int r = tid; r < np; r += kThreads) {
      cd[r] = cs[r];
    }
    const uint4* ds = reinterpret_cast<const uint4*>(s.desc) + (size_t) b * s.capacity * 2;
    uint4* dd       = reinterpret_cast<uint4*>(s.handover_desc) + (size_t) b * s.handover_stride * 2;
    for (int r = tid; r < 2 * np; r += kThreads) {
      dd[r] = ds[r];
    }
  }
  // n_meas[b][0 .. capacity) = 0: single words up to the first 16-byte boundary, 16-byte stores, single words for the rest
  uint32_t* nm   = s.n_meas + (size_t) b * s.capacity;
  const int mis  = (int) ((reinterpret_cast<uintptr_t>(nm) >> 2) & 3);
  int head       = (4 - mis) & 3;
  head           = head < s.capacity ? head : s.capacity;
  const int quad = (s.capacity - head) >> 2;
  uint4* body    = reinterpret_cast<uint4*>(nm + head);
  for (int r = tid; r < quad; r += kThreads) {
    body[r] = make_uint4(0u, 0u, 0u, 0u);
  }
  const int tail = head + 4 * quad;
  if (tid < head) {
    nm[tid] = 0u;
  }
  if (tid < 4 && tail + tid < s.capacity) {
    nm[tail + tid] = 0u;
  }
}

// one thread per (sequence, frame): out = (float) X[node] * frame_pose
__global__ __launch_bounds__(kThreads) void session_unroll_kernel(const prs_session_batch s, float* __restrict__ out) {
  const long long idx = (long long) blockIdx.x * kThreads + threadIdx.x;
  const int b         = (int) (idx / s.frame_stride);
  const int k         = (int) (idx % s.frame_stride);
  if (b >= s.batch || k >= s.n_frames[b]) {
    return;
  }
  const size_t row = (size_t) b * s.frame_stride + k;
  const int node   = s.frame_node[row];
  if (node < 0 || node >= s.node_stride) {
    return;
  }
  float G[16], P[16], R[16];
  const double* gx = s.graph_X + ((size_t) b * s.node_stride + node) * 16;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    G[i] = (float) gx[i];
    P[i] = s.frame_pose[row * 16 + i];
  }
  se3_mul(G, P, R);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    out[row * 16 + i] = R[i];
  }
}

bool aligned(const void* p, uintptr_t to) {
  return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0;
}

}  // namespace

int session_step_launch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch) {
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_session_step_batch: parameters not set");
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  const prs_session_batch& s = *batch;
  if (!s.pose || !s.prev || !s.prediction || !s.slot || !s.cur_node || !s.n_frames || !s.frame_node || !s.frame_pose || !s.status ||
      !s.reason || !s.X || !s.result || !s.n_corr || !s.coords || !s.desc || !s.n_points || !s.n_meas || !s.frame || !s.n_corr_merge ||
      !s.measurement_in_world || !s.measurement_in_scene || !s.graph_X || !s.fixed || !s.n_nodes || !s.from || !s.to || !s.Z ||
      !s.n_edges || (s.handover_desc && (!s.handover_xyz || !s.handover_n_query || !s.handover_graph_id))) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_session_step_batch: input or output buffer not set");
  }
  if (s.frame_stride < 1 || s.capacity < 1 || s.node_stride < 1 || s.edge_stride < 1 || !std::isfinite(params->local_map_distance) ||
      params->local_map_distance < 0.0f || !std::isfinite(params->local_map_angle_distance_radians) ||
      !std::isfinite(params->split_information) || !std::isfinite(params->lost_information)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_session_step_batch: a stride or the capacity below 1, a parameter not finite or a negative distance");
  }
  if (s.handover_desc && s.handover_stride < s.capacity) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_session_step_batch: handover_stride below the maps' capacity");
  }
  if (!aligned(s.coords, 16) || !aligned(s.desc, 16) || !aligned(s.graph_X, 8) || !aligned(s.n_meas, 4) ||
      (s.handover_desc && (!aligned(s.handover_desc, 16) || !aligned(s.handover_xyz, 16)))) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_session_step_batch: coords, desc and the hand-over arrays must be 16-byte aligned, graph_X 8-byte");
  }
  if (!s.omega && (params->split_information != 1.0f || params->lost_information != 1.0f)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_session_step_batch: graphs without omega hold identity information only");
  }
  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.s          = s;
  a.d2         = params->local_map_distance * params->local_map_distance;
  a.cos_a      = (double) params->local_map_angle_distance_radians >= M_PI ? -INFINITY
                                                                            : (float) cos((double) params->local_map_angle_distance_radians);
  a.info_split = params->split_information;
  a.info_lost  = params->lost_information;
  hipLaunchKernelGGL(session_step_kernel, dim3((unsigned) s.batch), dim3(kThreads), 0, ctx_stream(ctx), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_session_step_batch launch");
  }
  return PRS_OK;
}

int session_unroll_launch(prs_context* ctx, const prs_session_batch* batch, float* out) {
  if (!batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_session_unroll_batch: batch not set");
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  if (!batch->n_frames || !batch->frame_node || !batch->frame_pose || !batch->graph_X || !out) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_session_unroll_batch: input or output buffer not set");
  }
  if (batch->frame_stride < 1 || batch->node_stride < 1) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_session_unroll_batch: a stride below 1");
  }
  const long long total  = (long long) batch->batch * batch->frame_stride;
  const long long blocks = (total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffll) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_session_unroll_batch: batch * frame_stride beyond one grid");
  }
  hipLaunchKernelGGL(session_unroll_kernel, dim3((unsigned) blocks), dim3(kThreads), 0, ctx_stream(ctx), *batch, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_session_unroll_batch launch");
  }
  return PRS_OK;
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_session_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_session_params);
  sizes2[1] = sizeof(prs_session_batch);
}

int prs_session_step_batch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return session_step_launch(ctx, params, batch);
}

int prs_session_unroll_batch(prs_context* ctx, const prs_session_batch* batch, float* out) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return session_unroll_launch(ctx, batch, out);
}

}  // extern "C"
