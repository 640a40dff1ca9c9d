// session.hip -- local-map manager on the device: the per-frame step between the aligner and the merger (pose update, trajectory
// log, splitting criterion, growth of the pose graph, hand-over and reset of the finished map, next prediction) and the unrolling
// of the logged trajectories through the graph.  The rule is stated in include/proslam_hip.h (BUILD-DEFINED) and restated in
// tests/session_ref.py; every float expression is an explicit two-operand operation in a fixed order (prs_se3.h).
// Map re-entry (prs_session_step_archive_batch, prs_session_reenter_batch; restated in tests/reentry_ref.py): the step instantiated
// with a block-uniform archive flag keeps a finished map's whole state in a slot of the caller's archive, and the re-entry kernel
// chooses a closure, loads the old map back, re-expresses the session in it and arms the closure merger.
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <string>
#include <type_traits>

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

// the live map's arrays the session batch does not carry, and the archive (prs_session_step_archive_batch)
struct ArchiveArgs {
  prs_map_archive ar;
  const float* state;
  const float* covariance;
  const uint32_t* n_opt;
  const uint8_t* inlier;
  const prs_camera_measurement* meas;  // nullptr: the history is not kept
  const prs_frame_pose* poses;
};

// n bytes from src to dst by the workgroup.  16 bytes per access where src and dst sit alike within 16 bytes, with single bytes up
// to the first boundary and behind the last; words where they sit alike within 4 bytes only; bytes otherwise.  A live row and an
// archive row lie k * capacity rows apart: coords, desc and state (16- and 32-byte rows) always sit alike, covariance, n_opt and
// n_meas (36- and 4-byte rows) when capacity is a multiple of 4, inlier (1-byte rows) when it is a multiple of 16.
__device__ __forceinline__ void copy_span(void* dst_, const void* src_, const size_t n, const int tid) {
  unsigned char* dst       = static_cast<unsigned char*>(dst_);
  const unsigned char* src = static_cast<const unsigned char*>(src_);
  const uintptr_t d = reinterpret_cast<uintptr_t>(dst), q = reinterpret_cast<uintptr_t>(src);
  if (((d ^ q) & 15) == 0) {
    size_t head = (size_t) ((16 - (d & 15)) & 15);
    head        = head < n ? head : n;
    const size_t quads = (n - head) >> 4;
    const uint4* sb    = reinterpret_cast<const uint4*>(src + head);
    uint4* db          = reinterpret_cast<uint4*>(dst + head);
    for (size_t r = tid; r < quads; r += kThreads) {
      db[r] = sb[r];
    }
    const size_t tail = head + (quads << 4);
    if ((size_t) tid < head) {
      dst[tid] = src[tid];
    }
    if (tid < 16 && tail + tid < n) {
      dst[tail + tid] = src[tail + tid];
    }
  } else if (((d | q | n) & 3) == 0) {
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dw       = reinterpret_cast<uint32_t*>(dst);
    for (size_t r = tid; r < (n >> 2); r += kThreads) {
      dw[r] = sw[r];
    }
  } else {
    for (size_t r = tid; r < n; r += kThreads) {
      dst[r] = src[r];
    }
  }
}

// words [first, capacity) of a row of n_meas = 0: single words up to the first 16-byte boundary, 16-byte stores, single words for
// the rest
__device__ __forceinline__ void zero_words(uint32_t* nm, const int first, const int capacity, const int tid) {
  uint32_t* p    = nm + first;
  const int n    = capacity - first;
  const int mis  = (int) ((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
  int head       = (4 - mis) & 3;
  head           = head < n ? head : n;
  const int quad = (n - head) >> 2;
  uint4* body    = reinterpret_cast<uint4*>(p + head);
  for (int r = tid; r < quad; r += kThreads) {
    body[r] = make_uint4(0u, 0u, 0u, 0u);
  }
  const int tail = head + 4 * quad;
  if (tid < head) {
    p[tid] = 0u;
  }
  if (tid < 4 && tail + tid < n) {
    p[tail + tid] = 0u;
  }
}

// the per-landmark arrays of one map: a slot of the archive, or the live map of a sequence
struct MapRows {
  float* coords;
  uint8_t* desc;
  float* state;
  float* covariance;
  uint32_t* n_opt;
  uint8_t* inlier;
  uint32_t* n_meas;
  prs_camera_measurement* meas;
  prs_frame_pose* poses;
};

__device__ __forceinline__ MapRows archive_rows(const prs_map_archive& ar, const int b, const int slot) {
  const size_t row = ((size_t) b * ar.slot_stride + slot) * ar.capacity;
  MapRows m;
  m.coords     = ar.coords + row * 4;
  m.desc       = ar.desc + row * 32;
  m.state      = ar.state + row * 4;
  m.covariance = ar.covariance + row * 9;
  m.n_opt      = ar.n_opt + row;
  m.inlier     = ar.inlier + row;
  m.n_meas     = ar.n_meas + row;
  m.meas       = ar.meas ? ar.meas + row * ar.max_measurements : nullptr;
  m.poses      = ar.meas ? ar.poses + ((size_t) b * ar.slot_stride + slot) * ar.max_frames : nullptr;
  return m;
}

// rows [0, n) of every per-landmark array and, where both sides keep them, of the history and the whole pose table
// (N_MEAS = false: the caller clears the whole row of n_meas instead)
template <bool N_MEAS = true>
__device__ __forceinline__ void copy_map(const MapRows& dst, const MapRows& src, const int n, const int max_measurements,
                                         const int max_frames, const int tid) {
  copy_span(dst.coords, src.coords, (size_t) n * 16, tid);
  copy_span(dst.desc, src.desc, (size_t) n * 32, tid);
  copy_span(dst.state, src.state, (size_t) n * 16, tid);
  copy_span(dst.covariance, src.covariance, (size_t) n * 36, tid);
  copy_span(dst.n_opt, src.n_opt, (size_t) n * 4, tid);
  copy_span(dst.inlier, src.inlier, (size_t) n, tid);
  if (N_MEAS) {
    copy_span(dst.n_meas, src.n_meas, (size_t) n * 4, tid);
  }
  if (dst.meas && src.meas) {
    copy_span(dst.meas, src.meas, (size_t) n * max_measurements * sizeof(prs_camera_measurement), tid);
    copy_span(dst.poses, src.poses, (size_t) max_frames * sizeof(prs_frame_pose), tid);
  }
}

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
  int arch_slot;  // (archive) the slot the finished map goes to, -1: none
};

// one workgroup per sequence: the first wave loads, thread 0 does the pose arithmetic and publishes the decision through LDS, the
// workgroup stores the matrices and, on a split (block-uniform), copies the finished map out and clears its measurement counts
// The archive entry's kernel arguments: the step's, then the archive's.  The body reads the second part from the kernel-argument
// segment where it uses it (fetch_archive_args), so that its 23 words are not held in scalar registers across thread 0's arithmetic:
// taken as an ordinary by-value argument they were loaded at the top of the kernel and spilled (54 scalar spills against the plain
// instantiation's 20: 0.45 us a launch at B = 1, 1 us at B = 4096, profiles/reentry/README.md).  The kernel is held to the plain
// instantiation's 6 waves per SIMD (amdgpu_waves_per_eu): left alone the inlined copies took it to 104 VGPRs and 4 waves, which
// cost every no-split frame of a large batch a quarter of its time for a copy that runs on one frame in ten to twenty.
struct ArchiveStepArgs {
  StepArgs a;
  ArchiveArgs aa;
};

// the archive's arguments, loaded here and not earlier (the empty asm hides the pointer's origin from the scheduler).  This reads
// the kernel-argument segment directly, so it holds only in a kernel that takes ONE argument, an ArchiveStepArgs by value: the
// code-object ABI puts the first argument at offset 0 of the segment when its alignment is at most 16.
static_assert(alignof(ArchiveStepArgs) <= 16 && offsetof(ArchiveStepArgs, a) == 0 && offsetof(ArchiveStepArgs, aa) % alignof(ArchiveArgs) == 0 &&
                  offsetof(ArchiveStepArgs, aa) >= sizeof(StepArgs) && std::is_trivially_copyable<ArchiveStepArgs>::value,
              "fetch_archive_args reads ArchiveStepArgs::aa at its offset in the kernel-argument segment");
__device__ __forceinline__ ArchiveArgs fetch_archive_args() {
  typedef const char __attribute__((address_space(4))) * kernarg_ptr;
  kernarg_ptr p = (kernarg_ptr) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ArchiveStepArgs, aa);
  asm volatile("" : "+s"(p));
  ArchiveArgs out;
  __builtin_memcpy(&out, p, sizeof(out));
  return out;
}

// ARCHIVE (block-uniform, prs_session_step_archive_batch): the finished map's whole state is kept before the reset
template <bool ARCHIVE>
__device__ __forceinline__ void session_step_body(const StepArgs& a) {
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
    int arch_status = PRS_OK, arch_slot = -1;
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
        if (ARCHIVE) {
          const ArchiveArgs fetched = fetch_archive_args();
          const prs_map_archive& ar  = fetched.ar;
          int32_t* son = ar.slot_of_node + (size_t) b * ar.node_stride + cur;
          arch_slot    = *son;
          if (arch_slot >= ar.slot_stride) {
            arch_status = PRS_ERR_RANGE;
            arch_slot   = -1;
          } else if (arch_slot < 0) {
            const int ns = ar.n_slots[b];
            if (ns < 0 || ns >= ar.slot_stride) {
              arch_status = PRS_ERR_CAPACITY;
              arch_slot   = -1;
            } else {
              arch_slot    = ns;
              ar.n_slots[b] = ns + 1;
              *son          = ns;
            }
          }
          if (arch_slot >= 0) {
            const size_t as   = (size_t) b * ar.slot_stride + arch_slot;
            ar.n_points[as]   = np;
            ar.next_frame[as] = slot;
          }
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
    if (ARCHIVE) {
      sh.arch_slot         = arch_slot;
      int32_t* const __restrict__ arch_status_out = fetch_archive_args().ar.status;
      arch_status_out[b] = arch_status;
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
  if (ARCHIVE) {
    if (sh.arch_slot >= 0) {  // block-uniform
      const ArchiveArgs fetched = fetch_archive_args();
      const ArchiveArgs* aa     = &fetched;
      const size_t row = (size_t) b * s.capacity;
      MapRows live;
      live.coords     = const_cast<float*>(s.coords) + row * 4;
      live.desc       = const_cast<uint8_t*>(s.desc) + row * 32;
      live.state      = const_cast<float*>(aa->state) + row * 4;
      live.covariance = const_cast<float*>(aa->covariance) + row * 9;
      live.n_opt      = const_cast<uint32_t*>(aa->n_opt) + row;
      live.inlier     = const_cast<uint8_t*>(aa->inlier) + row;
      live.n_meas     = s.n_meas + row;
      live.meas       = aa->meas ? const_cast<prs_camera_measurement*>(aa->meas) + row * aa->ar.max_measurements : nullptr;
      live.poses      = aa->meas ? const_cast<prs_frame_pose*>(aa->poses) + (size_t) b * aa->ar.max_frames : nullptr;
      copy_map(archive_rows(aa->ar, b, sh.arch_slot), live, np, aa->ar.max_measurements, aa->ar.max_frames, tid);
    }
    __syncthreads();  // n_meas has been read by other threads than those that clear it
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

__global__ __launch_bounds__(kThreads) void session_step_kernel(const StepArgs a) {
  session_step_body<false>(a);
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(6, 6))) void session_step_archive_kernel(const ArchiveStepArgs k) {
  session_step_body<true>(k.a);
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

struct ReenterArgs {
  prs_session_batch s;
  ArchiveArgs aa;
  prs_reentry_batch r;
  prs_reentry_params p;
  float max_t2;  // max_translation^2, formed in float on the host
};

struct ReenterShared {
  float pose[16], prev[16], pred[16], Xk[16], siw[16];
  int go;       // 1: re-enter (block-uniform)
  int e;        // the odometry edge into m
  int ne;       // n_edges as found
  int o;        // the node re-entered
  int k;        // the winning slot of the sequence's candidates
  int aslot;    // its archive slot
  int np;       // points archived there
  int nc;       // the winner's correspondences
  int frame;    // the pose-table slot the frame takes
};

// one workgroup per sequence: thread 0 checks, chooses the closure and does the pose arithmetic; the workgroup moves the edges down,
// stores the matrices, loads the archived map and copies the winner's correspondences
__global__ __launch_bounds__(kThreads) void session_reenter_kernel(const ReenterArgs a) {
  __shared__ ReenterShared sh;
  const prs_session_batch& s = a.s;
  const prs_reentry_batch& r = a.r;
  const prs_map_archive& ar  = a.aa.ar;
  const int b   = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int status = PRS_OK, go = 0;
    if (s.reason[b] == PRS_SESSION_SPLIT_VIEWPOINT && s.status[b] == PRS_OK) {
      const int nn = s.n_nodes[b], ne = s.n_edges[b], cur = s.cur_node[b];
      const int m  = nn - 1;
      int e = -1, n_into = 0;
      if (nn < 1 || nn > s.node_stride || ne < 0 || ne > s.edge_stride || cur != m) {
        status = PRS_ERR_RANGE;
      } else {
        for (int j = 0; j < ne; ++j) {
          if (s.to[(size_t) b * s.edge_stride + j] == m) {
            e = n_into == 0 ? j : e;
            ++n_into;
          }
        }
        const int f = n_into == 1 ? s.from[(size_t) b * s.edge_stride + e] : -1;
        if (n_into != 1 || f < 0 || f >= m) {
          status = PRS_ERR_RANGE;
        } else {
          float Z[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            Z[i] = s.Z[((size_t) b * s.edge_stride + e) * 16 + i];
          }
          int best = -1, best_inliers = 0, best_o = -1;
          float bestP[16];
          for (int k = 0; k < r.max_candidates; ++k) {
            const size_t sl = (size_t) b * r.max_candidates + k;
            const int c     = r.candidates_flat[sl];
            const int mi    = c - b * r.map_stride;
            if (c < 0 || mi < 0 || mi >= r.map_stride || r.result[sl].accepted == 0) {
              continue;
            }
            const int o = r.node_of_map[(size_t) b * r.map_stride + mi];
            if (o < 0 || o >= nn || o == f || o == m || ar.slot_of_node[(size_t) b * ar.node_stride + o] < 0) {
              continue;
            }
            const int ni   = r.result[sl].num_inliers;
            const float fi = (float) ni;
            if (!(ni >= a.p.relocalize_min_inliers) || !(fi / (float) r.result[sl].num_correspondences >= a.p.relocalize_min_inliers_ratio) ||
                !(r.result[sl].chi_inliers / fi <= a.p.relocalize_max_chi_inliers)) {
              continue;
            }
            float Xk[16], Xi[16], P[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              Xk[i] = r.X[sl * 16 + i];
            }
            se3_inverse(Xk, Xi);
            se3_mul(Xi, Z, P);
            const float t2 = (P[3] * P[3] + P[7] * P[7]) + P[11] * P[11];
            if (!(t2 <= a.max_t2)) {
              continue;
            }
            if (best < 0 || ni > best_inliers) {
              best         = k;
              best_inliers = ni;
              best_o       = o;
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                bestP[i] = P[i];
              }
            }
          }
          if (best >= 0) {
            const size_t sl = (size_t) b * r.max_candidates + best;
            const int aslot = ar.slot_of_node[(size_t) b * ar.node_stride + best_o];
            const int np    = aslot < ar.slot_stride ? ar.n_points[(size_t) b * ar.slot_stride + aslot] : -1;
            const int nc    = r.n_corr[sl];
            if (aslot >= ar.slot_stride || np < 0 || np > s.capacity || nc < 0 || nc > r.corr_stride) {
              status = PRS_ERR_RANGE;
            } else {
              go = 1;
              float prev_old[16], prev_new[16], pred[16];
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                prev_old[i] = s.prev[(size_t) b * 16 + i];
              }
              se3_mul(bestP, prev_old, prev_new);
              motion_predict(prev_new, bestP, pred);
              const double* gx = s.graph_X + ((size_t) b * s.node_stride + best_o) * 16;
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                sh.pose[i] = bestP[i];
                sh.prev[i] = prev_new[i];
                sh.pred[i] = pred[i];
                sh.Xk[i]   = r.X[sl * 16 + i];
                sh.siw[i]  = (float) gx[i];
              }
              sh.e     = e;
              sh.ne    = ne;
              sh.o     = best_o;
              sh.k     = best;
              sh.aslot = aslot;
              sh.np    = np;
              sh.nc    = nc;
              sh.frame = ar.meas ? ar.next_frame[(size_t) b * ar.slot_stride + aslot] : 0;
              s.n_edges[b]      = ne - 1;
              s.n_nodes[b]      = nn - 1;
              s.cur_node[b]     = best_o;
              s.n_points[b]     = np;
              s.frame[b]        = sh.frame;
              s.slot[b]         = sh.frame + 1;
              s.n_corr_merge[b] = 0;
              r.n_measured[b]   = 0;
              r.merge_n_corr[b] = nc;
            }
          }
        }
      }
    }
    sh.go          = go;
    r.status[b]    = status;
    r.reentered[b] = go;
    if (!go && status == PRS_OK) {
      r.gate[b].accepted = 0;
      r.merge_n_corr[b]  = 0;
    }
  }
  __syncthreads();
  if (!sh.go) {
    return;
  }
  // the edges behind e move down by one: a thread keeps its element of the edge, so the rows it reads and writes are its own
  for (int j = sh.e + 1; j < sh.ne; ++j) {
    const size_t src = (size_t) b * s.edge_stride + j, dst = src - 1;
    if (tid < 16) {
      s.Z[dst * 16 + tid] = s.Z[src * 16 + tid];
    } else if (tid < 52) {
      if (s.omega) {
        s.omega[dst * 36 + (tid - 16)] = s.omega[src * 36 + (tid - 16)];
      }
    } else if (tid == 52) {
      s.from[dst] = s.from[src];
    } else if (tid == 53) {
      s.to[dst] = s.to[src];
    }
  }
  const size_t sl = (size_t) b * r.max_candidates + sh.k;
  if (tid >= 64 && tid < 80) {
    const float v = sh.pose[tid - 64];
    s.pose[(size_t) b * 16 + (tid - 64)]                 = v;
    s.measurement_in_world[(size_t) b * 16 + (tid - 64)] = v;
    s.measurement_in_scene[(size_t) b * 16 + (tid - 64)] = v;
  } else if (tid >= 80 && tid < 96) {
    s.prev[(size_t) b * 16 + (tid - 80)] = sh.prev[tid - 80];
  } else if (tid >= 96 && tid < 112) {
    s.prediction[(size_t) b * 16 + (tid - 96)] = sh.pred[tid - 96];
  } else if (tid >= 112 && tid < 128) {
    r.merge_transform[(size_t) b * 16 + (tid - 112)] = sh.Xk[tid - 112];
  } else if (tid >= 128 && tid < 144) {
    r.scene_in_world[(size_t) b * 16 + (tid - 128)] = sh.siw[tid - 128];
  } else if (tid >= 144 && tid < 144 + (int) (sizeof(prs_point_align_result) / 4)) {
    const int w       = tid - 144;
    const int32_t* gs = reinterpret_cast<const int32_t*>(r.result + sl);
    int32_t* gd       = reinterpret_cast<int32_t*>(r.gate + b);
    gd[w]             = w == (int) (offsetof(prs_point_align_result, accepted) / 4) ? 1 : gs[w];
  }
  // the archived map back into the live arrays
  const size_t row = (size_t) b * s.capacity;
  MapRows live;
  live.coords     = const_cast<float*>(s.coords) + row * 4;
  live.desc       = const_cast<uint8_t*>(s.desc) + row * 32;
  live.state      = const_cast<float*>(a.aa.state) + row * 4;
  live.covariance = const_cast<float*>(a.aa.covariance) + row * 9;
  live.n_opt      = const_cast<uint32_t*>(a.aa.n_opt) + row;
  live.inlier     = const_cast<uint8_t*>(a.aa.inlier) + row;
  live.n_meas     = s.n_meas + row;
  live.meas       = a.aa.meas ? const_cast<prs_camera_measurement*>(a.aa.meas) + row * ar.max_measurements : nullptr;
  live.poses      = a.aa.meas ? const_cast<prs_frame_pose*>(a.aa.poses) + (size_t) b * ar.max_frames : nullptr;
  if (ar.meas) {
    copy_map(live, archive_rows(ar, b, sh.aslot), sh.np, ar.max_measurements, ar.max_frames, tid);
    zero_words(live.n_meas, sh.np, s.capacity, tid);
  } else {  // no history: no count survives, so none is copied
    copy_map<false>(live, archive_rows(ar, b, sh.aslot), sh.np, ar.max_measurements, ar.max_frames, tid);
    zero_words(live.n_meas, 0, s.capacity, tid);
  }
  // the winner's matcher vector
  copy_span(r.merge_corr + (size_t) b * r.corr_stride, r.corr + sl * r.corr_stride, (size_t) sh.nc * sizeof(prs_corr), tid);
}

}  // namespace

// the message of a refused call, built on the failure path only
static std::string fail_text(const char* who, const char* what) {
  return std::string(who) + what;
}

// the checks and the launcher's arithmetic of the step, shared by its two entry points (who: the entry point's name)
static int step_prepare(prs_context* ctx, const char* who, const prs_session_params* params, const prs_session_batch* batch, StepArgs* out) {
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": parameters not set").c_str());
  }
  const prs_session_batch& s = *batch;
  if (!s.pose || !s.prev || !s.prediction || !s.slot || !s.cur_node || !s.n_frames || !s.frame_node || !s.frame_pose || !s.status ||
      !s.reason || !s.X || !s.result || !s.n_corr || !s.coords || !s.desc || !s.n_points || !s.n_meas || !s.frame || !s.n_corr_merge ||
      !s.measurement_in_world || !s.measurement_in_scene || !s.graph_X || !s.fixed || !s.n_nodes || !s.from || !s.to || !s.Z ||
      !s.n_edges || (s.handover_desc && (!s.handover_xyz || !s.handover_n_query || !s.handover_graph_id))) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": input or output buffer not set").c_str());
  }
  if (s.frame_stride < 1 || s.capacity < 1 || s.node_stride < 1 || s.edge_stride < 1 || !std::isfinite(params->local_map_distance) ||
      params->local_map_distance < 0.0f || !std::isfinite(params->local_map_angle_distance_radians) ||
      !std::isfinite(params->split_information) || !std::isfinite(params->lost_information)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, fail_text(who, ": a stride or the capacity below 1, a parameter not finite or a negative distance").c_str());
  }
  if (s.handover_desc && s.handover_stride < s.capacity) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, fail_text(who, ": handover_stride below the maps' capacity").c_str());
  }
  if (!aligned_to(s.coords, 16) || !aligned_to(s.desc, 16) || !aligned_to(s.graph_X, 8) || !aligned_to(s.n_meas, 4) ||
      (s.handover_desc && (!aligned_to(s.handover_desc, 16) || !aligned_to(s.handover_xyz, 16)))) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, fail_text(who, ": coords, desc and the hand-over arrays must be 16-byte aligned, graph_X 8-byte").c_str());
  }
  if (!s.omega && (params->split_information != 1.0f || params->lost_information != 1.0f)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, fail_text(who, ": graphs without omega hold identity information only").c_str());
  }
  StepArgs& a = *out;
  memset(&a, 0, sizeof(a));
  a.s          = s;
  a.d2         = params->local_map_distance * params->local_map_distance;
  a.cos_a      = (double) params->local_map_angle_distance_radians >= M_PI ? -INFINITY
                                                                            : (float) cos((double) params->local_map_angle_distance_radians);
  a.info_split = params->split_information;
  a.info_lost  = params->lost_information;
  return PRS_OK;
}

int session_step_launch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch) {
  const char* who = "prs_session_step_batch";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": parameters not set").c_str());
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  StepArgs a;
  PRS_TRY(step_prepare(ctx, who, params, batch, &a));
  return Launches(ctx, who, ctx_stream(ctx)).one(batch->batch, kThreads, session_step_kernel, 0, a);
}

// the archive and the live map's statistics arrays against the session batch (who: the entry point's name)
static int archive_prepare(prs_context* ctx, const char* who, const prs_session_batch& s, const prs_merge_batch* maps,
                           const prs_map_archive* archive, ArchiveArgs* out) {
  if (!maps || !archive) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": maps or archive not set").c_str());
  }
  const prs_map_archive& ar = *archive;
  if (!ar.coords || !ar.desc || !ar.state || !ar.covariance || !ar.n_opt || !ar.inlier || !ar.n_meas || !ar.n_points || !ar.next_frame ||
      !ar.slot_of_node || !ar.n_slots || !ar.status || !maps->state || !maps->covariance || !maps->n_opt || !maps->inlier ||
      (ar.meas != nullptr) != (ar.poses != nullptr) || (ar.meas && (!maps->meas || !maps->poses))) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": an array of the archive or of the live map not set, or the history without the pose table").c_str());
  }
  if (ar.batch != s.batch || maps->batch != s.batch || ar.capacity != s.capacity || maps->capacity != s.capacity ||
      ar.node_stride != s.node_stride || ar.slot_stride < 1 ||
      (ar.meas && (ar.max_measurements < 1 || ar.max_frames < 1 || ar.max_measurements != maps->max_measurements ||
                   ar.max_frames != maps->max_frames))) {
    return ctx_fail(ctx, PRS_ERR_RANGE, fail_text(who, ": batch, capacity, node_stride or the history's shape differ between the structs, or slot_stride below 1").c_str());
  }
  if (!aligned_to(ar.coords, 16) || !aligned_to(ar.desc, 16) || !aligned_to(ar.state, 16) || !aligned_to(maps->state, 16) || !aligned_to(ar.covariance, 4) ||
      !aligned_to(maps->covariance, 4) || !aligned_to(ar.n_opt, 4) || !aligned_to(maps->n_opt, 4) || !aligned_to(ar.n_meas, 4) ||
      (ar.meas && (!aligned_to(ar.meas, 4) || !aligned_to(maps->meas, 4) || !aligned_to(ar.poses, 4) || !aligned_to(maps->poses, 4)))) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, fail_text(who, ": coords, desc and state must be 16-byte aligned, the other arrays 4-byte").c_str());
  }
  ArchiveArgs& aa = *out;
  memset(&aa, 0, sizeof(aa));
  aa.ar         = ar;
  aa.state      = maps->state;
  aa.covariance = maps->covariance;
  aa.n_opt      = maps->n_opt;
  aa.inlier     = maps->inlier;
  aa.meas       = ar.meas ? maps->meas : nullptr;
  aa.poses      = ar.meas ? maps->poses : nullptr;
  return PRS_OK;
}

int session_step_archive_launch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch,
                                const prs_merge_batch* maps, const prs_map_archive* archive) {
  const char* who = "prs_session_step_archive_batch";
  if (!params || !batch || !maps || !archive) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": parameters not set").c_str());
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  ArchiveStepArgs k;
  PRS_TRY(step_prepare(ctx, who, params, batch, &k.a));
  PRS_TRY(archive_prepare(ctx, who, *batch, maps, archive, &k.aa));
  return Launches(ctx, who, ctx_stream(ctx)).one(batch->batch, kThreads, session_step_archive_kernel, 0, k);
}

int session_reenter_launch(prs_context* ctx, const prs_reentry_params* params, const prs_session_batch* batch, const prs_merge_batch* maps,
                           const prs_map_archive* archive, const prs_reentry_batch* reentry) {
  const char* who = "prs_session_reenter_batch";
  if (!params || !batch || !maps || !archive || !reentry) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": parameters not set").c_str());
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  const prs_session_batch& s = *batch;
  const prs_reentry_batch& r = *reentry;
  if (!s.pose || !s.prev || !s.prediction || !s.slot || !s.cur_node || !s.status || !s.reason || !s.coords || !s.desc || !s.n_points ||
      !s.n_meas || !s.frame || !s.n_corr_merge || !s.measurement_in_world || !s.measurement_in_scene || !s.graph_X || !s.n_nodes ||
      !s.from || !s.to || !s.Z || !s.n_edges || !r.candidates_flat || !r.result || !r.X || !r.corr || !r.n_corr || !r.node_of_map ||
      !r.n_measured || !r.reentered || !r.status || !r.merge_corr || !r.merge_n_corr || !r.merge_transform || !r.scene_in_world || !r.gate) {
    return ctx_fail(ctx, PRS_ERR_NULL, fail_text(who, ": input or output buffer not set").c_str());
  }
  if (s.capacity < 1 || s.node_stride < 1 || s.edge_stride < 1 || r.max_candidates < 1 || r.map_stride < 1 || r.corr_stride < 1 ||
      !std::isfinite(params->max_translation) || params->max_translation < 0.0f || std::isnan(params->relocalize_min_inliers_ratio) ||
      std::isnan(params->relocalize_max_chi_inliers)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, fail_text(who, ": a stride, the capacity or max_candidates below 1, or a parameter not finite or negative").c_str());
  }
  if (!aligned_to(s.coords, 16) || !aligned_to(s.desc, 16) || !aligned_to(s.graph_X, 8) || !aligned_to(s.n_meas, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, fail_text(who, ": coords and desc must be 16-byte aligned, graph_X 8-byte").c_str());
  }
  ReenterArgs a;
  memset(&a, 0, sizeof(a));
  PRS_TRY(archive_prepare(ctx, who, s, maps, archive, &a.aa));
  a.s      = s;
  a.r      = r;
  a.p      = *params;
  a.max_t2 = params->max_translation * params->max_translation;
  return Launches(ctx, who, ctx_stream(ctx)).one(s.batch, kThreads, session_reenter_kernel, 0, a);
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
  const int64_t total = (int64_t) batch->batch * batch->frame_stride;
  return Launches(ctx, "prs_session_unroll_batch", ctx_stream(ctx)).one((total + kThreads - 1) / kThreads, kThreads, session_unroll_kernel,
                                                                        0, *batch, out);
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

void prs_map_archive_struct_sizes(uint64_t* sizes3) {
  sizes3[0] = sizeof(prs_map_archive);
  sizes3[1] = sizeof(prs_reentry_params);
  sizes3[2] = sizeof(prs_reentry_batch);
}

int prs_session_step_archive_batch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch,
                                   const prs_merge_batch* maps, const prs_map_archive* archive) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return session_step_archive_launch(ctx, params, batch, maps, archive);
}

int prs_session_reenter_batch(prs_context* ctx, const prs_reentry_params* params, const prs_session_batch* batch,
                              const prs_merge_batch* maps, const prs_map_archive* archive, const prs_reentry_batch* reentry) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return session_reenter_launch(ctx, params, batch, maps, archive, reentry);
}

int prs_session_unroll_batch(prs_context* ctx, const prs_session_batch* batch, float* out) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return session_unroll_launch(ctx, batch, out);
}

}  // extern "C"
