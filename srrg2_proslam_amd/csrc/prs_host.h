// prs_host.h -- host-side context shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/proslam_hip.h"
#include "prs_launch.h"

namespace prs {

// The context's grow-only scratch blocks.  The rule that keeps two users of one block apart: a launch function (*_launch)
// takes work arenas only, and what it puts there is dead when its kernels have run; a host-pointer entry point stages its
// arguments and results only in a staging arena (through prs::Staging below), never in a work arena.
enum Arena {
  ARENA_WORK_0,            // launches: candidates (brute force), kept features (extractor), smoother items (merger)
  ARENA_WORK_1,            // launches: candidates by level (brute force), blurred images (extractors), carry (merger)
  ARENA_WORK_2,            // launches: bitmaps (brute force), raw detections (extractor), tail items (merger)
  ARENA_WORK_3,            // launches: tile counts (scene clipper), work block (selective extractor)
  ARENA_STAGE,             // device side of the host-pointer entry points' staging block
  ARENA_STAGE_BRUTEFORCE,  // the same for prs_bruteforce_match, whose block stays live across its relaunches
  ARENA_STAGE_SOLVER,      // the same for prs_gn_step_ex and prs_selftest_reciprocal
  ARENA_STAGE_POSE_GRAPH,  // the same for prs_pose_graph_optimize, whose block also holds the graph's envelope
  ARENA_PINNED,            // host side (pinned) of all of them: an entry point synchronises before it returns
  ARENA_COUNT
};

// ---- memory the library owns.  Every device or pinned block of the library is allocated and freed through owned_alloc /
// owned_free (api.hip), each with a short name.  guard_layout is the one rule for how large a block is and where its user bytes
// lie: with guard off it is the size the site always asked for (the exact bytes, or the grow-only blocks' slack on top); with
// guard on (PRS_GUARD_FILL=00 / ff at prs_context_create) the block is [front band | user bytes | tail band], the tail band
// begins at the first byte behind `bytes` and is never smaller than the slack, so what stayed inside its block stays inside it.
inline uint64_t guard_slack(uint64_t bytes, int rule) {
  return rule == PRS_GUARD_SLACK_QUARTER ? bytes / 4 + 4096 : (rule == PRS_GUARD_SLACK_HALF ? bytes / 2 + 4096 : 0);
}
inline prs_guard_extent guard_layout(uint64_t bytes, int rule, bool guard) {
  const uint64_t slack = guard_slack(bytes, rule);
  if (!guard) {
    return {bytes + slack, 0, slack};
  }
  const uint64_t tail = slack > PRS_GUARD_BAND ? slack : PRS_GUARD_BAND;
  return {PRS_GUARD_BAND + bytes + tail, PRS_GUARD_BAND, tail};
}
struct GuardBlock {  // a live block of a context in guard mode
  void* user;
  size_t bytes, tail;
  const char* name;  // a string literal of the allocating site
  bool pinned;
};

}  // namespace prs

struct prs_context {
  int device            = 0;
  int cus               = 256;      // compute units of `device`, read once at prs_context_create (256 when the query fails)
  hipStream_t stream    = nullptr;  // stream work is enqueued on
  hipStream_t own       = nullptr;  // stream created (and destroyed) by the context
  std::string last_error;
  bool fused_align      = false;    // PRS_FUSED_ALIGN=1: one fused kernel per frame loop instead of the split search/GN pipeline
  bool matcher_v3       = false;    // PRS_MATCHER_V3=1: always use the first-generation matcher kernel
  bool force_unstaged   = false;    // test hook: PRS_FORCE_UNSTAGED=1 selects the no-LDS-staging variant
  bool merge_fused      = false;    // PRS_MERGE_FUSED=1: pose-based smoother merger as one kernel instead of front | smoother | back
  bool no_prefilter     = false;    // PRS_NO_PREFILTER=1: the search scan scores every candidate in full (diagnostic: what the irrelevance bound buys)
  int prefilter_96_limit = 32;      // PRS_PREFILTER_96_LIMIT: largest irrelevance bound the search scan tests on 96 instead of 128 bits (diagnostic / A-B)
  int bf_mfma           = 1;        // PRS_BF_DENSE_*: the brute-force matcher's dense phase (prs_context_set_bruteforce_dense_phase; PRS_BF_MFMA=0 / auto / 1)
  bool no_search_reuse  = false;    // PRS_NO_SEARCH_REUSE=1: every projective search of the split pipeline scans (no query cache; diagnostic / A-B)
  bool no_lone_gn       = false;    // PRS_NO_LONE_GN=1: small batches use the throughput instantiation of the Gauss-Newton kernel too (diagnostic)
  bool stamps_split     = false;    // PRS_STAMPS_SPLIT=1 (with PRS_STAMPS=1): phase stamps of the split search kernel
  struct {
    void* p     = nullptr;
    size_t size = 0;
  } arena[prs::ARENA_COUNT];        // reusable scratch (prs::ctx_arena)
  float* d_info_lut     = nullptr;  // information scale by landmark age, 4096 entries (scene clipper)
  // per-kernel HIP-event timing of the split aligner pipeline (prs_context_enable_timing; measurement only)
  bool timing           = false;
  double t_search_ms = 0.0, t_gn_ms = 0.0;
  long long n_search = 0, n_gn = 0;
  double t_search_round[16] = {}, t_gn_round[16] = {};  // the same, by round of the batch (round 15 collects the rest)
  long long n_batches_timed = 0;
  hipEvent_t timing_ev[3 * 64] = {};
  // the batch of the split aligner pipeline that has been enqueued and not yet finished (owned by align.hip)
  void* align_job               = nullptr;
  void (*align_job_free)(void*) = nullptr;
  // diagnostic phase stamps (PRS_STAMPS=1): never enabled in timed runs
  bool stamps_enabled   = false;
  unsigned long long* d_stamps = nullptr;
  size_t d_stamps_size  = 0;
  // guard mode (PRS_GUARD_FILL=00 / ff, tests): -1 = off, else the byte every owned block is painted with
  int guard_fill        = -1;
  std::vector<prs::GuardBlock> guard_blocks;  // live blocks, in allocation order
  std::vector<std::string> guard_latched;     // damaged bands found when a block was freed: "name side offset"
};

namespace prs {

inline hipStream_t ctx_stream(prs_context* ctx) {
  return ctx->stream;
}
// a step that returns a PRS status: anything but PRS_OK leaves the enclosing function with it (the step has set the message)
#define PRS_TRY(step)         \
  do {                        \
    const int rc_ = (step);   \
    if (rc_ != PRS_OK) {      \
      return rc_;             \
    }                         \
  } while (0)

// (ctx_fail, ctx_fail_hip, grid_fits and the launch path: prs_launch.h)
inline bool aligned_to(const void* p, uintptr_t to) {
  return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0;
}
// v rounded up to a multiple of 16, the alignment of every part of a workspace or an LDS layout (uint32_t or uint64_t)
template <class T>
constexpr T up16(const T v) {
  static_assert(std::is_unsigned<T>::value, "up16 takes an unsigned size");
  return (v + 15) & ~(T) 15;
}
// whether two arrays of a batch share a byte
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

inline size_t align256(size_t v) {
  return (v + 255) / 256 * 256;
}
// grows (never shrinks) one of the context's arenas to at least `bytes`, after the stream has drained if a block has to be
// freed; returns nullptr on failure
void* ctx_arena(prs_context* ctx, Arena arena, size_t bytes);
// one owned block of `bytes` user bytes (device, or pinned host memory), sized by guard_layout: *p is the user pointer, nullptr
// when the request is 0 bytes with guard off, as hipMalloc answers it.  In guard mode the bands are painted with
// PRS_GUARD_PATTERN and the user bytes with the context's fill before it returns.  `name` is a string literal.
hipError_t owned_alloc(prs_context* ctx, const char* name, void** p, size_t bytes, int rule = PRS_GUARD_SLACK_EXACT, bool pinned = false);
template <class T>
inline hipError_t owned_alloc(prs_context* ctx, const char* name, T** p, size_t bytes, int rule = PRS_GUARD_SLACK_EXACT, bool pinned = false) {
  void* v            = nullptr;
  const hipError_t e = owned_alloc(ctx, name, &v, bytes, rule, pinned);
  *p                 = static_cast<T*>(v);
  return e;
}
// frees a block of owned_alloc (nullptr: nothing).  In guard mode its bands are checked first and a damaged one is latched in
// the context; the caller has drained whatever stream still used the block, as it always had to
void owned_free(prs_context* ctx, void* p, bool pinned = false);
// guard mode: the first `bytes` user bytes of a reused block painted with the fill again, on `stream` in front of the launches
// (a pinned block: on the host, after the context's stream has drained).  Nothing with guard off
void owned_repaint(prs_context* ctx, void* p, size_t bytes, hipStream_t stream, bool pinned = false);

// The staging block of a host-pointer entry point: sections in declaration order, each starting on a 256-byte boundary, with
// the same layout in a device arena and in the pinned arena.  Declare the sections, commit(), fill the .h() side, upload()
// (ONE copy over the span of the up / both sections), point the batch descriptor at the .d() side and launch, download()
// (ONE copy over the span of the both / down sections, then a stream synchronise), read the .h() side.  Every error it
// returns has set the context's message, prefixed with the entry point's name.
class Staging {
 public:
  template <class T>
  struct Section {
    const Staging* st;
    int index;
    T* h() const {  // pinned side (not for device-only sections)
      return reinterpret_cast<T*>(st->h_ + st->rec_[index].off);
    }
    T* d() const {
      return reinterpret_cast<T*>(st->d_ + st->rec_[index].off);
    }
  };
  static constexpr size_t kAll = ~(size_t) 0;

  Staging(prs_context* ctx, const char* entry, Arena arena = ARENA_STAGE) : ctx_(ctx), entry_(entry), arena_(arena) {}
  template <class T>
  Section<T> up(size_t n) {  // uploaded
    return {this, add(kUp, n * sizeof(T))};
  }
  template <class T>
  Section<T> down(size_t n) {  // downloaded
    return {this, add(kDown, n * sizeof(T))};
  }
  template <class T>
  Section<T> both(size_t n) {  // uploaded and downloaded
    return {this, add(kUp | kDown, n * sizeof(T))};
  }
  template <class T>
  Section<T> device(size_t n) {  // on the device only: no pinned mirror, so these come after every mirrored section
    return {this, add(0, n * sizeof(T))};
  }
  // sizes both arenas and resolves the sections.  Refuses a layout in which a copy would overwrite live bytes with stale
  // ones: a section that lies inside the upload (download) span has to be an uploaded (downloaded) one itself
  int commit();
  // last_bytes: how much of the last uploaded section has been filled (the copy ends there)
  int upload(size_t last_bytes = kAll);
  template <class T>
  int upload(const Section<T>& s) {  // that section alone, again
    return copy(rec_[s.index].off, rec_[s.index].bytes, true);
  }
  int download();

 private:
  enum { kUp = 1, kDown = 2, kMaxSections = 10 };
  struct Rec {
    size_t off, bytes;
    int flags;
  };
  int add(int flags, size_t bytes) {
    if (n_ < kMaxSections) {
      rec_[n_] = {end_, bytes, flags};
      end_ += align256(bytes);
    }
    return n_++;
  }
  int copy(size_t off, size_t bytes, bool to_device);
  prs_context* ctx_;
  const char* entry_;
  Arena arena_;
  Rec rec_[kMaxSections];
  int n_                = 0;
  size_t end_           = 0;
  int first_[2]         = {-1, -1}, last_[2] = {-1, -1};  // the up [0] and down [1] spans, by section
  unsigned char *h_ = nullptr, *d_ = nullptr;
};

// device table scale[n] = n > 2 ? 1 + log(n) : 1 for n < 4096 (built once per context)
const float* ctx_info_scale_table(prs_context* ctx);
// diagnostic: device buffer for phase stamps when PRS_STAMPS=1, else nullptr
unsigned long long* ctx_stamps(prs_context* ctx, size_t bytes);
// synchronises and prints mean per-phase cycle counts (n_stamps consecutive stamps per block)
void ctx_report_stamps(prs_context* ctx, int blocks, int n_stamps, const char* legend, bool raw = false, size_t first_block = 0);  // raw: the words are per-phase totals, not cumulative stamps

// ---- dispatch: plan, then launch.  The five launchers that choose among kernel instantiations (stereo matcher, v5 matcher, aligner,
// brute-force matcher, merger) each have a *_plan function next to them: pure host code (no HIP call, no getenv, no context, no
// batch pointer followed) from the parameter structs, the batch descriptor's strides / counts / which optional pointers are set
// and a DispatchEnv to a plan -- a refusal, or the launches (kernel = index into the family's variant table, grid, block, dynamic
// LDS bytes) plus the kernel argument struct with every layout field set.  Plan::add checks every grid it takes (prs_launch.h), so a
// plan that is PRS_OK holds launches HIP accepts.  The launcher validates pointers, takes the plan, allocates what the plan sizes,
// adds the pointers and launches through launch_planned.  The prs_*_plan entry points show the same plans to tests.
using DispatchEnv = prs_dispatch_env;  // everything outside the arguments a dispatch depends on
// the context's knobs and CU count, and the two brute-force switches from the environment as it is now
DispatchEnv dispatch_env(const prs_context* ctx);

// one kernel instantiation: the function and its name as a kernel trace prints it, both from ONE template-argument list; key = that
// list as integers, which is how a plan finds the entry (find_variant) once it has worked out the arguments it wants
template <class Args>
struct Variant {
  void (*fn)(Args);
  const char* name;
  int key[6];
};
#define PRS_VARIANT(scope, kernel, args, ...) \
  { kernel<__VA_ARGS__>, "void " scope #kernel "<" #__VA_ARGS__ ">(" scope #args ")", { __VA_ARGS__ } }
#define PRS_VARIANT_PLAIN(scope, kernel, args, id) \
  { kernel, scope #kernel "(" scope #args ")", { id } }
template <class Args, size_t N>
inline int find_variant(const Variant<Args> (&table)[N], const int (&key)[6]) {
  for (size_t i = 0; i < N; ++i) {
    bool same = true;
    for (int k = 0; k < 6; ++k) {
      same = same && table[i].key[k] == key[k];
    }
    if (same) {
      return (int) i;
    }
  }
  return -1;  // (a plan turns this into a refusal: a missing instantiation is an error, never another kernel)
}

struct Plan {
  int status          = PRS_OK;
  const char* message = nullptr;
  int n_launches      = 0;  // 0 with PRS_OK: an empty batch
  const char* too_large = "dispatch: more work-items than one launch holds";  // (each family puts its entry point's name in front)
  struct Launch {
    int kernel;  // index into the family's variant table
    Grid grid;
    size_t lds;
  } launch[PRS_PLAN_MAX_LAUNCHES];
  void refuse(int code, const char* what) {
    status     = code;
    message    = what;
    n_launches = 0;
  }
  void add(int kernel, int64_t grid_x, int64_t grid_y, int block, size_t lds) {
    const Grid grid = Grid::checked(grid_x, grid_y, 1, block);
    if (kernel < 0) {
      refuse(PRS_ERR_UNSUPPORTED, "dispatch: no kernel instantiation for this shape");
    } else if (!grid) {
      refuse(PRS_ERR_UNSUPPORTED, too_large);
    } else if (status == PRS_OK) {
      launch[n_launches++] = {kernel, grid, lds};
    }
  }
};
// status, message and launches of a plan in the ABI's form (facts zeroed: the family's entry point fills them)
template <class Args, size_t N>
inline void export_plan(const Plan& p, const Variant<Args> (&table)[N], prs_dispatch_plan* out) {
  *out            = prs_dispatch_plan{};
  out->status     = p.status;
  out->message    = p.message;
  out->n_launches = p.n_launches;
  for (int i = 0; i < p.n_launches; ++i) {
    const Plan::Launch& l = p.launch[i];
    out->launch[i]        = {table[l.kernel].name, (int32_t) l.grid.x(), (int32_t) l.grid.y(), (int32_t) l.grid.threads(), (uint32_t) l.lds};
  }
}
// the index-th name of each family's variant tables, nullptr past the end (prs_dispatch_kernel_name)
const char* stereo_kernel_name(int index);
const char* align_kernel_name(int index);
const char* bruteforce_kernel_name(int index);
const char* merge_kernel_name(int index);
// exact integer form of `best < max_distance && best / second < max_ratio` (epipolar_impl.cpp:171-173),
// evaluated on the host with the same IEEE float operations the reference performs:
// accept iff best < *best_lim && best <= bmax[second] (index 257 = no second candidate)
void fill_accept_table(const prs_stereo_params* params, int* best_lim, int16_t* bmax258);
// The stereo matcher's two generations live in two translation units; stereo_plan (stereo_match.hip) decides between them in one
// place and asks the v5 unit for its kernel's layout: `why` says whether the shape is v5's (kV5Taken) or what keeps it out
enum { kV5Taken = 0, kV5Stride, kV5Knob, kV5Cap, kV5Lds, kV5BestLim };
constexpr int kStereoV5Variants = 8;
struct StereoV5Layout {
  int why    = kV5Taken;
  int kernel = -1;  // index into the v5 variant table
  int cap = 0, nwords = 0, pool_cap = 0;
  uint32_t off_desc_r = 0, off_kp_r = 0, off_sorted_l = 0, off_sorted_r = 0, off_bucket = 0, off_hist = 0, off_rs = 0, off_len = 0, off_rowcnt = 0,
           off_out = 0, off_bits = 0, off_misc = 0, off_tab = 0, off_pool = 0;
  uint32_t lds = 0;  // dynamic LDS bytes (the arrays alone when they do not fit)
};
StereoV5Layout stereo_v5_layout(const prs_stereo_params& params, int stride, bool epilogue, int best_lim, const DispatchEnv& env);
const char* stereo_v5_kernel_name(int index);
int stereo_match_v5_launch(prs_context* ctx, const prs_stereo_params* params, const prs_stereo_batch* batch, const StereoV5Layout& layout,
                           const Plan::Launch& launch);
int stereo_match_batch_launch(prs_context* ctx, const prs_stereo_params* params, const prs_stereo_batch* batch);
int align_batch_launch(prs_context* ctx, const prs_pcf_params* finder, const prs_aligner_params* aligner, const prs_align_batch* batch, int mode, int rounds);
int align_batch_finish(prs_context* ctx);
int align_batch_rearm(prs_context* ctx, hipStream_t replay_stream);
bool align_job_active(const prs_context* ctx);
int align_reuse_counts(prs_context* ctx, long long* hits, long long* misses);
int gn_step_launch(prs_context* ctx, const float* dH, const float* db, float damping, int damping_form, float* dX, int* dok);
int recip_selftest_launch(prs_context* ctx, unsigned long long* d_counts);
int bruteforce_batch_launch(prs_context* ctx, const prs_bruteforce_params* params, const prs_bruteforce_batch* batch);
int selection_order_launch(prs_context* ctx, const uint8_t* response_dev, int n, int32_t* order_dev, int32_t* status_dev);
int extract_features_launch(prs_context* ctx, const prs_extractor_params* params, const prs_extract_batch* batch);
// descriptors of keypoints another unit selected: that unit declares these grids among its own, checks, and launches last
struct DescribeGrids {
  Grid tiles, describe;
  int chunks = 0;
};
DescribeGrids describe_selected_grids(Launches& on, const prs_extract_batch& batch);
int describe_selected_launch(prs_context* ctx, const Launches& on, const DescribeGrids& grids, const prs_extract_batch* batch, uint32_t* kept);
int selective_extract_launch(prs_context* ctx, const prs_selective_extractor_params* params, const prs_selective_extract_batch* batch);
int depth_measurements_launch(prs_context* ctx, const prs_depth_params* params, const prs_depth_batch* batch);
int point_align_launch(prs_context* ctx, const prs_point_align_params* params, const prs_point_align_pairs* batch);
int pose_graph_launch(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs);
int pose_graph_lm_launch(prs_context* ctx, const prs_pose_graph_lm_params* params, const prs_pose_graphs* graphs,
                         prs_pose_graph_lm_result* result);
int pose_graph_append_launch(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs,
                             const prs_pose_graph_closures* closures);
int session_step_launch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch);
int session_unroll_launch(prs_context* ctx, const prs_session_batch* batch, float* out);
int session_step_archive_launch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch,
                                const prs_merge_batch* maps, const prs_map_archive* archive);
int session_reenter_launch(prs_context* ctx, const prs_reentry_params* params, const prs_session_batch* batch, const prs_merge_batch* maps,
                           const prs_map_archive* archive, const prs_reentry_batch* reentry);
int trajectory_eval_launch(prs_context* ctx, const prs_trajectory_params* params, const prs_trajectory_batch* batch);
int world_map_launch(prs_context* ctx, const prs_world_map_params* params, const prs_session_batch* session, const prs_merge_batch* maps,
                     const prs_map_archive* archive, const prs_world_map_batch* out);
int world_voxel_launch(prs_context* ctx, const prs_world_voxel_params* params, const prs_world_voxel_batch* batch);
int depth_cloud_launch(prs_context* ctx, const prs_depth_cloud_params* params, const prs_depth_cloud_batch* batch);
int dense_stereo_launch(prs_context* ctx, const prs_dense_stereo_params* params, const prs_dense_stereo_batch* batch);
// dense stereo's census and finish launches, shared with the semi-global stage (checked batches only): *_blocks is the grid the
// caller declares, at kDenseThreads a workgroup, and has checked when it enqueues
constexpr int kDenseThreads = 256;
int64_t dense_census_blocks(const prs_dense_stereo_batch& o);
int64_t dense_finish_blocks(const prs_dense_stereo_batch& o);
void dense_census_enqueue(const Launches& on, const Grid& grid, const prs_dense_stereo_batch& o, uint64_t* census_l, uint64_t* census_r);
void dense_finish_enqueue(const Launches& on, const Grid& grid, const prs_dense_stereo_params& p, const prs_dense_stereo_batch& o, uint2* rec_l,
                          int16_t* win_r);
// what a dense and a semi-global call share on the host.  The checks of both entry points in their order and words: pointers, parameters
// (stage_ok / stage_rule: the stage's own fields and how the refusal names them), sizes (stage_size / stage_size_name: one more that
// must be at least 1) and pitches, alignment, pixel count.  And the workspace's parts in bytes, pixels 0 for a size the launchers refuse
int stereo_call_check(prs_context* ctx, const std::string& who, const prs_dense_stereo_params& p, const prs_dense_stereo_batch& o, bool stage_ok,
                      const char* stage_rule, int64_t stage_size = 1, const char* stage_size_name = "");
struct DenseLayout {
  uint64_t pixels, census, rec, right, total;
};
DenseLayout dense_layout_of(int64_t batch, int64_t frames, int64_t rows, int64_t cols, int64_t n_disparities, bool lr);
int sgm_stereo_launch(prs_context* ctx, const prs_sgm_stereo_params* params, const prs_sgm_stereo_batch* batch);
int speckle_launch(prs_context* ctx, const prs_speckle_params* params, const prs_speckle_batch* batch);
int depth_consistency_launch(prs_context* ctx, const prs_depth_consistency_params* params, const prs_depth_consistency_batch* batch);
int pose_compose_launch(prs_context* ctx, int batch, const float* prediction, const float* X, float* pose_out);
int motion_predict_launch(prs_context* ctx, int batch, const float* prev2, const float* prev1, float* pred);
int merge_batch_launch(prs_context* ctx, const prs_merger_params* params, const prs_merge_batch* batch);
int closure_merge_launch(prs_context* ctx, const prs_closure_merger_params* params, const prs_closure_merge_batch* batch);
int scene_clip_launch(prs_context* ctx, const prs_projector* projector, const float* sensor_in_robot, const prs_clip_batch* batch);
int triangulate_launch(prs_context* ctx, const prs_triangulator_params* params, const float* d_uvuv, int64_t n, float* d_xyz4);

} // namespace prs
