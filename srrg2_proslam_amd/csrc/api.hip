// api.hip -- extern "C" boundary of libproslam_hip.so (declared in include/proslam_hip.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "prs_host.h"

namespace prs {

int ctx_fail(prs_context* ctx, int status, const char* what) {
  if (ctx) {
    ctx->last_error = what ? what : "";
  }
  return status;
}

int ctx_fail_hip(prs_context* ctx, hipError_t e, const char* what) {
  if (ctx) {
    ctx->last_error = std::string(what ? what : "") + ": " + hipGetErrorString(e);
  }
  return PRS_ERR_HIP;
}

namespace {

// the two bands of a live block against PRS_GUARD_PATTERN: appends "name front|tail offset" for each damaged one.  The caller has
// drained the streams that use the block
hipError_t guard_examine(const GuardBlock& b, std::vector<std::string>* found) {
  const size_t front = PRS_GUARD_BAND;
  std::vector<unsigned char> host;
  const unsigned char* base = static_cast<const unsigned char*>(b.user) - front;
  const unsigned char* band[2] = {base, static_cast<const unsigned char*>(b.user) + b.bytes};
  const size_t len[2]          = {front, b.tail};
  for (int side = 0; side < 2; ++side) {
    const unsigned char* seen = band[side];
    if (!b.pinned) {
      host.resize(len[side]);
      const hipError_t e = hipMemcpy(host.data(), band[side], len[side], hipMemcpyDeviceToHost);
      if (e != hipSuccess) {
        return e;
      }
      seen = host.data();
    }
    for (size_t i = 0; i < len[side]; ++i) {
      if (seen[i] != PRS_GUARD_PATTERN) {
        found->push_back(std::string(b.name) + (side == 0 ? " front " : " tail ") + std::to_string(i));
        break;
      }
    }
  }
  return hipSuccess;
}

}  // namespace

hipError_t owned_alloc(prs_context* ctx, const char* name, void** p, size_t bytes, int rule, bool pinned) {
  *p                     = nullptr;
  const bool guard       = ctx->guard_fill >= 0;
  const prs_guard_extent x = guard_layout(bytes, rule, guard);
  void* base             = nullptr;
  hipError_t e           = pinned ? hipHostMalloc(&base, x.total, hipHostMallocDefault) : hipMalloc(&base, x.total);
  if (e != hipSuccess || !guard) {
    *p = e == hipSuccess ? base : nullptr;
    return e;
  }
  unsigned char* b = static_cast<unsigned char*>(base);
  if (pinned) {
    memset(b, PRS_GUARD_PATTERN, x.user_offset);
    memset(b + x.user_offset, ctx->guard_fill, bytes);
    memset(b + x.user_offset + bytes, PRS_GUARD_PATTERN, x.tail_bytes);
  } else {
    e = hipMemsetAsync(b, PRS_GUARD_PATTERN, x.user_offset, ctx->stream);
    if (e == hipSuccess && bytes > 0) {
      e = hipMemsetAsync(b + x.user_offset, ctx->guard_fill, bytes, ctx->stream);
    }
    if (e == hipSuccess) {
      e = hipMemsetAsync(b + x.user_offset + bytes, PRS_GUARD_PATTERN, x.tail_bytes, ctx->stream);
    }
    if (e == hipSuccess) {
      e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
      (void) hipFree(base);
      return e;
    }
  }
  ctx->guard_blocks.push_back({b + x.user_offset, bytes, (size_t) x.tail_bytes, name, pinned});
  *p = b + x.user_offset;
  return hipSuccess;
}

void owned_free(prs_context* ctx, void* p, bool pinned) {
  if (!p) {
    return;
  }
  if (ctx->guard_fill >= 0) {
    for (size_t i = 0; i < ctx->guard_blocks.size(); ++i) {
      if (ctx->guard_blocks[i].user == p) {
        // the evidence goes with the block: look at it first (a copy that fails is latched as such)
        if (guard_examine(ctx->guard_blocks[i], &ctx->guard_latched) != hipSuccess) {
          (void) hipGetLastError();
          ctx->guard_latched.push_back(std::string(ctx->guard_blocks[i].name) + " unreadable 0");
        }
        pinned = ctx->guard_blocks[i].pinned;
        ctx->guard_blocks.erase(ctx->guard_blocks.begin() + (ptrdiff_t) i);
        p = static_cast<unsigned char*>(p) - PRS_GUARD_BAND;
        break;
      }
    }
  }
  (void) (pinned ? hipHostFree(p) : hipFree(p));
}

void owned_repaint(prs_context* ctx, void* p, size_t bytes, hipStream_t stream, bool pinned) {
  if (ctx->guard_fill < 0 || !p || bytes == 0) {
    return;
  }
  if (pinned) {
    (void) hipStreamSynchronize(ctx->stream);  // (an entry point has synchronised before it returned; a copy still in flight would be a finding of its own)
    memset(p, ctx->guard_fill, bytes);
  } else {
    (void) hipMemsetAsync(p, ctx->guard_fill, bytes, stream);
  }
}

static const char* const kArenaName[ARENA_COUNT] = {"arena.work0", "arena.work1", "arena.work2", "arena.work3", "arena.stage",
                                                    "arena.stage_bruteforce", "arena.stage_solver", "arena.stage_pose_graph", "arena.pinned"};

void* ctx_arena(prs_context* ctx, Arena arena, size_t bytes) {
  auto& a           = ctx->arena[arena];
  const bool pinned = arena == ARENA_PINNED;
  if (bytes <= a.size) {
    // what a work or staging arena holds belongs to whatever call runs next: guard mode paints the request again
    owned_repaint(ctx, a.p, bytes, ctx->stream, pinned);
    return a.p;
  }
  if (a.p) {
    (void) hipStreamSynchronize(ctx->stream);  // whatever was enqueued on the old block finishes before it goes
    owned_free(ctx, a.p, pinned);
    a.p    = nullptr;
    a.size = 0;
  }
  // slack: the default staging pair grows by half, the work arenas and the two small staging arenas by a quarter
  const int rule = arena == ARENA_STAGE || pinned ? PRS_GUARD_SLACK_HALF : PRS_GUARD_SLACK_QUARTER;
  void* p        = nullptr;
  if (owned_alloc(ctx, kArenaName[arena], &p, bytes, rule, pinned) != hipSuccess) {
    return nullptr;
  }
  a.p    = p;
  a.size = ctx->guard_fill >= 0 ? bytes : (size_t) guard_layout(bytes, rule, false).total;  // (guard mode: the tail band begins behind the request)
  return p;
}

int Staging::commit() {
  if (n_ > kMaxSections) {
    return ctx_fail(ctx_, PRS_ERR_UNSUPPORTED, (std::string(entry_) + ": too many staging sections").c_str());
  }
  size_t mirrored = 0;
  for (int i = 0; i < n_; ++i) {
    for (int k = 0; k < 2; ++k) {
      if (rec_[i].flags & (k == 0 ? kUp : kDown)) {
        first_[k] = first_[k] < 0 ? i : first_[k];
        last_[k]  = i;
      }
    }
    if (rec_[i].flags) {
      mirrored = rec_[i].off + align256(rec_[i].bytes);
    }
  }
  for (int k = 0; k < 2; ++k) {
    for (int i = first_[k]; i < last_[k]; ++i) {
      if (rec_[i].bytes > 0 && !(rec_[i].flags & (k == 0 ? kUp : kDown))) {
        return ctx_fail(ctx_, PRS_ERR_UNSUPPORTED, (std::string(entry_) + ": a staging section lies inside a copy it is not part of").c_str());
      }
    }
  }
  d_ = static_cast<unsigned char*>(ctx_arena(ctx_, arena_, end_));
  h_ = static_cast<unsigned char*>(ctx_arena(ctx_, ARENA_PINNED, mirrored));
  if (!d_ || !h_) {
    return ctx_fail(ctx_, PRS_ERR_HIP, (std::string(entry_) + ": scratch allocation failed").c_str());
  }
  return PRS_OK;
}

int Staging::copy(size_t off, size_t bytes, bool to_device) {
  hipError_t e = to_device ? hipMemcpyAsync(d_ + off, h_ + off, bytes, hipMemcpyHostToDevice, ctx_->stream)
                           : hipMemcpyAsync(h_ + off, d_ + off, bytes, hipMemcpyDeviceToHost, ctx_->stream);
  if (e == hipSuccess && !to_device) {
    e = hipStreamSynchronize(ctx_->stream);
  }
  return e == hipSuccess ? PRS_OK : ctx_fail_hip(ctx_, e, (std::string(entry_) + (to_device ? " upload" : " download")).c_str());
}

int Staging::upload(size_t last_bytes) {
  const Rec &a = rec_[first_[0]], &b = rec_[last_[0]];
  return copy(a.off, b.off + (last_bytes == kAll ? b.bytes : last_bytes) - a.off, true);
}

int Staging::download() {
  const Rec &a = rec_[first_[1]], &b = rec_[last_[1]];
  return copy(a.off, b.off + b.bytes - a.off, false);
}

const float* ctx_info_scale_table(prs_context* ctx) {
  if (!ctx->d_info_lut) {
    constexpr int kN = 4096;
    uint32_t n[kN];
    float scale[kN];
    for (int i = 0; i < kN; ++i) {
      n[i] = (uint32_t) i;
    }
    prs_info_scale_from_nopt(n, kN, scale);
    float* d = nullptr;
    if (owned_alloc(ctx, "info_lut", &d, sizeof(scale)) != hipSuccess) {
      return nullptr;
    }
    if (hipMemcpy(d, scale, sizeof(scale), hipMemcpyHostToDevice) != hipSuccess) {
      owned_free(ctx, d);
      return nullptr;
    }
    ctx->d_info_lut = d;
  }
  return ctx->d_info_lut;
}

unsigned long long* ctx_stamps(prs_context* ctx, size_t bytes) {
  if (!ctx->stamps_enabled) {
    return nullptr;
  }
  if (bytes > ctx->d_stamps_size) {
    if (ctx->d_stamps) {
      owned_free(ctx, ctx->d_stamps);
    }
    if (owned_alloc(ctx, "stamps", &ctx->d_stamps, bytes) != hipSuccess) {
      ctx->d_stamps      = nullptr;
      ctx->d_stamps_size = 0;
      return nullptr;
    }
    ctx->d_stamps_size = bytes;
  }
  return ctx->d_stamps;
}

void ctx_report_stamps(prs_context* ctx, int blocks, int n_stamps, const char* legend, bool raw, size_t first_block) {
  (void) hipStreamSynchronize(ctx->stream);
  std::vector<unsigned long long> h((size_t) blocks * 16);
  (void) hipMemcpy(h.data(), ctx->d_stamps + first_block * 16, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  fprintf(stderr, "[prs stamps] %s\n[prs stamps] mean cycles per phase over %d blocks:", legend, blocks);
  double total = 0;
  for (int i = 1; i < n_stamps; ++i) {
    double acc = 0;
    for (int b = 0; b < blocks; ++b) {
      acc += raw ? (double) h[(size_t) b * 16 + i] : (double) (h[(size_t) b * 16 + i] - h[(size_t) b * 16 + i - 1]);
    }
    fprintf(stderr, " %.0f", acc / blocks);
    total += acc / blocks;
  }
  fprintf(stderr, " | total %.0f\n", total);
}

DispatchEnv dispatch_env(const prs_context* ctx) {
  DispatchEnv env;
  env.cus            = ctx->cus;
  env.fused_align    = ctx->fused_align;
  env.matcher_v3     = ctx->matcher_v3;
  env.force_unstaged = ctx->force_unstaged;
  env.no_lone_gn     = ctx->no_lone_gn;
  env.merge_fused    = ctx->merge_fused;
  env.bf_mfma        = ctx->bf_mfma;
  env.stamps         = ctx->stamps_enabled;
  env.stamps_split   = ctx->stamps_split;
  env.no_search_reuse = ctx->no_search_reuse;
  // (tests and A-B runs set these two after the library is loaded: read per launch)
  env.bf_global_state   = getenv("PRS_BF_GLOBAL_STATE") != nullptr;
  const char* two_wg    = getenv("PRS_BF_TWO_WORKGROUPS");
  env.bf_two_workgroups = two_wg ? (two_wg[0] == '1' ? 1 : 0) : -1;
  return env;
}

} // namespace prs

using namespace prs;

extern "C" {

int prs_version(void) {
  return PRS_ABI_VERSION;  // prs_aligner_params grew at its end: round 5 kernel_weight_form, damping_form, translation_weight_form; round 6 step_norm_exit
}

int prs_launch_fits(int64_t workgroups, int32_t threads) {
  return grid_fits(workgroups, threads) ? 1 : 0;
}

int prs_abi_check(int32_t header_version, uint64_t sizeof_stereo_params, uint64_t sizeof_pcf_params, uint64_t sizeof_aligner_params,
                  uint64_t sizeof_align_batch) {
  // (no context: the answer is the status alone)
  if (header_version != PRS_ABI_VERSION || sizeof_stereo_params != sizeof(prs_stereo_params) || sizeof_pcf_params != sizeof(prs_pcf_params) ||
      sizeof_aligner_params != sizeof(prs_aligner_params) || sizeof_align_batch != sizeof(prs_align_batch)) {
    return PRS_ERR_UNSUPPORTED;
  }
  return PRS_OK;
}

const char* prs_status_string(int status) {
  switch (status) {
    case PRS_OK: return "ok";
    case PRS_ERR_NULL: return "required input/output buffer not set";
    case PRS_ERR_CAPACITY: return "output capacity too small";
    case PRS_ERR_HIP: return "HIP runtime error";
    case PRS_ERR_RANGE: return "input outside the supported coordinate domain";
    case PRS_ERR_UNSUPPORTED: return "size beyond kernel limits";
    case PRS_ERR_NO_DEVICE: return "no HIP device";
    case PRS_ERR_HISTORY: return "measurement history of a landmark is full";
    case PRS_ERR_SCENE_FULL: return "map capacity exhausted";
    case PRS_ERR_DUPLICATE: return "scene index referenced by two correspondences";
    case PRS_ERR_NOT_POSITIVE_DEFINITE: return "normal matrix of the pose graph is not positive definite";
    default: return status > 0 ? "warning bits set" : "unknown error";
  }
}

int prs_context_create(int device_id, prs_context** out) {
  if (!out) {
    return PRS_ERR_NULL;
  }
  *out      = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    return PRS_ERR_NO_DEVICE;  // loud: there is no CPU fallback behind this library
  }
  if (device_id < 0 || device_id >= count) {
    return PRS_ERR_NO_DEVICE;
  }
  if (hipSetDevice(device_id) != hipSuccess) {
    return PRS_ERR_HIP;
  }
  prs_context* ctx = new prs_context();
  ctx->device      = device_id;
  if (hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return PRS_ERR_HIP;
  }
  ctx->stream          = ctx->own;
  int cus              = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) {
    ctx->cus = cus;
  }
  const char* unstaged = getenv("PRS_FORCE_UNSTAGED");
  ctx->force_unstaged  = unstaged && unstaged[0] == '1';
  const char* v3       = getenv("PRS_MATCHER_V3");
  ctx->matcher_v3      = v3 && v3[0] == '1';
  const char* fused    = getenv("PRS_FUSED_ALIGN");
  ctx->fused_align     = fused && fused[0] == '1';
  const char* stamps   = getenv("PRS_STAMPS");
  ctx->stamps_enabled  = stamps && stamps[0] == '1';
  const char* ssplit   = getenv("PRS_STAMPS_SPLIT");
  ctx->stamps_split    = ssplit && ssplit[0] == '1';
  const char* nopre    = getenv("PRS_NO_PREFILTER");
  ctx->no_prefilter    = nopre && nopre[0] == '1';
  const char* noreuse  = getenv("PRS_NO_SEARCH_REUSE");
  ctx->no_search_reuse = noreuse && noreuse[0] == '1';
  const char* nolone   = getenv("PRS_NO_LONE_GN");
  ctx->no_lone_gn      = nolone && nolone[0] == '1';
  const char* p96      = getenv("PRS_PREFILTER_96_LIMIT");
  ctx->prefilter_96_limit = p96 ? atoi(p96) : 32;
  const char* bfm      = getenv("PRS_BF_MFMA");
  ctx->bf_mfma         = !bfm || bfm[0] == 'a' ? PRS_BF_DENSE_MATRIX_WHEN_FULL : (bfm[0] == '1' ? PRS_BF_DENSE_MATRIX : PRS_BF_DENSE_POPCOUNT);
  const char* mfused   = getenv("PRS_MERGE_FUSED");
  ctx->merge_fused     = mfused && mfused[0] == '1';
  const char* gfill    = getenv("PRS_GUARD_FILL");  // guard mode (tests): "00" or "ff", anything else is off
  ctx->guard_fill      = gfill && !strcmp(gfill, "00") ? 0x00 : (gfill && !strcmp(gfill, "ff") ? 0xFF : -1);
  *out                 = ctx;
  return PRS_OK;
}

int prs_context_get_dispatch_env(const prs_context* ctx, prs_dispatch_env* env) {
  if (!ctx || !env) {
    return PRS_ERR_NULL;
  }
  *env = dispatch_env(ctx);
  return PRS_OK;
}

const char* prs_dispatch_kernel_name(int32_t family, int32_t index) {
  switch (family) {
    case PRS_DISPATCH_STEREO: return stereo_kernel_name(index);
    case PRS_DISPATCH_ALIGN: return align_kernel_name(index);
    case PRS_DISPATCH_BRUTEFORCE: return bruteforce_kernel_name(index);
    case PRS_DISPATCH_MERGE: return merge_kernel_name(index);
    default: return nullptr;
  }
}

void prs_dispatch_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_dispatch_env);
  sizes2[1] = sizeof(prs_dispatch_plan);
}

int prs_context_destroy(prs_context* ctx) {
  if (!ctx) {
    return PRS_OK;
  }
  (void) hipSetDevice(ctx->device);
  (void) hipStreamSynchronize(ctx->stream);
  if (ctx->align_job && ctx->align_job_free) {
    ctx->align_job_free(ctx->align_job);
  }
  owned_free(ctx, ctx->d_stamps);
  owned_free(ctx, ctx->d_info_lut);
  for (int i = 0; i < ARENA_COUNT; ++i) {
    owned_free(ctx, ctx->arena[i].p, i == ARENA_PINNED);
  }
  // guard mode: every block has been looked at before it went; what was damaged does not leave silently with the context
  const int damaged = (int) ctx->guard_latched.size();
  for (const std::string& v : ctx->guard_latched) {
    fprintf(stderr, "[prs guard] damaged band: %s\n", v.c_str());
  }
  if (ctx->own) {
    (void) hipStreamDestroy(ctx->own);
  }
  for (hipEvent_t e : ctx->timing_ev) {
    if (e) {
      (void) hipEventDestroy(e);
    }
  }
  delete ctx;
  return damaged;
}

int prs_guard_layout(uint64_t bytes, int32_t slack_rule, int32_t guard, prs_guard_extent* out) {
  if (!out) {
    return PRS_ERR_NULL;
  }
  if (slack_rule != PRS_GUARD_SLACK_EXACT && slack_rule != PRS_GUARD_SLACK_QUARTER && slack_rule != PRS_GUARD_SLACK_HALF) {
    return PRS_ERR_UNSUPPORTED;
  }
  *out = guard_layout(bytes, slack_rule, guard != 0);
  return PRS_OK;
}

void prs_guard_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_guard_extent);
  sizes2[1] = sizeof(prs_guard_region);
}

int prs_context_guard_regions(prs_context* ctx, prs_guard_region* out, int32_t capacity) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (ctx->guard_fill < 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_context_guard_regions: the context is not in guard mode (PRS_GUARD_FILL=00 or ff at prs_context_create)");
  }
  const int32_t n = (int32_t) ctx->guard_blocks.size();
  for (int32_t i = 0; out && i < n && i < capacity; ++i) {
    const GuardBlock& b = ctx->guard_blocks[(size_t) i];
    prs_guard_region r;
    memset(&r, 0, sizeof(r));
    r.user       = b.user;
    r.bytes      = b.bytes;
    r.tail_bytes = b.tail;
    r.pinned     = b.pinned ? 1 : 0;
    strncpy(r.name, b.name, sizeof(r.name) - 1);
    out[i] = r;
  }
  return n;
}

int prs_context_guard_check(prs_context* ctx, char* report, uint64_t report_bytes) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (ctx->guard_fill < 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_context_guard_check: the context is not in guard mode (PRS_GUARD_FILL=00 or ff at prs_context_create)");
  }
  (void) hipSetDevice(ctx->device);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  std::vector<std::string> found = ctx->guard_latched;
  for (size_t i = 0; e == hipSuccess && i < ctx->guard_blocks.size(); ++i) {
    e = guard_examine(ctx->guard_blocks[i], &found);
  }
  if (e != hipSuccess) {
    return ctx_fail_hip(ctx, e, "prs_context_guard_check");
  }
  if (report && report_bytes > 0) {
    std::string text;
    for (const std::string& v : found) {
      text += v + "\n";
    }
    const size_t n = text.size() < report_bytes - 1 ? text.size() : (size_t) report_bytes - 1;
    memcpy(report, text.data(), n);
    report[n] = 0;
  }
  return (int) found.size();
}

int prs_context_set_bruteforce_dense_phase(prs_context* ctx, int32_t mode) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (mode != PRS_BF_DENSE_POPCOUNT && mode != PRS_BF_DENSE_MATRIX_WHEN_FULL && mode != PRS_BF_DENSE_MATRIX) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_context_set_bruteforce_dense_phase: mode must be one of PRS_BF_DENSE_*");
  }
  ctx->bf_mfma = mode;
  return PRS_OK;
}

int prs_context_enable_timing(prs_context* ctx, int32_t on) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  ctx->timing      = on != 0;
  ctx->t_search_ms = ctx->t_gn_ms = 0.0;
  ctx->n_search = ctx->n_gn = 0;
  for (int i = 0; i < 16; ++i) {
    ctx->t_search_round[i] = ctx->t_gn_round[i] = 0.0;
  }
  ctx->n_batches_timed = 0;
  return PRS_OK;
}

int prs_context_get_align_round_timing(prs_context* ctx, double* search_ms16, double* gn_ms16, int64_t* batches) {
  if (!ctx || !search_ms16 || !gn_ms16 || !batches) {
    return PRS_ERR_NULL;
  }
  for (int i = 0; i < 16; ++i) {
    search_ms16[i] = ctx->t_search_round[i];
    gn_ms16[i]     = ctx->t_gn_round[i];
  }
  *batches = ctx->n_batches_timed;
  return PRS_OK;
}

int prs_context_get_align_timing(prs_context* ctx, double* search_ms, double* gn_ms, int64_t* search_launches, int64_t* gn_launches) {
  if (!ctx || !search_ms || !gn_ms || !search_launches || !gn_launches) {
    return PRS_ERR_NULL;
  }
  *search_ms       = ctx->t_search_ms;
  *gn_ms           = ctx->t_gn_ms;
  *search_launches = ctx->n_search;
  *gn_launches     = ctx->n_gn;
  return PRS_OK;
}

int prs_context_get_search_reuse(prs_context* ctx, int64_t* hits, int64_t* misses) {
  if (!ctx || !hits || !misses) {
    return PRS_ERR_NULL;
  }
  long long h = 0, m = 0;
  const int rc = align_reuse_counts(ctx, &h, &m);
  *hits        = h;
  *misses      = m;
  return rc;
}

int prs_context_set_stream(prs_context* ctx, void* hip_stream) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (align_job_active(ctx)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_context_set_stream: an enqueued aligner batch has not been finished (prs_align_batch_finish)");
  }
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);  // NULL = HIP's default (null) stream
  return PRS_OK;
}

int prs_context_use_own_stream(prs_context* ctx) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  ctx->stream = ctx->own;
  return PRS_OK;
}

int prs_context_synchronize(prs_context* ctx) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  hipError_t e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? PRS_OK : ctx_fail_hip(ctx, e, "hipStreamSynchronize");
}

const char* prs_last_error(const prs_context* ctx) {
  return ctx ? ctx->last_error.c_str() : "null context";
}

int prs_stereo_match_batch(prs_context* ctx, const prs_stereo_params* params, const prs_stereo_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return stereo_match_batch_launch(ctx, params, batch);
}

int prs_stereo_match(prs_context* ctx,
                     const prs_stereo_params* params,
                     const prs_kp2* left,
                     const uint8_t* desc_left,
                     int32_t n_left,
                     const prs_kp2* right,
                     const uint8_t* desc_right,
                     int32_t n_right,
                     prs_corr* out,
                     int32_t capacity,
                     int32_t* n_out) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  // _preCompute contract (CF/..bruteforce_impl.cpp:203-216): unset buffers are hard errors
  if (!params || !out || !n_out || n_left < 0 || n_right < 0 || (n_left > 0 && (!left || !desc_left)) ||
      (n_right > 0 && (!right || !desc_right))) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_stereo_match: fixed, moving or correspondences not set");
  }
  if (capacity < n_left) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_stereo_match: capacity < n_left");
  }
  (void) hipSetDevice(ctx->device);
  *n_out              = 0;
  const size_t stride = (size_t) (n_left > n_right ? (n_left > 0 ? n_left : 1) : (n_right > 0 ? n_right : 1));
  struct Meta {
    int32_t n_left, n_right, n_matches, status;
  };
  // [ matches | meta | left kp | right kp | left rows | right rows ]: ONE upload of [meta .. the last right row], the launch,
  // ONE download of [matches | meta]
  Staging st(ctx, "prs_stereo_match");
  auto matches = st.down<prs_corr>(stride);
  auto meta    = st.both<Meta>(1);
  auto kp_l    = st.up<prs_kp2>(stride);
  auto kp_r    = st.up<prs_kp2>(stride);
  auto desc_l  = st.up<uint8_t>(PRS_DESC_BYTES * stride);
  auto desc_r  = st.up<uint8_t>(PRS_DESC_BYTES * stride);
  PRS_TRY(st.commit());
  *meta.h() = {n_left, n_right, 0, 0};
  if (n_left > 0) {
    memcpy(kp_l.h(), left, sizeof(prs_kp2) * (size_t) n_left);
    memcpy(desc_l.h(), desc_left, (size_t) PRS_DESC_BYTES * (size_t) n_left);
  }
  if (n_right > 0) {
    memcpy(kp_r.h(), right, sizeof(prs_kp2) * (size_t) n_right);
    memcpy(desc_r.h(), desc_right, (size_t) PRS_DESC_BYTES * (size_t) n_right);
  }
  PRS_TRY(st.upload((size_t) PRS_DESC_BYTES * (size_t) n_right));
  prs_stereo_batch b;
  memset(&b, 0, sizeof(b));
  b.batch      = 1;
  b.stride     = (int32_t) stride;
  b.left_kp    = kp_l.d();
  b.left_desc  = desc_l.d();
  b.n_left     = &meta.d()->n_left;
  b.right_kp   = kp_r.d();
  b.right_desc = desc_r.d();
  b.n_right    = &meta.d()->n_right;
  b.matches    = matches.d();
  b.n_matches  = &meta.d()->n_matches;
  b.status     = &meta.d()->status;
  PRS_TRY(stereo_match_batch_launch(ctx, params, &b));
  PRS_TRY(st.download());
  const Meta& m = *meta.h();
  if (m.status < 0) {
    return ctx_fail(ctx, m.status, "prs_stereo_match: keypoint outside the supported domain (0<=u<32768, 0<=v<image_rows)");
  }
  if (m.n_matches > 0) {
    memcpy(out, matches.h(), sizeof(prs_corr) * (size_t) m.n_matches);
  }
  *n_out = m.n_matches;
  return m.status;
}

int prs_align_batch_run(prs_context* ctx, const prs_pcf_params* finder, const prs_aligner_params* aligner, const prs_align_batch* batch, int32_t mode) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  int rc = align_batch_launch(ctx, finder, aligner, batch, mode, 0);
  if (rc != PRS_OK) {
    return rc;
  }
  if (align_job_active(ctx)) {
    return align_batch_finish(ctx);
  }
  // (the one-launch paths -- finder / linearise modes, the fused kernel -- have nothing enqueued to finish)
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? PRS_OK : ctx_fail_hip(ctx, e, "prs_align_batch_run");
}

int prs_align_batch_enqueue(prs_context* ctx, const prs_pcf_params* finder, const prs_aligner_params* aligner, const prs_align_batch* batch, int32_t rounds) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  // (an explicit round count: the split pipeline, which is what a caller that enqueues -- and may capture -- asked for)
  return align_batch_launch(ctx, finder, aligner, batch, PRS_MODE_ALIGN, rounds > 0 ? rounds : 5);
}

int prs_align_batch_finish(prs_context* ctx) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return align_batch_finish(ctx);
}

int prs_align_batch_rearm(prs_context* ctx) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  return align_batch_rearm(ctx, nullptr);
}

int prs_align_batch_rearm_on(prs_context* ctx, void* hip_stream) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  return align_batch_rearm(ctx, static_cast<hipStream_t>(hip_stream));
}

int prs_triangulate_dev(prs_context* ctx, const prs_triangulator_params* params, const float* d_uvuv, int64_t n, float* d_xyz4) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return triangulate_launch(ctx, params, d_uvuv, n, d_xyz4);
}

int prs_triangulate(prs_context* ctx, const prs_triangulator_params* params, const float* uvuv, int32_t n, float* xyz, uint8_t* valid) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  // triangulator_rigid_stereo.cpp:9-16: unset buffers are reported, nothing is computed
  if (!params || n < 0 || (n > 0 && (!uvuv || !xyz || !valid))) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_triangulate: input or result buffer not set");
  }
  if (n == 0) {
    return PRS_WARN_EMPTY_INPUT;
  }
  (void) hipSetDevice(ctx->device);
  Staging st(ctx, "prs_triangulate");  // [measurements | points]: pinned both ways
  auto in  = st.up<float>(4 * (size_t) n);
  auto pts = st.down<float>(4 * (size_t) n);
  PRS_TRY(st.commit());
  memcpy(in.h(), uvuv, sizeof(float) * 4 * (size_t) n);
  PRS_TRY(st.upload());
  PRS_TRY(triangulate_launch(ctx, params, in.d(), n, pts.d()));
  PRS_TRY(st.download());
  const float* h = pts.h();
  for (int32_t i = 0; i < n; ++i) {
    xyz[3 * i + 0] = h[4 * i + 0];
    xyz[3 * i + 1] = h[4 * i + 1];
    xyz[3 * i + 2] = h[4 * i + 2];
    valid[i]       = h[4 * i + 3] != 0.0f ? 1 : 0;
  }
  return PRS_OK;
}

int prs_scene_clip_batch(prs_context* ctx, const prs_projector* projector, const float* sensor_in_robot16, const prs_clip_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return scene_clip_launch(ctx, projector, sensor_in_robot16, batch);
}

int prs_scene_clip(prs_context* ctx,
                   const prs_projector* projector,
                   const float* robot_in_local_map16,
                   const float* sensor_in_robot16,
                   const float* scene_xyzw,
                   const uint8_t* scene_desc,
                   int32_t n,
                   float* clipped_xyzw,
                   uint8_t* clipped_desc,
                   int32_t* global_indices,
                   int32_t capacity,
                   int32_t* n_clipped) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  // scene_clipper_projective_3d.cpp:12-20: missing projector / clipped scene / global scene throw
  if (!projector) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_scene_clip: missing projector");
  }
  if (!clipped_xyzw || !global_indices || !n_clipped) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_scene_clip: missing clipped scene");
  }
  if (n < 0 || (n > 0 && !scene_xyzw) || !robot_in_local_map16 || !sensor_in_robot16) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_scene_clip: missing global scene");
  }
  if ((scene_desc == nullptr) != (clipped_desc == nullptr)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_scene_clip: descriptor rows need both the scene and the clipped buffer");
  }
  if (n == 0) {
    return PRS_WARN_EMPTY_INPUT;  // :21-28, nothing is cleared
  }
  if (capacity < n) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_scene_clip: output capacity below the scene size");
  }
  (void) hipSetDevice(ctx->device);
  const size_t nn = (size_t) n;
  struct Meta {
    int32_t n_scene, n_clipped, status, pad;
    float robot_in_local_map[16];
  };
  // [inputs: xyzw | desc | meta] [outputs: xyzw | desc | idx]
  Staging st(ctx, "prs_scene_clip");
  auto in_xyzw  = st.up<float>(nn * 4);
  auto in_desc  = st.up<uint8_t>(scene_desc ? nn * PRS_DESC_BYTES : 0);
  auto meta     = st.both<Meta>(1);
  auto out_xyzw = st.down<float>(nn * 4);
  auto out_desc = st.down<uint8_t>(scene_desc ? nn * PRS_DESC_BYTES : 0);
  auto out_idx  = st.down<int32_t>(nn);
  PRS_TRY(st.commit());
  memcpy(in_xyzw.h(), scene_xyzw, nn * 16);
  if (scene_desc) {
    memcpy(in_desc.h(), scene_desc, nn * PRS_DESC_BYTES);
  }
  Meta& m = *meta.h();
  m.n_scene = n, m.n_clipped = 0, m.status = 0, m.pad = 0;
  memcpy(m.robot_in_local_map, robot_in_local_map16, 64);
  PRS_TRY(st.upload());
  prs_clip_batch b;
  b.batch              = 1;
  b.stride             = n;
  b.scene_xyzw         = in_xyzw.d();
  b.scene_desc         = scene_desc ? in_desc.d() : nullptr;
  b.n_scene            = &meta.d()->n_scene;
  b.robot_in_local_map = meta.d()->robot_in_local_map;
  b.clipped_xyzw       = out_xyzw.d();
  b.clipped_desc       = scene_desc ? out_desc.d() : nullptr;
  b.global_indices     = out_idx.d();
  b.n_clipped          = &meta.d()->n_clipped;
  b.status             = &meta.d()->status;
  b.scene_n_opt        = nullptr;
  PRS_TRY(scene_clip_launch(ctx, projector, sensor_in_robot16, &b));
  PRS_TRY(st.download());
  const size_t k = (size_t) m.n_clipped;
  memcpy(clipped_xyzw, out_xyzw.h(), k * 16);
  if (clipped_desc) {
    memcpy(clipped_desc, out_desc.h(), k * PRS_DESC_BYTES);
  }
  memcpy(global_indices, out_idx.h(), k * 4);
  *n_clipped = m.n_clipped;
  return m.status;
}

int prs_bruteforce_match_batch(prs_context* ctx, const prs_bruteforce_params* params, const prs_bruteforce_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return bruteforce_batch_launch(ctx, params, batch);
}

int prs_bruteforce_match(prs_context* ctx,
                         const prs_bruteforce_params* params,
                         const uint8_t* fixed_desc,
                         int32_t n_fixed,
                         const uint8_t* moving_desc,
                         int32_t n_moving,
                         prs_corr* correspondences,
                         int32_t capacity,
                         int32_t* n_correspondences) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  // bruteforce_impl.cpp:203-216: unset buffers throw
  if (!params || n_fixed < 0 || (n_fixed > 0 && !fixed_desc)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_bruteforce_match: fixed not set");
  }
  if (n_moving < 0 || (n_moving > 0 && !moving_desc)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_bruteforce_match: moving not set");
  }
  if (!correspondences || !n_correspondences) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_bruteforce_match: correspondences not set");
  }
  *n_correspondences = 0;
  if (n_fixed == 0 || n_moving == 0) {
    return PRS_WARN_EMPTY_INPUT | PRS_WARN_NO_MATCHES;  // :217-226, :237-242
  }
  const int32_t n_min = n_fixed < n_moving ? n_fixed : n_moving;
  if (capacity < n_min) {
    return ctx_fail(ctx, PRS_ERR_CAPACITY, "prs_bruteforce_match: output capacity below min(n_fixed, n_moving)");
  }
  (void) hipSetDevice(ctx->device);
  struct Meta {
    int32_t n_fixed, n_moving, n_matches, status;
  };
  // (an arena of its own: the block stays live while the launch is repeated below)
  Staging st(ctx, "prs_bruteforce_match", ARENA_STAGE_BRUTEFORCE);
  auto fixed   = st.up<uint8_t>((size_t) n_fixed * PRS_DESC_BYTES);
  auto moving  = st.up<uint8_t>((size_t) n_moving * PRS_DESC_BYTES);
  auto meta    = st.both<Meta>(1);
  auto matches = st.down<prs_corr>((size_t) n_min);
  PRS_TRY(st.commit());
  memcpy(fixed.h(), fixed_desc, (size_t) n_fixed * PRS_DESC_BYTES);
  memcpy(moving.h(), moving_desc, (size_t) n_moving * PRS_DESC_BYTES);
  Meta& m = *meta.h();
  m       = {n_fixed, n_moving, 0, 0};
  PRS_TRY(st.upload());
  prs_bruteforce_batch b;
  b.batch         = 1;
  b.fixed_stride  = n_fixed;
  b.moving_stride = n_moving;
  b.fixed_desc    = fixed.d();
  b.n_fixed       = &meta.d()->n_fixed;
  b.moving_desc   = moving.d();
  b.n_moving      = &meta.d()->n_moving;
  b.matches       = matches.d();
  b.n_matches     = &meta.d()->n_matches;
  b.status        = &meta.d()->status;
  // the candidate list defaults to 16 entries per descriptor; a loose threshold on correlated descriptors can need more
  // (at most every pair): grow and repeat, like the reference's std::vector would
  const long long all_pairs = (long long) n_fixed * (long long) n_moving;
  long long cand_cap        = 16ll * (long long) (n_fixed > n_moving ? n_fixed : n_moving);
  for (;;) {
    if (cand_cap > all_pairs) {
      cand_cap = all_pairs;
    }
    b.candidate_capacity = (int32_t) (cand_cap > 0x7fffffffll ? 0x7fffffffll : cand_cap);
    PRS_TRY(bruteforce_batch_launch(ctx, params, &b));
    PRS_TRY(st.download());
    if (m.status != PRS_ERR_CAPACITY || cand_cap >= all_pairs) {
      break;
    }
    cand_cap *= 8;
    m.n_matches = 0;
    m.status    = 0;
    PRS_TRY(st.upload(meta));  // the meta words only
  }
  if (m.status < 0) {
    return ctx_fail(ctx, m.status, "prs_bruteforce_match: more candidates below the threshold than the kernel's candidate capacity");
  }
  memcpy(correspondences, matches.h(), (size_t) m.n_matches * sizeof(prs_corr));
  *n_correspondences = m.n_matches;
  return m.status;
}

int prs_merge_batch_run(prs_context* ctx, const prs_merger_params* params, const prs_merge_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return merge_batch_launch(ctx, params, batch);
}

int prs_pose_compose_batch(prs_context* ctx, int32_t batch, const float* prediction, const float* X, float* pose_out) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return pose_compose_launch(ctx, batch, prediction, X, pose_out);
}

int prs_motion_predict_batch(prs_context* ctx, int32_t batch, const float* pose_prev2, const float* pose_prev1, float* pose_pred) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return motion_predict_launch(ctx, batch, pose_prev2, pose_prev1, pose_pred);
}

int prs_extract_features_batch(prs_context* ctx, const prs_extractor_params* params, const prs_extract_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return extract_features_launch(ctx, params, batch);
}

int prs_selection_order(prs_context* ctx, const uint8_t* response, int32_t n, int32_t* order) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (n < 0 || n > 32768) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_selection_order: more than 32768 keypoints in a region");
  }
  if (n == 0) {
    return PRS_OK;
  }
  if (!response || !order) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_selection_order: responses / order not set");
  }
  for (int32_t i = 0; i < n; ++i) {
    if (response[i] == 0) {
      return ctx_fail(ctx, PRS_ERR_RANGE, "prs_selection_order: a response of 0 (a detected corner scores at least 1)");
    }
  }
  (void) hipSetDevice(ctx->device);
  Staging st(ctx, "prs_selection_order");
  auto resp     = st.up<uint8_t>((size_t) n);
  auto order_st = st.down<int32_t>((size_t) n);
  auto status   = st.down<int32_t>(1);
  PRS_TRY(st.commit());
  memcpy(resp.h(), response, (size_t) n);
  PRS_TRY(st.upload());
  PRS_TRY(selection_order_launch(ctx, resp.d(), n, order_st.d(), status.d()));
  PRS_TRY(st.download());
  if (*status.h() != PRS_OK) {
    return ctx_fail(ctx, *status.h(), "prs_selection_order: the sort did not finish");
  }
  memcpy(order, order_st.h(), (size_t) n * 4);
  return PRS_OK;
}

int prs_extract_features(prs_context* ctx,
                         const prs_extractor_params* params,
                         const uint8_t* image,
                         int32_t rows,
                         int32_t cols,
                         int32_t pitch,
                         float* keypoints,
                         float* intensity,
                         uint8_t* descriptors,
                         int32_t capacity,
                         int32_t* n_features) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (!params || !image) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_extract_features: image not set");
  }
  if (!keypoints || !descriptors || !n_features) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_extract_features: target feature buffer not set");
  }
  if (rows <= 0 || cols <= 0 || pitch < cols || capacity <= 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_extract_features: invalid image size, pitch or capacity");
  }
  (void) hipSetDevice(ctx->device);
  const size_t cap = (size_t) capacity;
  struct Meta {
    int32_t n_features, status;
  };
  // image | n_features, status | keypoints | intensity | descriptors
  Staging st(ctx, "prs_extract_features");
  auto img   = st.up<uint8_t>((size_t) rows * (size_t) pitch);
  auto meta  = st.down<Meta>(1);
  auto kp    = st.down<prs_kp2>(cap);
  auto inten = st.down<float>(cap);
  auto desc  = st.down<uint8_t>(cap * PRS_DESC_BYTES);
  PRS_TRY(st.commit());
  // (the last row of a pitched view, e.g. a cv::Mat ROI, owns only `cols` bytes)
  const size_t image_bytes = (size_t) (rows - 1) * (size_t) pitch + (size_t) cols;
  memcpy(img.h(), image, image_bytes);
  PRS_TRY(st.upload(image_bytes));
  prs_extract_batch b;
  b.batch       = 1;
  b.rows        = rows;
  b.cols        = cols;
  b.pitch       = pitch;
  b.images      = img.d();
  b.stride      = capacity;
  b.keypoints   = kp.d();
  b.intensity   = inten.d();
  b.descriptors = desc.d();
  b.n_features  = &meta.d()->n_features;
  b.status      = &meta.d()->status;
  PRS_TRY(extract_features_launch(ctx, params, &b));
  PRS_TRY(st.download());
  const int32_t n = meta.h()->n_features, status = meta.h()->status;
  if (status < 0) {
    *n_features = 0;
    return ctx_fail(ctx, status, "prs_extract_features: more raw detections or features than the buffers hold");
  }
  memcpy(keypoints, kp.h(), (size_t) n * sizeof(prs_kp2));
  if (intensity) {
    memcpy(intensity, inten.h(), (size_t) n * sizeof(float));
  }
  memcpy(descriptors, desc.h(), (size_t) n * PRS_DESC_BYTES);
  *n_features = n;
  return status;
}


int prs_extract_features_selective_batch(prs_context* ctx, const prs_selective_extractor_params* params, const prs_selective_extract_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return selective_extract_launch(ctx, params, batch);
}

int prs_extract_features_selective(prs_context* ctx,
                                   const prs_selective_extractor_params* params,
                                   const uint8_t* image,
                                   int32_t rows,
                                   int32_t cols,
                                   int32_t pitch,
                                   const float* projections,
                                   int32_t n_projections,
                                   int32_t detection_radius,
                                   const uint8_t* seeding_mask,
                                   float* keypoints,
                                   float* intensity,
                                   uint8_t* descriptors,
                                   int32_t capacity,
                                   int32_t* n_features) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (!params || !image || (n_projections > 0 && !projections)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_extract_features_selective: image not set");
  }
  if (!keypoints || !descriptors || !n_features) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_extract_features_selective: target feature buffer not set");
  }
  if (rows <= 0 || cols <= 0 || pitch < cols || capacity <= 0 || n_projections < 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_extract_features_selective: invalid image size, pitch, capacity or projection count");
  }
  (void) hipSetDevice(ctx->device);
  const size_t cap         = (size_t) capacity;
  const size_t n_proj      = (size_t) (n_projections > 0 ? n_projections : 1);
  const size_t image_bytes = (size_t) (rows - 1) * (size_t) pitch + (size_t) cols;
  struct Meta {
    int32_t n_features, status, n_projections, detection_radius;
  };
  // image | seeding mask | projections | meta | keypoints | intensity | descriptors
  Staging st(ctx, "prs_extract_features_selective");
  auto img   = st.up<uint8_t>((size_t) rows * (size_t) pitch);
  auto mask  = st.up<uint8_t>(seeding_mask ? (size_t) rows * (size_t) pitch : 0);
  auto proj  = st.up<prs_kp2>(n_proj);
  auto meta  = st.both<Meta>(1);
  auto kp    = st.down<prs_kp2>(cap);
  auto inten = st.down<float>(cap);
  auto desc  = st.down<uint8_t>(cap * PRS_DESC_BYTES);
  PRS_TRY(st.commit());
  memcpy(img.h(), image, image_bytes);
  if (seeding_mask) {
    memcpy(mask.h(), seeding_mask, image_bytes);
  }
  if (n_projections > 0) {
    memcpy(proj.h(), projections, (size_t) n_projections * sizeof(prs_kp2));
  }
  *meta.h() = {0, 0, n_projections, detection_radius};
  PRS_TRY(st.upload());
  prs_selective_extract_batch b;
  memset(&b, 0, sizeof(b));
  b.batch             = 1;
  b.rows              = rows;
  b.cols              = cols;
  b.pitch             = pitch;
  b.images            = img.d();
  b.projection_stride = (int32_t) n_proj;
  b.projections       = proj.d();
  b.n_projections     = &meta.d()->n_projections;
  b.detection_radius  = &meta.d()->detection_radius;
  b.seeding_mask      = seeding_mask ? mask.d() : nullptr;
  b.stride            = capacity;
  b.keypoints         = kp.d();
  b.intensity         = inten.d();
  b.descriptors       = desc.d();
  b.n_features        = &meta.d()->n_features;
  b.status            = &meta.d()->status;
  PRS_TRY(selective_extract_launch(ctx, params, &b));
  PRS_TRY(st.download());
  const int32_t n = meta.h()->n_features, status = meta.h()->status;
  if (status < 0) {
    *n_features = 0;
    return ctx_fail(ctx, status, "prs_extract_features_selective: projection outside the image, or more candidates or features than the buffers hold");
  }
  memcpy(keypoints, kp.h(), (size_t) n * sizeof(prs_kp2));
  if (intensity) {
    memcpy(intensity, inten.h(), (size_t) n * sizeof(float));
  }
  memcpy(descriptors, desc.h(), (size_t) n * PRS_DESC_BYTES);
  *n_features = n;
  return status;
}
}  // extern "C"
