// prs_launch.h -- the one path by which host code launches a kernel: counts in int64 -> a checked Grid -> launch().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/proslam_hip.h"

namespace prs {

int ctx_fail(prs_context* ctx, int status, const char* what);
int ctx_fail_hip(prs_context* ctx, hipError_t e, const char* what);

// whether one launch may have this grid: HIP takes no launch of 2^32 or more work-items in a dimension (hip_runtime_api.h, the note
// on hipModuleLaunchKernel), which for 256 threads is 2^24 - 1 workgroups.  No product here overflows for any int64 count
inline bool grid_fits(const int64_t workgroups, const int threads) {
  return workgroups >= 1 && threads >= 1 && threads <= 1024 && workgroups <= 0xffffffffll / threads;
}

// A grid that launch() takes.  checked() is the only way to a Grid that holds work: grid_fits in x with the workgroup's threads,
// and in y and z, where a workgroup has one thread.  Counts stay int64 until then.  A refused grid is empty, and HIP takes no
// empty launch, so a kernel cannot be launched on counts that were never checked
class Grid {
 public:
  Grid() = default;
  static Grid checked(const int64_t x, const int64_t y, const int64_t z, const int threads) {
    Grid g;
    if (grid_fits(x, threads) && grid_fits(y, 1) && grid_fits(z, 1)) {
      g.x_ = (unsigned) x, g.y_ = (unsigned) y, g.z_ = (unsigned) z, g.threads_ = (unsigned) threads;
    }
    return g;
  }
  explicit operator bool() const {
    return threads_ != 0;
  }
  unsigned x() const { return x_; }
  unsigned y() const { return y_; }
  unsigned z() const { return z_; }
  unsigned threads() const { return threads_; }

 private:
  unsigned x_ = 0, y_ = 0, z_ = 0, threads_ = 0;
};

// the only kernel launch of the library
template <class... P, class... A>
inline void launch(void (*kernel)(P...), const Grid& g, const size_t lds, hipStream_t stream, const A&... args) {
  hipLaunchKernelGGL(kernel, dim3(g.x(), g.y(), g.z()), dim3(g.threads()), lds, stream, args...);
}

// the request a kernel needs before it may be launched with more than 64 KiB of dynamic LDS (always: made whatever the size)
template <class... P>
inline hipError_t allow_lds(void (*kernel)(P...), size_t lds, bool always = false) {
  return always || lds > 64u * 1024u ? hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds)
                                     : hipSuccess;
}
// one launch of a dispatch plan (prs::Plan, prs_host.h): the LDS request, the launch, and what either left
template <class Args>
inline hipError_t launch_planned(void (*kernel)(Args), const Grid& g, size_t lds, hipStream_t stream, const Args& a, bool always_request = false) {
  hipError_t e = allow_lds(kernel, lds, always_request);
  if (e == hipSuccess) {
    launch(kernel, g, lds, stream, a);
    e = hipGetLastError();
  }
  return e;
}

// The launches of one call of an entry point.  The call declares the grid of every launch it is going to make (and of no other),
// asks check() once -- a refusal has enqueued nothing and written nothing --, launches, and returns finish().
class Launches {
 public:
  Launches(prs_context* ctx, const char* entry, hipStream_t stream) : ctx_(ctx), entry_(entry), stream_(stream) {}
  Grid grid(const int64_t x, const int threads) {
    return grid(x, 1, 1, threads);
  }
  Grid grid(const int64_t x, const int64_t y, const int threads) {
    return grid(x, y, 1, threads);
  }
  Grid grid(const int64_t x, const int64_t y, const int64_t z, const int threads) {
    const Grid g = Grid::checked(x, y, z, threads);
    fit_         = fit_ && g;
    return g;
  }
  int check() const {  // PRS_ERR_UNSUPPORTED when a declared grid does not fit
    return fit_ ? PRS_OK : fail(PRS_ERR_UNSUPPORTED, hipSuccess, ": more work-items than one launch holds");
  }
  template <class... P, class... A>
  void launch(void (*kernel)(P...), const Grid& g, const size_t lds, const A&... args) const {
    prs::launch(kernel, g, lds, stream_, args...);
  }
  // a call of one launch of x workgroups: declared, checked, launched and closed
  template <class... P, class... A>
  int one(const int64_t x, const int threads, void (*kernel)(P...), const size_t lds, const A&... args) {
    const Grid g  = grid(x, threads);
    const int fit = check();
    if (fit == PRS_OK) {
      launch(kernel, g, lds, args...);
    }
    return fit == PRS_OK ? finish() : fit;
  }
  // what the launches (or the HIP calls between them: e) left: PRS_ERR_HIP with the entry point named
  int finish(hipError_t e = hipSuccess) const {
    e = e != hipSuccess ? e : hipGetLastError();
    return e == hipSuccess ? PRS_OK : fail(PRS_ERR_HIP, e, " launch");
  }

 private:
  int fail(const int status, const hipError_t e, const char* what) const {
    char text[160];
    snprintf(text, sizeof(text), "%s%s", entry_, what);
    return status == PRS_ERR_HIP ? ctx_fail_hip(ctx_, e, text) : ctx_fail(ctx_, status, text);
  }
  prs_context* ctx_;
  const char* entry_;
  hipStream_t stream_;
  bool fit_ = true;
};

}  // namespace prs
