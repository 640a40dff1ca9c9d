// speckle.hip -- the speckle filter on the device: the small 4-connected segments of a disparity or depth image are set to 0, in
// place (prs_speckle_batch_run; the rule is stated in include/proslam_hip.h, BUILD-DEFINED after OpenCV's filterSpeckles, and restated
// in tests/speckle_ref.py).  Connected-component labelling by union-find; a pixel's label is an index of its own image's raster,
// parent[i] <= i always, and a component's root is its least index.  Two int32 per pixel in the caller's workspace: the parent and,
// at a root, the component's size.
//   tile     one workgroup per 64 x 16 tile of one image, a wave a row at a time: the tile's values in LDS as floats, NaN for an
//            invalid pixel or one outside the image (a NaN connects to nothing, so one comparison is the whole rule).  The runs of a
//            row are found by a ballot of the lanes that are valid and not connected to their left neighbour; a lane's first parent
//            is its run's start.  Then the vertical unions in LDS, one per stretch of columns in which the same two runs touch, a
//            read-only flatten, and out go the global raster index of the tile-local root and a zero size
//   seam     one thread per pixel pair across a tile border: the same union on the parents in global memory, one per stretch again
//   flatten  a workgroup 2048 pixels of an image's raster, a lane a pixel at a time: walks to the root, stores it as the pixel's parent
//            (and as the parent of where the walk began, so the walks of later rows are short), and adds the length of each run of
//            equal roots in a wave to the root's size -- unless that size is already above max_size
//   apply    a workgroup 2048 pixels: the zeroes in image and companion, label, and n_kept / n_removed by wave ballots and one integer
//            atomic add a workgroup and counter (a workgroup per 256 pixels, built first, made this launch wait on 1800 adds to one
//            address an image: a grid runs image after image, so the adds of one image arrive together)
// The atomics are integer min and add: each result is the same whatever order they arrive in.  Which parent a pixel holds between two
// launches may differ from run to run; the root it leads to, and so every output byte, does not.  A size is exact while it is at most
// max_size; above it only "above" is used, and a size never falls, so skipping the adds to a size seen above max_size changes no
// decision.  Every loop below strictly lowers the index it holds or leaves: see union_in and find_in.  No workgroup waits for
// another: plain launches, no lock, no spinning, no flag.
#include <math.h>
#include <stddef.h>

#include <string>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"

namespace prs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves   = kThreads / PRS_WAVE;
constexpr int kTileW   = PRS_WAVE;  // a lane a column
constexpr int kTileH   = 16;
constexpr int kChunk   = 8 * kThreads;  // pixels of a flatten or apply workgroup

struct SpeckleArgs {
  prs_speckle_params p;
  prs_speckle_batch o;
  int32_t tiles_x, tiles_y;
  int32_t seams;    // pixel pairs across tile borders of one image: (tiles_x - 1) * rows + (tiles_y - 1) * cols
  int32_t sblocks;  // ceil(seams / kThreads)
  int32_t pblocks;  // ceil(rows * cols / kChunk): the flatten and apply workgroups of an image
  int32_t* parent;  // [images][rows * cols]
  int32_t* size;    // [images][rows * cols], read at roots
};

// element (v, u) of an image as a float, NaN when it is not valid.  valid: x > 0, which for a float is 0 < bits <= those of +inf
__device__ __forceinline__ float value_at(const void* image, const int type, const size_t row_bytes, const int u) {
  const char* row = static_cast<const char*>(image) + row_bytes;
  if (type == PRS_PIXEL_U16) {
    const uint16_t x = reinterpret_cast<const uint16_t*>(row)[u];
    return x > 0 ? (float) x : __builtin_nanf("");
  }
  const int32_t bits = reinterpret_cast<const int32_t*>(row)[u];
  return (bits > 0 && bits <= 0x7f800000) ? __int_as_float(bits) : __builtin_nanf("");
}

// connected: both valid and |a - b| <= max_diff in one float32 subtraction (false when either is NaN, and for inf - inf)
__device__ __forceinline__ bool linked(const float x, const float y, const float max_diff) {
  return fabsf(x - y) <= max_diff;
}

// The two walks, on LDS (a workgroup's tile) or global memory (the seams).  Invariant: parent[i] <= i, and parent[i] only ever falls
// (the writers are atomic min, and stores of an ancestor).
struct Lds {
  static __device__ __forceinline__ int load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ int lower(int* p, const int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
struct Global {
  static __device__ __forceinline__ int load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ int lower(int* p, const int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// the root above i.  Ends: a step goes on only to parent[i] < i, and i >= 0
template <class M>
__device__ __forceinline__ int find_in(const int* parent, int i) {
  for (;;) {
    const int p = M::load(parent + i);
    if (p >= i) {  // == i: a root (never above, by the invariant; >= so that the loop ends whatever it reads)
      return i;
    }
    i = p;
  }
}

// joins the components of i and j under the lesser root.  With a > b two roots as this thread saw them, atomic min(parent[a], b)
// returns a when a still was a root: it hangs under b now, done.  Otherwise another thread hung a under old < a in the meantime, and
// whichever of old and b the minimum kept as a's parent, the other one still has to be joined to it: go on with (old, b).
// Ends: every round replaces the pair by one whose greater member is smaller -- find_in never rises, old < a and b < a -- or leaves;
// indices are >= 0.  A thread never waits for another one's write.
template <class M>
__device__ __forceinline__ void union_in(int* parent, int i, int j) {
  for (;;) {
    int a = find_in<M>(parent, i), b = find_in<M>(parent, j);
    if (a == b) {
      return;
    }
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = M::lower(parent + a, b);
    if (old >= a) {  // == a: it was a root
      return;
    }
    i = old;  // < a
    j = b;    // < a
  }
}

// ---- tile: blockIdx.x = (image * tiles_y + ty) * tiles_x + tx ----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void speckle_tile_kernel(const SpeckleArgs a) {
  __shared__ float s_val[kTileH][kTileW];
  __shared__ int s_parent[kTileH * kTileW];
  const int tid = threadIdx.x, lane = tid & (PRS_WAVE - 1), w = tid >> 6;
  uint32_t id  = blockIdx.x;
  const int tx = (int) (id % (uint32_t) a.tiles_x);
  id /= (uint32_t) a.tiles_x;
  const int ty         = (int) (id % (uint32_t) a.tiles_y);
  const uint32_t image = id / (uint32_t) a.tiles_y;
  const int f = frame_of(image, a.o.frames), b = sequence_of(image, a.o.frames);
  const int n_img  = images_of(a.o, b);
  const bool first = tx == 0 && ty == 0 && tid == 0;
  if (first && f == 0) {
    a.o.status[b] = n_img < 0 ? PRS_ERR_RANGE : PRS_OK;
  }
  if (f >= n_img) {
    return;
  }
  if (first) {  // the apply launch adds to them
    if (a.o.n_kept) {
      a.o.n_kept[image] = 0;
    }
    if (a.o.n_removed) {
      a.o.n_removed[image] = 0;
    }
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const int x0 = tx * kTileW, y0 = ty * kTileH, x = x0 + lane;
  const float max_diff = a.p.max_diff;
  const size_t image_row0 = (size_t) image * (size_t) rows;
  // the values, and the runs of each row: a lane's first parent is the start of its run
  for (int ly = w; ly < kTileH; ly += kWaves) {
    const int y   = y0 + ly;
    const float v = (y < rows && x < cols) ? value_at(a.o.image, a.p.pixel_type, (image_row0 + (size_t) y) * (size_t) a.o.pitch, x)
                                           : __builtin_nanf("");
    s_val[ly][lane]   = v;
    const float left  = __shfl_up(v, 1, PRS_WAVE);
    const bool valid  = v == v;
    const bool joined = lane > 0 && linked(v, left, max_diff);
    const unsigned long long starts = __ballot(valid && !joined);
    // the highest start at or below the lane: a valid lane is a start or joined to a valid lane on its left, so there is one
    const unsigned long long mine = starts & (~0ull >> (PRS_WAVE - 1 - lane));
    s_parent[ly * kTileW + lane]  = valid ? ly * kTileW + (PRS_WAVE - 1 - __clzll((long long) mine)) : -1;
  }
  __syncthreads();
  // vertical unions.  The pixel and the one above it are joined here unless their left neighbours were joined already and each lies
  // in its neighbour's run: of a stretch of columns in which the same two runs touch, the first column makes the union
  for (int ly = w; ly < kTileH; ly += kWaves) {
    if (ly == 0) {
      continue;
    }
    const float v = s_val[ly][lane], up = s_val[ly - 1][lane];
    const float vl = lane > 0 ? s_val[ly][lane - 1] : __builtin_nanf(""), ul = lane > 0 ? s_val[ly - 1][lane - 1] : __builtin_nanf("");
    const bool need = linked(v, up, max_diff) && !(linked(v, vl, max_diff) && linked(up, ul, max_diff) && linked(vl, ul, max_diff));
    if (need) {
      union_in<Lds>(s_parent, ly * kTileW + lane, (ly - 1) * kTileW + lane);
    }
  }
  __syncthreads();
  // flatten (nothing writes s_parent any more) and hand over: the raster order of the tile is that of the image, so the least local
  // index is the least global one
  int32_t* parent = a.parent + (size_t) image * (size_t) rows * (size_t) cols;
  int32_t* size   = a.size + (size_t) image * (size_t) rows * (size_t) cols;
  for (int ly = w; ly < kTileH; ly += kWaves) {
    const int y = y0 + ly;
    if (y < rows && x < cols) {
      int root = s_parent[ly * kTileW + lane];
      if (root >= 0) {
        root = find_in<Lds>(s_parent, root);
        root = (y0 + root / kTileW) * cols + x0 + (root & (kTileW - 1));
      }
      parent[y * cols + x] = root;
      size[y * cols + x]   = 0;
    }
  }
}

// ---- seam: blockIdx.x = image * sblocks + block; a thread one pixel pair across a tile border ----------------------------------------
// pairs 0 .. (tiles_x - 1) * rows - 1: (y, x) and (y, x - 1), x = 64, 128, ..; behind them (y, x) and (y - 1, x), y = 16, 32, ..
// The pair is joined here unless the pair before it along the border was joined, lies in the same two tiles and each of its pixels is
// linked to this pair's pixel on its side: those two links are inside a tile, so the tile launch has made them
__global__ __launch_bounds__(kThreads) void speckle_seam_kernel(const SpeckleArgs a) {
  const int block      = (int) (blockIdx.x % (uint32_t) a.sblocks);
  const uint32_t image = blockIdx.x / (uint32_t) a.sblocks;
  const int f = frame_of(image, a.o.frames), b = sequence_of(image, a.o.frames);
  const int s = block * kThreads + (int) threadIdx.x;
  if (f >= images_of(a.o, b) || s >= a.seams) {
    return;
  }
  const int rows = a.o.rows, cols = a.o.cols;
  const int n_vertical = (a.tiles_x - 1) * rows;
  int y, x, dy, dx;  // the pair (y, x), (y - dy, x - dx); the pair before it along the border is (y - dx, x - dy), (y - dx - dy, x - dy - dx)
  bool inner;        // that pair exists and lies in the same two tiles
  if (s < n_vertical) {
    x = (s / rows + 1) * kTileW;
    y = s % rows;
    dy = 0, dx = 1;
    inner = y % kTileH != 0;
  } else {
    const int t = s - n_vertical;
    y = (t / cols + 1) * kTileH;
    x = t % cols;
    dy = 1, dx = 0;
    inner = x % kTileW != 0;
  }
  const int type = a.p.pixel_type;
  const size_t row0 = (size_t) image * (size_t) rows, pitch = (size_t) a.o.pitch;
  const float max_diff = a.p.max_diff;
  const float p = value_at(a.o.image, type, (row0 + (size_t) y) * pitch, x);
  const float q = value_at(a.o.image, type, (row0 + (size_t) (y - dy)) * pitch, x - dx);
  if (!linked(p, q, max_diff)) {
    return;
  }
  if (inner) {
    const float pp = value_at(a.o.image, type, (row0 + (size_t) (y - dx)) * pitch, x - dy);
    const float qq = value_at(a.o.image, type, (row0 + (size_t) (y - dx - dy)) * pitch, x - dy - dx);
    if (linked(pp, qq, max_diff) && linked(p, pp, max_diff) && linked(q, qq, max_diff)) {
      return;
    }
  }
  union_in<Global>(a.parent + (size_t) image * (size_t) rows * (size_t) cols, y * cols + x, (y - dy) * cols + (x - dx));
}

// ---- flatten: blockIdx.x = image * pblocks + block; a workgroup kChunk pixels of the image's raster ---------------------------------
__global__ __launch_bounds__(kThreads) void speckle_flatten_kernel(const SpeckleArgs a) {
  const int block      = (int) (blockIdx.x % (uint32_t) a.pblocks);
  const uint32_t image = blockIdx.x / (uint32_t) a.pblocks;
  if (!image_served(a.o, image)) {
    return;
  }
  const int pixels = a.o.rows * a.o.cols;
  int32_t* parent  = a.parent + (size_t) image * (size_t) pixels;
  int32_t* size    = a.size + (size_t) image * (size_t) pixels;
  const int lane = (int) threadIdx.x & (PRS_WAVE - 1), max_size = a.p.max_size;
  const int start = block * kChunk, count = min(kChunk, pixels - start);  // start < pixels: no sum here passes rows * cols
  int big = -1;  // a root this lane has seen above max_size
  for (int base = 0; base < count; base += kThreads) {  // the same trips for every lane: the ballot below sees whole waves
    const int k = base + (int) threadIdx.x, i = start + min(k, count - 1);
    int root = -1;
    if (k < count) {
      const int first = parent[i];
      if (first >= 0) {
        root = find_in<Global>(parent, first);
        // stores of the root, an ancestor at or below what stood there: the walks of other threads through i or first only get
        // shorter and end where they ended.  No union runs in this launch, so a root stays one
        if (root != first) {
          __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(parent + first, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    if (max_size == 0) {  // nothing is removed: no size is asked for
      continue;
    }
    // the runs of equal roots along the wave's 64 pixels: the first lane of a run adds its length
    const int before  = __shfl_up(root, 1, PRS_WAVE);
    const bool change = lane == 0 || root != before;
    const unsigned long long changes = __ballot(change);
    if (change && root >= 0 && root != big) {
      const unsigned long long above = lane == PRS_WAVE - 1 ? 0ull : changes & (~0ull << (lane + 1));
      const int length = (above ? __builtin_ctzll(above) : PRS_WAVE) - lane;
      // a size above max_size stays above it: only that is asked of it, so it needs no further adds
      if (__hip_atomic_load(size + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= max_size) {
        atomicAdd(size + root, length);  // at most rows * cols in all: no overflow
      } else {
        big = root;
      }
    }
  }
}

// ---- apply: blockIdx.x = image * pblocks + block; a workgroup kChunk pixels of the image's raster -----------------------------------
__device__ __forceinline__ void put_zero(void* image, const int type, const size_t row_bytes, const int u) {
  char* row = static_cast<char*>(image) + row_bytes;
  if (type == PRS_PIXEL_U16) {
    reinterpret_cast<uint16_t*>(row)[u] = 0;
  } else {
    reinterpret_cast<float*>(row)[u] = 0.0f;
  }
}

__global__ __launch_bounds__(kThreads) void speckle_apply_kernel(const SpeckleArgs a) {
  __shared__ int s_kept[kWaves], s_removed[kWaves];
  const int tid        = threadIdx.x;
  const int block      = (int) (blockIdx.x % (uint32_t) a.pblocks);
  const uint32_t image = blockIdx.x / (uint32_t) a.pblocks;
  if (!image_served(a.o, image)) {
    return;
  }
  const int rows = a.o.rows, cols = a.o.cols, pixels = rows * cols;
  const size_t at_image = (size_t) image * (size_t) pixels;
  const int start = block * kChunk, count = min(kChunk, pixels - start);  // start < pixels: no sum here passes rows * cols
  int kept = 0, gone = 0;  // the wave's
  for (int base = 0; base < count; base += kThreads) {
    const int k = base + tid, i = start + min(k, count - 1);
    bool valid = false, removed = false;
    if (k < count) {
      const int root = a.parent[at_image + i];
      valid   = root >= 0;
      removed = valid && a.p.max_size > 0 && a.size[at_image + root] <= a.p.max_size;
      const int v = i / cols, u = i - v * cols;
      const size_t row = (size_t) image * (size_t) rows + (size_t) v;
      if (removed) {
        put_zero(a.o.image, a.p.pixel_type, row * (size_t) a.o.pitch, u);
        if (a.o.companion) {
          put_zero(a.o.companion, a.p.companion_type, row * (size_t) a.o.companion_pitch, u);
        }
      }
      if (a.o.label) {
        a.o.label[row * (size_t) (a.o.label_pitch >> 2) + (size_t) u] = root;
      }
    }
    kept += (int) __popcll(__ballot(valid && !removed));
    gone += (int) __popcll(__ballot(removed));
  }
  if (a.o.n_kept || a.o.n_removed) {  // one integer atomic add a workgroup and counter: the sums do not depend on the order
    if ((tid & (PRS_WAVE - 1)) == 0) {
      s_kept[tid >> 6]    = kept;
      s_removed[tid >> 6] = gone;
    }
    __syncthreads();
    if (tid == 0) {
      int sum_kept = 0, sum_removed = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        sum_kept += s_kept[w];
        sum_removed += s_removed[w];
      }
      if (a.o.n_kept && sum_kept != 0) {
        atomicAdd(a.o.n_kept + image, sum_kept);
      }
      if (a.o.n_removed && sum_removed != 0) {
        atomicAdd(a.o.n_removed + image, sum_removed);
      }
    }
  }
}

// bytes of an element of a type the filter takes (disparity or depth: no 8-bit image), 0 for any other
inline int64_t element_bytes(const int type) {
  return type == PRS_PIXEL_U8 ? 0 : pixel_bytes(type);
}

}  // namespace

int speckle_launch(prs_context* ctx, const prs_speckle_params* params, const prs_speckle_batch* batch) {
  const std::string who = "prs_speckle_batch_run";
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": parameters not set").c_str());
  }
  const prs_speckle_params& p = *params;
  const prs_speckle_batch& o  = *batch;
  if (!o.image || !o.status || !o.workspace) {
    return ctx_fail(ctx, PRS_ERR_NULL, (who + ": image, status or the workspace not set").c_str());
  }
  if (!std::isfinite(p.max_diff) || p.max_diff < 0.0f || p.max_size < 0) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": max_diff not finite or below 0, or max_size below 0").c_str());
  }
  // a pitch is judged by its element; a type without one is refused below
  const int64_t es = element_bytes(p.pixel_type), ces = o.companion ? element_bytes(p.companion_type) : 0;
  const auto bad_pitch = [&](const int64_t pitch, const int64_t e) { return e > 0 && !pitch_ok(pitch, o.cols, e); };
  if (o.batch < 1 || o.frames < 1 || o.rows < 1 || o.cols < 1 || bad_pitch(o.pitch, es) || bad_pitch(o.companion_pitch, ces) ||
      (o.label && bad_pitch(o.label_pitch, 4))) {
    return ctx_fail(ctx, PRS_ERR_RANGE, (who + ": a size below 1, or a pitch below cols elements or not a multiple of the element size").c_str());
  }
  if (es == 0 || (o.companion && ces == 0)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": pixel_type and, with a companion, companion_type must be PRS_PIXEL_U16 or PRS_PIXEL_F32").c_str());
  }
  if (!aligned_to(o.image, (uintptr_t) es) || !aligned_to(o.companion, (uintptr_t) (ces ? ces : 1)) || !aligned_to(o.workspace, 16) ||
      !aligned_to(o.n_images, 4) || !aligned_to(o.label, 4) || !aligned_to(o.n_kept, 4) || !aligned_to(o.n_removed, 4) || !aligned_to(o.status, 4)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": the workspace must be 16-byte aligned, image and companion to their element, the other arrays 4-byte").c_str());
  }
  const uint64_t pixels = image_pixels(o.batch, o.frames, o.rows, o.cols);
  if (pixels < 1) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": rows * cols or batch * frames * rows * cols beyond 2^31 - 1").c_str());
  }
  const uint64_t image_rows = (uint64_t) o.batch * (uint64_t) o.frames * (uint64_t) o.rows;  // below 2^31
  const uint64_t image_bytes = image_rows * (uint64_t) o.pitch;
  if ((o.companion && overlap(o.image, image_bytes, o.companion, image_rows * (uint64_t) o.companion_pitch)) ||
      (o.label && overlap(o.image, image_bytes, o.label, image_rows * (uint64_t) o.label_pitch))) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, (who + ": companion and label must not overlap image").c_str());
  }
  SpeckleArgs a = {};
  a.p = p;
  a.o = o;
  a.tiles_x = (o.cols + kTileW - 1) / kTileW;
  a.tiles_y = (o.rows + kTileH - 1) / kTileH;
  const int64_t seams = (int64_t) (a.tiles_x - 1) * o.rows + (int64_t) (a.tiles_y - 1) * o.cols;  // below rows * cols
  a.seams   = (int32_t) seams;
  a.sblocks = (int32_t) ((seams + kThreads - 1) / kThreads);
  a.pblocks = (int32_t) (((int64_t) o.rows * o.cols + kChunk - 1) / kChunk);
  const int64_t images = (int64_t) o.batch * o.frames;
  Launches on(ctx, who.c_str(), ctx_stream(ctx));
  const Grid tiles  = on.grid(images * a.tiles_x * a.tiles_y, kThreads);
  const Grid seam   = a.sblocks > 0 ? on.grid(images * a.sblocks, kThreads) : Grid();  // an image of one tile has no border
  const Grid pixels_grid = on.grid(images * a.pblocks, kThreads);                       // flatten and apply
  PRS_TRY(on.check());
  uint8_t* ws = static_cast<uint8_t*>(o.workspace);
  a.parent    = reinterpret_cast<int32_t*>(ws);
  a.size      = reinterpret_cast<int32_t*>(ws + up16(4 * pixels));
  on.launch(speckle_tile_kernel, tiles, 0, a);
  if (seam) {
    on.launch(speckle_seam_kernel, seam, 0, a);
  }
  on.launch(speckle_flatten_kernel, pixels_grid, 0, a);
  on.launch(speckle_apply_kernel, pixels_grid, 0, a);
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

void prs_speckle_struct_sizes(uint64_t* sizes2) {
  sizes2[0] = sizeof(prs_speckle_params);
  sizes2[1] = sizeof(prs_speckle_batch);
}

uint64_t prs_speckle_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols) {
  return 2 * up16(4 * image_pixels(batch, frames, rows, cols));
}

int prs_speckle_batch_run(prs_context* ctx, const prs_speckle_params* params, const prs_speckle_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return speckle_launch(ctx, params, batch);
}

}  // extern "C"
