// rectify.hip -- the image rectifier on the device: raw frames are undistorted and stereo-rectified in front of the feature
// extractors and the RGB-D preprocessor (include/proslam_hip.h, "Image rectifier").  BUILD-DEFINED: the reference has no such
// stage; tests/rectify_ref.py restates the arithmetic and the kernel equals its float32 form byte for byte.
//
// One launch per batch:
//   rectify_kernel  a workgroup of 256 threads owns one destination tile of 16 rows x 64 pixels (a wave takes four rows, a lane
//                   four adjacent pixels) and a chunk of consecutive images.  The map of a pixel (two divisions, the distortion
//                   polynomial, the border test) costs about a hundred vector instructions and does not depend on the image, so
//                   the workgroup computes (source offset, ax, ay, tap validity) for its pixels once, keeps them in registers and
//                   walks its images with them; it computes them again only when map_of[b] differs from the map it holds (uniform
//                   over the workgroup).  With the map it reduces (shuffles, then the four waves through LDS) the tile's border
//                   count, whether every tap of the tile lies inside the source, and the box around the taps it holds: the
//                   tile's source footprint.
//                   Tap fetch (b), 8-bit bilinear: per image the workgroup stages the footprint in LDS with 16-byte loads (two
//                   buffers of 8 KB, one barrier an image) and the lanes read their taps from there.  Tap fetch (a), everything
//                   else -- nearest, a footprint that does not fit, a source that is not 16-byte aligned, PRS_RECTIFY_VARIANT=0:
//                   the lanes load their taps from global memory, adjacent rows served from L1 / L2.
//                   A lane writes its four pixels as one store (4 / 8 / 16 bytes; by element where the row is not aligned for
//                   that or the lane reaches over the image's edge).  n_border[b] gets the tile's count by one integer atomic
//                   per workgroup and image; the workgroup of tile 0 writes status[b].
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"

namespace prs {

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kPix = 4;
constexpr int kLanesX = 16, kRowsPerWave = 64 / kLanesX;  // a wave is 4 rows of 16 lanes (4 x 256 pixels a wave measured slower)
constexpr int kTileCols = kLanesX * kPix, kTileRows = kWaves * kRowsPerWave;
constexpr int kChunkMax = 16, kChunkLimit = 64;  // the automatic chunk's ceiling; PRS_RECTIFY_CHUNK's
constexpr int kStageBytes = 8192;                // one of the two staging buffers of tap-fetch (b)
constexpr int kStageLoads = kStageBytes / 16 / kThreads;  // 16-byte loads per thread that fill one

struct RectifyArgs {
  prs_rectify_batch b;
  uint32_t border;  // in the pixel type (float32: its bits)
  int chunk;        // images per workgroup
  int tiles_x, tiles_y;
  int vector_store;  // dst and dst_pitch are multiples of 4 elements: a lane's four pixels go out as one store
  int stage_ok;      // src and src_pitch are multiples of 16 bytes: footprints can be staged with 16-byte loads
};

// tap validity a, b, c, d in bits 0..3 (nearest: bit 0), x1 - x0 and y1 - y0 of the clamped taps in bits 4 and 5
constexpr uint32_t kTapA = 1u, kTapB = 2u, kTapC = 4u, kTapD = 8u, kTaps = 15u, kStepX = 16u, kStepY = 32u;

__device__ inline bool map_is_valid(const prs_rectify_map& m) {
  bool ok = m.model == PRS_DISTORTION_RADTAN;
  const float* f = &m.src_fx;
#pragma unroll
  for (int i = 0; i < 22; ++i) {
    ok = ok && isfinite(f[i]);
  }
  return ok && m.src_fx != 0.f && m.src_fy != 0.f && m.dst_fx != 0.f && m.dst_fy != 0.f;
}

// the source position of destination pixel (u, v); false: the pixel is border
__device__ inline bool source_of(const prs_rectify_map& m, int u, int v, int src_rows, int src_cols, float& us, float& vs) {
  const float x  = ((float) u - m.dst_cx) / m.dst_fx;
  const float y  = ((float) v - m.dst_cy) / m.dst_fy;
  const float rx = (m.R[0] * x + m.R[3] * y) + m.R[6];
  const float ry = (m.R[1] * x + m.R[4] * y) + m.R[7];
  const float rz = (m.R[2] * x + m.R[5] * y) + m.R[8];
  const float xn = rx / rz, yn = ry / rz;
  const float xx = xn * xn, yy = yn * yn, xy = xn * yn;
  const float r2  = xx + yy;
  const float rad = 1.f + r2 * (m.k1 + r2 * (m.k2 + r2 * m.k3));
  const float xd  = (xn * rad + (2.f * m.p1) * xy) + m.p2 * (r2 + 2.f * xx);
  const float yd  = (yn * rad + m.p1 * (r2 + 2.f * yy)) + (2.f * m.p2) * xy;
  us = m.src_fx * xd + m.src_cx;
  vs = m.src_fy * yd + m.src_cy;
  return rz > 0.f && us > -1.f && us < (float) src_cols && vs > -1.f && vs < (float) src_rows;  // NaN fails every comparison
}

template <typename T>
struct alignas(4 * sizeof(T)) Quad {
  T e[kPix];
};

// a lane's four pixels of one image from its held map; `base` is the image in global memory (ystep = its pitch in elements) or
// the staged footprint in LDS (ystep = the footprint's row length).  kInterior: every tap of the tile lies inside the source, so
// the four taps are t[0], t[1], t[ystep], t[ystep + 1] and nothing is selected (12 of 45 vector instructions a pixel less)
// The footprint is read through a volatile LDS pointer, which keeps the compiler from merging t[0] and t[1] into one 16-bit read:
// an unaligned ds_read_u16 costs about 41 LDS cycles (profiles/rectify/README.md), while from global memory the merged load pays.
template <typename T>
using LdsTaps = const volatile __attribute__((address_space(3))) T*;

template <typename T, bool kBilinear, bool kInterior, typename P>
__device__ inline Quad<T> sample(P base, int ystep, const int (&off)[kPix], const float (&ax)[kPix], const float (&ay)[kPix],
                                 const uint32_t (&bits)[kPix], T border) {
  Quad<T> q;
#pragma unroll
  for (int p = 0; p < kPix; ++p) {
    const P t = base + off[p];  // in bounds whatever the bits say
    if constexpr (kBilinear) {
      float fa, fb, fc, fd;
      if constexpr (kInterior) {
        const P t2 = t + ystep;
        fa = (float) t[0];
        fb = (float) t[1];
        fc = (float) t2[0];
        fd = (float) t2[1];
      } else {
        const int sx = bits[p] & kStepX ? 1 : 0, sy = bits[p] & kStepY ? ystep : 0;
        const T ta = t[0], tb = t[sx], tc = t[sy], td = t[sy + sx];
        const float fo = (float) border;
        fa = bits[p] & kTapA ? (float) ta : fo;
        fb = bits[p] & kTapB ? (float) tb : fo;
        fc = bits[p] & kTapC ? (float) tc : fo;
        fd = bits[p] & kTapD ? (float) td : fo;
      }
      const float top = fa + ax[p] * (fb - fa);
      const float bot = fc + ax[p] * (fd - fc);
      const float val = top + ay[p] * (bot - top);
      q.e[p] = (T) fminf(fmaxf(floorf(val + 0.5f), 0.f), 255.f);
    } else {
      const T ta = t[0];
      q.e[p] = bits[p] & kTapA ? ta : border;
    }
  }
  return q;
}

// kStage: tap fetch (b), 8-bit bilinear only
template <typename T, bool kBilinear, bool kStage>
__global__ __launch_bounds__(kThreads) void rectify_kernel(const RectifyArgs a) {
  static_assert(!kStage || (kBilinear && sizeof(T) == 1), "footprints are staged for 8-bit bilinear only");
  __shared__ int wave_red[kWaves][6];  // border count, pixels with a tap outside, footprint x min, x max, y min, y max
  __shared__ uint4 stage[kStage ? 2 * kStageBytes / 16 : 1];
  const prs_rectify_batch& B = a.b;
  const int tiles = a.tiles_x * a.tiles_y;
  const int tile = (int) (blockIdx.x % (unsigned) tiles), chunk = (int) (blockIdx.x / (unsigned) tiles);
  const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v = ty * kTileRows + wave * kRowsPerWave + lane / kLanesX, u0 = tx * kTileCols + (lane % kLanesX) * kPix;
  const int n_in   = v < B.dst_rows ? min(max(B.dst_cols - u0, 0), kPix) : 0;  // pixels of this lane inside the destination
  const int spitch = B.src_pitch / (int) sizeof(T), dpitch = B.dst_pitch / (int) sizeof(T);
  const int b0 = chunk * a.chunk, b1 = min(b0 + a.chunk, B.batch);
  const T border = (T) a.border;
  const size_t src_image = (size_t) B.src_rows * (size_t) spitch, dst_image = (size_t) B.dst_rows * (size_t) dpitch;

  // the held map: per pixel the element offset of tap a (clamped into the source; into the footprint when that is staged), the
  // weights and the validity bits
  int off[kPix];
  float ax[kPix], ay[kPix];
  uint32_t bits[kPix];
  bool have = false, map_ok = false, staged = false, interior = false;
  int held = 0, tile_border = 0, stage_step = 0;
  int stage_from[kStageLoads];  // where this thread's 16-byte pieces of the footprint lie in the image, -1: none

  for (int b = b0; b < b1; ++b) {
    const int mi = B.map_of ? B.map_of[b] : 0;
    if (!have || mi != held) {  // uniform over the workgroup
      have = true;
      held = mi;
      map_ok = mi >= 0 && mi < B.n_maps;
      prs_rectify_map m;
      memset(&m, 0, sizeof(m));
      if (map_ok) {
        m      = B.maps[mi];
        map_ok = map_is_valid(m);
      }
      int lane_border = 0, lane_partial = 0, px[kPix], py[kPix];
      int xmin = INT32_MAX, xmax = -1, ymin = INT32_MAX, ymax = -1;
#pragma unroll
      for (int p = 0; p < kPix; ++p) {
        float us = 0.f, vs = 0.f;
        const bool inside = p < n_in && map_ok && source_of(m, u0 + p, v, B.src_rows, B.src_cols, us, vs);
        px[p]   = 0;
        py[p]   = 0;
        ax[p]   = 0.f;
        ay[p]   = 0.f;
        bits[p] = 0u;
        if (inside) {
          if constexpr (kBilinear) {
            const float fx0 = floorf(us), fy0 = floorf(vs);
            ax[p] = us - fx0;
            ay[p] = vs - fy0;
            const int x0 = (int) fx0, y0 = (int) fy0;  // -1 .. cols - 1, -1 .. rows - 1
            const bool vx0 = x0 >= 0, vx1 = x0 + 1 < B.src_cols, vy0 = y0 >= 0, vy1 = y0 + 1 < B.src_rows;
            const int xc0 = max(x0, 0), xc1 = min(x0 + 1, B.src_cols - 1), yc0 = max(y0, 0), yc1 = min(y0 + 1, B.src_rows - 1);
            px[p]   = xc0;
            py[p]   = yc0;
            bits[p] = (vy0 && vx0 ? kTapA : 0u) | (vy0 && vx1 ? kTapB : 0u) | (vy1 && vx0 ? kTapC : 0u) | (vy1 && vx1 ? kTapD : 0u) |
                      (xc1 > xc0 ? kStepX : 0u) | (yc1 > yc0 ? kStepY : 0u);
            xmin = min(xmin, xc0);
            xmax = max(xmax, xc1);
            ymin = min(ymin, yc0);
            ymax = max(ymax, yc1);
          } else {
            const int xi = (int) floorf(us + 0.5f), yi = (int) floorf(vs + 0.5f);  // -1 .. cols, -1 .. rows
            if (xi >= 0 && xi < B.src_cols && yi >= 0 && yi < B.src_rows) {
              px[p]   = xi;
              py[p]   = yi;
              bits[p] = kTapA;
            }
          }
        }
        lane_border += (p < n_in && !inside) ? 1 : 0;
        lane_partial += (p < n_in && (bits[p] & kTaps) != kTaps) ? 1 : 0;
      }
      // the tile's border count (and footprint): the lanes of a wave by shuffles, the waves through LDS
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        lane_border += __shfl_xor(lane_border, s);
        lane_partial += __shfl_xor(lane_partial, s);
        if constexpr (kStage) {
          xmin = min(xmin, __shfl_xor(xmin, s));
          xmax = max(xmax, __shfl_xor(xmax, s));
          ymin = min(ymin, __shfl_xor(ymin, s));
          ymax = max(ymax, __shfl_xor(ymax, s));
        }
      }
      __syncthreads();  // the previous map's readers are done with wave_red
      if (lane == 0) {
        wave_red[wave][0] = lane_border;
        wave_red[wave][1] = lane_partial;
        if constexpr (kStage) {
          wave_red[wave][2] = xmin;
          wave_red[wave][3] = xmax;
          wave_red[wave][4] = ymin;
          wave_red[wave][5] = ymax;
        }
      }
      __syncthreads();
      tile_border = 0;
      int tile_partial = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        tile_border += wave_red[w][0];
        tile_partial += wave_red[w][1];
        if constexpr (kStage) {
          xmin = min(xmin, wave_red[w][2]);
          xmax = max(xmax, wave_red[w][3]);
          ymin = min(ymin, wave_red[w][4]);
          ymax = max(ymax, wave_red[w][5]);
        }
      }
      // every pixel of the tile inside the destination has its four taps inside the source (which then has two rows and two
      // columns): lanes outside the destination read the image's, or the footprint's, first two rows and columns and store nothing
      interior = kBilinear && tile_partial == 0;
      staged = false;
      if constexpr (kStage) {
        // the footprint is the box around the taps the tile holds (not around its corners: distortion bulges), widened to whole
        // 16-byte pieces of the source rows; a tile whose box does not fit fetches its taps from global memory
        const int xa = xmin & ~15, width = (xmax + 1 - xa + 15) & ~15, height = ymax - ymin + 1;
        staged = a.stage_ok && xmax >= xmin && width * height <= kStageBytes;
        if (staged) {
          stage_step = width;
#pragma unroll
          for (int p = 0; p < kPix; ++p) {
            off[p] = bits[p] & kTaps ? (py[p] - ymin) * width + (px[p] - xa) : 0;
          }
          const int per_row = width / 16, pieces = per_row * height;
#pragma unroll
          for (int j = 0; j < kStageLoads; ++j) {
            const int c = tid + j * kThreads, r = c / per_row;
            stage_from[j] = c < pieces ? (ymin + r) * spitch + xa + 16 * (c - r * per_row) : -1;
          }
        }
      }
      if (!staged) {
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
          off[p] = py[p] * spitch + px[p];
        }
      }
    }

    const T* src = static_cast<const T*>(B.src) + (size_t) b * src_image;
    Quad<T> q;
    if (kStage && staged) {  // uniform over the workgroup
      // two buffers, one barrier an image: a wave that fills buffer k & 1 again has passed the barrier of image k + 1, which
      // every wave reaches only after its reads of image k
      uint4* buf = stage + ((b - b0) & 1) * (kStageBytes / 16);
#pragma unroll
      for (int j = 0; j < kStageLoads; ++j) {
        if (stage_from[j] >= 0) {
          buf[tid + j * kThreads] = *reinterpret_cast<const uint4*>(src + stage_from[j]);
        }
      }
      __syncthreads();
      const LdsTaps<T> taps = (LdsTaps<T>) buf;
      q = interior ? sample<T, kBilinear, true>(taps, stage_step, off, ax, ay, bits, border)
                   : sample<T, kBilinear, false>(taps, stage_step, off, ax, ay, bits, border);
    } else {
      q = interior ? sample<T, kBilinear, true>(src, spitch, off, ax, ay, bits, border)
                   : sample<T, kBilinear, false>(src, spitch, off, ax, ay, bits, border);
    }
    if (n_in > 0) {
      T* out = static_cast<T*>(B.dst) + (size_t) b * dst_image + (size_t) v * (size_t) dpitch + (size_t) u0;
      if (n_in == kPix && a.vector_store) {
        *reinterpret_cast<Quad<T>*>(out) = q;
      } else {
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
          if (p < n_in) {
            out[p] = q.e[p];
          }
        }
      }
    }
    if (tid == 0) {
      if (B.n_border && tile_border > 0) {
        atomicAdd(&B.n_border[b], tile_border);
      }
      if (tile == 0) {
        B.status[b] = map_ok ? PRS_OK : PRS_ERR_RANGE;
      }
    }
  }
}

uint32_t border_value(const prs_rectify_params* params) {
  if (params->pixel_type == PRS_PIXEL_F32) {
    uint32_t bits;
    memcpy(&bits, &params->border, sizeof(bits));
    return bits;
  }
  const float top = params->pixel_type == PRS_PIXEL_U8 ? 255.f : 65535.f;
  const float r   = floorf(params->border + 0.5f);
  return r >= 0.f ? (uint32_t) fminf(r, top) : 0u;  // NaN: 0
}

template <typename T>
void launch_rectify(const Launches& on, const Grid& grid, const RectifyArgs& a, bool bilinear, bool stage) {
  if constexpr (sizeof(T) == 1) {  // bilinear exists for 8-bit pixels only, and only it stages
    if (bilinear && stage) {
      on.launch(rectify_kernel<T, true, true>, grid, 0, a);
      return;
    }
    if (bilinear) {
      on.launch(rectify_kernel<T, true, false>, grid, 0, a);
      return;
    }
  }
  on.launch(rectify_kernel<T, false, false>, grid, 0, a);
}

}  // namespace

int rectify_launch(prs_context* ctx, const prs_rectify_params* params, const prs_rectify_batch* batch) {
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_rectify_batch_run: parameters not set");
  }
  if (!batch->src || !batch->dst || !batch->maps || !batch->status) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_rectify_batch_run: src, dst, maps or status not set");
  }
  const int type = params->pixel_type, interp = params->interpolation;
  const int64_t elem = pixel_bytes(type);
  if (elem == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_rectify_batch_run: unknown pixel_type");
  }
  if (interp != PRS_RECTIFY_BILINEAR && interp != PRS_RECTIFY_NEAREST) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_rectify_batch_run: unknown interpolation");
  }
  if (interp == PRS_RECTIFY_BILINEAR && type != PRS_PIXEL_U8) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_rectify_batch_run: bilinear interpolation is for 8-bit pixels only (depth is sampled nearest)");
  }
  if (batch->batch < 1 || batch->n_maps < 1 || batch->src_rows < 1 || batch->src_cols < 1 || batch->dst_rows < 1 || batch->dst_cols < 1) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_rectify_batch_run: batch, n_maps or an image size below 1");
  }
  if (!pitch_ok(batch->src_pitch, batch->src_cols, elem) || !pitch_ok(batch->dst_pitch, batch->dst_cols, elem)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_rectify_batch_run: a pitch below cols * element size or not a multiple of the element size");
  }
  const int64_t src_image = (int64_t) batch->src_rows * batch->src_pitch, dst_image = (int64_t) batch->dst_rows * batch->dst_pitch;
  if (src_image > INT32_MAX || dst_image > INT32_MAX) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_rectify_batch_run: an image of 2^31 bytes or more");
  }
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(batch->src), d0 = reinterpret_cast<uintptr_t>(batch->dst);
  if ((d0 & 3u) != 0 || (s0 & (uintptr_t) (elem - 1)) != 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_rectify_batch_run: dst must be 4-byte aligned and src aligned to its element");
  }
  const uintptr_t s1 = s0 + (uintptr_t) src_image * (uintptr_t) batch->batch, d1 = d0 + (uintptr_t) dst_image * (uintptr_t) batch->batch;
  if (s0 < d1 && d0 < s1) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_rectify_batch_run: src and dst overlap");
  }
  RectifyArgs a;
  memset(&a, 0, sizeof(a));
  a.b       = *batch;
  a.border  = border_value(params);
  bool stage = true;
  if (const char* e = getenv("PRS_RECTIFY_VARIANT")) {  // tools: 0 fetches every tap from global memory (the A-B of (a) and (b))
    stage = strtol(e, nullptr, 10) != 0;
  }
  a.tiles_x = (batch->dst_cols + kTileCols - 1) / kTileCols;
  a.tiles_y = (batch->dst_rows + kTileRows - 1) / kTileRows;
  const int64_t tiles = (int64_t) a.tiles_x * a.tiles_y;
  // a workgroup's chunk: as many images as leave eight workgroups for every compute unit, 16 at the most; tests and tools fix it
  int64_t chunk = (int64_t) batch->batch * tiles / ((int64_t) ctx->cus * 8);
  chunk         = chunk < 1 ? 1 : chunk > kChunkMax ? kChunkMax : chunk;
  if (const char* e = getenv("PRS_RECTIFY_CHUNK")) {
    const long forced = strtol(e, nullptr, 10);
    if (forced >= 1 && forced <= kChunkLimit) {
      chunk = forced;
    }
  }
  a.chunk = (int) chunk;
  Launches on(ctx, "prs_rectify_batch_run", ctx_stream(ctx));
  const Grid grid = on.grid(tiles * ((batch->batch + chunk - 1) / chunk), kThreads);
  PRS_TRY(on.check());
  a.stage_ok     = (s0 % 16 == 0 && batch->src_pitch % 16 == 0) ? 1 : 0;
  a.vector_store = (d0 % (uintptr_t) (4 * elem) == 0 && batch->dst_pitch % (4 * elem) == 0) ? 1 : 0;
  if (batch->n_border) {
    const hipError_t e = hipMemsetAsync(batch->n_border, 0, sizeof(int32_t) * (size_t) batch->batch, ctx_stream(ctx));
    if (e != hipSuccess) {
      return ctx_fail_hip(ctx, e, "prs_rectify_batch_run clear");
    }
  }
  const bool bilinear = interp == PRS_RECTIFY_BILINEAR;
  if (type == PRS_PIXEL_U8) {
    launch_rectify<uint8_t>(on, grid, a, bilinear, stage);
  } else if (type == PRS_PIXEL_U16) {
    launch_rectify<uint16_t>(on, grid, a, false, false);
  } else {
    launch_rectify<uint32_t>(on, grid, a, false, false);
  }
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

int prs_rectify_batch_run(prs_context* ctx, const prs_rectify_params* params, const prs_rectify_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return rectify_launch(ctx, params, batch);
}

void prs_rectify_struct_sizes(uint64_t* sizes3) {
  sizes3[0] = sizeof(prs_rectify_map);
  sizes3[1] = sizeof(prs_rectify_params);
  sizes3[2] = sizeof(prs_rectify_batch);
}

}  // extern "C"
