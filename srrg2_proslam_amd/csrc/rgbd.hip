// rgbd.hip -- the RGB-D preprocessor on the device: RawDataPreprocessorMonocularDepth::_readDepth
// (sensor_processing/raw_data_preprocessor_monocular_depth.cpp:156-180) and its status rules (:131-145), run behind a feature
// extractor on its outputs in place (include/proslam_hip.h).
//
// One launch per batch:
//   depth_kernel  one workgroup of 256 threads per image walks the image's features in chunks of 256.  Each lane takes one
//                 feature: reads its (u, v) (8 B), rounds with rintf (half to even, like std::rint), checks the index against
//                 the depth image and gathers the depth element.  The kept lanes are compacted stably: a wave ballot of the
//                 keep flags, mbcnt for the rank inside the wave, an exclusive scan of the waves' counts through LDS (double
//                 buffered, so one barrier per chunk) and a running base carried to the next chunk.  Kept lanes write
//                 (u, v, d, 0) as one 16-byte store, the 32-byte descriptor row as two 16-byte stores and the intensity.
//                 A keypoint outside the image stops the image at the end of its chunk (PRS_ERR_RANGE for that image).
#include <math.h>
#include <string.h>

#include "prs_device.h"
#include "prs_host.h"
#include "prs_image.h"

namespace prs {

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

struct DepthArgs {
  prs_depth_batch b;
  int depth_type;
  float scale;
};

__global__ __launch_bounds__(kThreads) void depth_kernel(const DepthArgs a) {
  __shared__ int wave_kept[2][kWaves];
  __shared__ int wave_bad[2][kWaves];
  const prs_depth_batch& B = a.b;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int es = B.extract_status ? B.extract_status[f] : 0;
  const int n  = B.n_features[f];
  __syncthreads();  // extract_status may alias status: every lane has read it before lane 0 writes it
  int st = 0, kept = 0;
  if (es < 0) {
    st = es;
  } else if (n > B.stride) {
    st = PRS_ERR_CAPACITY;
  } else if (n < 0) {
    st = PRS_ERR_RANGE;
  } else {
    const size_t row0 = (size_t) f * (size_t) B.stride;
    const unsigned char* image = static_cast<const unsigned char*>(B.depth) + (size_t) f * (size_t) B.rows * (size_t) B.pitch;
    const float rows = (float) B.rows, cols = (float) B.cols;
    bool bad = false;
    for (int c0 = 0, k = 0; c0 < n; c0 += kThreads, ++k) {
      const int i = c0 + tid;
      bool keep = false, outside = false;
      float u = 0.f, v = 0.f, raw = 0.f;
      if (i < n) {
        const prs_kp2 kp = B.keypoints[row0 + i];
        u = kp.u;
        v = kp.v;
        const float r = rintf(v), c = rintf(u);
        if (r >= 0.f && r < rows && c >= 0.f && c < cols) {  // NaN fails every comparison: outside
          const unsigned char* line = image + (size_t) (int) r * (size_t) B.pitch;
          raw  = a.depth_type == PRS_DEPTH_U16 ? (float) reinterpret_cast<const uint16_t*>(line)[(int) c]
                                               : reinterpret_cast<const float*>(line)[(int) c];
          keep = raw > 0.f;
        } else {
          outside = true;
        }
      }
      const uint64_t keep_mask = __ballot(keep), bad_mask = __ballot(outside);
      const int buf = k & 1;
      if (lane == 0) {
        wave_kept[buf][wave] = __popcll(keep_mask);
        wave_bad[buf][wave]  = bad_mask != 0ull;
      }
      __syncthreads();
      int before = 0, total = 0, any_bad = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int cnt = wave_kept[buf][w];
        before += w < wave ? cnt : 0;
        total += cnt;
        any_bad |= wave_bad[buf][w];
      }
      if (any_bad) {  // uniform over the workgroup
        bad = true;
        break;
      }
      if (keep) {
        const size_t o = row0 + (size_t) (kept + before + lanes_below(keep_mask, 0));
        reinterpret_cast<float4*>(B.fixed)[o] = make_float4(u, v, a.scale * raw, 0.f);
        const uint4* src = reinterpret_cast<const uint4*>(B.descriptors + (row0 + i) * PRS_DESC_BYTES);
        uint4* dst       = reinterpret_cast<uint4*>(B.fixed_desc + o * PRS_DESC_BYTES);
        const uint4 d0 = src[0], d1 = src[1];
        dst[0] = d0;
        dst[1] = d1;
        if (B.intensity) {
          B.fixed_intensity[o] = B.intensity[row0 + i];
        }
      }
      kept += total;
    }
    if (bad) {
      st = PRS_ERR_RANGE;
    } else if (kept == 0) {
      st = PRS_WARN_NO_MATCHES;  // :131-136 (and the extractor's "no keypoints")
    } else if ((float) (n - kept) / (float) n > 0.25f) {
      st = PRS_WARN_SPARSE_DEPTH;  // :139-145, float division as in the reference
    }
  }
  if (tid == 0) {
    B.n_fixed[f] = st < 0 ? 0 : kept;
    B.status[f]  = st;
  }
}

// call-level checks shared by both entry points; returns PRS_OK or the failure (already recorded in ctx)
int check_params(prs_context* ctx, const prs_depth_params* params, int rows, int cols, int pitch, const char* who) {
  const int64_t elem = depth_bytes(params->depth_type);
  if (elem == 0) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, who);
  }
  if (!isfinite(params->depth_scaling_factor_to_meters)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, who);
  }
  if (rows < 1 || cols < 1 || !pitch_ok(pitch, cols, elem)) {
    return ctx_fail(ctx, PRS_ERR_RANGE, who);
  }
  return PRS_OK;
}

}  // namespace

int depth_measurements_launch(prs_context* ctx, const prs_depth_params* params, const prs_depth_batch* batch) {
  if (!params || !batch) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_depth_measurements_batch: parameters not set");
  }
  if (!batch->depth || !batch->keypoints || !batch->descriptors || !batch->n_features || !batch->fixed || !batch->fixed_desc ||
      !batch->n_fixed || !batch->status || (!batch->intensity != !batch->fixed_intensity)) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_depth_measurements_batch: input or output buffer not set (intensity and fixed_intensity go together)");
  }
  const int rc = check_params(ctx, params, batch->rows, batch->cols, batch->pitch,
                              "prs_depth_measurements_batch: unknown depth_type, non-finite scale, or invalid size or pitch");
  if (rc != PRS_OK) {
    return rc;
  }
  if (batch->batch <= 0) {
    return PRS_OK;
  }
  if (batch->stride < 1) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_depth_measurements_batch: stride below 1");
  }
  const int64_t elem = depth_bytes(params->depth_type);
  if (!aligned_to(batch->fixed, 16) || !aligned_to(batch->fixed_desc, 16) || !aligned_to(batch->descriptors, 16) || !aligned_to(batch->keypoints, 8) ||
      !aligned_to(batch->depth, (size_t) elem)) {
    return ctx_fail(ctx, PRS_ERR_UNSUPPORTED, "prs_depth_measurements_batch: fixed / descriptor rows must be 16-byte aligned");
  }
  Launches on(ctx, "prs_depth_measurements_batch", ctx_stream(ctx));
  const Grid grid = on.grid(batch->batch, kThreads);
  PRS_TRY(on.check());
  DepthArgs a;
  memset(&a, 0, sizeof(a));
  a.b          = *batch;
  a.depth_type = params->depth_type;
  a.scale      = params->depth_scaling_factor_to_meters;
  on.launch(depth_kernel, grid, 0, a);
  return on.finish();
}

}  // namespace prs

using namespace prs;

extern "C" {

int prs_depth_measurements_batch(prs_context* ctx, const prs_depth_params* params, const prs_depth_batch* batch) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  (void) hipSetDevice(ctx->device);
  return depth_measurements_launch(ctx, params, batch);
}

int prs_depth_measurements(prs_context* ctx, const prs_depth_params* params, const void* depth, int32_t rows, int32_t cols,
                           int32_t pitch, const float* keypoints, const float* intensity, const uint8_t* descriptors,
                           int32_t n, float* uvd, float* intensity_out, uint8_t* desc_out, int32_t* n_fixed) {
  if (!ctx) {
    return PRS_ERR_NULL;
  }
  if (!params || !depth || !n_fixed || (n > 0 && (!keypoints || !descriptors || !uvd || !desc_out))) {
    return ctx_fail(ctx, PRS_ERR_NULL, "prs_depth_measurements: input or output buffer not set");
  }
  *n_fixed = 0;
  PRS_TRY(check_params(ctx, params, rows, cols, pitch, "prs_depth_measurements: unknown depth_type, non-finite scale, or invalid size or pitch"));
  if (n < 0) {
    return ctx_fail(ctx, PRS_ERR_RANGE, "prs_depth_measurements: negative feature count");
  }
  (void) hipSetDevice(ctx->device);
  const bool with_int      = intensity && intensity_out;
  const size_t cap         = (size_t) (n > 0 ? n : 1);
  const size_t elem        = (size_t) depth_bytes(params->depth_type);
  const size_t depth_bytes = (size_t) (rows - 1) * (size_t) pitch + (size_t) cols * elem;
  struct Meta {
    int32_t n_features, status, n_fixed;
  };
  // depth | keypoints | intensity | descriptors (uploaded) | meta | fixed | fixed intensity | fixed descriptors (downloaded)
  Staging st(ctx, "prs_depth_measurements");
  auto dimg  = st.up<uint8_t>((size_t) rows * (size_t) pitch);
  auto kp    = st.up<prs_kp2>(cap);
  auto inten = st.up<float>(cap);
  auto desc  = st.up<uint8_t>(cap * PRS_DESC_BYTES);
  auto meta  = st.both<Meta>(1);
  auto fixed = st.down<float>(cap * 4);
  auto fint  = st.down<float>(cap);
  auto fdesc = st.down<uint8_t>(cap * PRS_DESC_BYTES);
  PRS_TRY(st.commit());
  memcpy(dimg.h(), depth, depth_bytes);
  if (n > 0) {
    memcpy(kp.h(), keypoints, (size_t) n * sizeof(prs_kp2));
    memcpy(desc.h(), descriptors, (size_t) n * PRS_DESC_BYTES);
    if (with_int) {
      memcpy(inten.h(), intensity, (size_t) n * sizeof(float));
    }
  }
  *meta.h() = {n, 0, 0};
  PRS_TRY(st.upload());
  prs_depth_batch b;
  memset(&b, 0, sizeof(b));
  b.batch           = 1;
  b.rows            = rows;
  b.cols            = cols;
  b.pitch           = pitch;
  b.depth           = dimg.d();
  b.stride          = (int32_t) cap;
  b.keypoints       = kp.d();
  b.intensity       = with_int ? inten.d() : nullptr;
  b.descriptors     = desc.d();
  b.n_features      = &meta.d()->n_features;
  b.fixed           = fixed.d();
  b.fixed_desc      = fdesc.d();
  b.fixed_intensity = with_int ? fint.d() : nullptr;
  b.n_fixed         = &meta.d()->n_fixed;
  b.status          = &meta.d()->status;
  PRS_TRY(depth_measurements_launch(ctx, params, &b));
  PRS_TRY(st.download());
  const int32_t status = meta.h()->status, k = meta.h()->n_fixed;
  if (status < 0) {
    return ctx_fail(ctx, status, "prs_depth_measurements: a keypoint lies outside the depth image");
  }
  const float* fx = fixed.h();
  for (int32_t i = 0; i < k; ++i) {
    uvd[3 * (size_t) i]     = fx[4 * (size_t) i];
    uvd[3 * (size_t) i + 1] = fx[4 * (size_t) i + 1];
    uvd[3 * (size_t) i + 2] = fx[4 * (size_t) i + 2];
  }
  if (with_int) {
    memcpy(intensity_out, fint.h(), (size_t) k * sizeof(float));
  }
  memcpy(desc_out, fdesc.h(), (size_t) k * PRS_DESC_BYTES);
  *n_fixed = k;
  return status;
}

}  // extern "C"
