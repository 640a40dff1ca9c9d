// prs_device.h -- device-side helpers shared by the gfx950 kernels (wave64, LDS, exact float ops).
// Everything that must agree bit-for-bit with a plain sequential float evaluation is written as
// explicit two-operand expressions and the library is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/proslam_hip.h"

#define PRS_WAVE 64

namespace prs {

// 1.0f / x, correctly rounded (the value the IEEE division of the CPU side produces), in 3 + 2 instructions instead of the twelve of
// the compiler's expansion (v_div_scale x 2, v_rcp, 4 x v_fma, v_div_fmas, v_div_fixup).  tools/probes/rcp_exact_probe.hip runs ALL 2^32
// bit patterns on gfx950: v_rcp_f32 followed by ONE Newton step in fused multiply-adds equals the IEEE quotient for every x whose biased
// exponent is 1 .. 252 (2^-126 <= |x| < 2^126; both signs, every mantissa); zeros, denormals, the two largest binades (denormal
// quotients), infinities and NaNs differ.  A wave that holds such an operand takes the compiler's division instead: the depths and
// chi-squares of live correspondences never are, but the stand-in rows of a partially filled wave and of points behind the camera
// carry chi = 0, so those waves take the long form (same bits).  Feeding the unread lanes a benign operand was measured slower
// (round 5: 13.54 / 13.64 ms against 13.34 / 13.38: the select costs every wave what the long form costs a few).
__device__ __forceinline__ float recip_exact(const float x) {
  const float ax  = __builtin_fabsf(x);
  const bool plain = ax >= 0x1p-126f && ax < 0x1p126f;
  if (__builtin_expect(__ballot(!plain) != 0ull, 0)) {
    return 1.0f / x;
  }
  const float y = __builtin_amdgcn_rcpf(x);
  return __builtin_fmaf(__builtin_fmaf(-x, y, 1.0f), y, y);
}

// 256-bit Hamming distance of two 32-byte rows held as 2 x V each, V any vector of four 32-bit words (.x .y .z .w)
// (replaces srrg2_core PointDescriptorField::distance; call site CF/..epipolar_impl.cpp:157)
template <typename V>
__device__ __forceinline__ int hamming256(const V& a0, const V& a1, const V& b0, const V& b1) {
  int d = __popc(a0.x ^ b0.x);
  d += __popc(a0.y ^ b0.y);
  d += __popc(a0.z ^ b0.z);
  d += __popc(a0.w ^ b0.w);
  d += __popc(a1.x ^ b1.x);
  d += __popc(a1.y ^ b1.y);
  d += __popc(a1.z ^ b1.z);
  d += __popc(a1.w ^ b1.w);
  return d;
}

// popcount(x) + acc in ONE instruction (v_bcnt_u32_b32 has the accumulate operand; left to itself the compiler
// reassociates eight of them into a tree of plain popcounts and three-operand adds: 19 instead of 16 instructions per
// 256-bit Hamming distance.  Used where instruction issue is the bound (the projective search); the matcher's scoring
// phase is latency-bound and 3 % faster with the tree)
__device__ __forceinline__ uint32_t popc_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

// LDS written by one lane is read by other lanes of the wave
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t wave_inclusive_scan_u64(uint64_t v) {
  const int lane = threadIdx.x & (PRS_WAVE - 1);
#pragma unroll
  for (int d = 1; d < PRS_WAVE; d <<= 1) {
    const uint64_t o = __shfl_up((unsigned long long) v, d, PRS_WAVE);
    if (lane >= d) {
      v += o;
    }
  }
  return v;
}

// inclusive prefix sum of a 32-bit count over the 64 lanes of a wave by shuffles; `lane` is the caller's lane index (a thread index
// below 64 will do).  The scans inside loops that also broadcast the total (bruteforce.hip, pose_graph.hip) and those of align.hip and
// the first-generation matcher's epilogue spell the same loop out: through this function their kernels compile to other code.
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan_shfl(T v, const int lane) {
#pragma unroll
  for (int d = 1; d < PRS_WAVE; d <<= 1) {
    const T o = __shfl_up(v, d, PRS_WAVE);
    if (lane >= d) {
      v += o;
    }
  }
  return v;
}

// the same sum on the DPP network (was six ds_bpermute round trips): Hillis-Steele inside every row of 16 lanes (row_shr 1, 2, 4, 8,
// lanes shifted in from outside a row read 0), then lane 15 of rows 0 / 2 onto rows 1 / 3 (row_bcast:15) and lane 31 onto the upper
// half (row_bcast:31)
__device__ __forceinline__ uint32_t wave_inclusive_scan_dpp(uint32_t v) {
  v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

// butterfly sum over the 64 lanes of a wave: every lane ends with the total (for floats: in this fixed order)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    v += __shfl_xor(v, m, PRS_WAVE);
  }
  return v;
}

// the least value over the 64 lanes of a wave, in every lane, on the DPP network: rotations inside every row of 16 lanes (row_ror 1, 2,
// 4, 8: every lane of a row holds the row's minimum), lane 15 of rows 0 / 2 onto rows 1 / 3 (row_bcast:15), lane 31 onto the upper half
// (row_bcast:31), and lane 63, which has seen all four rows, read back as a scalar.  Lanes a step does not write keep their own value
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  v = min(v, (uint32_t) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x121, 0xf, 0xf, false));  // row_ror:1
  v = min(v, (uint32_t) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x122, 0xf, 0xf, false));  // row_ror:2
  v = min(v, (uint32_t) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x124, 0xf, 0xf, false));  // row_ror:4
  v = min(v, (uint32_t) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x128, 0xf, 0xf, false));  // row_ror:8
  v = min(v, (uint32_t) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1, 3
  v = min(v, (uint32_t) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2, 3
  return (uint32_t) __builtin_amdgcn_readlane((int) v, 63);
}

// base + number of set bits of m below this lane
__device__ __forceinline__ int lanes_below(uint64_t m, int base) {
  return (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, (uint32_t) base));
}

// order-preserving map of a float onto unsigned integers (no NaN), and back
__device__ __forceinline__ uint32_t ordered(const float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered(const uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// triangulateRectifiedMidpoint (mapping/triangulator_rigid_stereo.cpp:39-45,60-85, operation order kept): the point of a rectified
// stereo pair in the left camera, w = 1; all zero when the disparity is below the minimum (a NaN disparity is not)
__device__ __forceinline__ float4 triangulate_rectified(const prs_triangulator_params& t, const float x_L, const float y_L, const float x_R,
                                                        const float y_R) {
  float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!(x_L - x_R < t.minimum_disparity_pixels)) {
    float depth = t.infinity_depth_meters;
    if (x_L > x_R) {
      depth = t.b_x / (x_L - x_R);
    }
    pt.z = depth;
    pt.x = 1 / t.fx * (x_L - t.cx) * depth;
    pt.y = 1 / t.fy * ((y_L + y_R) / 2 - t.cy) * depth;
    pt.w = 1.0f;
  }
  return pt;
}

// exclusive prefix over all threads of the block (blockDim.x multiple of 64, <= 1024).
// scratch: >= 17 uint64_t in LDS.  Contains two __syncthreads().
__device__ __forceinline__ uint64_t block_exclusive_scan_u64(uint64_t v, uint64_t* scratch, uint64_t& total) {
  const int lane   = threadIdx.x & (PRS_WAVE - 1);
  const int wave   = threadIdx.x >> 6;
  const int nwaves = blockDim.x >> 6;
  const uint64_t incl = wave_inclusive_scan_u64(v);
  if (lane == PRS_WAVE - 1) {
    scratch[wave] = incl;
  }
  __syncthreads();
  uint64_t base = 0;
  uint64_t all  = 0;
  for (int w = 0; w < nwaves; ++w) {
    const uint64_t t = scratch[w];
    if (w < wave) {
      base += t;
    }
    all += t;
  }
  total = all;
  __syncthreads();
  return base + incl - v;
}

} // namespace prs
