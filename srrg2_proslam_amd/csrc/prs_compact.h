// prs_compact.h -- the pieces the stable stream compactions share (world_map.hip, world_voxel.hip): rows in chunks of one workgroup,
// a count per chunk, one workgroup per sequence that turns the counts into chunk bases, and positions inside a chunk from wave
// ballots.  No atomic takes part: a row's position depends on the rows before it alone.
#pragma once
#include "prs_device.h"

namespace prs {

constexpr int kCompactBatch = 8;  // chunk counts a thread of a scan loads before it looks at one

__device__ __forceinline__ bool finite_bits(const float f) {
  return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u;
}

// n <= C counts at p from chunk c0 on, into v[kCompactBatch] (0 behind the row's end).  The loads are unconditional at a clamped index,
// so the compiler issues them back to back and waits once: a loop of one load per iteration pays one memory latency per chunk
__device__ __forceinline__ void load_counts(const int32_t* p, const int c0, const int C, int32_t (&v)[kCompactBatch]) {
#pragma unroll
  for (int j = 0; j < kCompactBatch; ++j) {
    v[j] = p[c0 + j < C ? c0 + j : C - 1];
  }
#pragma unroll
  for (int j = 0; j < kCompactBatch; ++j) {
    v[j] = c0 + j < C ? v[j] : 0;
  }
}

// the position of this thread's row among the kept rows: *base (the chunk's first output row, read behind the barrier) + the kept
// rows of the waves before this one + the set bits of this wave's ballot below this lane.  s_wave: one int of LDS per wave of the
// workgroup.  Contains one __syncthreads()
__device__ __forceinline__ int chunk_position(const uint64_t mask, int* s_wave, const int32_t* base) {
  const int lane = threadIdx.x & (PRS_WAVE - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_wave[wave] = __popcll(mask);
  }
  __syncthreads();
  int pos = *base;
  for (int v = 0; v < wave; ++v) {
    pos += s_wave[v];
  }
  return lanes_below(mask, pos);
}

}  // namespace prs
