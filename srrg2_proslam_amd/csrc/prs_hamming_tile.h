// prs_hamming_tile.h -- the binary dot-product tile of 256-bit Hamming distances on the matrix cores, shared by the brute-force
// matcher's dense phases (bruteforce.hip) and the place database's candidate search (place_db.hip).
//
// hamming(a, b) = pop(a) + pop(b) - 2 a.b.  With the rows of one side as 0 / 1 bytes and the rows of the other side as +1 / -1 bytes
// (b' = 1 - 2 b), sum_k a_k b'_k = pop(a) - 2 a.b, so hamming(a, b) = (A B'^T)[a][b] + pop(b): a 16 x 16 tile of distances is four
// v_mfma_i32_16x16x64_i8 (K = 256 bits), integer products and sums, exact.  The operand layout inside K is free as long as A and B
// agree: lane (i = l & 15, g = l >> 4) holds, for K block kb, the 16 bits [64 kb + 16 g, +16) of row i as 16 bytes.  The result
// layout is the one tools/probes/mfma_i8_probe.hip pins: register r of lane l = A row 4 (l >> 4) + r, B row l & 15.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prs {

typedef int bf_v4i __attribute__((ext_vector_type(4)));

// the 4-bit -> 4-byte tables for a 16-entry LDS array per side: `nibble` 0..15 -> 0 / 1 bytes (v01) and +1 / -1 bytes (vpm)
__device__ __forceinline__ void hamming_lut_entry(const int nibble, uint32_t& v01, uint32_t& vpm) {
  v01 = 0;
  vpm = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    v01 |= ((nibble >> b) & 1 ? 0x01u : 0x00u) << (8 * b);
    vpm |= ((nibble >> b) & 1 ? 0xffu : 0x01u) << (8 * b);
  }
}

// 16 bits -> the 16 operand bytes of one lane and K block, through one of the tables
__device__ __forceinline__ bf_v4i hamming_expand16(const uint32_t* lut, const uint32_t bits16) {
  bf_v4i v;
  v.x = (int) lut[bits16 & 15u];
  v.y = (int) lut[(bits16 >> 4) & 15u];
  v.z = (int) lut[(bits16 >> 8) & 15u];
  v.w = (int) lut[(bits16 >> 12) & 15u];
  return v;
}

// acc[t] = A[t] B'^T over the four K blocks for four A tiles against one B tile: 16 MFMAs, the four independent chains interleaved
__device__ __forceinline__ void hamming_tiles(const bf_v4i (&A)[4][4], const bf_v4i (&B)[4], bf_v4i (&acc)[4]) {
  const bf_v4i zero = {0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t][0], B[0], zero, 0, 0, 0);
  }
#pragma unroll
  for (int kb = 1; kb < 4; ++kb) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t][kb], B[kb], acc[t], 0, 0, 0);
    }
  }
}

}  // namespace prs
