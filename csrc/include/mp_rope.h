// Rotate-half RoPE arithmetic shared by rope_kernel (elementwise.hip: whole sequences, one
// host pos_offset) and rope_kv_append_kernel (generate.hip: one token per sequence at a
// device-side position), so both produce the same bits for the same position.
#pragma once
#include "mp_common.h"

namespace mp {

// four (x1, x2) pairs of one head: x1 = elements [j0, j0 + 4) of the first half, x2 the same
// of the second half; cs_row / sn_row = the position's row of the [S, Dh/2] f32 tables
__device__ __forceinline__ void rope_rot4(const u16x4 x1, const u16x4 x2, const float* __restrict__ cs_row,
                                          const float* __restrict__ sn_row, int j0, float sign, u16x4& o1,
                                          u16x4& o2) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = j0 + e;
    const float c = cs_row[j], s = sign * sn_row[j];
    const float a = bf2f(x1[e]), b = bf2f(x2[e]);
    o1[e] = f2bf(a * c - b * s);
    o2[e] = f2bf(b * c + a * s);
  }
}

}  // namespace mp
