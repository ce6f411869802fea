// The combine pass of the key-split attention kernels (attention_decode.hip,
// attention_append.hip): merges the per-split partial outputs of one (row, head) in split
// order.  Each including file gets its own copy (anonymous namespace).
#pragma once
#include "mp_common.h"

namespace {

constexpr int kSplitMaxSplits = 256;

// part_o [rows, H, nsplit, D] unnormalised f32 outputs, part_ml [rows, H, nsplit, 2] their
// (max, sum) in exp2 units; grid (H, min(rows, 65535), ceil(rows / 65535)), D threads.
// out[row, h, :] = sum_s o_s 2^(m_s - M) / sum_s l_s 2^(m_s - M), splits in index order
template <int D>
__global__ __launch_bounds__(D) void attn_split_combine(const float* __restrict__ part_o,
                                                        const float* __restrict__ part_ml,
                                                        mp::bf16_t* __restrict__ o, int rows, int H, int nsplit,
                                                        int64_t o_stride) {
  const int h = blockIdx.x, b = blockIdx.y + 65535 * blockIdx.z, d = threadIdx.x;
  if (b >= rows) return;     // uniform over the workgroup
  const int64_t row0 = ((int64_t)b * H + h) * nsplit;
  // the splits' (max, sum) pairs: loaded side by side, not one round trip per split
  __shared__ float sh_m[kSplitMaxSplits], sh_w[kSplitMaxSplits];
  for (int s = d; s < nsplit; s += D) {
    sh_m[s] = part_ml[(row0 + s) * 2];
    sh_w[s] = part_ml[(row0 + s) * 2 + 1];
  }
  __syncthreads();
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, sh_m[s]);
  const float ms = M == -INFINITY ? 0.f : M;
  // every thread sums in split order; an empty split, (-inf, 0) with a zero row, has weight 0
  float L = 0.f, O = 0.f;
#pragma unroll 8
  for (int s = 0; s < nsplit; ++s) {
    const float sc = __builtin_amdgcn_exp2f(sh_m[s] - ms);
    L += sh_w[s] * sc;
    O += part_o[(row0 + s) * D + d] * sc;
  }
  o[(int64_t)b * o_stride + (int64_t)h * D + d] = mp::f2bf(L > 0.f ? O / L : 0.f);
}

inline dim3 attn_split_combine_grid(int rows, int H) {
  return dim3(H, rows < 65535 ? rows : 65535, (rows + 65534) / 65535);
}

}  // namespace
