// Plan of the MXFP8 x MXFP4 GEMM (csrc/kernels/gemm_mx.hip): a pure host function of (M, N, K),
// never of the values.  It picks the tile of y a 4-wave workgroup owns; the K-chain of an output
// element -- one f32 accumulator, K-steps of 128 in ascending order -- is the same in every
// tile, so the plan changes where a row is computed and never its bits.
//
//   NARROW  64 x 32   M <= 64: the weight matrix is streamed once, and 32 columns per workgroup
//                     spread an N of a few thousand over every CU (N = 4096: 128 workgroups)
//   SQUARE  128 x 128 a prefill: each staged byte of x feeds 128 columns, each of w 128 rows
//
// Not reported through _C.gemv_plan: that entry's (N, K, wbytes, force_split) has no M.
#pragma once
#include <stdint.h>

namespace gemm_mx {

constexpr int KSTEP = 128;   // k per step: one scaled MFMA, four MX groups of a row
constexpr int GROUP = 32;    // k per e8m0 scale byte
constexpr int THREADS = 256;

enum Tile { NONE = 0, NARROW = 1, SQUARE = 2 };

struct Plan {
  int tile = NONE;   // NONE: the shape is not supported
  int bm = 0, bn = 0;
  int steps = 0;     // K / 128
  int64_t grid_m = 0, grid_n = 0;
};

// bytes of one MXFP8 activation row: K e4m3 codes, K / 32 e8m0 bytes, zero padding to 16
inline int64_t mx8_row_bytes(int64_t K) { return (K + K / GROUP + 15) / 16 * 16; }

inline Plan plan(int64_t M, int64_t N, int64_t K) {
  Plan p;
  if (M < 1 || N < 1 || K < KSTEP || K % KSTEP != 0 || K > (int64_t)1 << 24 || N > (int64_t)1 << 30 ||
      M > (int64_t)1 << 30)
    return p;
  p.tile = M <= 64 ? NARROW : SQUARE;
  p.bm = p.tile == NARROW ? 64 : 128;
  p.bn = p.tile == NARROW ? 32 : 128;
  p.steps = (int)(K / KSTEP);
  p.grid_m = (M + p.bm - 1) / p.bm;
  p.grid_n = (N + p.bn - 1) / p.bn;
  if (p.grid_m > 65535) return Plan();      // the grid's y dimension
  return p;
}

}  // namespace gemm_mx
