// Plan of the skinny-M weight-streaming kernel (csrc/kernels/gemv_skinny.hip): a pure host
// function of (N, K, weight bytes) -- never of M or of the values -- so a row of the result
// is computed the same way whatever shares the call with it.  Weight bytes 1 is int8, 2 bf16
// and the code 0 packed 4-bit with one scale per 128 k (a K-step is then one group, so K must
// be a multiple of 128).
//
// The kernel walks K in steps of 128 (one wave reads 16 weight rows x 128 k per step).  A
// workgroup owns `rows` = 16 G consecutive weight rows (G in {1, 2, 4}: the x fragment of a
// step is loaded once for G row groups) and has `ksplit` waves; wave s takes the K-steps
// [s per, (s + 1) per), per = ceil(steps / ksplit), and wave 0 sums the partial tiles of
// waves 1 .. ksplit - 1 from LDS in that order.  There is no split across workgroups.
#pragma once
#include <stdint.h>

namespace gemv {

constexpr int KSTEP = 128;       // k per wave step
constexpr int MAX_M = 16;        // x rows of one call (one MFMA operand)
constexpr int MAX_SPLIT_G1 = 16; // waves of a workgroup at G = 1 (1024 threads)
constexpr int MAX_SPLIT = 8;     // ... at G = 2, 4 (512 threads: up to 256 VGPRs each)

struct Plan {
  int rows = 0;    // weight rows per workgroup: 16, 32 or 64; 0: the shape is not supported
  int ksplit = 0;  // waves per workgroup, each with its own K-steps
  int steps = 0;   // ceil(K / 128)
  int64_t grid = 0;
};

inline int max_split(int rows) { return rows == 16 ? MAX_SPLIT_G1 : MAX_SPLIT; }

// force_split > 0: that many waves (tests reach every reduction path: 1 = none, a count that
// does not divide the steps, more waves than steps)
inline Plan plan(int64_t N, int64_t K, int wbytes, int force_split = 0) {
  Plan p;
  if (N < 1 || K < 32 || K % 32 != 0 || K > (int64_t)1 << 24 || N > (int64_t)1 << 30) return p;
  if (wbytes != 0 && wbytes != 1 && wbytes != 2) return p;
  if (wbytes == 0 && K % KSTEP != 0) return p;
  if (force_split < 0 || force_split > MAX_SPLIT_G1) return p;
  p.steps = (int)((K + KSTEP - 1) / KSTEP);
  // 64 rows per workgroup while that still leaves two workgroups for each of the 256 CUs,
  // then 32, then 16: a small N is spread over as many CUs as it has 16-row groups
  int rows = 64;
  while (rows > 16 && (N + rows - 1) / rows < 512) rows >>= 1;
  if (force_split > max_split(rows)) rows = 16;
  p.rows = rows;
  p.grid = (N + rows - 1) / rows;
  if (force_split > 0) {
    p.ksplit = force_split;
  } else if (wbytes == 0) {
    // a 4-bit step is half the bytes of an int8 one.  16-row workgroups: two steps per wave
    // and up to 16 waves whatever the grid (measured on 4096 x 14336 at M = 1: 13.2 us with
    // 16 waves, 14.7 with 8).  32 and 64 rows: four steps per wave and at most 4 waves, so
    // that two workgroups share a CU (192 VGPRs: 8 waves) and one's reduction runs under the
    // other's loads (128256 x 4096: 73 us with 4 waves, 92 with 8; 16384 x 2048: 8.7 and
    // 10.3; profiles/r13_w4_decode.md)
    const int s = rows == 16 ? p.steps / 2 : (p.steps + 3) / 4;
    const int cap = rows == 16 ? MAX_SPLIT_G1 : 4;
    p.ksplit = s < 1 ? 1 : (s > cap ? cap : s);
  } else {
    // two steps per wave keep a wave's loads deep; fewer than 256 workgroups (rows == 16
    // by then) take up to 16 waves so the CUs that do run hold more loads in flight
    const int cap = p.grid < 256 ? max_split(rows) : MAX_SPLIT;
    int s = p.steps / 2;
    p.ksplit = s < 1 ? 1 : (s > cap ? cap : s);
  }
  return p;
}

}  // namespace gemv
