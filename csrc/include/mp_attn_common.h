// Helpers that more than one kernel header of attention.hip uses (mp_attn_fwd.h,
// mp_attn_bwd_dkdv.h, mp_attn_bwd_dq.h, mp_attn_bwd_short.h): the dropout index, the LDS-DMA
// tile loaders (GTileP, GTile, BTile), the fused bias-gradient column sums, counted vmcnt
// waits and the one-compare mask / cross-half reductions of the v2 kernels.  Kept out of
// mp_attn_tiles.h, which attention_doc.hip and attention_append.hip also include.
#pragma once
#include "mp_attn_plan.h"   // MP_FWD_NBUF, MP_DKDV_NBUF
#include "mp_attn_tiles.h"

#include <type_traits>

// dropout element index of score (bh, q, k): bh in the high word, q * Sk + k in the low
// word (the kernels use drop_key(seed, bh) + the low word directly; this is the reference)
__device__ __forceinline__ uint64_t drop_idx(int bh, int q, int k, int Sk) {
  return ((uint64_t)bh * 0x100000000ull) + (uint64_t)q * (uint64_t)Sk + (uint64_t)k;
}

template <int DP>
struct GTileP {   // a [64][DP] tile by the 2 waves of one pair, LDS-DMA (the GTile scheme below)
  static constexpr int CPR = DP / 8;           // 16-byte chunks per row
  static constexpr int PR = 1024 / (DP * 2);   // rows per 1 KiB piece
  static constexpr int PPW = (64 / PR) / 2;    // pieces per wave
  int lr, phys;
  __device__ __forceinline__ void init() {
    const int lane = threadIdx.x & 63;
    lr = lane / CPR;
    phys = lane % CPR;
  }
  __device__ __forceinline__ void issue(const bf16_t* base, int64_t stride, int row0, int nrows, int D, char* img,
                                        int wv) const {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int p = wv + 2 * i;
      const int row = p * PR + lr;
      const int chunk = (phys & ~15) | ((phys & 15) ^ chunk_swz<DP>(row));
      int col = chunk * 8;
      col = col < D ? col : 0;
      int gr = row0 + row;
      gr = gr < nrows ? gr : nrows - 1;   // rows past the end: masked keys / zero probabilities
      __builtin_amdgcn_global_load_lds((const void*)(base + (int64_t)gr * stride + col),
                                       (__attribute__((address_space(3))) void*)(img + p * 1024), 16, 0, 0);
    }
  }
};

// ==========================================================================================
// glds staging of [64][DP] row tiles straight into the swizzled LDS image
// ==========================================================================================
// A 1 KiB LDS-DMA piece is PR = 1024 / (2 DP) image rows; lane l lands at byte 16 l of the
// piece, so the XOR swizzle is applied on the SOURCE column (cdna guide §5.4 rule 21).
// Columns past D (head dim padded to DP) read column 0 of the same row instead: finite
// data that only meets zero K/V columns or feeds unwritten output columns.
template <int DP>
struct GTile {
  static constexpr int CPR = DP / 8;           // 16-byte chunks per row
  static constexpr int PR = 1024 / (DP * 2);   // rows per piece
  static constexpr int PPW = (64 / PR) / 4;    // pieces per wave (4 waves)
  int lr, phys;
  __device__ __forceinline__ void init() {
    const int lane = threadIdx.x & 63;
    lr = lane / CPR;
    phys = lane % CPR;
  }
  // rows row0 .. row0+63 of a token-major tensor (row stride `stride`, column offset
  // already in `base`) -> LDS image `img`
  __device__ __forceinline__ void issue(const bf16_t* base, int64_t stride, int row0, int nrows, int D, char* img,
                                        int wave) const {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int p = wave + 4 * i;
      const int row = p * PR + lr;
      const int chunk = (phys & ~15) | ((phys & 15) ^ chunk_swz<DP>(row));
      int col = chunk * 8;
      col = col < D ? col : 0;
      int gr = row0 + row;
      gr = gr < nrows ? gr : nrows - 1;
      __builtin_amdgcn_global_load_lds((const void*)(base + (int64_t)gr * stride + col),
                                       (__attribute__((address_space(3))) void*)(img + p * 1024), 16, 0, 0);
    }
  }
};

// Column sums over a workgroup's 128 token rows of a [rows][D] f32 register tile (lane =
// row 32 w + l32, register 4g + e of acc[d] = column 32d + 8g + 4hl + e), times `mul`,
// atomically added to out[0 .. D): the bias gradient of the QKV projection, fused into the
// attention backward instead of a second pass over dQKV.  Sums over the 32 lanes of each
// half by xor-shuffles, over the 4 waves through LDS (`red`, >= 4 * DP floats; the caller
// has synchronised so it is free), then one atomic per column per workgroup.
template <int DP>
__device__ __forceinline__ void wg_colsum_atomic(const f32x16 (&acc)[DP / 32], float mul, bool valid, float* red,
                                                 float* __restrict__ out, int D) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, l32 = lane & 31;
#pragma unroll
  for (int d = 0; d < DP / 32; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x = valid ? acc[d][r] * mul : 0.f;
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) x += __shfl_xor(x, o, 64);
      if (l32 == 0) red[w * DP + 32 * d + 8 * (r >> 2) + 4 * hl + (r & 3)] = x;
    }
  __syncthreads();
  for (int c = threadIdx.x; c < DP; c += 256)
    if (c < D) atomicAdd(out + c, red[c] + red[DP + c] + red[2 * DP + c] + red[3 * DP + c]);
}

template <int N>
__device__ __forceinline__ void attn_wait_vmcnt() {
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | (((N >> 4) & 3) << 14));
}

__device__ __forceinline__ float xhalf_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return max3_raw(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// GTile's 1 KiB-piece layout issued as buffer_load ... lds: the per-lane byte offset of each
// piece is fixed at kernel entry (32-bit), the tile's row offset is a scalar, and rows past
// the buffer's range (keys >= Sk) land as zeros -- no 64-bit address math per tile
template <int DP>
struct BTile {
  static constexpr int CPR = DP / 8, PR = 1024 / (DP * 2), PPW = (64 / PR) / 4;
  int voff[PPW];
  __device__ __forceinline__ void init(int64_t stride, int D, int wave) {
    const int lane = threadIdx.x & 63, lr = lane / CPR, phys = lane % CPR;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int row = (wave + 4 * i) * PR + lr;
      const int chunk = (phys & ~15) | ((phys & 15) ^ chunk_swz<DP>(row));
      const int col = chunk * 8 < D ? chunk * 8 : 0;
      voff[i] = (int)(((int64_t)row * stride + col) * 2);
    }
  }
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rs, int soff, char* img, int wave) const {
    // (the builtin exists for the gfx950 pass only; the host pass would drop the kernel's stubs)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < PPW; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + (wave + 4 * i) * 1024),
                                               16, voff[i], soff, 0, 0);
#endif
  }
};

// max over the 32 scores of a lane (two 32x32 accumulators): 16 dependent v_max3_f32 in two
// asm blocks (fmaxf would canonicalise every MFMA output first; one asm statement per max3
// made the compiler pad each with an s_nop)
__device__ __forceinline__ float tile_max32(const f32x16& a, const f32x16& b) {
  float m;
  asm("v_max3_f32 %0, %1, %2, %3\n\t"
      "v_max3_f32 %0, %0, %4, %5\n\t"
      "v_max3_f32 %0, %0, %6, %7\n\t"
      "v_max3_f32 %0, %0, %8, %9\n\t"
      "v_max3_f32 %0, %0, %10, %11\n\t"
      "v_max3_f32 %0, %0, %12, %13\n\t"
      "v_max3_f32 %0, %0, %14, %15\n\t"
      "v_max3_f32 %0, %0, %16, %17"
      : "=&v"(m)
      : "v"(a[0]), "v"(b[0]), "v"(a[1]), "v"(b[1]), "v"(a[2]), "v"(b[2]), "v"(a[3]), "v"(b[3]), "v"(a[4]), "v"(b[4]),
        "v"(a[5]), "v"(b[5]), "v"(a[6]), "v"(b[6]), "v"(a[7]), "v"(b[7]), "v"(-INFINITY));
  float m2;
  asm("v_max3_f32 %0, %1, %2, %3\n\t"
      "v_max3_f32 %0, %0, %4, %5\n\t"
      "v_max3_f32 %0, %0, %6, %7\n\t"
      "v_max3_f32 %0, %0, %8, %9\n\t"
      "v_max3_f32 %0, %0, %10, %11\n\t"
      "v_max3_f32 %0, %0, %12, %13\n\t"
      "v_max3_f32 %0, %0, %14, %15\n\t"
      "v_max3_f32 %0, %0, %16, %17"
      : "=&v"(m2)
      : "v"(m), "v"(a[8]), "v"(b[8]), "v"(a[9]), "v"(b[9]), "v"(a[10]), "v"(b[10]), "v"(a[11]), "v"(b[11]),
        "v"(a[12]), "v"(b[12]), "v"(a[13]), "v"(b[13]), "v"(a[14]), "v"(b[14]), "v"(a[15]), "v"(b[15]));
  return m2;
}

// in-tile key offset of accumulator register r (lane half hl adds 4)
__device__ __forceinline__ constexpr int key_of(int r) { return (r & 3) + 8 * (r >> 2); }
