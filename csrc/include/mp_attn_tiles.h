// Tile helpers shared by the flash-attention kernels (attention.hip's kernel headers
// mp_attn_fwd.h / mp_attn_bwd_*.h through mp_attn_common.h, attention_doc.hip, attention_append.hip):
// the XOR-swizzled [rows][DP] bf16 LDS image, its row / transposed reads, the MFMA and
// pack wrappers and the register staging of a 64-row global tile.
#pragma once
#include "mp_common.h"

using namespace mp;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

#define LOG2E 1.4426950408889634f

// ------------------------------------------------------------------------------------------
// LDS image: [rows][DP] bf16, 16-byte chunks XOR-swizzled per row.
// ------------------------------------------------------------------------------------------
template <int DP>
__device__ __forceinline__ int chunk_swz(int row) {
  if constexpr (DP == 64) return (((row >> 1) & 1) << 2) | ((row >> 2) & 3);
  else return ((row & 3) << 2) | ((row >> 2) & 3);
}

template <int DP>
__device__ __forceinline__ int lds_off(int row, int chunk) {  // byte offset of a 16-byte chunk
  return row * (DP * 2) + 16 * (chunk ^ chunk_swz<DP>(row));
}

// 16-byte row read (A operand: rows on lanes 0..31, 8 consecutive columns)
template <int DP>
__device__ __forceinline__ bf16x8 lds_row8(const char* base, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(base + lds_off<DP>(row, chunk));
}

// Transposed read: returns for this lane the 4 rows r0..r0+3 of column (c0 + (lane&15)).
// Lane 4q+p of each 16-lane group addresses row r0+q, columns c0+4p..c0+4p+3.
template <int DP>
__device__ __forceinline__ s16x4 lds_tr4(const char* base, int r0, int c0) {
  const int i = threadIdx.x & 15;
  const int q = i >> 2, p = i & 3;
  const int row = r0 + q;
  const int col = c0 + 4 * p;
  const char* a = base + lds_off<DP>(row, col >> 3) + ((col & 7) << 1);
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
}

__device__ __forceinline__ bf16x8 cat44(s16x4 lo, s16x4 hi) {
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& acc, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)acc[8 * s + j];
  return r;
}

// load 8 bf16 of a global row (zero outside [0, D) or invalid row)
__device__ __forceinline__ u16x8 gload8(const bf16_t* rowp, int col, int D, bool valid) {
  u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!valid || col >= D) return z;
  return *reinterpret_cast<const u16x8*>(rowp + col);
}

// Stage a [64][DP] tile of rows (row0 .. row0+63 of a token-major tensor) into registers.
template <int DP>
struct Stage64 {
  static constexpr int PER = DP / 32;  // 16-byte chunks per thread
  u16x8 v[PER];
  __device__ __forceinline__ void load(const bf16_t* base, int64_t stride, int row0, int nrows, int D) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int r = idx / (DP / 8), c = idx % (DP / 8);
      const int gr = row0 + r;
      v[i] = gload8(base + (int64_t)gr * stride, c * 8, D, gr < nrows);
    }
  }
  __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int r = idx / (DP / 8), c = idx % (DP / 8);
      *reinterpret_cast<u16x8*>(lds + lds_off<DP>(r, c)) = v[i];
    }
  }
};
