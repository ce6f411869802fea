// Arguments and per-lane operand fragments shared by the weight-streaming linear kernels
// (csrc/kernels/gemv_skinny.hip: up to 16 x rows; csrc/kernels/gemv_rows64.hip: 17 .. 64).
// Both read a step's weights the same way and feed the same k to the same MFMA slot, which
// is what makes a row of their results bitwise equal.
#pragma once
#include "mp_common.h"

namespace mp {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

struct GemvArgs {
  const void* w;          // [N, K] int8 or bf16 or [N, K / 2] packed 4-bit, row-major, rows 16-byte aligned
  const float* scale;     // [N] (int8), [K / 128, N] (4-bit), the e8m0 bytes [N, K / 32] of MXFP4 weights, or null
  const bf16_t* x;        // [M, ldx]
  bf16_t* y;              // [M, ldy]
  const bf16_t* bias;     // [N] or null
  const bf16_t* res;      // [M, ldr] or null
  int M, N, K, gelu;
  int64_t ldx, ldy, ldr;
};

// The C entries' arguments as GemvArgs.  False: w is not 16-byte aligned (every kernel reads a
// lane's weights of a step as 16-byte loads).  What a scale must be is the entry's own condition.
inline bool gemv_args(GemvArgs& a, const void* w, const void* scale, const void* x, void* y, const void* bias,
                      const void* res, int M, int N, int K, int64_t ldx, int64_t ldy, int64_t ldr, int gelu) {
  a.w = w, a.scale = (const float*)scale, a.x = (const bf16_t*)x, a.y = (bf16_t*)y;
  a.bias = (const bf16_t*)bias, a.res = (const bf16_t*)res;
  a.M = M, a.N = N, a.K = K, a.gelu = gelu, a.ldx = ldx, a.ldy = ldy, a.ldr = ldr;
  return ((uintptr_t)w & 15) == 0;
}

// The f32 epilogue of one result element, y[m, n] = bf16(epi(v)): the per-row scale (int8
// weights), bias, GELU on the bf16-rounded pre-activation (as the bf16 GEMM's epilogue takes it:
// mp_gemm_core.h), residual.  One copy for every kernel here, so a row's bits cannot depend on
// which of them ran.
__device__ __forceinline__ void gemv_store(const GemvArgs& a, float v, int m, int64_t n, bool row_scale) {
  if (row_scale) v *= a.scale[n];
  if (a.bias) v += bf2f(a.bias[n]);
  if (a.gelu) v = gelu_tanh(IO8<bf16_t>::get_round(v));
  if (a.res) v += bf2f(a.res[(int64_t)m * a.ldr + n]);
  a.y[(int64_t)m * a.ldy + n] = f2bf(v);
}

// the lane's 32 weights of one step as four MFMA fragments
template <typename WT>
struct WFrag;
template <>
struct WFrag<bf16_t> {
  u16x8 v[4];
  __device__ __forceinline__ void load(const bf16_t* p) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const u16x8*>(p + 8 * j);
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (u16x8)(0);
  }
  __device__ __forceinline__ bf16x8 frag(int j) const { return __builtin_bit_cast(bf16x8, v[j]); }
};
template <>
struct WFrag<int8_t> {
  u32x4 v[2];
  __device__ __forceinline__ void load(const int8_t* p) {
    v[0] = *reinterpret_cast<const u32x4*>(p);
    v[1] = *reinterpret_cast<const u32x4*>(p + 16);
  }
  __device__ __forceinline__ void zero() { v[0] = v[1] = (u32x4)(0u); }
  // bytes + 128 are unsigned (v_cvt_f32_ubyteN), minus 128 is exact in f32, and an integer of
  // magnitude <= 128 keeps all its bits in the upper half of the f32 word
  static __device__ __forceinline__ uint32_t pair(uint32_t u, int lo) {
    const float a = (float)((u >> (8 * lo)) & 0xffu) - 128.0f;
    const float b = (float)((u >> (8 * lo + 8)) & 0xffu) - 128.0f;
    return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u);
  }
  __device__ __forceinline__ bf16x8 frag(int j) const {
    const uint32_t d0 = v[j >> 1][2 * (j & 1)] ^ 0x80808080u, d1 = v[j >> 1][2 * (j & 1) + 1] ^ 0x80808080u;
    u32x4 r = {pair(d0, 0), pair(d0, 2), pair(d1, 0), pair(d1, 2)};
    return __builtin_bit_cast(bf16x8, r);
  }
};

// the lane's 32 x values of one step; XA: 16-byte aligned rows (vector loads)
template <bool XA>
struct XFrag {
  u16x8 v[4];
  __device__ __forceinline__ void load(const bf16_t* p, bool on) {
    if (!on) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (u16x8)(0);
      return;
    }
    if constexpr (XA) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const u16x8*>(p + 8 * j);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = p[8 * j + e];
    }
  }
  __device__ __forceinline__ bf16x8 frag(int j) const { return __builtin_bit_cast(bf16x8, v[j]); }
};

// ---- 4-bit weights, one scale per 128 k (int4g128) ------------------------------------------
// Byte b of a row holds k = 2 b in its low nibble and k = 2 b + 1 in its high one, each as
// q + 8, so nibble t of a little-endian 32-bit word is the word's k = t.  Lane (i, c) reads the
// 16 bytes of its 32 k as one load; word j feeds MFMA j.  (u >> (4 t - 3)) & 0x00780078 puts
// nibbles t and t + 4 of a word into mantissa bits 3..6 of the two halves of a dword, and
// | 0x41804180 makes each half the bf16 16 + nibble = q + 24 exactly: a shift and a
// v_and_or_b32 per two weights.  The fragment's slots then hold the word's k in the order
// 0 4 1 5 2 6 3 7, and the x fragment is permuted to that order once per step for all G row
// groups.  The offset is taken out by the MFMAs themselves: a constant operand of -24 gives
// the tile -24 sum_k x[m, k] of the step (the same for every weight row, so once per step),
// and each row group's MFMAs accumulate on a copy of it.  Every product is an exact bf16 x
// bf16 one, the group's sum is the MFMA's f32 accumulation, and sum_k x (q + 24) - 24 sum_k x
// is the group's sum_k x q to f32 rounding of terms 24 / |q| larger than its own.
struct W4Frag {
  u32x4 v;
  __device__ __forceinline__ void load(const uint8_t* p) { v = *reinterpret_cast<const u32x4*>(p); }
  __device__ __forceinline__ bf16x8 frag(int j) const {
    const uint32_t u = v[j];
    u32x4 r = {((u << 3) & 0x00780078u) | 0x41804180u, ((u >> 1) & 0x00780078u) | 0x41804180u,
               ((u >> 5) & 0x00780078u) | 0x41804180u, ((u >> 9) & 0x00780078u) | 0x41804180u};
    return __builtin_bit_cast(bf16x8, r);
  }
};

// the four scales of the lane's rows n .. n + 3 of one group (sg: that group's row of the
// [K / 128, N] table); SV: N % 4 == 0 and a 16-byte aligned table, so the four are one load.
// No branches: rows past N re-read the last rows of the group (in bounds), as the weights do,
// and their results are never stored.
template <bool SV>
__device__ __forceinline__ f32x4 w4_scales(const float* sg, int64_t n, int64_t N) {
  if constexpr (SV) {
    return *reinterpret_cast<const f32x4*>(sg + min(n, N - 4));
  } else {
    f32x4 s;
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = sg[min(n + r, N - 1)];
    return s;
  }
}

// ---- MXFP4 weights: e2m1 nibbles, one e8m0 scale byte per 32 k ---------------------------------
// The bytes are laid out as int4g128's (byte b of a row = k 2 b low, k 2 b + 1 high), so lane (i, c)
// again reads the 16 bytes of its 32 k as one load -- and those 32 k are exactly one MX group, so
// the lane has ONE scale for the step, that of (row i, group 4 s + c), and the scale belongs to
// the weight operand.  v_cvt_scalef32_pk_bf16_fp4 turns byte `sel` of a dword (two e2m1 codes)
// into two bf16 values times 2^(exponent of its f32 scale operand), low nibble first: four of
// them per dword give the word's eight k in natural order, ready for MFMA j against the
// unpermuted x fragment.  e2m1 x 2^e is exact in bf16 (normal range), so What itself is the operand.
struct MX4Frag {
  u32x4 v;
  __device__ __forceinline__ void load(const uint8_t* p) { v = *reinterpret_cast<const u32x4*>(p); }
  // sc: 2^(e - 127) as f32 bits, mx4_scale()
  __device__ __forceinline__ bf16x8 frag(int j, float sc) const {
    typedef __attribute__((ext_vector_type(2))) __bf16 bfx2;
    const bfx2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v[j], sc, 0);
    const bfx2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v[j], sc, 1);
    const bfx2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v[j], sc, 2);
    const bfx2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v[j], sc, 3);
    const u32x4 r = {__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1),
                     __builtin_bit_cast(uint32_t, p2), __builtin_bit_cast(uint32_t, p3)};
    return __builtin_bit_cast(bf16x8, r);
  }
};

// the e8m0 byte as the f32 2^(byte - 127): the byte is the f32 exponent field
__device__ __forceinline__ float mx4_scale(uint32_t byte) { return __uint_as_float(byte << 23); }

// The scale bytes of one step of a row are 4 consecutive bytes at byte 4 s of its scale row
// (sr: the row's byte 4 s; a row has K / 32 bytes, a multiple of 4).  SA: the table is 4-byte
// aligned, so they are one dword that the row's four c lanes all load, and the lane picks byte
// c; otherwise the lane loads its own byte.
template <bool SA>
__device__ __forceinline__ uint32_t mx4_scale_load(const uint8_t* sr, int c) {
  if constexpr (SA)
    return *reinterpret_cast<const uint32_t*>(sr);
  else
    return (uint32_t)sr[c] << (8 * c);
}

}  // namespace mp
