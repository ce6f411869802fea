// Skinny-M linear layer for decoding: y[M, N] = epi(x[M, K] @ What[N, K]^T), 1 <= M <= 16,
// with What = q * scale (int8 weights, one f32 scale per output row) or a bf16 matrix.
//
// Memory-bound: the weight matrix is streamed once, straight into VGPRs (no LDS round trip
// for it), for all M rows.  One wave step covers 16 weight rows x 128 k: lane (i, c), i =
// lane & 15, c = lane >> 4, reads the 32 consecutive k of row n0 + i that start at k0 + 32 c
// (32 B of int8 or 64 B of bf16: the four lanes of a row read one contiguous 128 / 256 B),
// and the same k of x row i (zeros for i >= M: rows past M are never read).  Those 32 k feed
// four v_mfma_f32_16x16x32_bf16 (weights as the 16-row operand, the 16-padded x rows as the
// 16-column operand): MFMA j takes the lane's k 8 j .. 8 j + 7.  Which k a lane holds is
// free as long as both operands agree.  int8 becomes bf16 exactly (|q| <= 127 has 7 bits).
// A column of the MFMA result depends on that column of the x operand only, so row m of y
// does not depend on M or on the other rows.
//
// A workgroup owns 16 G weight rows and `ksplit` waves (plan: mp_gemv_plan.h); wave s runs
// its own K-steps for all G row groups (one x fragment per step serves them all), writes its
// f32 tile to LDS, and wave 0 adds the tiles of waves 1, 2, ... in that order, applies
// scale / bias / GELU / residual in f32 and stores bf16.  No atomics, no second launch.
//
// 4-bit weights with one f32 scale per 128 k of a row (int4g128: ops.quantize_w4) run the
// sibling kernel gemv_w4_kernel below: the same plan, lanes and reduction, but a step is
// exactly one group, so its MFMAs go into a tile of their own and acc += scale * tile in f32.
#include "mp_api.h"
#include "mp_common.h"
#include "mp_gemv_plan.h"

namespace mp {
namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

struct GemvArgs {
  const void* w;          // [N, K] int8 or bf16 or [N, K / 2] packed 4-bit, row-major, rows 16-byte aligned
  const float* scale;     // [N] (int8), [K / 128, N] (4-bit) or null
  const bf16_t* x;        // [M, ldx]
  bf16_t* y;              // [M, ldy]
  const bf16_t* bias;     // [N] or null
  const bf16_t* res;      // [M, ldr] or null
  int M, N, K, gelu;
  int64_t ldx, ldy, ldr;
};

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

// U whole steps from step s on: every load first, then the MFMAs.  PART: the one ragged
// last step (K % 128 != 0), where lane group c holds k only while k0 + 32 c < K.
template <typename WT, int G, bool XA, int U, bool PART>
__device__ __forceinline__ void run_steps(f32x4 (&acc)[G], const WT* const (&wrow)[G], const bf16_t* xrow, bool xon,
                                          int s, bool kon) {
  WFrag<WT> wf[U][G];
  XFrag<XA> xf[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t k0 = (int64_t)(s + u) * gemv::KSTEP;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (!PART || kon)
        wf[u][g].load(wrow[g] + k0);
      else
        wf[u][g].zero();
    }
    xf[u].load(xrow + k0, xon && (!PART || kon));
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 b = xf[u].frag(j);
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][g].frag(j), b, acc[g], 0, 0, 0);
    }
}

template <typename WT, int G, bool XA>
__global__ __launch_bounds__(G == 1 ? 1024 : 512) void gemv_skinny_kernel(GemvArgs a) {
  extern __shared__ f32x4 red[];      // [ksplit - 1][G][64]
  // steps loaded ahead of their MFMAs (G = 1 runs up to 16 waves: 128 VGPRs each)
  constexpr int U = sizeof(WT) == 1 ? (G == 4 ? 2 : 4) : 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int i = lane & 15, c = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * (16 * G);
  const int steps = (a.K + gemv::KSTEP - 1) / gemv::KSTEP, full = a.K / gemv::KSTEP;
  const int per = (steps + S - 1) / S;
  const int b = wave * per, e = min(b + per, steps), ef = min(e, full);

  const WT* wrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    // rows past N re-read row N - 1 (in bounds); their results are never stored
    const int64_t n = min(n0 + 16 * g + i, (int64_t)a.N - 1);
    wrow[g] = reinterpret_cast<const WT*>(a.w) + n * a.K + 32 * c;
  }
  const bool xon = i < a.M;
  const bf16_t* xrow = a.x + (xon ? (int64_t)i * a.ldx : 0) + 32 * c;

  f32x4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x4)(0.f);
  int s = b;
  for (; s + U <= ef; s += U) run_steps<WT, G, XA, U, false>(acc, wrow, xrow, xon, s, true);
  for (; s < ef; ++s) run_steps<WT, G, XA, 1, false>(acc, wrow, xrow, xon, s, true);
  if (s < e) run_steps<WT, G, XA, 1, true>(acc, wrow, xrow, xon, s, s * gemv::KSTEP + 32 * c < a.K);

  if (S > 1) {
    if (wave > 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) red[((wave - 1) * G + g) * 64 + lane] = acc[g];
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 1; w < S; ++w)
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] += red[((w - 1) * G + g) * 64 + lane];
  }

  // lane: x row m = i, weight rows n0 + 16 g + 4 c + r
  if (!xon) return;
  const int m = i;
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = n0 + 16 * g + 4 * c + r;
      if (n >= a.N) continue;
      float v = acc[g][r];
      if constexpr (sizeof(WT) == 1) v *= a.scale[n];
      if (a.bias) v += bf2f(a.bias[n]);
      if (a.gelu) v = gelu_tanh(IO8<bf16_t>::get_round(v));
      if (a.res) v += bf2f(a.res[(int64_t)m * a.ldr + n]);
      a.y[(int64_t)m * a.ldy + n] = f2bf(v);
    }
}

template <typename WT, int G>
int launch_g(const GemvArgs& a, const gemv::Plan& p, bool xa, hipStream_t st) {
  const size_t lds = (size_t)(p.ksplit - 1) * G * 64 * sizeof(f32x4);
  const dim3 grid((unsigned)p.grid), block(64 * p.ksplit);
  if (xa)
    gemv_skinny_kernel<WT, G, true><<<grid, block, lds, st>>>(a);
  else
    gemv_skinny_kernel<WT, G, false><<<grid, block, lds, st>>>(a);
  return (int)hipGetLastError();
}

template <typename WT>
int launch(const GemvArgs& a, const gemv::Plan& p, bool xa, hipStream_t st) {
  if (p.rows == 64) return launch_g<WT, 4>(a, p, xa, st);
  if (p.rows == 32) return launch_g<WT, 2>(a, p, xa, st);
  return launch_g<WT, 1>(a, p, xa, st);
}

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

// U steps (= groups) from step s on: every load first, then per step the offset tile and per
// row group its MFMAs and acc += scale * tile
template <int G, bool XA, int U, bool SV>
__device__ __forceinline__ void run_steps_w4(f32x4 (&acc)[G], const uint8_t* const (&wrow)[G], const float* scale,
                                             int64_t nl, int64_t N, const bf16_t* xrow, bool xon, int s) {
  W4Frag wf[U][G];
  f32x4 sc[U][G];
  XFrag<XA> xf[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t st = s + u;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      wf[u][g].load(wrow[g] + st * (gemv::KSTEP / 2));
      sc[u][g] = w4_scales<SV>(scale + st * N, nl + 16 * g, N);
    }
    xf[u].load(xrow + st * gemv::KSTEP, xon);
  }
  const u32x4 m24 = (u32x4)(0xc1c0c1c0u);      // bf16 -24 in every slot
#pragma unroll
  for (int u = 0; u < U; ++u) {
    bf16x8 b[4];
    f32x4 off = (f32x4)(0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u16x8 p = __builtin_shufflevector(xf[u].v[j], xf[u].v[j], 0, 4, 1, 5, 2, 6, 3, 7);
      b[j] = __builtin_bit_cast(bf16x8, p);
      off = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, m24), b[j], off, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      f32x4 t = off;
#pragma unroll
      for (int j = 0; j < 4; ++j) t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][g].frag(j), b[j], t, 0, 0, 0);
      acc[g] += sc[u][g] * t;
    }
  }
}

template <int G, bool XA>
__global__ __launch_bounds__(G == 1 ? 1024 : 512) void gemv_w4_kernel(GemvArgs a) {
  extern __shared__ f32x4 red[];      // [ksplit - 1][G][64]
  // steps loaded ahead of their MFMAs: a step holds 16 VGPRs of x beside 8 G of weights and
  // scales, and G = 1 has 128 VGPRs (U = 4 spills there)
  constexpr int U = G == 2 ? 4 : 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int i = lane & 15, c = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * (16 * G);
  const int steps = a.K / gemv::KSTEP;          // K % 128 == 0: whole groups only
  const int per = (steps + S - 1) / S;
  const int b = wave * per, e = min(b + per, steps);

  const uint8_t* wrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    // rows past N re-read row N - 1 (in bounds); their results are never stored
    const int64_t n = min(n0 + 16 * g + i, (int64_t)a.N - 1);
    wrow[g] = reinterpret_cast<const uint8_t*>(a.w) + n * (a.K / 2) + 16 * c;
  }
  const bool xon = i < a.M;
  const bf16_t* xrow = a.x + (xon ? (int64_t)i * a.ldx : 0) + 32 * c;
  const bool sv = a.N % 4 == 0 && ((uintptr_t)a.scale & 15) == 0;
  const int64_t nl = n0 + 4 * c;     // the lane's result rows of group g: nl + 16 g + r

  f32x4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x4)(0.f);
  int s = b;
  if (sv) {
    for (; s + U <= e; s += U) run_steps_w4<G, XA, U, true>(acc, wrow, a.scale, nl, a.N, xrow, xon, s);
    for (; s < e; ++s) run_steps_w4<G, XA, 1, true>(acc, wrow, a.scale, nl, a.N, xrow, xon, s);
  } else {
    for (; s + U <= e; s += U) run_steps_w4<G, XA, U, false>(acc, wrow, a.scale, nl, a.N, xrow, xon, s);
    for (; s < e; ++s) run_steps_w4<G, XA, 1, false>(acc, wrow, a.scale, nl, a.N, xrow, xon, s);
  }

  if (S > 1) {
    if (wave > 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) red[((wave - 1) * G + g) * 64 + lane] = acc[g];
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 1; w < S; ++w)
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] += red[((w - 1) * G + g) * 64 + lane];
  }

  if (!xon) return;
  const int m = i;
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = nl + 16 * g + r;
      if (n >= a.N) continue;
      float v = acc[g][r];
      if (a.bias) v += bf2f(a.bias[n]);
      if (a.gelu) v = gelu_tanh(IO8<bf16_t>::get_round(v));
      if (a.res) v += bf2f(a.res[(int64_t)m * a.ldr + n]);
      a.y[(int64_t)m * a.ldy + n] = f2bf(v);
    }
}

template <int G>
int launch_w4_g(const GemvArgs& a, const gemv::Plan& p, bool xa, hipStream_t st) {
  const size_t lds = (size_t)(p.ksplit - 1) * G * 64 * sizeof(f32x4);
  const dim3 grid((unsigned)p.grid), block(64 * p.ksplit);
  if (xa)
    gemv_w4_kernel<G, true><<<grid, block, lds, st>>>(a);
  else
    gemv_w4_kernel<G, false><<<grid, block, lds, st>>>(a);
  return (int)hipGetLastError();
}

int launch_w4(const GemvArgs& a, const gemv::Plan& p, bool xa, hipStream_t st) {
  if (p.rows == 64) return launch_w4_g<4>(a, p, xa, st);
  if (p.rows == 32) return launch_w4_g<2>(a, p, xa, st);
  return launch_w4_g<1>(a, p, xa, st);
}

// out[n, k] = bf16(q[n, k] * scale[n]); 16 elements per thread
__global__ __launch_bounds__(256) void dequant_w8_kernel(const int8_t* __restrict__ q, const float* __restrict__ scale,
                                                         bf16_t* __restrict__ out, int64_t chunks, int chunks_per_row) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= chunks) return;
  const float sc = scale[t / chunks_per_row];
  const u32x4 v = *reinterpret_cast<const u32x4*>(q + 16 * t);
  u16x8 o[2];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int qi = (int)(int8_t)((v[d] >> (8 * k)) & 0xffu);
      o[d >> 1][4 * (d & 1) + k] = f2bf((float)qi * sc);
    }
  *reinterpret_cast<u16x8*>(out + 16 * t) = o[0];
  *reinterpret_cast<u16x8*>(out + 16 * t + 8) = o[1];
}

// out[n, k] = bf16((nibble - 8) * scale[k / 128, n]); 32 elements (16 bytes of q) per thread
__global__ __launch_bounds__(256) void dequant_w4_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scale,
                                                         bf16_t* __restrict__ out, int64_t chunks, int chunks_per_row,
                                                         int64_t N) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= chunks) return;
  const int64_t n = t / chunks_per_row;
  const int ch = (int)(t - n * chunks_per_row);      // k = 32 ch .. 32 ch + 31: group ch / 4
  const float sc = scale[(int64_t)(ch >> 2) * N + n];
  const u32x4 v = *reinterpret_cast<const u32x4*>(q + 16 * t);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    u16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = f2bf((float)((int)((v[d] >> (4 * k)) & 0xfu) - 8) * sc);
    *reinterpret_cast<u16x8*>(out + 32 * t + 8 * d) = o;
  }
}

}  // namespace
}  // namespace mp

// wbytes 1: w = int8 q with scale [N]; 2: w = bf16; 0: w = packed 4-bit [N, K / 2] with scale
// [K / 128, N].  Returns 0, -1 for a shape or alignment the kernel does not take, or the HIP
// error of the launch.
extern "C" int mp_gemv_skinny(const void* w, const float* scale, int wbytes, const void* x, void* y, const void* bias,
                              const void* res, int M, int N, int K, int64_t ldx, int64_t ldy, int64_t ldr, int gelu,
                              int force_split, hipStream_t st) {
  const gemv::Plan p = gemv::plan(N, K, wbytes, force_split);
  if (p.rows == 0 || M < 1 || M > gemv::MAX_M) return -1;
  if ((wbytes != 2) != (scale != nullptr) || ((uintptr_t)w & 15) || ((uintptr_t)scale & 3)) return -1;
  mp::GemvArgs a;
  a.w = w, a.scale = scale, a.x = (const mp::bf16_t*)x, a.y = (mp::bf16_t*)y;
  a.bias = (const mp::bf16_t*)bias, a.res = (const mp::bf16_t*)res;
  a.M = M, a.N = N, a.K = K, a.gelu = gelu, a.ldx = ldx, a.ldy = ldy, a.ldr = ldr;
  const bool xa = ((uintptr_t)x & 15) == 0 && (M == 1 || ldx % 8 == 0);
  if (wbytes == 0) return mp::launch_w4(a, p, xa, st);
  return wbytes == 1 ? mp::launch<int8_t>(a, p, xa, st) : mp::launch<mp::bf16_t>(a, p, xa, st);
}

extern "C" int mp_dequant_w8(const void* q, const float* scale, void* out, int64_t N, int64_t K, hipStream_t st) {
  if (N < 1 || K < 16 || K % 16 != 0 || ((uintptr_t)q & 15) || ((uintptr_t)out & 15)) return -1;
  const int64_t chunks = N * K / 16;
  if ((chunks + 255) / 256 > 0x7fffffff) return -1;
  mp::dequant_w8_kernel<<<dim3((unsigned)((chunks + 255) / 256)), 256, 0, st>>>(
      (const int8_t*)q, scale, (mp::bf16_t*)out, chunks, (int)(K / 16));
  return (int)hipGetLastError();
}

// q [N, K / 2] packed 4-bit, scale [K / 128, N], out bf16 [N, K]
extern "C" int mp_dequant_w4(const void* q, const float* scale, void* out, int64_t N, int64_t K, hipStream_t st) {
  if (N < 1 || K < 128 || K % 128 != 0 || ((uintptr_t)q & 15) || ((uintptr_t)out & 15)) return -1;
  const int64_t chunks = N * (K / 32);
  if ((chunks + 255) / 256 > 0x7fffffff || K / 32 > 0x7fffffff) return -1;
  mp::dequant_w4_kernel<<<dim3((unsigned)((chunks + 255) / 256)), 256, 0, st>>>(
      (const uint8_t*)q, scale, (mp::bf16_t*)out, chunks, (int)(K / 32), N);
  return (int)hipGetLastError();
}
