// Skinny-M linear layer for decoding: y[M, N] = epi(x[M, K] @ What[N, K]^T), 1 <= M <= 16,
// with What a bf16 matrix or quantised weights: int8 (q * scale, one f32 scale per output
// row), int4g128 (4 bits, one f32 scale per 128 k of a row: ops.quantize_w4) or MXFP4 (e2m1
// values, one e8m0 scale byte per 32 k: ops.quant.quantize_mx4).
//
// One kernel frame, gemv_kernel<Fmt, G, XA>, holds what the formats share -- the plan, the
// lanes, the K-chains, the reduction and the epilogue -- and a format policy `Fmt` holds what
// differs: how a lane reads and converts the weights of a step.
//
// The frame.  Memory-bound: the weight matrix is streamed once, straight into VGPRs (no LDS
// round trip for it), for all M rows.  One wave step covers 16 weight rows x 128 k: lane
// (i, c), i = lane & 15, c = lane >> 4, reads the 32 consecutive k of row n0 + i that start
// at k0 + 32 c (32 B of int8, 64 B of bf16 or 16 B of a 4-bit format: the four lanes of a row
// read one contiguous piece), and the same k of x row i (zeros for i >= M: rows past M are
// never read).  Those 32 k feed four v_mfma_f32_16x16x32_bf16 (weights as the 16-row operand,
// the 16-padded x rows as the 16-column operand): MFMA j takes the lane's k 8 j .. 8 j + 7.
// Which k a lane holds is free as long as both operands agree.  A column of the MFMA result
// depends on that column of the x operand only, so row m of y does not depend on M or on the
// other rows.
//
// A workgroup owns 16 G weight rows and `ksplit` waves (plan: mp_gemv_plan.h); wave s runs
// its own K-steps for all G row groups (one x fragment per step serves them all), writes its
// f32 tile to LDS, and wave 0 adds the tiles of waves 1, 2, ... in that order, applies
// scale / bias / GELU / residual in f32 (gemv_store of mp_gemv_frags.h, shared with
// gemv_rows64.hip) and stores bf16.  No atomics, no second launch.
//
// A format policy provides
//   RAGGED      whether K % 128 != 0 is allowed, so that a ragged last step exists (PART);
//   ROW_SCALE   whether the epilogue multiplies by scale[n];
//   VARIANT, variant(a)   whether the format has a run-time variant V of its scale loads, and
//               which one a call takes.  The kernel picks once, before its K loop; a format
//               without one compiles V = false only;
//   unroll(G)   U, the steps whose loads are issued ahead of their MFMAs;
//   Rows<G>     the lane's pointers: Rows(a, nl, c) once, row(g, a, n, c) for each row group,
//               n its (clamped) weight row;
//   steps<G, XA, U, PART, V>(acc, rows, xrow, xon, s, kon)   U whole steps from step s on, every
//               load first, then the MFMAs; PART: the one ragged last step.
// Everything else the frame asks of a format is a compile-time constant: nothing in the K loop
// depends on the format at run time.
//
// The formats.  int8 becomes bf16 exactly (|q| <= 127 has 7 bits), and its MFMAs accumulate
// straight into acc.  An int4g128 step is exactly one group, so its MFMAs go into a tile of
// their own and acc += scale * tile in f32; the -24 offset tile is explained at W4Frag.  A
// lane's 32 k of MXFP4 are exactly one MX group, so its scale is folded into the conversion
// (v_cvt_scalef32_pk_bf16_fp4) and the MFMAs of a step accumulate straight into acc, as int8's do.
#include "mp_api.h"
#include "mp_common.h"
#include "mp_gemv_frags.h"
#include "mp_gemv_plan.h"

namespace mp {
namespace {

// int8 weights with one f32 scale per row, and bf16 weights (WFrag of mp_gemv_frags.h)
template <typename WT>
struct DenseFmt {
  static constexpr bool RAGGED = true, ROW_SCALE = sizeof(WT) == 1, VARIANT = false;
  // G = 1 runs up to 16 waves: 128 VGPRs each
  static constexpr int unroll(int G) { return sizeof(WT) == 1 ? (G == 4 ? 2 : 4) : 2; }
  static __device__ bool variant(const GemvArgs&) { return false; }

  template <int G>
  struct Rows {
    const WT* w[G];
    __device__ __forceinline__ Rows(const GemvArgs&, int64_t, int) {}
    __device__ __forceinline__ void row(int g, const GemvArgs& a, int64_t n, int c) {
      w[g] = reinterpret_cast<const WT*>(a.w) + n * a.K + 32 * c;
    }
  };

  // PART: lane group c holds k only while k0 + 32 c < K (kon)
  template <int G, bool XA, int U, bool PART, bool V>
  static __device__ __forceinline__ void steps(f32x4 (&acc)[G], const Rows<G>& rows, const bf16_t* xrow, bool xon,
                                               int s, bool kon) {
    WFrag<WT> wf[U][G];
    XFrag<XA> xf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t k0 = (int64_t)(s + u) * gemv::KSTEP;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (!PART || kon)
          wf[u][g].load(rows.w[g] + k0);
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
        for (int g = 0; g < G; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][g].frag(j), b, acc[g], 0, 0, 0);
      }
  }
};

// 4-bit weights, one scale per 128 k (int4g128): W4Frag and w4_scales of mp_gemv_frags.h
struct W4Fmt {
  static constexpr bool RAGGED = false, ROW_SCALE = false, VARIANT = true;
  // a step holds 16 VGPRs of x beside 8 G of weights and scales, and G = 1 has 128 VGPRs
  // (U = 4 spills there)
  static constexpr int unroll(int G) { return G == 2 ? 4 : 2; }
  // V: the four scales of a lane's rows are one 16-byte load
  static __device__ bool variant(const GemvArgs& a) { return a.N % 4 == 0 && ((uintptr_t)a.scale & 15) == 0; }

  template <int G>
  struct Rows {
    const uint8_t* w[G];
    const float* scale;
    int64_t nl, N;      // the lane's result rows of group g: nl + 16 g + r
    __device__ __forceinline__ Rows(const GemvArgs& a, int64_t nl_, int) : scale(a.scale), nl(nl_), N(a.N) {}
    __device__ __forceinline__ void row(int g, const GemvArgs& a, int64_t n, int c) {
      w[g] = reinterpret_cast<const uint8_t*>(a.w) + n * (a.K / 2) + 16 * c;
    }
  };

  // a step is a group: per step the offset tile and per row group its MFMAs and acc += scale * tile
  template <int G, bool XA, int U, bool PART, bool V>
  static __device__ __forceinline__ void steps(f32x4 (&acc)[G], const Rows<G>& rows, const bf16_t* xrow, bool xon,
                                               int s, bool) {
    static_assert(!PART, "K % 128 == 0: whole groups only");
    W4Frag wf[U][G];
    f32x4 sc[U][G];
    XFrag<XA> xf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t st = s + u;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        wf[u][g].load(rows.w[g] + st * (gemv::KSTEP / 2));
        sc[u][g] = w4_scales<V>(rows.scale + st * rows.N, rows.nl + 16 * g, rows.N);
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
};

// MXFP4 weights (e2m1, one e8m0 byte per 32 k): MX4Frag and mx4_scale_load of mp_gemv_frags.h
struct MX4Fmt {
  static constexpr bool RAGGED = false, ROW_SCALE = false, VARIANT = true;
  // a step holds 16 VGPRs of x beside 5 G of packed weights and scale bytes; the 16 G of a
  // step's converted operand live only around its MFMAs
  static constexpr int unroll(int G) { return G == 4 ? 2 : 4; }
  // V: a step's four scale bytes of a row are one dword load
  static __device__ bool variant(const GemvArgs& a) { return ((uintptr_t)a.scale & 3) == 0; }

  template <int G>
  struct Rows {
    const uint8_t* w[G];
    const uint8_t* s[G];
    int c;
    __device__ __forceinline__ Rows(const GemvArgs&, int64_t, int c_) : c(c_) {}
    // a row past N re-reads the scales of row N - 1 as it does the weights
    __device__ __forceinline__ void row(int g, const GemvArgs& a, int64_t n, int c) {
      w[g] = reinterpret_cast<const uint8_t*>(a.w) + n * (a.K / 2) + 16 * c;
      s[g] = reinterpret_cast<const uint8_t*>(a.scale) + n * (a.K / 32);
    }
  };

  // loads: weights, the step's scale dword, x; then per step and MFMA slot the conversion with
  // the lane's scale folded in and the MFMAs straight into acc
  template <int G, bool XA, int U, bool PART, bool V>
  static __device__ __forceinline__ void steps(f32x4 (&acc)[G], const Rows<G>& rows, const bf16_t* xrow, bool xon,
                                               int s, bool) {
    static_assert(!PART, "K % 128 == 0: four whole MX groups per row and step");
    MX4Frag wf[U][G];
    uint32_t sc[U][G];
    XFrag<XA> xf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t st = s + u;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        wf[u][g].load(rows.w[g] + st * (gemv::KSTEP / 2));
        sc[u][g] = mx4_scale_load<V>(rows.s[g] + st * 4, rows.c);
      }
      xf[u].load(xrow + st * gemv::KSTEP, xon);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float f[G];
#pragma unroll
      for (int g = 0; g < G; ++g) f[g] = mx4_scale((sc[u][g] >> (8 * rows.c)) & 0xffu);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 b = xf[u].frag(j);
#pragma unroll
        for (int g = 0; g < G; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][g].frag(j, f[g]), b, acc[g], 0, 0, 0);
      }
    }
  }
};

// A wave's chain: its K-steps [b, e), of which [b, ef) are whole; U at a time, then singly
template <typename Fmt, int G, bool XA, bool V>
__device__ __forceinline__ void run_chain(f32x4 (&acc)[G], const typename Fmt::template Rows<G>& rows,
                                          const bf16_t* xrow, bool xon, int b, int e, int ef, int c, int K) {
  constexpr int U = Fmt::unroll(G);
  int s = b;
  for (; s + U <= ef; s += U) Fmt::template steps<G, XA, U, false, V>(acc, rows, xrow, xon, s, true);
  for (; s < ef; ++s) Fmt::template steps<G, XA, 1, false, V>(acc, rows, xrow, xon, s, true);
  if constexpr (Fmt::RAGGED) {
    if (s < e) Fmt::template steps<G, XA, 1, true, V>(acc, rows, xrow, xon, s, s * gemv::KSTEP + 32 * c < K);
  }
}

template <typename Fmt, int G, bool XA>
__global__ __launch_bounds__(G == 1 ? 1024 : 512) void gemv_kernel(GemvArgs a) {
  extern __shared__ f32x4 red[];      // [ksplit - 1][G][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int i = lane & 15, c = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * (16 * G);
  const int64_t nl = n0 + 4 * c;      // the lane's result rows of group g: nl + 16 g + r
  const int full = a.K / gemv::KSTEP, steps = Fmt::RAGGED ? (a.K + gemv::KSTEP - 1) / gemv::KSTEP : full;
  const int per = (steps + S - 1) / S;
  const int b = wave * per, e = min(b + per, steps), ef = min(e, full);

  typename Fmt::template Rows<G> rows(a, nl, c);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    // rows past N re-read row N - 1 (in bounds); their results are never stored
    rows.row(g, a, min(n0 + 16 * g + i, (int64_t)a.N - 1), c);
  }
  const bool xon = i < a.M;
  const bf16_t* xrow = a.x + (xon ? (int64_t)i * a.ldx : 0) + 32 * c;

  f32x4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = (f32x4)(0.f);
  // the variant is picked here, once: a format without one has a single chain
  if (Fmt::VARIANT && Fmt::variant(a))
    run_chain<Fmt, G, XA, Fmt::VARIANT>(acc, rows, xrow, xon, b, e, ef, c, a.K);
  else
    run_chain<Fmt, G, XA, false>(acc, rows, xrow, xon, b, e, ef, c, a.K);

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
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = nl + 16 * g + r;
      if (n < a.N) gemv_store(a, acc[g][r], i, n, Fmt::ROW_SCALE);
    }
}

// G from the plan's rows, XA from x (16-byte aligned rows that vector loads can read)
template <typename Fmt>
int launch(const GemvArgs& a, const gemv::Plan& p, hipStream_t st) {
  const bool xa = ((uintptr_t)a.x & 15) == 0 && (a.M == 1 || a.ldx % 8 == 0);
  void (*kernel)(GemvArgs);
  if (p.rows == 64)
    kernel = xa ? gemv_kernel<Fmt, 4, true> : gemv_kernel<Fmt, 4, false>;
  else if (p.rows == 32)
    kernel = xa ? gemv_kernel<Fmt, 2, true> : gemv_kernel<Fmt, 2, false>;
  else
    kernel = xa ? gemv_kernel<Fmt, 1, true> : gemv_kernel<Fmt, 1, false>;
  const size_t lds = (size_t)(p.ksplit - 1) * (p.rows / 16) * 64 * sizeof(f32x4);
  kernel<<<dim3((unsigned)p.grid), dim3(64 * p.ksplit), lds, st>>>(a);
  return (int)hipGetLastError();
}

// out[n, k] = bf16(e2m1(nibble) * 2^(scale[n, k / 32] - 127)): one MX group (16 bytes of q, one
// scale byte) per thread, so thread t's scale is byte t of the table.  The conversion is exact.
__global__ __launch_bounds__(256) void dequant_mx4_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ scale,
                                                          bf16_t* __restrict__ out, int64_t chunks) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= chunks) return;
  MX4Frag f;
  f.load(q + 16 * t);
  const float sc = mx4_scale(scale[t]);
#pragma unroll
  for (int j = 0; j < 4; ++j) *reinterpret_cast<bf16x8*>(out + 32 * t + 8 * j) = f.frag(j, sc);
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
  mp::GemvArgs a;
  if (!mp::gemv_args(a, w, scale, x, y, bias, res, M, N, K, ldx, ldy, ldr, gelu)) return -1;
  if ((wbytes != 2) != (scale != nullptr) || ((uintptr_t)scale & 3)) return -1;
  if (wbytes == 0) return mp::launch<mp::W4Fmt>(a, p, st);
  return wbytes == 1 ? mp::launch<mp::DenseFmt<int8_t>>(a, p, st) : mp::launch<mp::DenseFmt<mp::bf16_t>>(a, p, st);
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

// MXFP4: w = packed e2m1 [N, K / 2], scale = e8m0 bytes [N, K / 32] (any alignment).  The plan is
// the 4-bit one: the streamed bytes per row are int4g128's.  Returns as mp_gemv_skinny does.
extern "C" int mp_gemv_mx4(const void* w, const uint8_t* scale, const void* x, void* y, const void* bias,
                           const void* res, int M, int N, int K, int64_t ldx, int64_t ldy, int64_t ldr, int gelu,
                           int force_split, hipStream_t st) {
  const gemv::Plan p = gemv::plan(N, K, 0, force_split);
  if (p.rows == 0 || M < 1 || M > gemv::MAX_M || scale == nullptr) return -1;
  mp::GemvArgs a;
  if (!mp::gemv_args(a, w, scale, x, y, bias, res, M, N, K, ldx, ldy, ldr, gelu)) return -1;
  return mp::launch<mp::MX4Fmt>(a, p, st);
}

// q [N, K / 2] packed e2m1, scale [N, K / 32] e8m0 bytes, out bf16 [N, K]
extern "C" int mp_dequant_mx4(const void* q, const uint8_t* scale, void* out, int64_t N, int64_t K, hipStream_t st) {
  if (N < 1 || K < 128 || K % 128 != 0 || ((uintptr_t)q & 15) || ((uintptr_t)out & 15)) return -1;
  const int64_t chunks = N * (K / 32);
  if ((chunks + 255) / 256 > 0x7fffffff) return -1;
  mp::dequant_mx4_kernel<<<dim3((unsigned)((chunks + 255) / 256)), 256, 0, st>>>((const uint8_t*)q, scale,
                                                                                 (mp::bf16_t*)out, chunks);
  return (int)hipGetLastError();
}
