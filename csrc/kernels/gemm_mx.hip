// MXFP8 x MXFP4 GEMM on the scaled MFMA, and the quantiser of its activation rows.
//
//   y[M, N] = epi(Xhat[M, K] @ What[N, K]^T),  any M >= 1, K % 128 == 0
//
// Xhat: MXFP8 rows (ops.quant.quantize_mx8_rows): K e4m3 codes in k order, then the K / 32 e8m0
// bytes of the row's groups of 32, then zeros up to a multiple of 16 bytes.  What: the MXFP4
// matrices as ops.quant.quantize_mx4 stores them, q4 [N, K / 2] (element 2 b in the low nibble of
// byte b) and scale [N, K / 32].  Neither operand is ever converted: the multiply is
// v_mfma_scale_f32_16x16x128_f8f6f4 with A = the e4m3 codes of 16 x rows and B = the e2m1 codes
// of 16 weight rows.  The instruction reads a lane's operand as two 128-bit halves, and half h of
// lane (i, c), i = lane & 15, c = lane >> 4, is the (4 h + c)-th run of 128 bits of row i's 128 k
// (measured on the MI355X with one-hot rows; tests/test_gemm_mx_gpu.py holds it).  For e2m1 that
// is the 32 consecutive k [32 c, 32 c + 32) in the low half, one MX group in 16 bytes; for e4m3
// it is k [16 c, 16 c + 16) in the low and [64 + 16 c, 64 + 16 c + 16) in the high half.  The
// e8m0 byte of group c of row i goes in with lane (i, c) for either operand, copied into all four
// bytes of the scale register (one v_perm_b32), so the result does not depend on which byte the
// instruction's op_sel picks.  The lane ends up with y[4 c + r][i], r = 0 .. 3, in f32.
//
// Tiling (mp_gemm_mx_plan.h).  A workgroup of 4 waves owns a BM x BN tile of y and walks K in
// steps of 128:
//   NARROW  64 x 32   waves 4 x 1, each 1 x 2 MFMA tiles: 17 .. 64 rows, the matrix streamed once
//   SQUARE  128 x 128 waves 2 x 2, each 4 x 4 MFMA tiles: a prefill
// An output element has one accumulator and its K-steps run in ascending order in both shapes,
// there is no split of K and there are no atomics: row m of y has the same bits whatever M is,
// whatever the other rows hold and whichever tile the plan picks.
//
// Staging.  Per step the workgroup loads the x tile (BM x 128 bytes), the w tile (BN x 64 bytes)
// and one dword of scale bytes per row of either with coalesced 16-byte global loads into
// registers, runs the MFMAs of the step before on the other LDS buffer while those loads are in
// flight, then writes the registers to LDS: one barrier per step.  LDS rows are padded by 16
// bytes (x: 144, w: 80) so the 16 rows a b128 read touches spread over the banks.  The x scale
// dword of a step is always 4-byte aligned (rows are 16-byte aligned and K % 128 == 0); the
// weight scale table may sit at any address, and is read as dwords when it is 4-byte aligned and
// as bytes otherwise (SA), as the skinny kernel's MX4Fmt does.
//
// Bounds.  Tile rows past M and columns past N load row M - 1 / N - 1 again (an address inside
// the operand) and are never stored.  No array content becomes an address.  No allocation, no
// synchronisation: a call can be captured in a graph.
//
// mx8_quantize_rows_kernel: one lane owns one group (32 consecutive k of a row): its amax, its
// e8m0 byte and its 32 codes need no other lane.  E = floor(log2 amax) - 8 from the exponent
// field, + 1 when amax * 2^-E > 448, so no scaled element exceeds e4m3's largest value and no
// saturation rule exists.  The scale is applied in f32 (an exact multiplication by a power of two
// built from its bits) and v_cvt_scalef32_pk_fp8_f32 then converts with a scale of 1.0: the bits
// do not rest on how the instruction applies its scale operand.  A code of -0 is stored as 0,
// as the tensor code does.  The lane of a row's last group also writes the row's zero padding.
// The price of one lane per group: a lane reads 64 contiguous bytes of bf16 (128 of f32) as 16-byte
// loads, so the lanes of one load instruction are 64 (128) bytes apart and it touches 64 segments;
// the two 16-byte payload stores are 32 bytes apart the same way and the scale is a byte store.
// Every byte of a line is still used by the neighbouring loads of the same wave, but the kernel
// issues four (eight) times the memory instructions a lane-interleaved layout would.
#include "mp_api.h"
#include "mp_common.h"
#include "mp_gemm_mx_plan.h"

namespace mp {
namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) short i16x2;

struct GemmMxArgs {
  const uint8_t* x;    // MXFP8 rows, ldx bytes apart
  const uint8_t* w;    // q4 [N, K / 2]
  const uint8_t* ws;   // e8m0 [N, K / 32]
  bf16_t* y;
  const bf16_t* bias;
  const bf16_t* res;
  int M, N, K, gelu;
  int64_t ldx, ldy, ldr;
};

constexpr int XP = 144;   // LDS bytes of a staged x row: 128 + 16
constexpr int WP = 80;    // ... of a staged w row: 64 + 16

// the four bytes of `dw` at byte c, in every byte of the result
__device__ __forceinline__ int scale_byte(uint32_t dw, int c) {
  return (int)__builtin_amdgcn_perm(0u, dw, (uint32_t)c * 0x01010101u);
}

template <int WM, int WN, int TM, int TN, bool SA>
__global__ __launch_bounds__(gemm_mx::THREADS) void gemm_mx_kernel(GemmMxArgs a) {
  constexpr int BM = 16 * WM * TM, BN = 16 * WN * TN;
  constexpr int XCH = BM * 8, WCH = BN * 4;                       // 16-byte chunks of a step
  constexpr int XL = (XCH + 255) / 256, WL = (WCH + 255) / 256;   // ... per thread
  constexpr int OFF_W = BM * XP, OFF_XS = OFF_W + BN * WP, OFF_WS = OFF_XS + 4 * BM, STAGE = OFF_WS + 4 * BN;
  static_assert(WM * WN == 4 && BM + BN <= 256 && STAGE % 16 == 0 && 2 * STAGE <= 65536, "tile");
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, c = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  const int64_t m0 = (int64_t)blockIdx.y * BM, n0 = (int64_t)blockIdx.x * BN;
  const int steps = a.K / gemm_mx::KSTEP;

  // what this thread stages per step: global source (step 0) and LDS offset of each chunk
  const uint8_t* xsrc[XL];
  const uint8_t* wsrc[WL];
  int xdst[XL], wdst[WL];
#pragma unroll
  for (int l = 0; l < XL; ++l) {
    const int idx = tid + 256 * l, row = idx >> 3, ch = idx & 7;
    const int64_t m = min(m0 + row, (int64_t)a.M - 1);
    xsrc[l] = a.x + m * a.ldx + 16 * ch;
    xdst[l] = row * XP + 16 * ch;
  }
#pragma unroll
  for (int l = 0; l < WL; ++l) {
    const int idx = tid + 256 * l, row = idx >> 2, ch = idx & 3;
    const int64_t n = min(n0 + row, (int64_t)a.N - 1);
    wsrc[l] = a.w + n * (a.K / 2) + 16 * ch;
    wdst[l] = OFF_W + row * WP + 16 * ch;
  }
  // threads [0, BM): the x scale dword of tile row tid; [BM, BM + BN): the w scale dword
  const bool s_x = tid < BM, s_w = !s_x && tid < BM + BN;
  const uint8_t* ssrc = a.x;
  int sdst = 0;
  if (s_x) {
    ssrc = a.x + min(m0 + tid, (int64_t)a.M - 1) * a.ldx + a.K;
    sdst = OFF_XS + 4 * tid;
  } else if (s_w) {
    ssrc = a.ws + min(n0 + (tid - BM), (int64_t)a.N - 1) * (a.K / gemm_mx::GROUP);
    sdst = OFF_WS + 4 * (tid - BM);
  }

  i32x4 xr[XL], wr[WL];
  uint32_t sr = 0;
  auto load_step = [&](int s) {
#pragma unroll
    for (int l = 0; l < XL; ++l)
      if (XCH % 256 == 0 || tid + 256 * l < XCH) xr[l] = *reinterpret_cast<const i32x4*>(xsrc[l] + (int64_t)s * 128);
#pragma unroll
    for (int l = 0; l < WL; ++l)
      if (WCH % 256 == 0 || tid + 256 * l < WCH) wr[l] = *reinterpret_cast<const i32x4*>(wsrc[l] + (int64_t)s * 64);
    if (s_x || (SA && s_w)) {
      sr = *reinterpret_cast<const uint32_t*>(ssrc + 4 * (int64_t)s);
    } else if (s_w) {
      const uint8_t* p = ssrc + 4 * (int64_t)s;
      sr = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
  };
  auto store_step = [&](int buf) {
    uint8_t* base = lds + buf * STAGE;
#pragma unroll
    for (int l = 0; l < XL; ++l)
      if (XCH % 256 == 0 || tid + 256 * l < XCH) *reinterpret_cast<i32x4*>(base + xdst[l]) = xr[l];
#pragma unroll
    for (int l = 0; l < WL; ++l)
      if (WCH % 256 == 0 || tid + 256 * l < WCH) *reinterpret_cast<i32x4*>(base + wdst[l]) = wr[l];
    if (s_x || s_w) *reinterpret_cast<uint32_t*>(base + sdst) = sr;
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = (f32x4)(0.f);

  load_step(0);
  store_step(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const bool more = s + 1 < steps;
    if (more) load_step(s + 1);
    const uint8_t* base = lds + (s & 1) * STAGE;
    i32x8 af[TM], bfr[TN];
    int sa[TM], sb[TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int row = (wm * TM + tm) * 16 + i;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(base + row * XP + 16 * c);
      const i32x4 hi = *reinterpret_cast<const i32x4*>(base + row * XP + 64 + 16 * c);
      af[tm] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      sa[tm] = scale_byte(*reinterpret_cast<const uint32_t*>(base + OFF_XS + 4 * row), c);
    }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int row = (wn * TN + tn) * 16 + i;
      const i32x4 v = *reinterpret_cast<const i32x4*>(base + OFF_W + row * WP + 16 * c);
      // an fp4 operand is the low four registers; the high four are not read
      bfr[tn] = __builtin_shufflevector(v, (i32x4)(0), 0, 1, 2, 3, 4, 5, 6, 7);
      sb[tn] = scale_byte(*reinterpret_cast<const uint32_t*>(base + OFF_WS + 4 * row), c);
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
        acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[tm], bfr[tn], acc[tm][tn], 0, 4, 0, sa[tm],
                                                                       0, sb[tn]);
    if (more) store_step((s + 1) & 1);
    __syncthreads();
  }

  // lane: rows m0 + 16 (wm TM + tm) + 4 c + r, column n0 + 16 (wn TN + tn) + i
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int64_t n = n0 + (wn * TN + tn) * 16 + i;
    if (n >= a.N) continue;
    const float b = a.bias ? bf2f(a.bias[n]) : 0.f;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + (wm * TM + tm) * 16 + 4 * c + r;
        if (m >= a.M) continue;
        float v = acc[tm][tn][r];
        if (a.bias) v += b;
        if (a.gelu) v = gelu_tanh(IO8<bf16_t>::get_round(v));
        if (a.res) v += bf2f(a.res[m * a.ldr + n]);
        a.y[m * a.ldy + n] = f2bf(v);
      }
  }
}

template <int WM, int WN, int TM, int TN>
int launch_gemm_mx(const GemmMxArgs& a, const gemm_mx::Plan& p, hipStream_t st) {
  const dim3 grid((unsigned)p.grid_n, (unsigned)p.grid_m);
  if (((uintptr_t)a.ws & 3) == 0)
    gemm_mx_kernel<WM, WN, TM, TN, true><<<grid, gemm_mx::THREADS, 0, st>>>(a);
  else
    gemm_mx_kernel<WM, WN, TM, TN, false><<<grid, gemm_mx::THREADS, 0, st>>>(a);
  return (int)hipGetLastError();
}

// ---- the quantiser of MXFP8 rows

// 2^-E as an f32, E in [-127, 127 - 1]: the exponent field 127 - E
__device__ __forceinline__ float pow2_neg(int E) { return __uint_as_float((uint32_t)(127 - E) << 23); }

template <typename T, bool XA>
__global__ __launch_bounds__(256) void mx8_quantize_rows_kernel(const T* __restrict__ x, int64_t ldx,
                                                                uint8_t* __restrict__ out, int64_t ldo, int64_t groups,
                                                                int K) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= groups) return;
  const int G = K / gemm_mx::GROUP;
  const int64_t m = t / G;
  const int g = (int)(t - m * G);
  const T* src = x + m * ldx + 32 * g;
  float v[32];
  if constexpr (XA) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const typename IO8<T>::Raw raw = IO8<T>::load(src + 8 * j);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[8 * j + e] = IO8<T>::get(raw, e);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 32; ++e) v[e] = IO8<T>::load1(src + e);
  }
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 32; ++e) amax = fmaxf(amax, fabsf(v[e]));
  // floor(log2 amax) is the exponent field - 127 (a subnormal amax lands below the clamp either way)
  int E = max((int)(__float_as_uint(amax) >> 23) - 127 - 8, -127);
  if (amax * pow2_neg(E) > 448.f) E += 1;
  const float inv = amax > 0.f ? pow2_neg(E) : 0.f;      // a group of zeros: codes 0, whatever the signs
  const uint8_t sbyte = amax > 0.f ? (uint8_t)(E + 127) : (uint8_t)0;

  uint32_t dw[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    i16x2 p = (i16x2)(0);
    p = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(p, v[4 * d] * inv, v[4 * d + 1] * inv, 1.0f, false);
    p = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(p, v[4 * d + 2] * inv, v[4 * d + 3] * inv, 1.0f, true);
    uint32_t u = __builtin_bit_cast(uint32_t, p);
    // bytes equal to 0x80 (-0) become 0: z has 0x80 exactly where a byte of u ^ 0x80808080 is 0
    const uint32_t q = u ^ 0x80808080u;
    const uint32_t z = ~(((q & 0x7f7f7f7fu) + 0x7f7f7f7fu) | q) & 0x80808080u;
    dw[d] = u ^ z;
  }
  uint8_t* row = out + m * ldo;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
  u32x4_t lo = {dw[0], dw[1], dw[2], dw[3]}, hi = {dw[4], dw[5], dw[6], dw[7]};
  *reinterpret_cast<u32x4_t*>(row + 32 * g) = lo;
  *reinterpret_cast<u32x4_t*>(row + 32 * g + 16) = hi;
  row[K + g] = sbyte;
  if (g == G - 1) {
    for (int p = K + G; p < (int)ldo; p += 4) *reinterpret_cast<uint32_t*>(row + p) = 0u;      // K + G is a multiple of 4
  }
}

template <typename T>
int launch_quantize(const void* x, int64_t ldx, void* out, int64_t M, int K, hipStream_t st) {
  const int64_t groups = M * (K / gemm_mx::GROUP);
  const unsigned grid = (unsigned)((groups + 255) / 256);
  const int64_t rb = gemm_mx::mx8_row_bytes(K);
  const bool xa = ((uintptr_t)x & 15) == 0 && (M == 1 || (ldx * sizeof(T)) % 16 == 0);
  if (xa)
    mx8_quantize_rows_kernel<T, true><<<grid, 256, 0, st>>>((const T*)x, ldx, (uint8_t*)out, rb, groups, K);
  else
    mx8_quantize_rows_kernel<T, false><<<grid, 256, 0, st>>>((const T*)x, ldx, (uint8_t*)out, rb, groups, K);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace mp

// x: M rows of K bf16 (f32 != 0: f32) elements, ldx elements apart; out: M contiguous MXFP8 rows of
// mx8_row_bytes(K) bytes, 16-byte aligned.  Returns 0, -1 for a shape or alignment the kernel does
// not take, or the HIP error of the launch.
extern "C" int mp_mx8_quantize_rows(const void* x, int f32, int64_t ldx, void* out, int64_t M, int K, hipStream_t st) {
  if (M < 1 || K < gemm_mx::KSTEP || K % gemm_mx::KSTEP != 0 || K > 1 << 24 || ((uintptr_t)out & 15)) return -1;
  if ((M * (K / gemm_mx::GROUP) + 255) / 256 > 0x7fffffff || (M > 1 && ldx < K)) return -1;
  return f32 ? mp::launch_quantize<float>(x, ldx, out, M, K, st) : mp::launch_quantize<mp::bf16_t>(x, ldx, out, M, K, st);
}

// x: MXFP8 rows ldx bytes apart (16-byte aligned); w / scale: MXFP4 as stored; y / res: bf16 rows.
// Returns as above.
extern "C" int mp_gemm_mx(const void* x, const void* w, const uint8_t* scale, void* y, const void* bias, const void* res,
                          int M, int N, int K, int64_t ldx, int64_t ldy, int64_t ldr, int gelu, hipStream_t st) {
  const gemm_mx::Plan p = gemm_mx::plan(M, N, K);
  if (p.tile == gemm_mx::NONE || scale == nullptr) return -1;
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || (M > 1 && (ldx % 16 != 0 || ldx < gemm_mx::mx8_row_bytes(K))))
    return -1;
  mp::GemmMxArgs a;
  a.x = (const uint8_t*)x, a.w = (const uint8_t*)w, a.ws = scale, a.y = (mp::bf16_t*)y;
  a.bias = (const mp::bf16_t*)bias, a.res = (const mp::bf16_t*)res;
  a.M = M, a.N = N, a.K = K, a.gelu = gelu, a.ldx = ldx, a.ldy = ldy, a.ldr = ldr;
  if (p.tile == gemm_mx::NARROW) return mp::launch_gemm_mx<4, 1, 1, 2>(a, p, st);
  return mp::launch_gemm_mx<2, 2, 4, 4>(a, p, st);
}
