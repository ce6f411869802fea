// v2 bf16 MFMA GEMM: 8 waves, large tiles, direct-to-LDS staging (global_load_lds_dwordx4).
//
//   C[M,N] (+)= alpha * op(A) op(B) (+ fused epilogue); same contract as gemm.hip
//   (TA/TB layouts, epilogues, f32 split-K accumulate), different engine:
//
// * Tiles BMxBN (256x256, 256x192, 256x128, 128x128) chosen per problem by the host so
//   the tile count fills whole "waves" of 256 CUs (GPT-2: N = 768 / 2304 / 3072 divide
//   by 192/256 -> zero quantisation loss at T = 16384 tokens).
// * Staging: every 1 KiB piece of a tile is one wave-instruction of global_load_lds
//   (no VGPR round trip, no ds_write).  The LDS destination is lane-linear, so the
//   bank-conflict swizzle of the image is applied on the *source* address (cdna guide
//   §5.4 rule 21): lane l fetches the logical chunk that belongs at its physical slot.
// * Pipeline: 2 LDS stages; tile t+1 is in flight while tile t is consumed; counted
//   `s_waitcnt vmcnt(P)` (P = pieces per wave per tile) + raw s_barrier, never
//   __syncthreads() (which would drain the in-flight DMA).
// * MFMA 32x32x16 bf16, per wave (BM/WM)x(BN/WN); fragments by ds_read_b128 (K-contiguous
//   images) or two ds_read_b64_tr_b16 (outer-contiguous images).
// * Epilogue staged through LDS one wave-row group at a time -> coalesced 16-byte bias /
//   residual / activation / store, or lane-consecutive f32 atomics for split-K.
#include <climits>
#include <type_traits>

#include "mp_api.h"
#include "mp_gemm_core.h"
#include "mp_gemm_tiles.h"
#include "mp_gemm_pingpong.h"
#include "mp_gemm_regstage.h"
#ifdef MP_PROBE_ENGINES
#include "mp_gemm_probe.h"
#endif
#include "mp_gemm_small.h"
#include "mp_gemm_plan.h"

using namespace g2;

template <bool TA, bool TB, int EPI, bool ACC>
static int dispatch(int cfg, const void* A, const void* B, void* C, const void* bias, const void* R, void* X, float* ws,
                    int M,
                    int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx, float alpha,
                    int split, float p_drop, uint64_t seed, hipStream_t st) {
  if constexpr (TA && TB && ACC && EPI == EPI_NONE) {
    if (cfg == CFG_S_TT) return launchs<64, 64, EPI, ACC, true, true>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    if (cfg == CFG_PP_TT) return launch3<EPI, ACC, true, true>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
  }
  if constexpr (!TA && !TB) {
    if (cfg == CFG_S64x64) return launchs<64, 64, EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    if (cfg == CFG_S64x32) return launchs<64, 32, EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    if (cfg == CFG_S32x32) return launchs<32, 32, EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    if (cfg == CFG_PP_M32) return launch3<EPI, ACC, false>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    if (cfg == CFG_PP_M16) return launch3<EPI, ACC, true>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    if (cfg == CFG_G6) return launch6<EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed, st);
    if (cfg == CFG_G8) return launch8<EPI, ACC, 2>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed, st);
    if (cfg == CFG_G8_PGR3) return launch8<EPI, ACC, 3>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed, st);
#ifdef MP_PROBE_ENGINES
    if constexpr (!ACC) {
      if (cfg == CFG_G5) return launch5<EPI>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed, st);
    }
#endif
  }
  switch (cfg) {
    case CFG_T256x256: return launch<256, 256, 2, 4, TA, TB, EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    case CFG_T256x192: return launch<256, 192, 4, 2, TA, TB, EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    case CFG_T256x128: return launch<256, 128, 4, 2, TA, TB, EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
    default: return launch<128, 128, 2, 4, TA, TB, EPI, ACC>(A, B, C, bias, R, X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, split, p_drop, seed, st);
  }
}

// C[M,N] (f32, row stride ldc) += sum over the split-K slabs ws[s][M][N]
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ C, int M,
                                                            int N, int64_t ldc, int split) {
  const int64_t n4 = (int64_t)M * N / 4;
  const int64_t slab = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i * 4;
    const int m = (int)(e / N), n = (int)(e % N);
    float4 acc = *reinterpret_cast<const float4*>(ws + e);
    for (int s = 1; s < split; ++s) {
      const float4 v = *reinterpret_cast<const float4*>(ws + s * slab + e);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float4* cp = reinterpret_cast<float4*>(C + (int64_t)m * ldc + n);
    float4 c = *cp;
    c.x += acc.x; c.y += acc.y; c.z += acc.z; c.w += acc.w;
    *cp = c;
  }
}

// bf16 C[M,N] = epilogue(alpha-scaled sum of the split-K slabs ws[s][M][N])
template <int EPI>
__global__ void __launch_bounds__(256) splitk_epi_kernel(const float* __restrict__ ws, bf16_t* __restrict__ C, int M,
                                                         int N, int64_t ldc, int split, const bf16_t* __restrict__ bias,
                                                         const bf16_t* __restrict__ R, int64_t ldr,
                                                         bf16_t* __restrict__ AUX, int64_t ldx, float p_drop,
                                                         uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  const int64_t n8 = (int64_t)M * N / 8;
  const int64_t slab = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i * 8;
    const int m = (int)(e / N), n = (int)(e % N);
    float4 a = *reinterpret_cast<const float4*>(ws + e), b = *reinterpret_cast<const float4*>(ws + e + 4);
    for (int s = 1; s < split; ++s) {
      const float4 c = *reinterpret_cast<const float4*>(ws + s * slab + e);
      const float4 d = *reinterpret_cast<const float4*>(ws + s * slab + e + 4);
      a.x += c.x; a.y += c.y; a.z += c.z; a.w += c.w;
      b.x += d.x; b.y += d.y; b.z += d.z; b.w += d.w;
    }
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    epi_store8<EPI>(v, m, n, C, ldc, bias, R, ldr, AUX, ldx, p_drop, seed);
  }
}

template <int EPI>
static int launch_splitk_epi(const float* ws, void* C, int M, int N, int64_t ldc, int split, const void* bias,
                             const void* R, int64_t ldr, void* X, int64_t ldx, float p_drop, uint64_t seed,
                             hipStream_t st) {
  const int64_t n8 = (int64_t)M * N / 8;
  const int blocks = (int)std::min<int64_t>((n8 + 255) / 256, 4096);
  splitk_epi_kernel<EPI><<<blocks, 256, 0, st>>>(ws, (bf16_t*)C, M, N, ldc, split, (const bf16_t*)bias,
                                                 (const bf16_t*)R, ldr, (bf16_t*)X, ldx, p_drop, seed);
  return (int)hipGetLastError();
}

static_assert(PLAN_BK == BK, "the planner counts K-tiles of the engines' BK");

// f(std::integral_constant<int, E>) for the runtime epilogue E; -2 for a number that is none
template <class F>
static int with_epi(int epilogue, F&& f) {
  switch (epilogue) {
#define MP_E(E_) case E_: return f(std::integral_constant<int, E_>{});
    MP_E(EPI_NONE) MP_E(EPI_BIAS) MP_E(EPI_BIAS_GELU) MP_E(EPI_BIAS_RELU) MP_E(EPI_BIAS_RES) MP_E(EPI_RES)
    MP_E(EPI_DGELU) MP_E(EPI_DRELU)
#undef MP_E
    default: return -2;
  }
}

// 1 when the probe engines (gemm4 cfg 7 / 100+G, gemm5 cfg 8, gemm7 cfg 14) are compiled in
extern "C" int mp_gemm2_has_probe_engines() {
#ifdef MP_PROBE_ENGINES
  return 1;
#else
  return 0;
#endif
}

// f32 workspace elements the planned engine needs (split-K slabs, or the stream-K flags +
// partial-tile slots)
extern "C" int64_t mp_gemm2_ws_floats(int cfg, int split, int M, int N, int K) {
#ifdef MP_PROBE_ENGINES
  if (cfg == CFG_SK) {
    // partial slots are indexed by block id; contributors are blocks x + 8 l with
    // l < c (S - 1) for the fullest XCD group's c tail tiles
    Plan7 pl{};
    if (!plan7(M, N, K, PlanEnv::process(), &pl)) return (int64_t)SK_FLAGS + (int64_t)SK_MAX_G * SK_SLOT;
    const int cmax = (pl.tail + 7) / 8;
    const int64_t slots = (int64_t)8 * cmax * (pl.S - 1);
    return (int64_t)SK_FLAGS + slots * SK_SLOT;
  }
#endif
  return split > 1 ? (int64_t)split * M * N : 0;
}

// Runs the planned engine: cfg / split are plan_gemm's answer for this problem and force_cfg
// (mp_gemm_plan.h; the caller plans once and sizes ws with mp_gemm2_ws_floats).
// returns -2 if the (layout, epilogue) combination is not instantiated here (caller falls back to v1).
// With split-K (f32 accumulate) and a workspace of split*M*N floats the partial products go
// to slabs + one reduce pass; without a workspace they are added with f32 atomics.
extern "C" int mp_gemm2(const void* A, const void* B, void* C, const void* bias, const void* residual, void* aux,
                        int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ld_res, int64_t ld_aux,
                        int transA, int transB, int epilogue, int c_f32_accum, float alpha, int cfg, int split,
                        int force_cfg, float* ws, float* colsum, float p_drop, uint64_t seed, hipStream_t st) {
  if (K % BK != 0 || N % 8 != 0 || M % 8 != 0) return -1;
#ifdef MP_PROBE_ENGINES
  if (cfg == CFG_SK) {
    if (ws == nullptr) return -1;
    return with_epi(epilogue, [&](auto E) {
      return launch7<decltype(E)::value>(A, B, C, bias, residual, aux, colsum, ws, M, N, K, lda, ldb, ldc, ld_res,
                                         ld_aux, alpha, p_drop, seed, st);
    });
  }
#endif
  if (colsum != nullptr) {
    // fused output column sums: bf16 outputs, one pass (no split-K); -3 tells the caller
    // to sum separately
    if (c_f32_accum || split > 1) return -3;
    ws = colsum;
  }
  if (cfg < 0) return -1;
#ifdef MP_PROBE_ENGINES
  // plain / bias NT GEMMs of more 256x256 tiles than CUs: the persistent engine that
  // writes part of each tile's C during the next tile's main loop.  Opt-in
  // (MIPIPE_GEMM4=1): correct, but 1.2-2x slower than gemm3 -- the 64-VGPR stash does not
  // fit beside gemm3's 222 VGPRs at 2 waves/SIMD, and the spill reloads in the MFMA loop
  // drain the DMA pipeline (profiles/r2_probes.md "gemm4")
  const bool g4_ok = split == 1 && colsum == nullptr && !c_f32_accum && !transA && !transB &&
                     (epilogue == EPI_NONE || epilogue == EPI_BIAS) && ldc % 4 == 0;
  const bool use4 = PlanEnv::process().gemm4 && cfg == CFG_PP_M16 && force_cfg < 0 && tiles256(M, N) > 256;
  if (g4_ok && (cfg == CFG_G4 || use4)) {
    const int grid = force_cfg >= 100 ? force_cfg - 100 : 0;
    if (epilogue == EPI_NONE) return launch4<EPI_NONE>(A, B, C, nullptr, M, N, K, lda, ldb, ldc, alpha, grid, st);
    return launch4<EPI_BIAS>(A, B, C, bias, M, N, K, lda, ldb, ldc, alpha, grid, st);
  }
#endif
  if (cfg == CFG_G4) return -2;
  if (!c_f32_accum && split > 1) {
    // bf16 output, split-K: partial products into f32 slabs (alpha applied there), then
    // one pass sums them and applies the fused epilogue
    if (ws == nullptr) return -1;
    int rc = -2;
    if (transA && transB) rc = dispatch<true, true, EPI_NONE, true>(cfg, A, B, nullptr, nullptr, nullptr, nullptr, ws, M, N, K,
                                                              lda, ldb, N, 0, 0, alpha, split, p_drop, seed, st);
    else rc = dispatch<false, false, EPI_NONE, true>(cfg, A, B, nullptr, nullptr, nullptr, nullptr, ws, M, N, K, lda, ldb,
                                                     N, 0, 0, alpha, split, p_drop, seed, st);
    if (rc != 0) return rc;
    return with_epi(epilogue, [&](auto E) {
      return launch_splitk_epi<decltype(E)::value>(ws, C, M, N, ldc, split, bias, residual, ld_res, aux, ld_aux, p_drop,
                                                   seed, st);
    });
  }
  // instantiated: every epilogue for NT bf16 outputs; plain f32 accumulate for NT and TT
  float* wsp = (split > 1 || colsum != nullptr) ? ws : nullptr;
  int rc = -2;
  if (!transA && !transB && !c_f32_accum) {
    rc = with_epi(epilogue, [&](auto E) {
      return dispatch<false, false, decltype(E)::value, false>(cfg, A, B, C, bias, residual, aux, wsp, M, N, K, lda, ldb,
                                                               ldc, ld_res, ld_aux, alpha, split, p_drop, seed, st);
    });
  } else if ((bool)transA == (bool)transB && epilogue == EPI_NONE && c_f32_accum) {
    rc = transA ? dispatch<true, true, EPI_NONE, true>(cfg, A, B, C, bias, residual, aux, wsp, M, N, K, lda, ldb, ldc,
                                                      ld_res, ld_aux, alpha, split, p_drop, seed, st)
                : dispatch<false, false, EPI_NONE, true>(cfg, A, B, C, bias, residual, aux, wsp, M, N, K, lda, ldb, ldc,
                                                        ld_res, ld_aux, alpha, split, p_drop, seed, st);
  }
  if (rc == 0 && wsp != nullptr && split > 1) {
    const int64_t n4 = (int64_t)M * N / 4;
    const int blocks = (int)std::min<int64_t>((n4 + 255) / 256, 4096);
    splitk_reduce_kernel<<<blocks, 256, 0, st>>>(wsp, reinterpret_cast<float*>(C), M, N, ldc, split);
    rc = (int)hipGetLastError();
  }
  return rc;
}

MP_DROP_STEP_SETTER(mp_set_drop_step_gemm)

// C_g += alpha * A_g^T B_g for n <= MP_GROUP_MAX problems (A_g [K_g][M_g], B_g [K_g][N_g]
// bf16 k-major, C_g f32 [M_g][N_g] row stride ldc_g) in one launch; -1 if a shape does not
// fit the 64x64 TT tile contract (M, N multiples of 8, K of 64)
extern "C" int mp_gemm_tt_grouped(int n, const void* const* A, const void* const* B, float* const* C, const int* M,
                                  const int* N, const int* K, const int64_t* lda, const int64_t* ldb,
                                  const int64_t* ldc, float alpha, hipStream_t st) {
  if (n <= 0) return 0;
  if (n > MP_GROUP_MAX) return -1;
  GroupTT g{};
  g.n = n;
  g.alpha = alpha;
  int t = 0;
  for (int i = 0; i < n; ++i) {
    if (M[i] % 8 || N[i] % 8 || K[i] % BK || M[i] <= 0 || N[i] <= 0) return -1;
    g.A[i] = (const bf16_t*)A[i];
    g.B[i] = (const bf16_t*)B[i];
    g.C[i] = C[i];
    g.M[i] = M[i];
    g.N[i] = N[i];
    g.K[i] = K[i];
    g.lda[i] = lda[i];
    g.ldb[i] = ldb[i];
    g.ldc[i] = ldc[i];
    g.tile_start[i] = t;
    t += ((M[i] + 63) / 64) * ((N[i] + 63) / 64);
  }
  for (int i = n; i <= MP_GROUP_MAX; ++i) g.tile_start[i] = t;
  constexpr int STAGE = (64 + 64) * BK * 2;
  constexpr int EPI_BYTES = 32 * (64 + 4) * 4;
  constexpr int LDS = 2 * STAGE > EPI_BYTES ? 2 * STAGE : EPI_BYTES;
  static bool attr = false;
  lds_attr_once(attr, (const void*)gemms_tt_grouped_kernel, LDS);
  gemms_tt_grouped_kernel<<<t, 256, LDS, st>>>(g);
  return (int)hipGetLastError();
}

// split-K factor a grouped long-token dW launch will use (force_split > 0 or
// MIPIPE_DW_GROUP_SPLIT set it) and the f32 workspace it needs: S * sum(M_g * N_g) for S > 1
extern "C" int mp_gemm3_tt_grouped_plan(int n, const int* M, const int* N, int K, int force_split,
                                        int64_t* ws_floats) {
  int tiles = 0;
  int64_t elems = 0;
  for (int i = 0; i < n; ++i) {
    tiles += ((M[i] + 255) / 256) * ((N[i] + 255) / 256);
    elems += (int64_t)M[i] * N[i];
  }
  const int S = choose_group_split(tiles, K / BK, force_split, PlanEnv::process());
  *ws_floats = S > 1 ? (int64_t)S * elems : 0;
  return S;
}

// C_g += alpha * A_g^T B_g for n <= MP_GROUP_MAX problems over one common K (A_g [K][M_g],
// B_g [K][N_g] bf16 k-major, C_g f32 [M_g][N_g] row stride ldc_g): one launch of 256x256
// tiles at split S (from mp_gemm3_tt_grouped_plan; ws holds its workspace) plus, for S > 1,
// one reduce launch.  -1 if a shape does not fit (M, N multiples of 8, K of 64, 1 <= S <= K / 64)
extern "C" int mp_gemm3_tt_grouped(int n, const void* const* A, const void* const* B, float* const* C, const int* M,
                                   const int* N, int K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc,
                                   float alpha, int S, float* ws, hipStream_t st) {
  if (n <= 0) return 0;
  if (n > MP_GROUP_MAX || K <= 0 || K % BK || S < 1 || S > K / BK || (S > 1 && ws == nullptr)) return -1;
  GroupTT3 g{};
  g.n = n;
  g.K = K;
  g.S = S;
  g.alpha = alpha;
  g.ws = ws;
  int t = 0;
  int64_t e = 0;
  for (int i = 0; i < n; ++i) {
    if (M[i] % 8 || N[i] % 8 || M[i] <= 0 || N[i] <= 0) return -1;
    g.A[i] = (const bf16_t*)A[i];
    g.B[i] = (const bf16_t*)B[i];
    g.C[i] = C[i];
    g.M[i] = M[i];
    g.N[i] = N[i];
    g.lda[i] = lda[i];
    g.ldb[i] = ldb[i];
    g.ldc[i] = ldc[i];
    g.tile_start[i] = t;
    g.elem_start[i] = e;
    t += ((M[i] + 255) / 256) * ((N[i] + 255) / 256);
    e += (int64_t)M[i] * N[i];
  }
  for (int i = n; i <= MP_GROUP_MAX; ++i) {
    g.tile_start[i] = t;
    g.elem_start[i] = e;
  }
  if ((int64_t)t * S > INT_MAX) return -1;
  constexpr int LDS_MAIN = 2 * 4 * 128 * 128;
  constexpr int EPI_BYTES = 128 * (256 + 4) * 4;
  constexpr int LDS = LDS_MAIN > EPI_BYTES ? LDS_MAIN : EPI_BYTES;
  static bool attr = false;
  lds_attr_once(attr, (const void*)gemm3_tt_grouped_kernel, LDS);
  gemm3_tt_grouped_kernel<<<t * S, NT, LDS, st>>>(g);
  int rc = (int)hipGetLastError();
  if (rc == 0 && S > 1) {
    const int blocks = (int)std::min<int64_t>((e / 4 + 255) / 256, 4096);
    splitk_reduce_grouped_kernel<<<blocks, 256, 0, st>>>(g);
    rc = (int)hipGetLastError();
  }
  return rc;
}
