// The small-tile engine (cfg 10-12 NT, cfg 13 TT dW) and its grouped dW kernel.
#pragma once

#include "mp_gemm_core.h"

namespace g2 {

// ---------------------------------------------------------------------------------------
// gemms: small-tile NT engine for short-token problems (the reference model's 1024-token
// microbatches: M = 1024, N = 768..2304).  A 256x256 grid there has 12-36 tiles for 256
// CUs, and split-K to fill the chip costs an f32 slab round trip plus a reduce/epilogue
// kernel per GEMM (~40 % of those GEMMs' time, profiles/r2_ref_L8H8_kernel_stats.csv).
// Here: 256-thread workgroups (2x2 waves), BM x BN in {64x64, 64x32, 32x32}, 16x16x32
// MFMAs, the same 2-stage global_load_lds pipeline / swizzled K-contiguous images as
// gemm2, several workgroups per CU (32 KiB LDS at 64x64), and the fused epilogue applied
// directly -- one launch per GEMM, no split-K.
// ---------------------------------------------------------------------------------------
// one BM x BN output tile (workgroup-linear index wg of the problem's tile grid, split
// ``split`` of ``nsplit``) of the small engine; shared by gemms_kernel and the grouped
// weight-gradient kernel below
template <int BM, int BN, int EPI, bool ACC, bool TA, bool TB>
__device__ __forceinline__ void gemms_tile(char* smem, const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                           void* __restrict__ Cv, const bf16_t* __restrict__ bias,
                                           const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
                                           float* __restrict__ WS, int M, int N, int K, int64_t lda, int64_t ldb,
                                           int64_t ldc, int64_t ldr, int64_t ldx, float alpha, float p_drop,
                                           uint64_t seed, int wg, int nsplit, int split) {
  constexpr int NTH = 256, WM = 2, WN = 2;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  static_assert(TM >= 1 && TN >= 1 && TM * 16 * WM == BM && TN * 16 * WN == BN, "tile/wave mismatch");
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
  constexpr int PIECES = STAGE / 1024, PW = PIECES / 4;
  static_assert(PW * 4 == PIECES, "pieces must split over 4 waves");

  const int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  constexpr int GROUP = 8;
  const int group = wg / (GROUP * gn);
  const int first_m = group * GROUP;
  const int gsz = min(gm - first_m, GROUP);
  const int tm = first_m + (wg % (GROUP * gn)) % gsz;
  const int tn = (wg % (GROUP * gn)) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int wm = wr * (BM / WM), wn = wc * (BN / WN);

  const int ktiles = K / BK;
  const int kt0 = split * ktiles / nsplit;
  const int nk = (split + 1) * ktiles / nsplit - kt0;
  const int kbase = kt0 * BK;

  const bf16_t* psrc[PW];
  bool pisA[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int p = wave + 4 * i;
    const int pos = p * 1024 + lane * 16;
    pisA[i] = p * 1024 < A_BYTES;
    if (pisA[i]) psrc[i] = src_of<TA, BM, true>(A, lda, pos, m0, M, kbase);
    else psrc[i] = src_of<TB, BN, true>(B, ldb, pos - A_BYTES, n0, N, kbase);
  }
  auto issue = [&](int stage, int kt) {
    char* sb = smem + stage * STAGE;
    const int64_t dA = TA ? (int64_t)kt * BK * lda : (int64_t)kt * BK;
    const int64_t dB = TB ? (int64_t)kt * BK * ldb : (int64_t)kt * BK;
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int p = wave + 4 * i;
      __builtin_amdgcn_global_load_lds((const void*)(psrc[i] + (pisA[i] ? dA : dB)),
                                       (__attribute__((address_space(3))) void*)(sb + p * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{};

  if (nk > 0) {
    issue(0, 0);
    if (nk > 1) {
      issue(1, 1);
      wait_vmcnt<PW>();
    } else {
      wait_vmcnt<0>();
    }
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  for (int t = 0; t < nk; ++t) {
    const char* sa = smem + (t & 1) * STAGE;
    const char* sbB = sa + A_BYTES;
    bf16x8 af[2][TM], bfr[2][TN];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
#pragma unroll
      for (int i = 0; i < TM; ++i) af[s_][i] = frag16<TA, BM>(sa, wm + 16 * i, s_);
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[s_][j] = frag16<TB, BN>(sbB, wn + 16 * j, s_);
    }
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(af[s_][i], bfr[s_][j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 2 < nk) {
      issue(t & 1, t + 2);
      wait_vmcnt<PW>();
    } else {
      wait_vmcnt<0>();
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  epilogue<BM, BN, WM, WN, EPI, ACC, NTH>(Stage16<TM, TN>{acc, wn, lane}, smem, m0, n0, wr, Cv, bias, R, AUX, WS, M,
                                          N, ldc, ldr, ldx, alpha, nsplit, p_drop, seed);
}

template <int BM, int BN, int EPI, bool ACC, bool TA = false, bool TB = false>
__global__ void __launch_bounds__(256) gemms_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                                    void* __restrict__ Cv, const bf16_t* __restrict__ bias,
                                                    const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
                                                    float* __restrict__ WS, int M, int N, int K, int64_t lda,
                                                    int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx, float alpha, float p_drop, uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nwg = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  gemms_tile<BM, BN, EPI, ACC, TA, TB>(smem, A, B, Cv, bias, R, AUX, WS, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop,
                                       seed, xcd_remap((int)blockIdx.x, nwg), (int)gridDim.y, (int)blockIdx.y);
}

// ---------------------------------------------------------------------------------------
// Grouped weight-gradient GEMMs: up to MP_GROUP_MAX independent TT problems
// C_g[M_g, N_g] += alpha * A_g^T B_g (A_g [K_g][M_g], B_g [K_g][N_g] k-major, f32 C) in ONE
// launch of 64x64 tiles.  A layer's dW GEMMs at 1024-token microbatches are 144-432 tiles
// each: one launch per GEMM leaves most of the 256 CUs idle and pays the short k-loop's
// latency per GEMM (97-230 TF, tools/wbatch_probe.py); grouped, ~1900 tiles of a layer
// share the chip, several workgroups per CU hide each other's load latency.  Workgroup
// b -> problem g with tile_start[g] <= b' < tile_start[g + 1] (b' = XCD-remapped b;
// wave-uniform scan of <= 8 entries), then the problem-local tile of gemms_tile.
// ---------------------------------------------------------------------------------------
struct GroupTT {
  const bf16_t* A[MP_GROUP_MAX];
  const bf16_t* B[MP_GROUP_MAX];
  float* C[MP_GROUP_MAX];
  int64_t lda[MP_GROUP_MAX], ldb[MP_GROUP_MAX], ldc[MP_GROUP_MAX];
  int M[MP_GROUP_MAX], N[MP_GROUP_MAX], K[MP_GROUP_MAX];
  int tile_start[MP_GROUP_MAX + 1];
  int n;
  float alpha;
};

__global__ void __launch_bounds__(256) gemms_tt_grouped_kernel(const GroupTT g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int total = g.tile_start[g.n];
  const int b = xcd_remap((int)blockIdx.x, total);
  int p = 0;
#pragma unroll
  for (int i = 1; i < MP_GROUP_MAX; ++i)
    if (i < g.n && b >= g.tile_start[i]) p = i;
  gemms_tile<64, 64, EPI_NONE, true, true, true>(smem, g.A[p], g.B[p], g.C[p], nullptr, nullptr, nullptr, nullptr,
                                                 g.M[p], g.N[p], g.K[p], g.lda[p], g.ldb[p], g.ldc[p], 0, 0, g.alpha,
                                                 0.f, 0, b - g.tile_start[p], 1, 0);
}

template <int BM, int BN, int EPI, bool ACC, bool TA = false, bool TB = false>
static int launchs(const void* A, const void* B, void* C, const void* bias, const void* R, void* X, float* ws, int M,
                   int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx, float alpha, int split,
                   float p_drop, uint64_t seed, hipStream_t st) {
  constexpr int STAGE = (BM + BN) * BK * 2;
  constexpr int EPI_BYTES = (BM / 2) * (BN + 4) * 4;
  constexpr int RED_BYTES = 256 * 8 * 4;   // the column-sum reduction reuses the staging area
  constexpr int LDS0 = 2 * STAGE > EPI_BYTES ? 2 * STAGE : EPI_BYTES;
  constexpr int LDS = LDS0 > RED_BYTES ? LDS0 : RED_BYTES;
  auto kern = gemms_kernel<BM, BN, EPI, ACC, TA, TB>;
  static bool attr = false;
  lds_attr_once(attr, (const void*)kern, LDS);
  const int nwg = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  kern<<<dim3(nwg, split), 256, LDS, st>>>((const bf16_t*)A, (const bf16_t*)B, C, (const bf16_t*)bias,
                                           (const bf16_t*)R, (bf16_t*)X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed);
  return (int)hipGetLastError();
}

}  // namespace g2
