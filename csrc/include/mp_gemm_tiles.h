// The 2-stage tile engine (cfg 0-3): gemm2_kernel on 256x256 / 256x192 / 256x128 / 128x128
// tiles, every layout, and its launcher.
#pragma once

#include "mp_gemm_core.h"
#include "mp_gemm_plan.h"

namespace g2 {

template <int BM, int BN, int WM, int WN, bool TA, bool TB, int EPI, bool ACC, bool M16>
__global__ void __launch_bounds__(NT, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) gemm2_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                                      void* __restrict__ Cv, const bf16_t* __restrict__ bias,
                                                      const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
                                                      float* __restrict__ WS, int M, int N, int K, int64_t lda,
                                                      int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx,
                                                      float alpha, float p_drop, uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  static_assert(WM * WN == 8, "8 waves");
  constexpr int WTM = BM / WM / 32, WTN = BN / WN / 32;
  static_assert(WTM * 32 * WM == BM && WTN * 32 * WN == BN, "tile/wave mismatch");
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
  constexpr int PIECES = STAGE / 1024, PW = PIECES / 8;
  static_assert(PW * 8 == PIECES, "pieces must split over 8 waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  const int nwg = gm * gn;
  const int wg = xcd_remap((int)blockIdx.x, nwg);
  constexpr int GROUP = 8;
  const int group = wg / (GROUP * gn);
  const int first_m = group * GROUP;
  const int gsz = min(gm - first_m, GROUP);
  const int tm = first_m + (wg % (GROUP * gn)) % gsz;
  const int tn = (wg % (GROUP * gn)) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int wm = wr * (BM / WM), wn = wc * (BN / WN);

  // split-K: split y owns k-tiles [y*KT/S, (y+1)*KT/S) (uneven splits allowed, so the
  // split count can be chosen for CU fill rather than divisibility)
  const int nsplit = gridDim.y;
  const int ktiles = K / BK;
  const int kt0 = (int)blockIdx.y * ktiles / nsplit;
  const int nk = ((int)blockIdx.y + 1) * ktiles / nsplit - kt0;
  const int kbase = kt0 * BK;

  // per-lane source pointers of every piece this wave stages, at k = kbase; a later
  // k-tile only adds a wave-uniform offset (k0 elements for K-contiguous images,
  // k0 rows for outer-contiguous ones)
  const bf16_t* psrc[PW];
  bool pisA[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int p = wave + 8 * i;            // wave-uniform piece index
    const int pos = p * 1024 + lane * 16;  // this lane's byte in the stage
    pisA[i] = p * 1024 < A_BYTES;
    if (pisA[i]) psrc[i] = src_of<TA, BM, M16>(A, lda, pos, m0, M, kbase);
    else psrc[i] = src_of<TB, BN, M16>(B, ldb, pos - A_BYTES, n0, N, kbase);
  }
  auto issue = [&](int stage, int kt) {
    char* sb = smem + stage * STAGE;
    const int64_t dA = TA ? (int64_t)kt * BK * lda : (int64_t)kt * BK;
    const int64_t dB = TB ? (int64_t)kt * BK * ldb : (int64_t)kt * BK;
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int p = wave + 8 * i;
      const bf16_t* src = psrc[i] + (pisA[i] ? dA : dB);
      __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(sb + p * 1024),
                                       16, 0, 0);
    }
  };

  if constexpr (!M16) {
  f32x16 acc[WTM][WTN];
#pragma unroll
  for (int i = 0; i < WTM; ++i)
#pragma unroll
    for (int j = 0; j < WTN; ++j) acc[i][j] = {};

  issue(0, 0);
  if (nk > 1) {
    issue(1, 1);
    wait_vmcnt<PW>();
  } else {
    wait_vmcnt<0>();
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  for (int t = 0; t < nk; ++t) {
    const char* sa = smem + (t & 1) * STAGE;
    const char* sbB = sa + A_BYTES;
    // fragments double-buffered in registers: k-substep s+1 is read from LDS while the
    // MFMAs of substep s issue (the loop is fully unrolled, so [s & 1] is static)
    bf16x8 af[2][WTM], bfr[2][WTN];
#pragma unroll
    for (int i = 0; i < WTM; ++i) af[0][i] = frag<TA, BM>(sa, wm + 32 * i + l32, 0, hl);
#pragma unroll
    for (int j = 0; j < WTN; ++j) bfr[0][j] = frag<TB, BN>(sbB, wn + 32 * j + l32, 0, hl);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      const int c = s & 1;
      if (s + 1 < BK / 16) {
#pragma unroll
        for (int i = 0; i < WTM; ++i) af[c ^ 1][i] = frag<TA, BM>(sa, wm + 32 * i + l32, s + 1, hl);
#pragma unroll
        for (int j = 0; j < WTN; ++j) bfr[c ^ 1][j] = frag<TB, BN>(sbB, wn + 32 * j + l32, s + 1, hl);
      }
      // pin the order: substep s+1's LDS reads are in flight under substep s's MFMAs
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < WTM; ++i)
#pragma unroll
        for (int j = 0; j < WTN; ++j) acc[i][j] = mfma32(af[c][i], bfr[c][j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // everyone finished reading this stage before it is refilled
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 2 < nk) {
      issue(t & 1, t + 2);
      wait_vmcnt<PW>();  // tile t+1 landed, tile t+2 still in flight
    } else {
      wait_vmcnt<0>();
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }

  epilogue<BM, BN, WM, WN, EPI, ACC>(Stage32<WTM, WTN>{acc, wn, hl, l32}, smem, m0, n0, wr, Cv, bias, R, AUX, WS, M,
                                     N, ldc, ldr, ldx, alpha, nsplit, p_drop, seed);  } else {
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{};

  issue(0, 0);
  if (nk > 1) {
    issue(1, 1);
    wait_vmcnt<PW>();
  } else {
    wait_vmcnt<0>();
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  for (int t = 0; t < nk; ++t) {
    const char* sa = smem + (t & 1) * STAGE;
    const char* sbB = sa + A_BYTES;
    // two 32-deep k-substeps; substep 1's fragments are read under substep 0's MFMAs
    // (transposed layouts: one fragment set, the compiler overlaps what registers allow --
    // double-buffering the 256x256 TT tile spilled)
    if constexpr (TA || TB) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 af1[TM], bf1[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af1[i] = frag16<TA, BM>(sa, wm + 16 * i, s);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf1[j] = frag16<TB, BN>(sbB, wn + 16 * j, s);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(af1[i], bf1[j], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
    } else {
    bf16x8 af[2][TM], bfr[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[0][i] = frag16<TA, BM>(sa, wm + 16 * i, 0);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[0][j] = frag16<TB, BN>(sbB, wn + 16 * j, 0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) af[1][i] = frag16<TA, BM>(sa, wm + 16 * i, 1);
#pragma unroll
        for (int j = 0; j < TN; ++j) bfr[1][j] = frag16<TB, BN>(sbB, wn + 16 * j, 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(af[s][i], bfr[s][j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
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

  epilogue<BM, BN, WM, WN, EPI, ACC>(Stage16<TM, TN>{acc, wn, lane}, smem, m0, n0, wr, Cv, bias, R, AUX, WS, M, N, ldc,
                                     ldr, ldx, alpha, nsplit, p_drop, seed);
  }

}

template <int BM, int BN, int WM, int WN, bool TA, bool TB, int EPI, bool ACC>
static int launch(const void* A, const void* B, void* C, const void* bias, const void* R, void* X, float* ws, int M,
                  int N, int K,
                  int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx, float alpha, int split,
                  float p_drop, uint64_t seed, hipStream_t st) {
  constexpr int STAGE = (BM + BN) * BK * 2;
  constexpr int EPI_BYTES = (BM / WM) * (BN + 4) * 4;
  constexpr int LDS = 2 * STAGE > EPI_BYTES ? 2 * STAGE : EPI_BYTES;
  // 16x16x32 (MIPIPE_GEMM_M16=0: never) only for K-contiguous operands: with the transposed
  // (tr-read) images of the TT dW GEMMs it measured 1.8x slower (dw_qkv 374 vs 688 TF), so
  // those keep 32x32x16 (MIPIPE_GEMM_M16T=1: they take it too)
  const PlanEnv& env = PlanEnv::process();
  auto kern = (env.m16 && (env.m16t || (!TA && !TB))) ? gemm2_kernel<BM, BN, WM, WN, TA, TB, EPI, ACC, true>
                                  : gemm2_kernel<BM, BN, WM, WN, TA, TB, EPI, ACC, false>;
  static bool attr = false;
  lds_attr_once(attr, (const void*)kern, LDS);
  const int nwg = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  kern<<<dim3(nwg, split), NT, LDS, st>>>((const bf16_t*)A, (const bf16_t*)B, C, (const bf16_t*)bias,
                                          (const bf16_t*)R, (bf16_t*)X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed);
  return (int)hipGetLastError();
}

}  // namespace g2
