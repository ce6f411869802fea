// The ping-pong engines: gemm3 (cfg 4 / 5 NT, cfg 6 TT dW) with its grouped dW kernel and
// grouped split-K reduce, and gemm6 (cfg 9), the same schedule on 256x192 tiles.
#pragma once

#include "mp_gemm_core.h"

namespace g2 {

// ---------------------------------------------------------------------------------------
// gemm3: 256x256 NT (both operands K-contiguous) with a ping-pong phase schedule.
//
// The K-tile (BK = 64) is cut into four 16 KiB half-tiles, each one LDS image of 128 rows:
//   A0 = rows {0..63, 128..191}   A1 = rows {64..127, 192..255}     (wave-row halves)
//   B0 = cols {0..31, 64..95, ..} B1 = cols {32..63, 96..127, ..}  (wave-col halves)
// A wave (wr, wc) owns a 128x64 output tile = four 64x32 quadrants, one per phase:
//   phase 1: A0 x B0 (reads A0 + B0)  phase 2: A0 x B1 (reads B1)
//   phase 3: A1 x B0 (reads A1)       phase 4: A1 x B1 (no reads)
// Phase p of K-tile t also streams half-tile p of K-tile t+1 into the other LDS buffer
// (2 glds per thread) -- DMA is spread evenly over the loop instead of bursting once
// per K-tile -- and a counted vmcnt(4) retires the half-tile the NEXT phase reads.
// Wave rows run one barrier apart (waves 4-7 take an extra s_barrier up front), so on
// every SIMD one wave issues MFMAs while its partner issues ds_reads / DMA: the
// cdna guide's 8-phase template (§5 "256^2 8-phase template"), with 32x32x16 MFMAs.
// ---------------------------------------------------------------------------------------
// One 256x256 tile of gemm3: tile `wg` (raster order below) of K-slice `split` of `nsplit`.
// gemm3_kernel and the grouped dW kernel (gemm3_tt_grouped_kernel) differ only in how a
// workgroup finds (problem, wg, split).
template <int EPI, bool ACC, bool M16, bool TT>
__device__ __forceinline__ void gemm3_tile(char* smem, const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                           void* __restrict__ Cv, const bf16_t* __restrict__ bias,
                                           const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
                                           float* __restrict__ WS, int M, int N, int K, int64_t lda, int64_t ldb,
                                           int64_t ldc, int64_t ldr, int64_t ldx, float alpha, float p_drop,
                                           uint64_t seed, int tile_lim, int wg, int split, int nsplit) {
  constexpr int BM = 256, BN = 256, WM = 2, WN = 4;
  constexpr int HALF = 128 * 128;          // one half-tile image: 128 rows x 128 B
  constexpr int BUF = 4 * HALF;            // A0 A1 B0 B1

  const int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  constexpr int GROUP = MP_G3_GROUP;   // tile rows per raster group (L2 reuse of the A panels)
  const int group = wg / (GROUP * gn);
  const int first_m = group * GROUP;
  const int gsz = min(gm - first_m, GROUP);
  // tile_lim > 0 (gemm7's leading rounds): the first tile_lim tiles in row-major order
  const int tm = tile_lim > 0 ? wg / gn : first_m + (wg % (GROUP * gn)) % gsz;
  const int tn = tile_lim > 0 ? wg % gn : (wg % (GROUP * gn)) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int wm = wr * (BM / WM), wn = wc * (BN / WN);

  const int ktiles = K / BK;
  const int kt0 = split * ktiles / nsplit;
  const int nk = (split + 1) * ktiles / nsplit - kt0;

  // staging: this wave's two 1 KiB pieces (j = 0, 1) of every half-tile.  Piece rows
  // i = 64 j + 8 wave + (lane >> 3); swz8 reads row bits 1-3, i.e. i & 15 = 8 (wave & 1) + lr.
  static_assert(!TT || M16, "the TT build exists with 16x16x32 MFMAs only");
  const int lr = lane >> 3;
  const int lc = (lane & 7) ^ (M16 ? swzq(8 * (wave & 1) + lr) : swz8(8 * (wave & 1) + lr));
  const bf16_t* pa[2];
  const bf16_t* pb[2];
  // TT (both operands stored k-major: A^T [K][M], B [K][N], the dW GEMMs): a half-tile is a
  // [64 k][128 col] image with 256-byte rows; piece p = wave + 8 j holds k-rows 4p..4p+3,
  // lane l lands at k-row 4p + (l >> 4), physical chunk l & 15 = logical chunk ^ swz16(k-row)
  // (swz16 of that row = ((l >> 4) << 2) | (wave & 3)).  Image column c of A0 is tile row
  // c < 64 ? c : c + 64 (A1: + 64); of B0 tile column 64 (c / 32) + c % 32 (B1: + 32).
  const bf16_t* ta1[2];
  const bf16_t* tb1[2];
  if constexpr (TT) {
    const int kr = lane >> 4;
    const int ic = 8 * ((lane & 15) ^ ((kr << 2) | (wave & 3)));
    const int am = ic < 64 ? ic : ic + 64, bn = 64 * (ic >> 5) + (ic & 31);
    auto cm = [&](int m) { return m < M ? m : M - 8; };
    auto cn = [&](int n) { return n < N ? n : N - 8; };
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t krow = (int64_t)kt0 * BK + 4 * wave + 32 * j + kr;
      pa[j] = A + krow * lda + cm(m0 + am);
      ta1[j] = A + krow * lda + cm(m0 + am + 64);
      pb[j] = B + krow * ldb + cn(n0 + bn);
      tb1[j] = B + krow * ldb + cn(n0 + bn + 32);
    }
  }
#pragma unroll
  for (int j = 0; j < 2 && !TT; ++j) {
    int ra = m0 + 128 * j + 8 * wave + lr;          // A0 row; A1 = +64
    ra = ra < M ? ra : M - 1;
    int rb = n0 + 64 * ((wave >> 2) + 2 * j) + 8 * (wave & 3) + lr;   // B0 row (= output col); B1 = +32
    rb = rb < N ? rb : N - 1;
    pa[j] = A + (int64_t)ra * lda + (int64_t)kt0 * BK + lc * 8;
    pb[j] = B + (int64_t)rb * ldb + (int64_t)kt0 * BK + lc * 8;
  }
  // rows past the M/N edge of the A1/B1 halves: clamp by pointer (the +64/+32 offsets)
  const bool a1_ok0 = m0 + 64 + 8 * wave + lr < M, a1_ok1 = m0 + 192 + 8 * wave + lr < M;
  const bool b1_ok0 = n0 + 64 * (wave >> 2) + 32 + 8 * (wave & 3) + lr < N;
  const bool b1_ok1 = n0 + 64 * ((wave >> 2) + 2) + 32 + 8 * (wave & 3) + lr < N;
  const int64_t a1_off0 = a1_ok0 ? 64 * lda : 0, a1_off1 = a1_ok1 ? 64 * lda : 0;
  const int64_t b1_off0 = b1_ok0 ? 32 * ldb : 0, b1_off1 = b1_ok1 ? 32 * ldb : 0;

  // half-tile h (0 = A0, 1 = B0, 2 = B1, 3 = A1: consumption order) of K-tile kt -> buffer kt & 1
  auto issue = [&](int h, int kt) {
    char* img = smem + (kt & 1) * BUF + (h == 0 ? 0 : h == 3 ? HALF : h == 1 ? 2 * HALF : 3 * HALF);
    if constexpr (TT) {
      const int64_t da = (int64_t)kt * BK * lda, db = (int64_t)kt * BK * ldb;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16_t* src = h == 0 ? pa[j] + da : h == 3 ? ta1[j] + da : h == 1 ? pb[j] + db : tb1[j] + db;
        __builtin_amdgcn_global_load_lds((const void*)src,
                                         (__attribute__((address_space(3))) void*)(img + (wave + 8 * j) * 1024), 16,
                                         0, 0);
      }
      return;
    }
    const int64_t dk = (int64_t)kt * BK;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bf16_t* src;
      if (h == 0) src = pa[j] + dk;
      else if (h == 3) src = pa[j] + dk + (j ? a1_off1 : a1_off0);
      else if (h == 1) src = pb[j] + dk;
      else src = pb[j] + dk + (j ? b1_off1 : b1_off0);
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (__attribute__((address_space(3))) void*)(img + (wave + 8 * j) * 1024), 16, 0,
                                       0);
    }
  };

  if constexpr (!M16) {
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x16{};

  // Half-tile DMA runs ~1.5 K-tiles ahead, one half-tile (2 glds per thread) per phase so
  // the DMA issue cost is spread evenly; a slot is re-filled >= 2 phases after its last
  // ds_read (WAR across the staggered wave rows, cdna guide §5 "8-phase template"):
  //   tile t  phase 1: B1(t+1)   phase 2: A1(t+1)   phase 3: A0(t+2)   phase 4: B0(t+2)
  // Each phase's counted vmcnt(8) retires exactly the half-tile the next phase reads; the
  // last two K-tiles drain with vmcnt(0).
  issue(0, 0);
  issue(1, 0);
  issue(2, 0);
  issue(3, 0);
  if (nk > 1) {
    issue(0, 1);
    issue(1, 1);
    wait_vmcnt<8>();
  } else {
    wait_vmcnt<4>();
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // stagger the wave rows by one barrier
  asm volatile("" ::: "memory");

  bf16x8 af[2][4], b0[4], b1[4];
  const int rA = wr * 64 + l32;   // image row of this wave's quadrant row-block 0
  const int rB = wc * 32 + l32;

#define G3_MFMA(I0, BF, CI)                                                           \
  __builtin_amdgcn_sched_barrier(0);                                                  \
  __builtin_amdgcn_s_setprio(1);                                                      \
  _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) {                                  \
    acc[I0][CI] = mfma32(af[0][s_], BF[s_], acc[I0][CI]);                             \
    acc[I0 + 1][CI] = mfma32(af[1][s_], BF[s_], acc[I0 + 1][CI]);                     \
  }                                                                                   \
  __builtin_amdgcn_s_setprio(0);                                                      \
  __builtin_amdgcn_sched_barrier(0);
#define G3_BAR()                          \
  asm volatile("" ::: "memory");          \
  __builtin_amdgcn_s_barrier();           \
  asm volatile("" ::: "memory");

  for (int t = 0; t < nk; ++t) {
    const char* buf = smem + (t & 1) * BUF;
    const bool steady = t + 2 < nk;
    // ---- phase 1: A0 x B0
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) {
      af[0][s_] = frag<false, BM>(buf, rA, s_, hl);
      af[1][s_] = frag<false, BM>(buf, rA + 32, s_, hl);
      b0[s_] = frag<false, BN>(buf + 2 * HALF, rB, s_, hl);
    }
    if (t + 1 < nk) issue(2, t + 1);
    if (steady) wait_vmcnt<8>(); else wait_vmcnt<0>();   // B1(t) landed
    G3_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G3_MFMA(0, b0, 0);
    G3_BAR();
    // ---- phase 2: A0 x B1
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) b1[s_] = frag<false, BN>(buf + 3 * HALF, rB, s_, hl);
    if (t + 1 < nk) issue(3, t + 1);
    if (steady) wait_vmcnt<8>(); else wait_vmcnt<0>();   // A1(t) landed
    G3_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G3_MFMA(0, b1, 1);
    G3_BAR();
    // ---- phase 3: A1 x B0; refill A0 of this buffer for K-tile t+2
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) {
      af[0][s_] = frag<false, BM>(buf + HALF, rA, s_, hl);
      af[1][s_] = frag<false, BM>(buf + HALF, rA + 32, s_, hl);
    }
    if (steady) issue(0, t + 2);
    G3_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G3_MFMA(2, b0, 0);
    G3_BAR();
    // ---- phase 4: A1 x B1; refill B0; A0/B0 of K-tile t+1 retired for the next phase 1
    if (steady) {
      issue(1, t + 2);
      wait_vmcnt<8>();
    } else {
      wait_vmcnt<0>();
    }
    G3_BAR();
    G3_MFMA(2, b1, 1);
    G3_BAR();
  }
#undef G3_MFMA
#undef G3_BAR
  if (wr == 0) __builtin_amdgcn_s_barrier();  // re-align the staggered wave rows
  __syncthreads();
  epilogue<BM, BN, WM, WN, EPI, ACC>(Stage32<4, 2>{acc, wn, hl, l32}, smem, m0, n0, wr, Cv, bias, R, AUX, WS, M,
                                     N, ldc, ldr, ldx, alpha, nsplit, p_drop, seed, nullptr, 0, 0, split);
  } else {
  // 16x16x32 MFMAs: same phases, DMA and barriers; a phase quadrant (64 rows x 32 cols)
  // is 4 x 2 blocks of 16x16, K = 64 in two 32-deep steps (16 MFMAs of 16 cycles)
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{};

  // Half-tile DMA runs ~1.5 K-tiles ahead, one half-tile (2 glds per thread) per phase so
  // the DMA issue cost is spread evenly; a slot is re-filled >= 2 phases after its last
  // ds_read (WAR across the staggered wave rows, cdna guide §5 "8-phase template"):
  //   tile t  phase 1: B1(t+1)   phase 2: A1(t+1)   phase 3: A0(t+2)   phase 4: B0(t+2)
  // Each phase's counted vmcnt(8) retires exactly the half-tile the next phase reads; the
  // last two K-tiles drain with vmcnt(0).
  issue(0, 0);
  issue(1, 0);
  issue(2, 0);
  issue(3, 0);
  if (nk > 1) {
    issue(0, 1);
    issue(1, 1);
    wait_vmcnt<8>();
  } else {
    wait_vmcnt<4>();
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // stagger the wave rows by one barrier
  asm volatile("" ::: "memory");

  bf16x8 af[4][2], b0[2][2], b1[2][2];
  const int q = lane >> 4;
  const int rA = wr * 64 + (lane & 15);
  const int rB = wc * 32 + (lane & 15);
  auto fq = [&](const char* img, int row, int st) -> bf16x8 {
    if constexpr (TT) return frag16<true, 128>(img, row - (lane & 15), st);   // row = base + (lane & 15)
    else return *reinterpret_cast<const bf16x8*>(img + row * 128 + 16 * ((4 * st + q) ^ swzq(row)));
  };

#define G4_MFMA(R0, BF, C0)                                                              \
  __builtin_amdgcn_sched_barrier(0);                                                     \
  __builtin_amdgcn_s_setprio(1);                                                         \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_)                                       \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                       \
  _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                       \
    acc[R0 + i_][C0 + j_] = mfma16(af[i_][s_], BF[j_][s_], acc[R0 + i_][C0 + j_]);       \
  __builtin_amdgcn_s_setprio(0);                                                         \
  __builtin_amdgcn_sched_barrier(0);
#define G3_BAR()                          \
  asm volatile("" ::: "memory");          \
  __builtin_amdgcn_s_barrier();           \
  asm volatile("" ::: "memory");

  for (int t = 0; t < nk; ++t) {
    const char* buf = smem + (t & 1) * BUF;
    const bool steady = t + 2 < nk;
    // ---- phase 1: A0 x B0
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i][s_] = fq(buf, rA + 16 * i, s_);
#pragma unroll
      for (int j = 0; j < 2; ++j) b0[j][s_] = fq(buf + 2 * HALF, rB + 16 * j, s_);
    }
    if (t + 1 < nk) issue(2, t + 1);
    if (steady) wait_vmcnt<8>(); else wait_vmcnt<0>();   // B1(t) landed
    G3_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G4_MFMA(0, b0, 0);
    G3_BAR();
    // ---- phase 2: A0 x B1
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int j = 0; j < 2; ++j) b1[j][s_] = fq(buf + 3 * HALF, rB + 16 * j, s_);
    if (t + 1 < nk) issue(3, t + 1);
    if (steady) wait_vmcnt<8>(); else wait_vmcnt<0>();   // A1(t) landed
    G3_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G4_MFMA(0, b1, 2);
    G3_BAR();
    // ---- phase 3: A1 x B0; refill A0 of this buffer for K-tile t+2
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i][s_] = fq(buf + HALF, rA + 16 * i, s_);
    if (steady) issue(0, t + 2);
    G3_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G4_MFMA(4, b0, 0);
    G3_BAR();
    // ---- phase 4: A1 x B1; refill B0
    if (steady) {
      issue(1, t + 2);
      wait_vmcnt<8>();
    } else {
      wait_vmcnt<0>();
    }
    G3_BAR();
    G4_MFMA(4, b1, 2);
    G3_BAR();
  }
#undef G4_MFMA
#undef G3_BAR
  if (wr == 0) __builtin_amdgcn_s_barrier();  // re-align the staggered wave rows
  __syncthreads();
  epilogue<BM, BN, WM, WN, EPI, ACC>(Stage16<8, 4>{acc, wn, lane}, smem, m0, n0, wr, Cv, bias, R, AUX, WS, M, N, ldc,
                                     ldr, ldx, alpha, nsplit, p_drop, seed, nullptr, 0, 0, split);
  }
}

template <int EPI, bool ACC, bool M16, bool TT = false>
__global__ void __launch_bounds__(NT, 1) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm3_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, void* __restrict__ Cv,
             const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
             float* __restrict__ WS, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr,
             int64_t ldx, float alpha, float p_drop, uint64_t seed, int tile_lim) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nwg = tile_lim > 0 ? tile_lim : ((M + 255) / 256) * ((N + 255) / 256);
  // split-K grids: workgroups are dealt to the 8 XCDs round-robin in LINEAR id order
  // (x + gridDim.x * y), so remap that id, then cut it into (split, tile): an XCD's L2 holds
  // the panels of ONE split's neighbouring tiles.  Remapping blockIdx.x alone assumed XCD =
  // x % 8, which is wrong for y > 0 whenever gridDim.x % 8 != 0 and scattered the tiles that
  // share a panel over all XCDs (the dW GEMMs read ~4x their unique bytes from HBM)
  int wg, split;
  if (gridDim.y > 1 && tile_lim == 0) {   // (tile_lim = -1: the x-only remap, the default)
    const int v = xcd_remap((int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y, nwg * (int)gridDim.y);
    split = v / nwg;
    wg = v % nwg;
  } else {
    wg = xcd_remap((int)blockIdx.x, nwg);
    split = (int)blockIdx.y;
  }
  gemm3_tile<EPI, ACC, M16, TT>(smem, A, B, Cv, bias, R, AUX, WS, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed,
                                tile_lim, wg, split, (int)gridDim.y);
}

// ---------------------------------------------------------------------------------------
// Grouped long-token weight-gradient GEMMs: up to MP_GROUP_MAX TT problems
// C_g[M_g, N_g] (f32) += alpha * A_g^T B_g over ONE common K (a microbatch's tokens), 256x256
// tiles of gemm3's TT build, one split factor S for the group: grid = S * (sum of tiles).
// One at a time, a layer's four dW GEMMs are 9-36 tiles each and need split 7-28 to cover
// 256 CUs (choose()): ~1000 f32 partial tiles per layer through HBM and back plus four reduce
// launches.  Together their 108 tiles fill the chip at S = 2.
//
// Mapping: the XCD-remapped id v walks problem -> split -> tile (gemm3's raster), so the
// workgroups that run together on an XCD (consecutive v) are neighbouring tiles of one
// problem and one split and share its A / B panels in that XCD's L2.
// S > 1: partial tiles go to slabs ws[elem_start[g] * S + s * M_g * N_g] (row stride N_g) and
// splitk_reduce_grouped_kernel adds them into C_g in split order; S = 1: read-modify-write of
// C_g in the epilogue, no workspace.
// ---------------------------------------------------------------------------------------
struct GroupTT3 {
  const bf16_t* A[MP_GROUP_MAX];
  const bf16_t* B[MP_GROUP_MAX];
  float* C[MP_GROUP_MAX];
  int64_t lda[MP_GROUP_MAX], ldb[MP_GROUP_MAX], ldc[MP_GROUP_MAX];
  int64_t elem_start[MP_GROUP_MAX + 1];   // prefix sums of M_g * N_g
  int M[MP_GROUP_MAX], N[MP_GROUP_MAX];
  int tile_start[MP_GROUP_MAX + 1];       // prefix sums of the 256x256 tile counts
  int n, K, S;
  float alpha;
  float* ws;
};

__global__ void __launch_bounds__(NT, 1) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm3_tt_grouped_kernel(const GroupTT3 g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int total = g.tile_start[g.n];
  const int v = xcd_remap((int)blockIdx.x, total * g.S);
  int p = 0;
#pragma unroll
  for (int i = 1; i < MP_GROUP_MAX; ++i)
    if (i < g.n && v >= g.tile_start[i] * g.S) p = i;
  const int tiles = g.tile_start[p + 1] - g.tile_start[p];
  const int local = v - g.tile_start[p] * g.S;
  const int split = local / tiles, wg = local % tiles;
  float* ws = g.S > 1 ? g.ws + g.elem_start[p] * g.S : nullptr;
  gemm3_tile<EPI_NONE, true, true, true>(smem, g.A[p], g.B[p], g.C[p], nullptr, nullptr, nullptr, ws, g.M[p], g.N[p],
                                         g.K, g.lda[p], g.ldb[p], g.ldc[p], 0, 0, g.alpha, 0.f, 0, 0, wg, split, g.S);
}

// C_g[M_g, N_g] (row stride ldc_g) += the group's split-K slabs, summed in split order
__global__ void __launch_bounds__(256) splitk_reduce_grouped_kernel(const GroupTT3 g) {
  const int64_t n4 = g.elem_start[g.n] / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i * 4;
    int p = 0;
#pragma unroll
    for (int j = 1; j < MP_GROUP_MAX; ++j)
      if (j < g.n && e >= g.elem_start[j]) p = j;
    const int64_t le = e - g.elem_start[p], slab = (int64_t)g.M[p] * g.N[p];
    const float* w = g.ws + g.elem_start[p] * g.S + le;
    const int m = (int)(le / g.N[p]), n = (int)(le % g.N[p]);
    float4 acc = *reinterpret_cast<const float4*>(w);
    for (int s = 1; s < g.S; ++s) {
      const float4 t = *reinterpret_cast<const float4*>(w + s * slab);
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
    float4* cp = reinterpret_cast<float4*>(g.C[p] + (int64_t)m * g.ldc[p] + n);
    float4 c = *cp;
    c.x += acc.x; c.y += acc.y; c.z += acc.z; c.w += acc.w;
    *cp = c;
  }
}

template <int EPI, bool ACC, bool M16, bool TT = false>
static int launch3(const void* A, const void* B, void* C, const void* bias, const void* R, void* X, float* ws, int M,
                   int N, int K,
                   int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx, float alpha, int split,
                   float p_drop, uint64_t seed, hipStream_t st, int tile_lim = 0) {
  constexpr int LDS_MAIN = 2 * 4 * 128 * 128;
  constexpr int EPI_BYTES = 128 * (256 + 4) * 4;
  constexpr int LDS = LDS_MAIN > EPI_BYTES ? LDS_MAIN : EPI_BYTES;
  auto kern = gemm3_kernel<EPI, ACC, M16, TT>;
  static bool attr = false;
  lds_attr_once(attr, (const void*)kern, LDS);
  const int nwg = tile_lim > 0 ? tile_lim : ((M + 255) / 256) * ((N + 255) / 256);
  // opt-in (MIPIPE_G3_SPLIT_REMAP=1): +3-10 % on GPT-2 small's dW GEMMs standalone, neutral
  // in that step, but -0.8 % on the GPT-2 large step (2 same-box pairs,
  // profiles/r5_gemm3_splitk_xcd_remap.md)
  static const bool split_remap = [] {
    const char* e = getenv("MIPIPE_G3_SPLIT_REMAP");
    return e && e[0] == '1';
  }();
  if (tile_lim == 0 && !split_remap) tile_lim = -1;
  kern<<<dim3(nwg, split), NT, LDS, st>>>((const bf16_t*)A, (const bf16_t*)B, C, (const bf16_t*)bias,
                                          (const bf16_t*)R, (bf16_t*)X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed,
                                          tile_lim);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// gemm6: gemm3's ping-pong phase schedule (16x16x32 MFMAs, NT) on 256x192 tiles.
//
// Why: at the 32K-token microbatch of a PP > 1 rank the N = 768 GEMMs (fwd wo / fc2, dX of
// qkv / wo / fc1) are 128 x 3 = 384 tiles of 256x256 = 1.5 rounds of 256 CUs: the second
// round runs on half the chip (profiles/r3_gemm_tail_probe.txt: 0.83-0.92x hipBLASLt there,
// 1.0x+ at M = 65536 where the grid is 3 whole rounds).  256x192 tiles make N = 768 four
// tile columns (512 tiles = 2 whole rounds) and N = 2304 twelve (6 rounds instead of 4.5).
// gemm2's 256x192 build (cfg 1) has the tile but not the schedule (2 stages, 4x slower
// feed: 0.95x of gemm3 in the same probe).
//
// Layout: 8 waves as 4 (rows) x 2 (cols), 64 x 96 outputs each.  A K-tile (BK = 64) is four
// LDS images, streamed one per phase exactly as in gemm3:
//   A0 = rows {0..31, 64..95, 128..159, 192..223} (the first 32 rows of each wave row)
//   A1 = the other 128 rows                                      (16 KiB each)
//   B0 = cols {0..47, 96..143}   B1 = cols {48..95, 144..191}    (96 rows, 12 KiB each)
// phase 1: A0 x B0, 2: A0 x B1, 3: A1 x B0, 4: A1 x B1 -- 2 x 3 blocks of 16x16, K = 64
// in two 32-deep steps = 12 MFMAs per phase.  An A image is 16 one-KiB pieces (2 per
// wave); a B image 12 (waves 0-3 issue 2, waves 4-7 one), so each wave's counted vmcnt
// is 4 + 2 b (b = its B pieces per image): the wait retires exactly the image the next
// phase reads, per issuing wave, and the barrier after it publishes it to all waves.
// Waves 4-7 (one per SIMD, the partner of wave w - 4) run one barrier behind waves 0-3.
// ---------------------------------------------------------------------------------------
template <int EPI, bool ACC>
__global__ void __launch_bounds__(NT, 1) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm6_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, void* __restrict__ Cv,
             const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
             float* __restrict__ WS, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr,
             int64_t ldx, float alpha, float p_drop, uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  constexpr int BM = 256, BN = 192, WM = 4, WN = 2;
  constexpr int HA = 32, HB = 48;                 // a wave's rows / cols in one A / B image
  constexpr int IMG_A = 128 * 128, IMG_B = 96 * 128;
  constexpr int O_A1 = IMG_A, O_B0 = 2 * IMG_A, O_B1 = 2 * IMG_A + IMG_B;
  constexpr int BUF = 2 * IMG_A + 2 * IMG_B;      // 56 KiB per K-tile, two buffers
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  const int nwg = gm * gn;
  const int wg = xcd_remap((int)blockIdx.x, nwg);
  constexpr int GROUP = MP_G3_GROUP;
  const int group = wg / (GROUP * gn);
  const int first_m = group * GROUP;
  const int gsz = min(gm - first_m, GROUP);
  const int tm = first_m + (wg % (GROUP * gn)) % gsz;
  const int tn = (wg % (GROUP * gn)) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int grp = wave >> 2;                      // ping-pong group (waves w, w + 4 share a SIMD)
  const int wn = wc * (BN / WN);

  const int nk = K / BK;

  // staging: piece p = wave + 8 j holds image rows 8 p .. 8 p + 7 (lane row lr = lane >> 3,
  // 16-byte chunk lane & 7); image row r & 15 = 8 (wave & 1) + lr for every piece
  const int lr = lane >> 3;
  const int lc = (lane & 7) ^ swzq(8 * (wave & 1) + lr);
  const bool two_b = wave < 4;                    // B images: 12 pieces, waves 0-3 take the last 4
  const bf16_t* pa0[2];
  const bf16_t* pa1[2];
  const bf16_t* pb0[2];
  const bf16_t* pb1[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = 8 * (wave + 8 * j) + lr;        // image row
    int a0 = m0 + (r / HA) * (BM / WM) + r % HA, a1 = a0 + HA;
    a0 = a0 < M ? a0 : M - 1;                     // rows past the edge only feed masked outputs
    a1 = a1 < M ? a1 : M - 1;
    pa0[j] = A + (int64_t)a0 * lda + lc * 8;
    pa1[j] = A + (int64_t)a1 * lda + lc * 8;
    const int rb = r < 96 ? r : r - 64;           // waves 4-7, j = 1: no piece (never issued)
    int b0 = n0 + (rb / HB) * (BN / WN) + rb % HB, b1 = b0 + HB;
    b0 = b0 < N ? b0 : N - 1;
    b1 = b1 < N ? b1 : N - 1;
    pb0[j] = B + (int64_t)b0 * ldb + lc * 8;
    pb1[j] = B + (int64_t)b1 * ldb + lc * 8;
  }

  // image h (0 = A0, 1 = B0, 2 = B1, 3 = A1: consumption order) of K-tile kt -> buffer kt & 1
  auto issue = [&](int h, int kt) {
    char* img = smem + (kt & 1) * BUF + (h == 0 ? 0 : h == 3 ? O_A1 : h == 1 ? O_B0 : O_B1);
    const int64_t dk = (int64_t)kt * BK;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j == 1 && (h == 1 || h == 2) && !two_b) continue;
      const bf16_t* src = (h == 0 ? pa0[j] : h == 3 ? pa1[j] : h == 1 ? pb0[j] : pb1[j]) + dk;
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (__attribute__((address_space(3))) void*)(img + (wave + 8 * j) * 1024), 16, 0,
                                       0);
    }
  };
  // counted waits (derivation in the header): 4 + 2 b outstanding pieces, 2 + b for nk = 1
  auto wait_steady = [&]() {
    if (two_b) wait_vmcnt<8>(); else wait_vmcnt<6>();
  };

  f32x4 acc[4][6];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[i][j] = f32x4{};

  issue(0, 0);
  issue(1, 0);
  issue(2, 0);
  issue(3, 0);
  if (nk > 1) {
    issue(0, 1);
    issue(1, 1);
    wait_steady();
  } else {
    if (two_b) wait_vmcnt<4>(); else wait_vmcnt<3>();
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (grp == 1) __builtin_amdgcn_s_barrier();  // stagger the two wave groups by one barrier
  asm volatile("" ::: "memory");

  bf16x8 af[2][2], b0[3][2], b1[3][2];
  const int q = lane >> 4;
  const int rA = wr * HA + (lane & 15);
  const int rB = wc * HB + (lane & 15);
  auto fq = [&](const char* img, int row, int st) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(img + row * 128 + 16 * ((4 * st + q) ^ swzq(row)));
  };

#define G6_MFMA(R0, BF, C0)                                                              \
  __builtin_amdgcn_sched_barrier(0);                                                     \
  __builtin_amdgcn_s_setprio(1);                                                         \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_)                                       \
  _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_)                                       \
  _Pragma("unroll") for (int j_ = 0; j_ < 3; ++j_)                                       \
    acc[R0 + i_][C0 + j_] = mfma16(af[i_][s_], BF[j_][s_], acc[R0 + i_][C0 + j_]);       \
  __builtin_amdgcn_s_setprio(0);                                                         \
  __builtin_amdgcn_sched_barrier(0);
#define G6_BAR()                          \
  asm volatile("" ::: "memory");          \
  __builtin_amdgcn_s_barrier();           \
  asm volatile("" ::: "memory");

  for (int t = 0; t < nk; ++t) {
    const char* buf = smem + (t & 1) * BUF;
    const bool steady = t + 2 < nk;
    // ---- phase 1: A0 x B0
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i][s_] = fq(buf, rA + 16 * i, s_);
#pragma unroll
      for (int j = 0; j < 3; ++j) b0[j][s_] = fq(buf + O_B0, rB + 16 * j, s_);
    }
    if (t + 1 < nk) issue(2, t + 1);
    if (steady) wait_steady(); else wait_vmcnt<0>();   // B1(t) landed
    G6_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G6_MFMA(0, b0, 0);
    G6_BAR();
    // ---- phase 2: A0 x B1
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int j = 0; j < 3; ++j) b1[j][s_] = fq(buf + O_B1, rB + 16 * j, s_);
    if (t + 1 < nk) issue(3, t + 1);
    if (steady) wait_steady(); else wait_vmcnt<0>();   // A1(t) landed
    G6_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G6_MFMA(0, b1, 3);
    G6_BAR();
    // ---- phase 3: A1 x B0; refill A0 of this buffer for K-tile t+2
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i][s_] = fq(buf + O_A1, rA + 16 * i, s_);
    if (steady) issue(0, t + 2);
    G6_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G6_MFMA(2, b0, 0);
    G6_BAR();
    // ---- phase 4: A1 x B1; refill B0; A0/B0 of K-tile t+1 retired for the next phase 1
    if (steady) {
      issue(1, t + 2);
      wait_steady();
    } else {
      wait_vmcnt<0>();
    }
    G6_BAR();
    G6_MFMA(2, b1, 3);
    G6_BAR();
  }
#undef G6_MFMA
#undef G6_BAR
  if (grp == 0) __builtin_amdgcn_s_barrier();  // re-align the staggered groups
  __syncthreads();
  epilogue<BM, BN, WM, WN, EPI, ACC>(Stage16<4, 6>{acc, wn, lane}, smem, m0, n0, wr, Cv, bias, R, AUX, WS, M, N, ldc,
                                     ldr, ldx, alpha, 1, p_drop, seed);
}

template <int EPI, bool ACC>
static int launch6(const void* A, const void* B, void* C, const void* bias, const void* R, void* X, float* ws, int M,
                   int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx, float alpha,
                   float p_drop, uint64_t seed, hipStream_t st) {
  constexpr int LDS_MAIN = 2 * (2 * 128 * 128 + 2 * 96 * 128);
  constexpr int EPI_BYTES = 64 * (192 + 4) * 4;
  constexpr int LDS = LDS_MAIN > EPI_BYTES ? LDS_MAIN : EPI_BYTES;
  auto kern = gemm6_kernel<EPI, ACC>;
  static bool attr = false;
  lds_attr_once(attr, (const void*)kern, LDS);
  const int nwg = ((M + 255) / 256) * ((N + 191) / 192);
  kern<<<dim3(nwg, 1), NT, LDS, st>>>((const bf16_t*)A, (const bf16_t*)B, C, (const bf16_t*)bias, (const bf16_t*)R,
                                      (bf16_t*)X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed);
  return (int)hipGetLastError();
}

}  // namespace g2
