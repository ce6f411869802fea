// What every bf16 GEMM engine of gemm2.hip shares: the epilogue kinds, the K-tile and block
// size, the LDS swizzles, MFMA wrappers and fragment reads, the direct-to-LDS source
// address, the XCD remap, counted waits and the LDS-staged fused epilogue.
#pragma once

#include "mp_common.h"

using namespace mp;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// tile rows per raster group of the ping-pong engine: GPT-2 bench (3 interleaved runs
// each, one box) 841K tok/s at 8, 851K at 4, 856K at 2, 863-864K vs 870K at 1 vs 2 on a
// second box, 829K at 16 -- the isolated GEMM is flat (+-1 %); inside the step (dW GEMMs on
// the side stream sharing L2) short groups win
#ifndef MP_G3_GROUP
#define MP_G3_GROUP 2
#endif
#ifndef MP_G2_GROUP
#define MP_G2_GROUP 8
#endif

// gemm4: accumulator row blocks (of 8) whose store is deferred into the next tile
#ifndef MP_G4_SR
#define MP_G4_SR 2
#endif

#ifndef MP_GROUP_MAX
#define MP_GROUP_MAX 8
#endif

namespace g2 {

enum Epi { EPI_NONE = 0, EPI_BIAS = 1, EPI_BIAS_GELU = 2, EPI_BIAS_RELU = 3, EPI_BIAS_RES = 4, EPI_RES = 5,
           EPI_DGELU = 6, EPI_DRELU = 7 };

constexpr int BK = 64;
constexpr int NT = 512;

__device__ __forceinline__ int swz8(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int swz16(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
// K-contiguous image swizzle for the 16x16x32 fragment read (lane = 16 q + i reads row
// r0 + i, chunk c + q): chunk ^ g(row bits 1-3) with g mapping row pairs {0,1,6,7} ->
// {6,7,4,5} and {2..5} -> {0..3} makes all four ds_read_b128 lane groups hit 16
// distinct 16-byte bank slots (MI355X_MICROARCH.md LDS table); swz8 would be 2-way here
__device__ __forceinline__ int swzq(int row) { return (((row >> 1) & 7) + 6) & 7; }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// K-contiguous image [rows][64 k]: 128-byte rows, 8 chunks
__device__ __forceinline__ int offK(int row, int chunk) { return row * 128 + 16 * (chunk ^ swz8(row)); }
// outer-contiguous image [64 k][COLS]: 2*COLS-byte rows; swizzle the low 4 chunk bits
// (COLS = 64, the small engine's TT tiles: 8 chunks per row, chunk pairs XORed by row bits
// 1 and 3 -- the 8 rows a 32-lane ds_read_b64_tr_b16 group touches land in 8 distinct
// 8-bank groups, conflict-free)
__device__ __forceinline__ int swz8o(int row) { return 2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1)); }
template <int COLS>
__device__ __forceinline__ int offO(int row, int chunk) {
  if constexpr (COLS == 64) return row * 128 + 16 * (chunk ^ swz8o(row));
  return row * (COLS * 2) + 16 * ((chunk & ~15) | ((chunk & 15) ^ swz16(row)));
}

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <bool OUTER, int COLS>
__device__ __forceinline__ bf16x8 frag(const char* img, int rc, int s, int hl) {
  if constexpr (!OUTER) {
    return *reinterpret_cast<const bf16x8*>(img + offK(rc, 2 * s + hl));
  } else {
    const int i = threadIdx.x & 15, q = i >> 2, p = i & 3;
    const int col = (rc & ~15) + 4 * p;
    const int r0 = 16 * s + 8 * hl;
    const char* a0 = img + offO<COLS>(r0 + q, col >> 3) + ((col & 7) << 1);
    const char* a1 = img + offO<COLS>(r0 + 4 + q, col >> 3) + ((col & 7) << 1);
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a1));
    s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
  }
}

// 16x16x32 fragment: lane l holds rows/cols base + (l & 15), k = 32 s + 8 (l >> 4) + 0..7
// (K-contiguous images use the swzq swizzle; outer-contiguous ones two tr reads, 8 k-rows
// per 16-lane group, conflict-free under offO's swz16)
template <bool OUTER, int COLS>
__device__ __forceinline__ bf16x8 frag16(const char* img, int base, int s) {
  const int lane = threadIdx.x & 63;
  if constexpr (!OUTER) {
    const int row = base + (lane & 15), chunk = 4 * s + (lane >> 4);
    return *reinterpret_cast<const bf16x8*>(img + row * 128 + 16 * (chunk ^ swzq(row)));
  } else {
    const int i = lane & 15, q = i >> 2, p = i & 3;
    const int col = base + 4 * p;
    const int r0 = 32 * s + 8 * (lane >> 4);
    const char* a0 = img + offO<COLS>(r0 + q, col >> 3) + ((col & 7) << 1);
    const char* a1 = img + offO<COLS>(r0 + 4 + q, col >> 3) + ((col & 7) << 1);
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a1));
    s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
  }
}

// global source (bf16 element pointer) of the 16 bytes that land at byte `pos` of an image
template <bool OUTER, int ROWS, bool M16 = false>
__device__ __forceinline__ const bf16_t* src_of(const bf16_t* base, int64_t ld, int pos, int outer0, int outer_lim,
                                                int k0) {
  if constexpr (!OUTER) {  // [ROWS][64k]
    const int row = pos >> 7, phys = (pos >> 4) & 7;
    const int chunk = phys ^ (M16 ? swzq(row) : swz8(row));
    int o = outer0 + row;
    o = o < outer_lim ? o : outer_lim - 1;  // clamp: rows past the edge only feed masked outputs
    return base + (int64_t)o * ld + k0 + chunk * 8;
  } else {  // [64k][ROWS cols]
    constexpr int PITCH = ROWS * 2;
    const int row = pos / PITCH, phys = (pos % PITCH) >> 4;
    const int chunk = ROWS == 64 ? (phys ^ swz8o(row)) : ((phys & ~15) | ((phys & 15) ^ swz16(row)));
    int o = outer0 + chunk * 8;
    o = o < outer_lim ? o : outer_lim - 8;
    return base + (int64_t)(k0 + row) * ld + o;
  }
}

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  // s_waitcnt simm16 for gfx9: vmcnt[3:0] | expcnt[6:4]=7 | lgkmcnt[11:8]=15 | vmcnt_hi[15:14]
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | (((N >> 4) & 3) << 14));
}

// ---- epilogue: one wave-row group at a time through LDS -> coalesced 16-byte bias /
// residual / activation / store, or lane-consecutive f32 atomics for split-K
// -DMP_EPI_ROLLED (tools/build_ext.py --variant rolled -DMP_EPI_ROLLED) builds the epilogue
// as it was before the in-flight store loop, for A/B on one box: a rolled chunk loop that
// loads at the point of use, and the p_drop test once per element
#ifdef MP_EPI_ROLLED
constexpr bool EPI_ROLLED = true, EPI_DROP_PER_ELEM = true;
#else
constexpr bool EPI_ROLLED = false, EPI_DROP_PER_ELEM = false;
#endif

constexpr bool epi_has_bias(int epi) {
  return epi == EPI_BIAS || epi == EPI_BIAS_GELU || epi == EPI_BIAS_RELU || epi == EPI_BIAS_RES;
}
// epilogues that read a second [M, N] stream: the residual R, or the saved activation input AUX
constexpr bool epi_has_row(int epi) {
  return epi == EPI_BIAS_RES || epi == EPI_RES || epi == EPI_DGELU || epi == EPI_DRELU;
}

// the fused epilogue of 8 consecutive outputs (row gr, columns gc..gc+7) -> bf16 C
// bv: the bias chunk bias[gc..gc+7]; xv: the row-input chunk (R or AUX at row gr, columns
// gc..gc+7) -- loaded by the caller (each read only by the epilogues that have one), so the
// store loop can keep them in flight ahead of the chunk that consumes them
template <int EPI>
__device__ __forceinline__ void epi_apply8(float (&v)[8], int gr, int gc, bf16_t* __restrict__ C, int64_t ldc,
                                           const u16x8& bv, const u16x8& xv, bf16_t* __restrict__ AUX, int64_t ldx,
                                           float p_drop, uint64_t seed) {
  if constexpr (epi_has_bias(EPI)) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += bf2f(bv[e]);
  }
  if constexpr (EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_RELU) {
    // AUX: what the backward's dX epilogue needs -- the pre-activation for ReLU (its sign),
    // GELU's derivative for GELU (computed here beside the activation from one sigmoid, so
    // the backward multiplies instead of re-evaluating it: dGELU dX 505 -> ~440 us at 64K x
    // 3072, profiles/r5_gemm_epilogue_cost.md)
    u16x8 sv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = bf2f(f2bf(v[e]));   // the activation of the bf16-rounded pre-activation
      if constexpr (EPI == EPI_BIAS_GELU) {
        float d;
        gelu_tanh_and_grad(x, v[e], d);
        sv[e] = f2bf(d);
      } else {
        sv[e] = f2bf(x);
        v[e] = fmaxf(x, 0.f);
      }
      // dropout after the activation (the reference FFN's drop(relu(.))), mask index =
      // element index of the contiguous output, as act_fwd / act_bwd regenerate it
      if (EPI_DROP_PER_ELEM && p_drop > 0.f) v[e] *= dropout_scale(seed, (uint64_t)gr * ldc + gc + e, p_drop);
    }
    // p_drop is wave-uniform: one branch per chunk (it compiled to one per element inside the loop)
    if (!EPI_DROP_PER_ELEM && p_drop > 0.f) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= dropout_scale(seed, (uint64_t)gr * ldc + gc + e, p_drop);
    }
    *reinterpret_cast<u16x8*>(AUX + (int64_t)gr * ldx + gc) = sv;
  }
  if constexpr (EPI == EPI_BIAS_RES || EPI == EPI_RES) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += bf2f(xv[e]);
  }
  if constexpr (EPI == EPI_DGELU || EPI == EPI_DRELU) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = bf2f(xv[e]);   // GELU: the saved derivative; ReLU: the pre-activation
      v[e] *= EPI == EPI_DGELU ? x : (x > 0.f ? 1.f : 0.f);
      if (EPI_DROP_PER_ELEM && p_drop > 0.f) v[e] *= dropout_scale(seed, (uint64_t)gr * ldc + gc + e, p_drop);
    }
    if (!EPI_DROP_PER_ELEM && p_drop > 0.f) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= dropout_scale(seed, (uint64_t)gr * ldc + gc + e, p_drop);
    }
  }
  u16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
#ifndef MP_GEMM_PLAIN_STORE
  // non-temporal: the bf16 C tiles stream out without displacing the A/B panels other
  // workgroups still read from L2 (GPT-2 bench +0.9 %, 3 interleaved pairs on one box;
  // MP_GEMM_PLAIN_STORE builds the plain store for A/B)
  __builtin_nontemporal_store(o, reinterpret_cast<u16x8*>(C + (int64_t)gr * ldc + gc));
#else
  *reinterpret_cast<u16x8*>(C + (int64_t)gr * ldc + gc) = o;
#endif
}

// the same with the bias / row-input chunks loaded here, at the point of use (the rolled
// store loop and the split-K reduce pass)
template <int EPI>
__device__ __forceinline__ void epi_store8(float (&v)[8], int gr, int gc, bf16_t* __restrict__ C, int64_t ldc,
                                           const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R,
                                           int64_t ldr, bf16_t* __restrict__ AUX, int64_t ldx, float p_drop,
                                           uint64_t seed) {
  u16x8 bv = {}, xv = {};
  if constexpr (epi_has_bias(EPI)) bv = *reinterpret_cast<const u16x8*>(bias + gc);
  if constexpr (EPI == EPI_BIAS_RES || EPI == EPI_RES) xv = *reinterpret_cast<const u16x8*>(R + (int64_t)gr * ldr + gc);
  if constexpr (EPI == EPI_DGELU || EPI == EPI_DRELU) xv = *reinterpret_cast<const u16x8*>(AUX + (int64_t)gr * ldx + gc);
  epi_apply8<EPI>(v, gr, gc, C, ldc, bv, xv, AUX, ldx, p_drop, seed);
}

// accumulator layout of the 32x32x16 engines: acc[i][j] element r -> wave-local
// row 32 i + (r & 3) + 8 (r >> 2) + 4 hl, column wn + 32 j + l32
template <int WTM, int WTN>
struct Stage32 {
  static constexpr bool M16 = false;
  f32x16 (&acc)[WTM][WTN];
  int wn, hl, l32;
  __device__ __forceinline__ void operator()(float* ct, int CP) const {
#pragma unroll
    for (int i = 0; i < WTM; ++i)
#pragma unroll
      for (int j = 0; j < WTN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hl;
          const int col = wn + 32 * j + l32;
          ct[row * CP + col] = acc[i][j][r];
        }
  }
};

// accumulator layout of the 16x16x32 engines: acc[i][j] element r -> wave-local
// row 16 i + 4 (lane >> 4) + r, column wn + 16 j + (lane & 15)
template <int TM, int TN>
struct Stage16 {
  static constexpr bool M16 = true;
  f32x4 (&acc)[TM][TN];
  int wn, lane;
  __device__ __forceinline__ void operator()(float* ct, int CP) const {
    const int rq = 4 * (lane >> 4), c = wn + (lane & 15);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) ct[(16 * i + rq + r) * CP + c + 16 * j] = acc[i][j][r];
  }
};

template <int BM, int BN, int WM, int WN, int EPI, bool ACC, int NTH = NT, bool PARTS = false, class StageF>
__device__ __forceinline__ void epilogue(const StageF& stage, char* smem, int m0, int n0, int wr,
                                         void* __restrict__ Cv,
                                         const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R,
                                         bf16_t* __restrict__ AUX, float* __restrict__ WS, int M, int N, int64_t ldc,
                                         int64_t ldr, int64_t ldx, float alpha, int nsplit, float p_drop,
                                         uint64_t seed, const float* __restrict__ parts = nullptr,
                                         int64_t pstep = 0, int nparts = 0, int split_idx = -1) {
  // parts (gemm7's tile owner): nparts row-major [BM][BN] f32 partial tiles at parts + p *
  // pstep, added to the accumulator before the epilogue (published with sc1 stores; the
  // caller's agent-scope acquire precedes)
  constexpr int RG = BM / WM;      // rows per group
  constexpr int CP = BN + 4;       // f32 pitch
  // 8-column chunks per tile row; the store loop runs on the first NTE threads, a multiple
  // of CH (all NTH threads for power-of-two widths; 504 of 512 for BN = 192)
  constexpr int CH = BN / 8, NTE = (NTH / CH) * CH;
  float* ct = reinterpret_cast<float*>(smem);
  // bf16 outputs with WS != nullptr: also accumulate the column sums of the final values
  // into WS[N] (f32; the bias gradient of the next layer).  Every thread keeps the same 8
  // columns over all its rows (its chunk idx % CH is fixed because the loop strides by NTE),
  // so the sums stay in registers until one LDS reduction and BN atomics per tile.
  constexpr bool CS_OK = !ACC;
  const bool cs = CS_OK && WS != nullptr;
  float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // In-flight store loop (fused bf16 epilogues, whole tiles whose chunk count is a multiple
  // of the thread count: 256x256, 256x128, 128x128, 64x64).  gfx950 counts loads and stores
  // in one vmcnt, so a rolled loop that loads a chunk's bias / row input at its point of use
  // waits, every iteration, for the previous iteration's store to be acknowledged as well:
  // NL serial round trips of store ack + HBM load per pass.  Here the bias chunk (a thread's
  // columns are fixed) is loaded once, all NL row-input chunks of a pass are issued before
  // the staging barrier, and the chunk loop is unrolled and unguarded, so chunk u waits
  // vmcnt(NL - 1): row load u landed, the younger loads and the u stores of this pass stay
  // in flight.  (Behind a per-chunk range guard the compiler counts the minimum over the
  // paths that skipped their stores, vmcnt(NL - 1 - u), which in the in-order counter covers
  // this pass's first stores from chunk NL / 2 on -- so tiles on the M / N edge keep the
  // rolled loop, as do EPI_NONE, which has no load to wait for, BN = 192 (NTE = 504), the
  // stream-K owner (PARTS) and the f32 accumulate paths.)  Arithmetic per element and its
  // order are the rolled loop's.
  // (the 32x32x16 builds of the 256x256 tile, MIPIPE_GEMM_M16=0, also keep the rolled loop:
  // with the 8 row chunks in registers beside the accumulators their dGELU build spills)
  constexpr bool INFLIGHT = !EPI_ROLLED && !ACC && !PARTS && EPI != EPI_NONE && (RG * CH) % NTE == 0 && NTE == NTH &&
                            (StageF::M16 || BM * BN < 256 * 256);
  constexpr int NL = INFLIGHT ? RG * CH / NTH : 1;   // chunks per thread and pass
  constexpr int RSTEP = NTH / CH;                    // tile rows between a thread's consecutive chunks
  const bool inflight = INFLIGHT && m0 + BM <= M && n0 + BN <= N;
  // without a row input there is nothing to keep in flight: with the bias hoisted the loop
  // has no load and so no vmcnt wait, and it stays rolled (unrolled, the bias+GELU build of
  // gemm3 -- the accumulators of wave row 1 stay live through pass 0 -- spills)
  constexpr int UNR = epi_has_row(EPI) ? NL : 1;
  const int trow = (int)threadIdx.x / CH, tgc = n0 + ((int)threadIdx.x % CH) * 8;
  u16x8 bvec = {};
  if constexpr (INFLIGHT && epi_has_bias(EPI)) {
    if (inflight) bvec = *reinterpret_cast<const u16x8*>(bias + tgc);
  }
#pragma unroll 1
  for (int pass = 0; pass < WM; ++pass) {
    u16x8 xrow[NL] = {};
    if constexpr (INFLIGHT && epi_has_row(EPI)) {
      // Aliasing: R may be C itself (the in-place `linear_dx(..., residual=dh, out=dh)` of
      // models/native.py's cross-attention backward; every other caller in ops/kernels.py and
      // models/native.py passes R / AUX distinct from C).  A thread reads here exactly the
      // chunks it overwrites itself later in this pass, and no other thread writes them, so
      // in-place use stays correct.
      if (inflight) {
        const bf16_t* xp = (EPI == EPI_DGELU || EPI == EPI_DRELU) ? AUX : R;
        const int64_t ldxp = (EPI == EPI_DGELU || EPI == EPI_DRELU) ? ldx : ldr;
#pragma unroll
        for (int u = 0; u < NL; ++u)
          xrow[u] = *reinterpret_cast<const u16x8*>(xp + (int64_t)(m0 + pass * RG + trow + u * RSTEP) * ldxp + tgc);
      }
    }
    if (wr == pass) stage(ct, CP);
    __syncthreads();
    if constexpr (!ACC && PARTS) {
      if (nparts > 0) {
        // the partial row blocks added into the staged rows: every thread's loads of one
        // partial in flight at once (a load inside the store loop would wait per element)
        constexpr int Q4 = RG * BN / 4, N4 = (Q4 + NTH - 1) / NTH;
        for (int pp = 0; pp < nparts; ++pp) {
          const float* src = parts + pp * pstep + (int64_t)(pass * RG) * BN;
          float4 pv[N4];
#pragma unroll
          for (int u = 0; u < N4; ++u) {
            const int idx = min((int)threadIdx.x + u * NTH, Q4 - 1);
            pv[u] = *reinterpret_cast<const float4*>(src + (idx / (BN / 4)) * BN + (idx % (BN / 4)) * 4);
          }
#pragma unroll
          for (int u = 0; u < N4; ++u) {
            const int idx = threadIdx.x + u * NTH;
            if (idx >= Q4) break;
            float4* d = reinterpret_cast<float4*>(ct + (idx / (BN / 4)) * CP + (idx % (BN / 4)) * 4);
            float4 t = *d;
            t.x += pv[u].x; t.y += pv[u].y; t.z += pv[u].z; t.w += pv[u].w;
            *d = t;
          }
        }
        __syncthreads();
      }
    }
    const int rbase = m0 + pass * RG;
    if constexpr (ACC) {
      if (nsplit > 1 && WS != nullptr) {
        // split-K partial slab [split][M][N] with plain 16-byte stores; a reduce kernel
        // adds the slabs into C (f32 atomics run at ~1.3 TB/s chip-wide and bounded the
        // dW GEMMs; MI355X_MICROARCH.md "Global float atomics")
        float* slab = WS + (int64_t)(split_idx >= 0 ? split_idx : (int)blockIdx.y) * M * N;
        for (int idx = threadIdx.x; idx < RG * BN / 4; idx += NTH) {
          const int row = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
          const int gr = rbase + row, gc = n0 + c4;
          if (gr < M && gc < N) {
            float4 v = *reinterpret_cast<const float4*>(ct + row * CP + c4);
            v.x *= alpha; v.y *= alpha; v.z *= alpha; v.w *= alpha;
            *reinterpret_cast<float4*>(slab + (int64_t)gr * N + gc) = v;
          }
        }
        __syncthreads();
        continue;
      }
      if (nsplit > 1) {
        float* C = reinterpret_cast<float*>(Cv);
        for (int idx = threadIdx.x; idx < RG * BN; idx += NTH) {
          const int row = idx / BN, col = idx % BN;
          const int gr = rbase + row, gc = n0 + col;
          if (gr < M && gc < N) atomicAdd(C + (int64_t)gr * ldc + gc, alpha * ct[row * CP + col]);
        }
        __syncthreads();
        continue;
      }
    }
    if (inflight) {
      bf16_t* C = reinterpret_cast<bf16_t*>(Cv);
#pragma unroll UNR
      for (int u = 0; u < NL; ++u) {
        const int row = trow + u * RSTEP, gr = rbase + row;
        float v[8];
        const float4 lo = *reinterpret_cast<const float4*>(ct + row * CP + (tgc - n0));
        const float4 hi = *reinterpret_cast<const float4*>(ct + row * CP + (tgc - n0) + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= alpha;
        epi_apply8<EPI>(v, gr, tgc, C, ldc, bvec, xrow[epi_has_row(EPI) ? u : 0], AUX, ldx, p_drop, seed);
        if (cs) {
#pragma unroll
          for (int e = 0; e < 8; ++e) csum[e] += v[e];
        }
      }
    } else
    for (int idx = threadIdx.x < NTE ? (int)threadIdx.x : RG * CH; idx < RG * CH; idx += NTE) {
      const int row = idx / CH, c8 = (idx % CH) * 8;
      const int gr = rbase + row, gc = n0 + c8;
      if (gr >= M || gc >= N) continue;
      float v[8];
      const float4 lo = *reinterpret_cast<const float4*>(ct + row * CP + c8);
      const float4 hi = *reinterpret_cast<const float4*>(ct + row * CP + c8 + 4);
      v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= alpha;
      if constexpr (ACC) {
        float* cp = reinterpret_cast<float*>(Cv) + (int64_t)gr * ldc + gc;
        float4 c0 = *reinterpret_cast<float4*>(cp), c1 = *reinterpret_cast<float4*>(cp + 4);
        c0.x += v[0]; c0.y += v[1]; c0.z += v[2]; c0.w += v[3];
        c1.x += v[4]; c1.y += v[5]; c1.z += v[6]; c1.w += v[7];
        *reinterpret_cast<float4*>(cp) = c0;
        *reinterpret_cast<float4*>(cp + 4) = c1;
      } else {
        epi_store8<EPI>(v, gr, gc, reinterpret_cast<bf16_t*>(Cv), ldc, bias, R, ldr, AUX, ldx, p_drop, seed);
        if (cs) {
#pragma unroll
          for (int e = 0; e < 8; ++e) csum[e] += v[e];
        }
      }
    }
    __syncthreads();
  }
  if constexpr (CS_OK) {
    if (cs) {
      float* red = ct;   // [NTH][8]
#pragma unroll
      for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = csum[e];
      __syncthreads();
      constexpr int GRP = NTE / CH;   // threads per column chunk
      for (int c = threadIdx.x; c < BN; c += NTH) {
        float t = 0.f;
#pragma unroll 4
        for (int g = 0; g < GRP; ++g) t += red[(g * CH + c / 8) * 8 + (c & 7)];
        if (n0 + c < N) atomicAdd(WS + n0 + c, t);
      }
    }
  }
}

// launchers: raise a kernel's dynamic-LDS limit before the first launch from a call site
// (`done` is that site's static flag)
inline void lds_attr_once(bool& done, const void* kern, int bytes) {
  if (done) return;
  (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done = true;
}

}  // namespace g2
