// Weight-streaming linear layer for 17 .. 64 rows: y[M, N] = epi(x[M, K] @ What[N, K]^T) with
// What int8 x per-row scale, int4g128 or bf16, the sibling of gemv_skinny.hip for the batches
// a 16-row call cannot hold.  Each weight is read from HBM once and converted once (int8 ->
// bf16, nibble -> bf16) for all MT = ceil(M / 16) x tiles.
//
// Arithmetic: that of the skinny kernel, bit for bit.  A column of a v_mfma_f32_16x16x32_bf16
// result depends on that column of the x operand only, so a result tile of x tile t is what
// the skinny kernel computes for rows 16 t .. 16 t + 15 as long as the chains are the same:
// `ksplit` chains from gemv::plan, chain s over the K-steps [s per, (s + 1) per), a step =
// MFMAs j = 0..3 with the lane's k 8 j .. 8 j + 7 of its 32 (mp_gemv_frags.h), chains added
// in order by wave 0, the same f32 epilogue.  4-bit weights keep the -24 offset tile and
// acc += scale * tile per group.
//
// Work split: a workgroup owns 16 G weight rows (G <= 2: gemv::plan_rows64) and one wave per
// chain.  A wave holds acc[G][MT], the converted fragments of the current step (16 G VGPRs),
// the raw weights of the next step (in flight) and 32 staged x rows.
//
// The x path.  The skinny kernel's lane (i, c) reads 16 bytes of x row i per MFMA: 64
// different cache lines for 1 KB.  Here x goes through a wave-private LDS slab of 32 rows x
// 128 k (two M-tiles; 16 rows at G = 1, whose 16 waves have 128 VGPRs each): a load
// instruction covers four rows, 16 consecutive lanes reading the 256 contiguous bytes of one
// row's step (8 lines per KB), the rows are written to the slab at a stride of 272 bytes and
// the MFMA fragments come back as 16-byte LDS reads in the skinny kernel's slot order -- lane
// (i, c), fragment j: row i, bytes 64 c + 16 j -- which the 16-byte skew per row spreads over
// all banks.  A step runs its passes over the same converted weights.  While a pass
// computes, the next pass's rows are already in flight to registers.  The slab belongs to
// one wave and a wave's LDS operations execute in order, so there is no workgroup barrier in
// the loop.  Rows >= M and k >= K are never read: their slab entries are zeros.  For 4-bit
// weights the 0 4 1 5 2 6 3 7 slot permutation is applied once, before the slab.
//
// The other x path is register-direct: one XFrag-style fragment per tile straight from global
// memory.  It is what int4g128 runs at G = 2, where it measured faster on the wide matrices
// (profiles/r15_rows64.md); -DMP_ROWS64_XREG builds it for every instantiation, for A/B timing.
//
// LDS: one region per wave, max(slab: 8704 B, 4352 B at G = 1, none on the register path;
// G MT KB); after the loop wave s > 0 leaves its f32 tiles in its own region (the reduction
// needs no space of its own).  No atomics.
#include "mp_api.h"
#include "mp_common.h"
#include "mp_gemv_frags.h"
#include "mp_gemv_plan.h"

namespace mp {
namespace {

// which instantiations take the slab path
constexpr bool x_lds(int WB, int G) {
#ifdef MP_ROWS64_XREG
  return false;
#else
  return !(WB == 0 && G == 2);
#endif
}
constexpr int SLAB_STRIDE = 272;                  // bytes of a slab row: 256 of x and a 16-byte skew
// M-tiles of one pass: two where a lane has 256 VGPRs, one under the 128 of a 16-wave workgroup
constexpr int tiles_per_pass(int G) { return G == 1 ? 1 : 2; }

constexpr int region_bytes(int WB, int G, int MT) {
  const int red = G * MT * 64 * (int)sizeof(f32x4), slab = 16 * tiles_per_pass(G) * SLAB_STRIDE;
  return x_lds(WB, G) && slab > red ? slab : red;
}

// orders a wave's own LDS writes and reads for the compiler; the hardware runs them in order
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// weight operand by the plan's code: 0 packed 4-bit, 1 int8, 2 bf16
template <int WB>
struct Wt;
template <>
struct Wt<0> {
  typedef uint8_t T;
  typedef W4Frag Frag;
  static constexpr int LANE = 16, STEP = gemv::KSTEP / 2;     // elements of T per lane / per step
};
template <>
struct Wt<1> {
  typedef int8_t T;
  typedef WFrag<int8_t> Frag;
  static constexpr int LANE = 32, STEP = gemv::KSTEP;
};
template <>
struct Wt<2> {
  typedef bf16_t T;
  typedef WFrag<bf16_t> Frag;
  static constexpr int LANE = 32, STEP = gemv::KSTEP;
};

// The x rows of one pass (at most TP M-tiles of one step): stage() starts their loads into
// registers, commit() makes them the current pass, frag(tl, j) is MFMA j's operand of tile tl.
template <bool W4, int TP, bool XLDS>
struct XPass {
  u16x8 st[4 * TP], cur[4 * TP];
  char* slab;
  const GemvArgs& a;
  int lane;
  uint32_t lo;       // byte offset of the lane's row and chunk inside a load instruction's rows
  __device__ __forceinline__ XPass(const GemvArgs& a_, char* slab_, int lane_) : slab(slab_), a(a_), lane(lane_) {
    lo = XLDS ? (uint32_t)(lane >> 4) * (uint32_t)a.ldx * 2u + 16u * (lane & 15)
              : (uint32_t)(lane & 15) * (uint32_t)a.ldx * 2u + 64u * (lane >> 4);
  }

  // nt tiles from x row m0 on, k from k0 on
  __device__ __forceinline__ void stage(int m0, int k0, int nt) {
#pragma unroll
    for (int r = 0; r < 4 * TP; ++r) {
      if (r >= 4 * nt) continue;
      // slab path: row 4 r + lane / 16, its 16-byte chunk lane % 16; register path: tile
      // r / 4, row lane % 16, chunk 4 (lane / 16) + r % 4 -- fragment r % 4 of the lane.  The
      // address is a uniform part (scalar registers) plus the lane's 32-bit offset `lo`
      const int mu = m0 + (XLDS ? 4 * r : 16 * (r >> 2)), ku = k0 + (XLDS ? 0 : 8 * (r & 3));
      const int m = mu + (XLDS ? lane >> 4 : lane & 15), k = ku + (XLDS ? 8 * (lane & 15) : 32 * (lane >> 4));
      const char* base = reinterpret_cast<const char*>(a.x + (int64_t)mu * a.ldx + ku);
      u16x8 v = (u16x8)(0);
      if (m < a.M && k < a.K) v = *reinterpret_cast<const u16x8*>(base + lo);
      st[r] = W4 ? __builtin_shufflevector(v, v, 0, 4, 1, 5, 2, 6, 3, 7) : v;
    }
  }
  __device__ __forceinline__ void commit(int nt) {
    if constexpr (XLDS) {
      wave_sync();       // the previous pass's reads are issued
#pragma unroll
      for (int r = 0; r < 4 * TP; ++r)
        if (r < 4 * nt)
          *reinterpret_cast<u16x8*>(slab + (4 * r + (lane >> 4)) * SLAB_STRIDE + 16 * (lane & 15)) = st[r];
      wave_sync();
    } else {
#pragma unroll
      for (int r = 0; r < 4 * TP; ++r) cur[r] = st[r];
    }
  }
  __device__ __forceinline__ bf16x8 frag(int tl, int j) const {
    if constexpr (XLDS) {
      const u16x8 v = *reinterpret_cast<const u16x8*>(slab + (16 * tl + (lane & 15)) * SLAB_STRIDE +
                                                      16 * (4 * (lane >> 4) + j));
      return __builtin_bit_cast(bf16x8, v);
    } else {
      return __builtin_bit_cast(bf16x8, cur[4 * tl + j]);
    }
  }
};

template <int WB, int G, int MT>
__global__ __launch_bounds__(G == 1 ? 1024 : 512) void gemv_rows64_kernel(GemvArgs a) {
  extern __shared__ char smem[];      // [ksplit] regions: the wave's slab, then its f32 tiles
  typedef typename Wt<WB>::T T;
  typedef typename Wt<WB>::Frag Frag;
  constexpr int TP = tiles_per_pass(G), P = (MT + TP - 1) / TP;     // passes of TP M-tiles per step
  constexpr int REGION = region_bytes(WB, G, MT);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int i = lane & 15, c = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * (16 * G);
  const int steps = (a.K + gemv::KSTEP - 1) / gemv::KSTEP;
  const int per = (steps + S - 1) / S;
  const int b = wave * per, e = min(b + per, steps);

  const T* wrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    // rows past N re-read row N - 1 (in bounds); their results are never stored
    const int64_t n = min(n0 + 16 * g + i, (int64_t)a.N - 1);
    wrow[g] = reinterpret_cast<const T*>(a.w) + n * (WB == 0 ? a.K / 2 : a.K) + Wt<WB>::LANE * c;
  }
  const bool sv = a.N % 4 == 0 && ((uintptr_t)a.scale & 15) == 0;
  const int64_t nl = n0 + 4 * c;      // the lane's result rows of group g: nl + 16 g + r

  // raw weights (and group scales) of step s; lane group c of a ragged last step holds k
  // only while k0 + 32 c < K
  Frag nxt[G];
  f32x4 nsc[G];
  auto load_w = [&](int s) {
    const bool kon = s * gemv::KSTEP + 32 * c < a.K;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if constexpr (WB == 0) {
        nxt[g].load(wrow[g] + (int64_t)s * Wt<WB>::STEP);
        nsc[g] = sv ? w4_scales<true>(a.scale + (int64_t)s * a.N, nl + 16 * g, a.N)
                    : w4_scales<false>(a.scale + (int64_t)s * a.N, nl + 16 * g, a.N);
      } else {
        if (kon)
          nxt[g].load(wrow[g] + (int64_t)s * Wt<WB>::STEP);
        else
          nxt[g].zero();
      }
    }
  };

  XPass<WB == 0, TP, x_lds(WB, G)> xp(a, smem + wave * REGION, lane);
  f32x4 acc[G][MT];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[g][t] = (f32x4)(0.f);

  if (b < e) {
    load_w(b);
    xp.stage(0, b * gemv::KSTEP, TP);
  }
  const u32x4 m24 = (u32x4)(0xc1c0c1c0u);      // bf16 -24 in every slot
#pragma unroll 1
  for (int s = b; s < e; ++s) {
    bf16x8 wc[G][4];
    f32x4 sc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) wc[g][j] = nxt[g].frag(j);
      if constexpr (WB == 0) sc[g] = nsc[g];
    }
    if (s + 1 < e) load_w(s + 1);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int nt = MT - TP * p < TP ? MT - TP * p : TP;
      xp.commit(nt);
      if (p + 1 < P)
        xp.stage(16 * TP * (p + 1), s * gemv::KSTEP, MT - TP * (p + 1) < TP ? MT - TP * (p + 1) : TP);
      else if (s + 1 < e)
        xp.stage(0, (s + 1) * gemv::KSTEP, TP);
      if constexpr (WB == 0) {
#pragma unroll
        for (int tl = 0; tl < nt; ++tl) {
          bf16x8 xb[4];
          f32x4 off = (f32x4)(0.f);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            xb[j] = xp.frag(tl, j);
            off = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, m24), xb[j], off, 0, 0, 0);
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            f32x4 t = off;
#pragma unroll
            for (int j = 0; j < 4; ++j) t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[g][j], xb[j], t, 0, 0, 0);
            acc[g][TP * p + tl] += sc[g] * t;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int tl = 0; tl < nt; ++tl) {
            const bf16x8 xb = xp.frag(tl, j);
#pragma unroll
            for (int g = 0; g < G; ++g)
              acc[g][TP * p + tl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[g][j], xb, acc[g][TP * p + tl], 0, 0, 0);
          }
      }
    }
  }

  if (S > 1) {
    // a wave's tiles go over its own slab: no other wave's region is written
    f32x4* red = reinterpret_cast<f32x4*>(smem + wave * REGION);
    if (wave > 0) {
      wave_sync();
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int t = 0; t < MT; ++t) red[(g * MT + t) * 64 + lane] = acc[g][t];
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 1; w < S; ++w) {
      const f32x4* rw = reinterpret_cast<const f32x4*>(smem + w * REGION);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[g][t] += rw[(g * MT + t) * 64 + lane];
    }
  }

  // lane: x rows m = 16 t + i, weight rows n0 + 16 g + 4 c + r
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + i;
    if (m >= a.M) continue;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = nl + 16 * g + r;
        if (n < a.N) gemv_store(a, acc[g][t][r], m, n, WB == 1);
      }
  }
}

template <int WB, int G, int MT>
int launch_gm(const GemvArgs& a, const gemv::Plan& p, hipStream_t st) {
  const size_t lds = (size_t)p.ksplit * region_bytes(WB, G, MT);
  if (lds > 64 * 1024) {
    // more dynamic LDS than the default limit is opted into on the current device, per call
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_rows64_kernel<WB, G, MT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  gemv_rows64_kernel<WB, G, MT><<<dim3((unsigned)p.grid), dim3(64 * p.ksplit), lds, st>>>(a);
  return (int)hipGetLastError();
}

template <int WB>
int launch(const GemvArgs& a, const gemv::Plan& p, hipStream_t st) {
  const int mt = (a.M + 15) / 16;
  if (p.rows == 32) {
    if (mt == 2) return launch_gm<WB, 2, 2>(a, p, st);
    return mt == 3 ? launch_gm<WB, 2, 3>(a, p, st) : launch_gm<WB, 2, 4>(a, p, st);
  }
  if (mt == 2) return launch_gm<WB, 1, 2>(a, p, st);
  return mt == 3 ? launch_gm<WB, 1, 3>(a, p, st) : launch_gm<WB, 1, 4>(a, p, st);
}

}  // namespace
}  // namespace mp

// mp_gemv_skinny's arguments and return values, for 17 <= M <= 64
extern "C" int mp_gemv_rows64(const void* w, const float* scale, int wbytes, const void* x, void* y, const void* bias,
                              const void* res, int M, int N, int K, int64_t ldx, int64_t ldy, int64_t ldr, int gelu,
                              int force_split, hipStream_t st) {
  const gemv::Plan p = gemv::plan_rows64(N, K, wbytes, M, force_split);
  if (p.rows == 0) return -1;
  mp::GemvArgs a;
  if (!mp::gemv_args(a, w, scale, x, y, bias, res, M, N, K, ldx, ldy, ldr, gelu)) return -1;
  if ((wbytes != 2) != (scale != nullptr) || ((uintptr_t)scale & 3)) return -1;
  // x rows are read as 16-byte chunks at 32-bit offsets from a tile's first row
  if (((uintptr_t)x & 15) || ldx % 8 != 0 || ldx >= (int64_t)1 << 26) return -1;
  if (wbytes == 0) return mp::launch<0>(a, p, st);
  return wbytes == 1 ? mp::launch<1>(a, p, st) : mp::launch<2>(a, p, st);
}
