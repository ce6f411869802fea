// The dQ kernels of attention.hip's two-kernel backward (they also write delta = rowsum(dO o O)
// for the dK / dV kernel): v1 (attn_bwd_dq_kernel, every head dim) and v2 / v3 in one template
// (attn_bwd_dq23_kernel, d_h <= 64).  Which one a problem runs: mp_attn_plan.h.
#pragma once
#include "mp_attn_common.h"

// ==========================================================================================
// backward dQ: workgroup = 128 queries of one (b, h) (forward structure)
// ==========================================================================================
template <int DP, bool CAUSAL, bool DROP>
__global__ void __launch_bounds__(256, DP <= 64 ? 2 : 1) attn_bwd_dq_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, const float* __restrict__ LSE,
    float* __restrict__ DELTA,
    bf16_t* __restrict__ dQ, int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs,
    int64_t os, int64_t dqs, float scale, float p_drop, uint64_t seed, float* __restrict__ CSQ) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
  const int nmb = (Sq + 127) / 128;
  // causal: longest-first over the whole grid (see attn_fwd_kernel)
  const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
  const int nbh = (int)gridDim.y;
  const int mb = CAUSAL ? (nmb - 1 - lin / nbh) : (int)blockIdx.x;
  const int bh = CAUSAL ? lin % nbh : (int)blockIdx.y;
  const int b = bh / H, h = bh % H, hk = h / (H / Hkv);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, l32 = lane & 31;
  const int m0 = mb * 128;
  const int qrow = m0 + 32 * w + l32;
  const bool qvalid = qrow < Sq;
  const int shift = Sk - Sq;
  const bf16_t* Kb = K + (int64_t)b * Sk * ks + (int64_t)hk * D;
  const bf16_t* Vb = V + (int64_t)b * Sk * vs + (int64_t)hk * D;
  bf16x8 qf[DP / 16], gf[DP / 16];
  const bf16_t* Qrow = Q + ((int64_t)b * Sq + qrow) * qs + (int64_t)h * D;
  const bf16_t* Grow = dO + ((int64_t)b * Sq + qrow) * os + (int64_t)h * D;
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    qf[s] = __builtin_bit_cast(bf16x8, gload8(Qrow, 16 * s + 8 * hl, D, qvalid));
    gf[s] = __builtin_bit_cast(bf16x8, gload8(Grow, 16 * s + 8 * hl, D, qvalid));
  }
  const int64_t sidx = (int64_t)bh * Sq + qrow;
  const float lse = qvalid ? LSE[sidx] : INFINITY;
  // delta = rowsum(dO * O), fused here (each lane holds half of the row's d range)
  float dlt = 0.f;
  {
    const bf16_t* Orow = O + ((int64_t)b * Sq + qrow) * os + (int64_t)h * D;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
      const u16x8 ov = gload8(Orow, 16 * s + 8 * hl, D, qvalid);
      const bf16x8 g = gf[s];
#pragma unroll
      for (int j = 0; j < 8; ++j) dlt += bf2f(ov[j]) * (float)g[j];
    }
    dlt += __shfl_xor(dlt, 32, 64);
    if (qvalid && hl == 0) DELTA[sidx] = dlt;
  }
  const float c = scale * LOG2E;
  const DropKey dkey = drop_key(seed, (uint32_t)bh);
  const uint32_t dthr = drop_thr(p_drop), qoff = (uint32_t)qrow * (uint32_t)Sk;
  const float dinv = 1.0f / (1.0f - p_drop);
  f32x16 dq[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) dq[d] = {};
  int n_end = Sk;
  if (CAUSAL) n_end = min(Sk, m0 + 128 + shift);
  const int ntiles = (n_end + 63) / 64;
  // K / V tiles stream through an NBUF-deep LDS ring by LDS-DMA (the dK/dV kernel's
  // scheme): LOOK tiles in flight, counted vmcnt, one raw barrier per tile
  constexpr int NBUF = DP <= 128 ? 4 : 2;
  constexpr int LOOK = NBUF - 1;
  constexpr int BUFB = 2 * TILE;
  using GT = GTile<DP>;
  constexpr int PER_TILE = 2 * GT::PPW;
  GT gt;
  gt.init();
  const int wv = __builtin_amdgcn_readfirstlane(w);
  auto issue = [&](int t) {
    char* buf = smem + (t % NBUF) * BUFB;
    gt.issue(Kb, ks, t * 64, Sk, D, buf, wv);
    gt.issue(Vb, vs, t * 64, Sk, D, buf + TILE, wv);
  };
#pragma unroll
  for (int i = 0; i < LOOK; ++i)
    if (i < ntiles) issue(i);
  const int wave_last_q = m0 + 32 * w + 31 + shift;
  for (int t = 0; t < ntiles; ++t) {
    const int n0 = t * 64;
    if (LOOK >= 3 && t + 2 < ntiles) attn_wait_vmcnt<2 * PER_TILE>();
    else if (LOOK >= 2 && t + 1 < ntiles) attn_wait_vmcnt<PER_TILE>();
    else attn_wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // every wave is done with tile t-1: its buffer takes tile t+LOOK
    if (t + LOOK < ntiles) issue(t + LOOK);
    if (!(CAUSAL && n0 > wave_last_q)) {
      const char* kb = smem + (t % NBUF) * BUFB;
      const char* vb = kb + TILE;
      f32x16 s0 = {}, s1 = {}, p0 = {}, p1 = {};
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        bf16x8 ak0 = lds_row8<DP>(kb, l32, 2 * s + hl);
        bf16x8 ak1 = lds_row8<DP>(kb, 32 + l32, 2 * s + hl);
        bf16x8 av0 = lds_row8<DP>(vb, l32, 2 * s + hl);
        bf16x8 av1 = lds_row8<DP>(vb, 32 + l32, 2 * s + hl);
        s0 = mfma32(ak0, qf[s], s0);
        s1 = mfma32(ak1, qf[s], s1);
        p0 = mfma32(av0, gf[s], p0);  // dP^T = V dO^T
        p1 = mfma32(av1, gf[s], p1);
      }
      // causal / key-end mask only on edge tiles; invalid query rows have lse = +inf
      const bool edge = (n0 + 64 > Sk) || (CAUSAL && n0 + 63 > m0 + 32 * w + shift);
      // masked / unmasked element math behind one wave-uniform branch (see the dK/dV kernel)
      // dropout keep bits first (only the mask stays live across the hashes)
      uint32_t keep = 0xffffffffu;
      if (DROP) {
        keep = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const uint32_t kr = (uint32_t)(n0 + (r & 3) + 8 * (r >> 2) + 4 * hl);
          keep |= (hash_lo(dkey, qoff + kr) >= dthr ? 1u : 0u) << r;
          keep |= (hash_lo(dkey, qoff + kr + 32u) >= dthr ? 1u : 0u) << (16 + r);
        }
      }
      auto elems = [&](auto masked) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = (r & 3) + 8 * (r >> 2) + 4 * hl;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int kk = n0 + 32 * half + kr;
            float sv = half ? s1[r] : s0[r];
            float dpv = half ? p1[r] : p0[r];
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sv, c, -lse));
            if constexpr (decltype(masked)::value) {
              if (kk >= Sk || (CAUSAL && kk > qrow + shift)) p = 0.f;
            }
            if (DROP) dpv = (keep >> (16 * half + r)) & 1u ? dpv * dinv : 0.f;
            const float dsv = p * (dpv - dlt);
            if (half) s1[r] = dsv; else s0[r] = dsv;
          }
        }
      };
      if (edge) elems(std::true_type{});
      else elems(std::false_type{});
      const bf16x8 d00 = pack8(s0, 0), d01 = pack8(s0, 1), d10 = pack8(s1, 0), d11 = pack8(s1, 1);
#pragma unroll
      for (int d = 0; d < DP / 32; ++d) {
        const int c0 = 32 * d + 16 * ((lane >> 4) & 1);
        bf16x8 a;
        a = cat44(lds_tr4<DP>(kb, 0 + 4 * hl, c0), lds_tr4<DP>(kb, 8 + 4 * hl, c0));
        dq[d] = mfma32(a, d00, dq[d]);
        a = cat44(lds_tr4<DP>(kb, 16 + 4 * hl, c0), lds_tr4<DP>(kb, 24 + 4 * hl, c0));
        dq[d] = mfma32(a, d01, dq[d]);
        a = cat44(lds_tr4<DP>(kb, 32 + 4 * hl, c0), lds_tr4<DP>(kb, 40 + 4 * hl, c0));
        dq[d] = mfma32(a, d10, dq[d]);
        a = cat44(lds_tr4<DP>(kb, 48 + 4 * hl, c0), lds_tr4<DP>(kb, 56 + 4 * hl, c0));
        dq[d] = mfma32(a, d11, dq[d]);
      }
    }
  }
  if (CSQ != nullptr) {
    __syncthreads();   // K / V tiles no longer read
    wg_colsum_atomic<DP>(dq, scale, qvalid, reinterpret_cast<float*>(smem), CSQ + (int64_t)h * D, D);
  }
  if (qvalid) {
    bf16_t* drow = dQ + ((int64_t)b * Sq + qrow) * dqs + (int64_t)h * D;
#pragma unroll
    for (int d = 0; d < DP / 32; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * d + 8 * g + 4 * hl;
        if (col < D) {
          u16x4 pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = f2bf(dq[d][4 * g + e] * scale);
          *reinterpret_cast<u16x4*>(drow + col) = pk;
        }
      }
    }
  }
}

// backward dQ v2 and v3 (d_h 64): attn_bwd_dq_kernel's math on the forward v2 tile
// machinery -- buffer-load-to-LDS K/V ring with entry-time lane offsets, the tile loop
// unrolled over the 4-deep ring (immediate LDS offsets), one-compare masks.  PAIRED (v3, the
// default): paired causal query blocks on one XCD, a 1-D grid.  !PAIRED (v2,
// MIPIPE_ATTN_BWD_DQ=2, an A/B arm): one query block per workgroup of a 2-D grid.  Only the
// workgroup -> query block mapping and the pass count differ.
template <int DP, bool CAUSAL, bool DROP, bool PAIRED>
__global__ void __launch_bounds__(256, 2) attn_bwd_dq23_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, const float* __restrict__ LSE,
    float* __restrict__ DELTA,
    bf16_t* __restrict__ dQ, int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs,
    int64_t os, int64_t dqs, float scale, float p_drop, uint64_t seed, float* __restrict__ CSQ) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
  const int nmb = (Sq + 127) / 128;
  int bh, p;   // (b, h) and, PAIRED, the pair of query blocks; else the query block
  if constexpr (PAIRED) {
    // causal: one workgroup runs query block nmb-1-p and then block p of the same (b, h), the
    // pairs of one (b, h) consecutive on one XCD (the forward v2 mapping)
    const int npair = CAUSAL ? (nmb + 1) / 2 : nmb;
    const int nbh = B * H;
    const int lin = (int)blockIdx.x;
    if ((nbh & 7) == 0) {
      const int xcd = lin & 7, j = lin >> 3;
      bh = (j / npair) * 8 + xcd;
      p = j % npair;
    } else {
      bh = lin / npair;
      p = lin % npair;
    }
  } else {
    // causal: longest-first over the whole grid (see attn_fwd_kernel)
    const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
    const int nbh = (int)gridDim.y;
    p = CAUSAL ? (nmb - 1 - lin / nbh) : (int)blockIdx.x;
    bh = CAUSAL ? lin % nbh : (int)blockIdx.y;
  }
  const int b = bh / H, h = bh % H, hk = h / (H / Hkv);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, l32 = lane & 31;
  const int npass = PAIRED && CAUSAL && (nmb - 1 - p) != p ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {   // (the pass body keeps the indentation of a single pass)
  const int mb = PAIRED && CAUSAL ? (pass == 0 ? nmb - 1 - p : p) : p;
  if (pass > 0) {   // the ring and the column-sum scratch of the previous pass are free
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  const int m0 = mb * 128;
  const int qrow = m0 + 32 * w + l32;
  const bool qvalid = qrow < Sq;
  const int shift = Sk - Sq;
  const bf16_t* Kb = K + (int64_t)b * Sk * ks + (int64_t)hk * D;
  const bf16_t* Vb = V + (int64_t)b * Sk * vs + (int64_t)hk * D;
  bf16x8 qf[DP / 16], gf[DP / 16];
  const bf16_t* Qrow = Q + ((int64_t)b * Sq + qrow) * qs + (int64_t)h * D;
  const bf16_t* Grow = dO + ((int64_t)b * Sq + qrow) * os + (int64_t)h * D;
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    qf[s] = __builtin_bit_cast(bf16x8, gload8(Qrow, 16 * s + 8 * hl, D, qvalid));
    gf[s] = __builtin_bit_cast(bf16x8, gload8(Grow, 16 * s + 8 * hl, D, qvalid));
  }
  const int64_t sidx = (int64_t)bh * Sq + qrow;
  const float lse = qvalid ? LSE[sidx] : INFINITY;
  // delta = rowsum(dO * O), fused here (each lane holds half of the row's d range)
  float dlt = 0.f;
  {
    const bf16_t* Orow = O + ((int64_t)b * Sq + qrow) * os + (int64_t)h * D;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
      const u16x8 ov = gload8(Orow, 16 * s + 8 * hl, D, qvalid);
      const bf16x8 g = gf[s];
#pragma unroll
      for (int j = 0; j < 8; ++j) dlt += bf2f(ov[j]) * (float)g[j];
    }
    dlt += __shfl_xor(dlt, 32, 64);
    if (qvalid && hl == 0) DELTA[sidx] = dlt;
  }
  const float c = scale * LOG2E;
  const DropKey dkey = drop_key(seed, (uint32_t)bh);
  const uint32_t dthr = drop_thr(p_drop), qoff = (uint32_t)qrow * (uint32_t)Sk;
  const float dinv = 1.0f / (1.0f - p_drop);
  f32x16 dq[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) dq[d] = {};
  int n_end = Sk;
  if (CAUSAL) n_end = min(Sk, m0 + 128 + shift);
  const int ntiles = (n_end + 63) / 64;
  // K / V tiles stream through an NBUF-deep LDS ring by LDS-DMA (the dK/dV kernel's
  // scheme): LOOK tiles in flight, counted vmcnt, one raw barrier per tile
  // K / V ring (the forward v2 scheme): NBUF buffers, LOOK tiles in flight, buffer-load-to-LDS
  // DMA with per-lane offsets fixed here and a scalar tile offset; the tile loop is unrolled
  // over the ring so every LDS address is an immediate
  constexpr int NBUF = 4, LOOK = NBUF - 1, BUFB = 2 * TILE;
  constexpr int PER_TILE = 2 * BTile<DP>::PPW;
  const int wv = __builtin_amdgcn_readfirstlane(w);
  const __amdgpu_buffer_rsrc_t krs =
      __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, (int)(((int64_t)(Sk - 1) * ks + D) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t vrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, (int)(((int64_t)(Sk - 1) * vs + D) * 2), 0x00020000);
  BTile<DP> kt, vt;
  kt.init(ks, D, wv);
  vt.init(vs, D, wv);
  const int kstep = (int)(64 * ks * 2), vstep = (int)(64 * vs * 2);
  auto issue_to = [&](int t, char* buf) {
    kt.issue(krs, t * kstep, buf, wv);
    vt.issue(vrs, t * vstep, buf + TILE, wv);
  };
  int koff[DP / 16], ktoff[DP / 32][2];   // (see attn_fwd2_kernel)
  {
    const int i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) koff[s] = lds_off<DP>(l32, 2 * s + hl);
#pragma unroll
    for (int d = 0; d < DP / 32; ++d)
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int row = 8 * jp + 4 * hl + q, col = 32 * d + 16 * ((lane >> 4) & 1) + 4 * pp;
        ktoff[d][jp] = lds_off<DP>(row, col >> 3) + ((col & 7) << 1);
      }
  }
  // per-lane mask limit (see attn_fwd2_kernel): key k (+4 hl) of a tile at n0 is kept iff k <= lim0 - n0
  const int lim0 = (CAUSAL ? min(qrow + shift, Sk - 1) : Sk - 1) - 4 * hl;
#pragma unroll
  for (int i = 0; i < LOOK; ++i)
    if (i < ntiles) issue_to(i, smem + i * BUFB);
  const int wave_last_q = m0 + 32 * w + 31 + shift;
  auto tile = [&](auto bufc, int t) {
    constexpr int BUF = decltype(bufc)::value;
    const int n0 = t * 64;
    if (t + 2 < ntiles) attn_wait_vmcnt<2 * PER_TILE>();
    else if (t + 1 < ntiles) attn_wait_vmcnt<PER_TILE>();
    else attn_wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // every wave is done with tile t-1: its buffer takes tile t+LOOK
    if (t + LOOK < ntiles) issue_to(t + LOOK, smem + ((BUF + LOOK) % NBUF) * BUFB);
    if (!(CAUSAL && n0 > wave_last_q)) {
      const char* kb = smem + BUF * BUFB;
      const char* vb = kb + TILE;
      f32x16 s0 = {}, s1 = {}, p0 = {}, p1 = {};
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        const bf16x8 ak0 = *reinterpret_cast<const bf16x8*>(kb + koff[s]);
        const bf16x8 ak1 = *reinterpret_cast<const bf16x8*>(kb + koff[s] + 32 * DP * 2);
        const bf16x8 av0 = *reinterpret_cast<const bf16x8*>(vb + koff[s]);
        const bf16x8 av1 = *reinterpret_cast<const bf16x8*>(vb + koff[s] + 32 * DP * 2);
        s0 = mfma32(ak0, qf[s], s0);
        s1 = mfma32(ak1, qf[s], s1);
        p0 = mfma32(av0, gf[s], p0);  // dP^T = V dO^T
        p1 = mfma32(av1, gf[s], p1);
      }
      // causal / key-end mask only on edge tiles; invalid query rows have lse = +inf
      const bool edge = (n0 + 64 > Sk) || (CAUSAL && n0 + 63 > m0 + 32 * w + shift);
      // masked / unmasked element math behind one wave-uniform branch (see the dK/dV kernel)
      // dropout keep bits first (only the mask stays live across the hashes)
      uint32_t keep = 0xffffffffu;
      if (DROP) {
        keep = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const uint32_t kr = (uint32_t)(n0 + (r & 3) + 8 * (r >> 2) + 4 * hl);
          keep |= (hash_lo(dkey, qoff + kr) >= dthr ? 1u : 0u) << r;
          keep |= (hash_lo(dkey, qoff + kr + 32u) >= dthr ? 1u : 0u) << (16 + r);
        }
      }
      auto elems = [&](auto masked) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = (r & 3) + 8 * (r >> 2) + 4 * hl;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int kk = n0 + 32 * half + kr;
            float sv = half ? s1[r] : s0[r];
            float dpv = half ? p1[r] : p0[r];
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sv, c, -lse));
            if constexpr (decltype(masked)::value) {
              if (key_of(r) + 32 * half > lim0 - n0) p = 0.f;
            }
            if (DROP) dpv = (keep >> (16 * half + r)) & 1u ? dpv * dinv : 0.f;
            const float dsv = p * (dpv - dlt);
            if (half) s1[r] = dsv; else s0[r] = dsv;
          }
        }
      };
      if (edge) elems(std::true_type{});
      else elems(std::false_type{});
      const bf16x8 d00 = pack8(s0, 0), d01 = pack8(s0, 1), d10 = pack8(s1, 0), d11 = pack8(s1, 1);
#pragma unroll
      for (int d = 0; d < DP / 32; ++d) {
        auto tr = [&](int jp, int m) {
          return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(kb + ktoff[d][jp] + 16 * DP * 2 * m));
        };
        dq[d] = mfma32(cat44(tr(0, 0), tr(1, 0)), d00, dq[d]);
        dq[d] = mfma32(cat44(tr(0, 1), tr(1, 1)), d01, dq[d]);
        dq[d] = mfma32(cat44(tr(0, 2), tr(1, 2)), d10, dq[d]);
        dq[d] = mfma32(cat44(tr(0, 3), tr(1, 3)), d11, dq[d]);
      }
    }
  };
  for (int t0 = 0; t0 < ntiles; t0 += NBUF) {
    tile(std::integral_constant<int, 0>{}, t0);
    if (t0 + 1 < ntiles) tile(std::integral_constant<int, 1>{}, t0 + 1);
    if (t0 + 2 < ntiles) tile(std::integral_constant<int, 2>{}, t0 + 2);
    if (t0 + 3 < ntiles) tile(std::integral_constant<int, 3>{}, t0 + 3);
  }
  if (CSQ != nullptr) {
    __syncthreads();   // K / V tiles no longer read
    wg_colsum_atomic<DP>(dq, scale, qvalid, reinterpret_cast<float*>(smem), CSQ + (int64_t)h * D, D);
  }
  if (qvalid) {
    bf16_t* drow = dQ + ((int64_t)b * Sq + qrow) * dqs + (int64_t)h * D;
#pragma unroll
    for (int d = 0; d < DP / 32; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * d + 8 * g + 4 * hl;
        if (col < D) {
          u16x4 pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = f2bf(dq[d][4 * g + e] * scale);
          *reinterpret_cast<u16x4*>(drow + col) = pk;
        }
      }
    }
  }
  }
}
