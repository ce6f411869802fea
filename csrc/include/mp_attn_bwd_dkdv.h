// The dK / dV kernels of attention.hip's two-kernel backward: v1 (attn_bwd_dkdv_kernel, every
// head dim) and v2 / v3 in one template (attn_bwd_dkdv23_kernel, d_h <= 64).  Which one a
// problem runs: mp_attn_plan.h.
#pragma once
#include "mp_attn_common.h"

// ==========================================================================================
// backward dK / dV: workgroup = 128 keys (4 waves x 32) of one (b, kv head)
// ==========================================================================================
// Q / dO tiles and the per-row LSE / delta stream through an NBUF-deep LDS ring by
// LDS-DMA (2 tiles in flight for DP <= 128): no staging registers, one raw barrier per
// tile, counted vmcnt.  Same math as before: key on the MFMA lane, P and dS are the B
// operands of dV^T += dO^T P and dK^T += Q^T dS.
template <int DP, bool CAUSAL, bool DROP>
__global__ void __launch_bounds__(256, DP <= 64 ? 2 : 1) attn_bwd_dkdv_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const bf16_t* __restrict__ dO, const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16_t* __restrict__ dK, bf16_t* __restrict__ dV, int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs,
    int64_t ks, int64_t vs, int64_t os, int64_t dks, int64_t dvs, float scale, float p_drop, uint64_t seed,
    float* __restrict__ CSK, float* __restrict__ CSV) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
  constexpr int BUFB = 2 * TILE + 512;               // Q, dO, lse[64], delta[64]
  // ring depth: MIPIPE-tunable at build time (MP_DKDV_NBUF, mp_attn_plan.h); 4 buffers keep 3 tiles in flight
  constexpr int NBUF = DP <= 128 ? MP_DKDV_NBUF : 2;
  constexpr int LOOK = NBUF - 1;                     // tiles issued ahead
  using GT = GTile<DP>;

  // causal: key block 0 sees every query -> longest-first over the whole grid (all (b, h)'s
  // first key block, then the second, ...), as in the forward
  const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
  const int kb = CAUSAL ? lin / (int)gridDim.y : (int)blockIdx.x;
  const int bhk = CAUSAL ? lin % (int)gridDim.y : (int)blockIdx.y;
  const int b = bhk / Hkv, hk = bhk % Hkv;
  const int grp = H / Hkv;
  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = kb * 128;
  const int key = k0 + 32 * w + l32;  // this lane's key (MFMA column)
  const bool kvalid = key < Sk;
  const int shift = Sk - Sq;

  // K and V of this wave's 32 keys as B operands: lane holds K[key][16s + 8hl + j]
  bf16x8 kf[DP / 16], vf[DP / 16];
  const bf16_t* Krow = K + ((int64_t)b * Sk + key) * ks + (int64_t)hk * D;
  const bf16_t* Vrow = V + ((int64_t)b * Sk + key) * vs + (int64_t)hk * D;
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    kf[s] = __builtin_bit_cast(bf16x8, gload8(Krow, 16 * s + 8 * hl, D, kvalid));
    vf[s] = __builtin_bit_cast(bf16x8, gload8(Vrow, 16 * s + 8 * hl, D, kvalid));
  }
  f32x16 dk[DP / 32], dv[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) {
    dk[d] = {};
    dv[d] = {};
  }
  const float c = scale * LOG2E;
  const uint32_t dthr = drop_thr(p_drop);
  const float dinv = 1.0f / (1.0f - p_drop);
  // first query that can see key k0: q >= k0 - shift
  const int q_begin = CAUSAL ? max(0, ((k0 - shift) / 64) * 64) : 0;
  const int ntq = (Sq - q_begin + 63) / 64;
  const int total = ntq * grp;

  GT gt;
  gt.init();
  auto issue = [&](int it) {
    const int hq = hk * grp + it / ntq;
    const int q0 = q_begin + (it % ntq) * 64;
    char* buf = smem + (it % NBUF) * BUFB;
    gt.issue(Q + (int64_t)b * Sq * qs + (int64_t)hq * D, qs, q0, Sq, D, buf, w);
    gt.issue(dO + (int64_t)b * Sq * os + (int64_t)hq * D, os, q0, Sq, D, buf + TILE, w);
    if (w == 0) {  // per-row stats, 4 bytes per lane (rows past Sq are masked in the math)
      const int q = min(q0 + lane, Sq - 1);
      const int64_t idx = ((int64_t)b * H + hq) * Sq + q;
      __builtin_amdgcn_global_load_lds((const void*)(LSE + idx),
                                       (__attribute__((address_space(3))) void*)(buf + 2 * TILE), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(DELTA + idx),
                                       (__attribute__((address_space(3))) void*)(buf + 2 * TILE + 256), 4, 0, 0);
    }
  };
  constexpr int PER_TILE = 2 * GT::PPW;  // DMA instructions per tile per wave (+2 on wave 0)
#pragma unroll
  for (int i = 0; i < LOOK; ++i)
    if (i < total) issue(i);

  for (int it = 0; it < total; ++it) {
    const int hq = hk * grp + it / ntq;
    const int q0 = q_begin + (it % ntq) * 64;
    const int bhq = b * H + hq;
    const DropKey dkey = drop_key(seed, (uint32_t)bhq);
    // tile `it` landed (up to LOOK-1 younger tiles may stay in flight), then publish to all
    // waves; wave 0 issues 2 extra DMAs per tile (the row stats)
    if (LOOK >= 3 && it + 2 < total) {
      if (w == 0) attn_wait_vmcnt<2 * (PER_TILE + 2)>(); else attn_wait_vmcnt<2 * PER_TILE>();
    } else if (LOOK >= 2 && it + 1 < total) {
      if (w == 0) attn_wait_vmcnt<PER_TILE + 2>(); else attn_wait_vmcnt<PER_TILE>();
    } else {
      attn_wait_vmcnt<0>();
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // the buffer of tile it-1 is free now: refill it with tile it+LOOK
    if (it + LOOK < total) issue(it + LOOK);
    const char* qb = smem + (it % NBUF) * BUFB;
    const char* gb = qb + TILE;
    const float* ls = reinterpret_cast<const float*>(qb + 2 * TILE);
    const float* dl = ls + 64;
    const bool skip = CAUSAL && (k0 + 32 * w > q0 + 63 + shift);  // all of this wave's keys masked
    if (!skip) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // S[q][key] = Q K^T, dP[q][key] = dO V^T   (query rows u*32.. in registers, key on lane)
        f32x16 sacc = {}, pacc = {};
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) {
          bf16x8 aq = lds_row8<DP>(qb, 32 * u + l32, 2 * s + hl);
          bf16x8 ag = lds_row8<DP>(gb, 32 * u + l32, 2 * s + hl);
          sacc = mfma32(aq, kf[s], sacc);
          pacc = mfma32(ag, vf[s], pacc);
        }
        f32x16 pm, ds;
        // per-row stats: rows 32u + 8g + 4hl + 0..3 are contiguous -> one 16-byte LDS read
        float4 lsv[4], dlv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          lsv[g] = *reinterpret_cast<const float4*>(ls + 32 * u + 8 * g + 4 * hl);
          dlv[g] = *reinterpret_cast<const float4*>(dl + 32 * u + 8 * g + 4 * hl);
        }
        // masks only where needed: the causal diagonal and query rows past Sq (their
        // stats were clamped); keys past Sk only feed their own unwritten outputs
        const bool edge = (q0 + 64 > Sq) || (CAUSAL && (k0 + 32 * w + 31 > q0 + 32 * u + shift));
        // the element math twice, masked and unmasked, behind one wave-uniform branch: as a
        // per-element select the mask's index compares and cndmasks were issued on every
        // tile (~half of the loop's VALU, profiles/r2_attention_pmc_counters.json)
        // dropout keep bits first (only the mask stays live across the hashes)
        uint32_t keep = 0xffffu;
        if (DROP) {
          keep = 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const uint32_t q = (uint32_t)(q0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hl);
            keep |= (hash_lo(dkey, q * (uint32_t)Sk + (uint32_t)key) >= dthr ? 1u : 0u) << r;
          }
        }
        auto elems = [&](auto masked) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qr = 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hl;
            const int q = q0 + qr;
            const float lv = (&lsv[r >> 2].x)[r & 3], dv_ = (&dlv[r >> 2].x)[r & 3];
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], c, -lv));
            if constexpr (decltype(masked)::value) {
              if (q >= Sq || (CAUSAL && key > q + shift)) p = 0.f;
            }
            float dpv = pacc[r];
            float pd = p;
            if (DROP) {
              const float msk = (keep >> r) & 1u ? dinv : 0.f;
              pd = p * msk;
              dpv = dpv * msk;
            }
            pm[r] = pd;                      // dropped P for dV
            ds[r] = p * (dpv - dv_);         // dS
          }
        };
        if (edge) elems(std::true_type{});
        else elems(std::false_type{});
        // dV^T += dO^T P ;  dK^T += Q^T dS     (A via transposed LDS reads of the row images)
        const bf16x8 pb0 = pack8(pm, 0), pb1 = pack8(pm, 1);
        const bf16x8 db0 = pack8(ds, 0), db1 = pack8(ds, 1);
#pragma unroll
        for (int d = 0; d < DP / 32; ++d) {
          const int c0 = 32 * d + 16 * ((lane >> 4) & 1);
          const int rb = 32 * u + 4 * hl;
          bf16x8 ag0 = cat44(lds_tr4<DP>(gb, rb + 0, c0), lds_tr4<DP>(gb, rb + 8, c0));
          bf16x8 ag1 = cat44(lds_tr4<DP>(gb, rb + 16, c0), lds_tr4<DP>(gb, rb + 24, c0));
          dv[d] = mfma32(ag0, pb0, dv[d]);
          dv[d] = mfma32(ag1, pb1, dv[d]);
          bf16x8 aq0 = cat44(lds_tr4<DP>(qb, rb + 0, c0), lds_tr4<DP>(qb, rb + 8, c0));
          bf16x8 aq1 = cat44(lds_tr4<DP>(qb, rb + 16, c0), lds_tr4<DP>(qb, rb + 24, c0));
          dk[d] = mfma32(aq0, db0, dk[d]);
          dk[d] = mfma32(aq1, db1, dk[d]);
        }
      }
    }
  }
  // ---- fused bias-gradient column sums of dK (scaled) and dV
  if (CSK != nullptr) {
    __syncthreads();   // the Q / dO ring is free
    float* red = reinterpret_cast<float*>(smem);
    wg_colsum_atomic<DP>(dk, scale, kvalid, red, CSK + (int64_t)hk * D, D);
    __syncthreads();
    wg_colsum_atomic<DP>(dv, 1.f, kvalid, red, CSV + (int64_t)hk * D, D);
  }
  // ---- epilogue: lane = key, registers = d
  if (kvalid) {
    bf16_t* dkrow = dK + ((int64_t)b * Sk + key) * dks + (int64_t)hk * D;
    bf16_t* dvrow = dV + ((int64_t)b * Sk + key) * dvs + (int64_t)hk * D;
#pragma unroll
    for (int d = 0; d < DP / 32; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * d + 8 * g + 4 * hl;
        if (col < D) {
          u16x4 a, bb;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[e] = f2bf(dk[d][4 * g + e] * scale);
            bb[e] = f2bf(dv[d][4 * g + e]);
          }
          *reinterpret_cast<u16x4*>(dkrow + col) = a;
          *reinterpret_cast<u16x4*>(dvrow + col) = bb;
        }
      }
    }
  }
}

// backward dK / dV v2 and v3 (d_h 64): attn_bwd_dkdv_kernel's math on the forward v2
// tile machinery (buffer-load-to-LDS Q / dO ring, lane offsets fixed at entry, the tile loop
// unrolled over the 4-deep ring so every LDS address is an immediate).  PAIRED (v3, the
// default): paired causal key blocks on one XCD, a 1-D grid.  !PAIRED (v2,
// MIPIPE_ATTN_BWD_DKDV=2, an A/B arm): one key block per workgroup of a 2-D grid.  Only the
// workgroup -> key block mapping and the pass count differ.
template <int DP, bool CAUSAL, bool DROP, bool PAIRED>
__global__ void __launch_bounds__(256, 2) attn_bwd_dkdv23_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const bf16_t* __restrict__ dO, const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16_t* __restrict__ dK, bf16_t* __restrict__ dV, int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs,
    int64_t ks, int64_t vs, int64_t os, int64_t dks, int64_t dvs, float scale, float p_drop, uint64_t seed,
    float* __restrict__ CSK, float* __restrict__ CSV) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
  constexpr int BUFB = 2 * TILE + 512;               // Q, dO, lse[64], delta[64]
  constexpr int NBUF = 4;                            // 4 buffers keep 3 tiles in flight
  constexpr int LOOK = NBUF - 1;                     // tiles issued ahead

  const int nkb = (Sk + 127) / 128;
  int bhk, p;   // (b, kv head) and, PAIRED, the pair of key blocks; else the key block
  if constexpr (PAIRED) {
    // causal: one workgroup runs key block p (it sees the most queries) and then block
    // nkb-1-p of the same (b, kv head), so every workgroup does about the same work; the pairs
    // of one (b, kv head) are consecutive on one XCD (workgroup id mod 8), so their Q / dO tiles
    // are read while the others still hold them in that XCD's L2 (the forward v2 mapping)
    const int npair = CAUSAL ? (nkb + 1) / 2 : nkb;
    const int nbhk = B * Hkv;
    const int lin = (int)blockIdx.x;
    if ((nbhk & 7) == 0) {
      const int xcd = lin & 7, j = lin >> 3;
      bhk = (j / npair) * 8 + xcd;
      p = j % npair;
    } else {
      bhk = lin / npair;
      p = lin % npair;
    }
  } else {
    // causal: key block 0 sees every query -> longest-first over the whole grid (all (b, h)'s
    // first key block, then the second, ...), as in the forward
    const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
    p = CAUSAL ? lin / (int)gridDim.y : (int)blockIdx.x;
    bhk = CAUSAL ? lin % (int)gridDim.y : (int)blockIdx.y;
  }
  const int b = bhk / Hkv, hk = bhk % Hkv;
  const int grp = H / Hkv;
  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int shift = Sk - Sq;
  const float c = scale * LOG2E;
  const uint32_t dthr = drop_thr(p_drop);
  const float dinv = 1.0f / (1.0f - p_drop);
  BTile<DP> qt, gt2;
  qt.init(qs, D, w);
  gt2.init(os, D, w);
  // per-lane fragment offsets (see attn_fwd2_kernel): row reads of rows 32u + l32 at chunk
  // 2s + hl; transposed reads of rows 32u + 8j + 4hl + q at column 32d + 16 (lane>>4 & 1) + 4p
  int roff[DP / 16], troff[DP / 32][2];
  {
    const int i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) roff[s] = lds_off<DP>(l32, 2 * s + hl);
#pragma unroll
    for (int d = 0; d < DP / 32; ++d)
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int row = 8 * jp + 4 * hl + q, col = 32 * d + 16 * ((lane >> 4) & 1) + 4 * pp;
        troff[d][jp] = lds_off<DP>(row, col >> 3) + ((col & 7) << 1);
      }
  }
  const int npass = PAIRED && CAUSAL && (nkb - 1 - p) != p ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {   // (the pass body keeps the indentation of a single pass)
  const int kb = PAIRED && CAUSAL ? (pass == 0 ? p : nkb - 1 - p) : p;
  const int k0 = kb * 128;
  const int key = k0 + 32 * w + l32;  // this lane's key (MFMA column)
  const bool kvalid = key < Sk;
  if (pass > 0) {   // the ring and the column-sum scratch of the previous pass are free
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }

  // K and V of this wave's 32 keys as B operands: lane holds K[key][16s + 8hl + j]
  bf16x8 kf[DP / 16], vf[DP / 16];
  const bf16_t* Krow = K + ((int64_t)b * Sk + key) * ks + (int64_t)hk * D;
  const bf16_t* Vrow = V + ((int64_t)b * Sk + key) * vs + (int64_t)hk * D;
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    kf[s] = __builtin_bit_cast(bf16x8, gload8(Krow, 16 * s + 8 * hl, D, kvalid));
    vf[s] = __builtin_bit_cast(bf16x8, gload8(Vrow, 16 * s + 8 * hl, D, kvalid));
  }
  f32x16 dk[DP / 32], dv[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) {
    dk[d] = {};
    dv[d] = {};
  }
  // first query that can see key k0: q >= k0 - shift
  const int q_begin = CAUSAL ? max(0, ((k0 - shift) / 64) * 64) : 0;
  const int ntq = (Sq - q_begin + 63) / 64;
  const int total = ntq * grp;

  // Q / dO tiles by buffer-load-to-LDS DMA (the forward v2 scheme): per-lane offsets fixed
  // here, the tile's row offset a scalar, one buffer resource per query head (rows past Sq
  // land as zeros); the loop below is unrolled over the ring, so LDS addresses are immediates
  auto issue_to = [&](int it, char* buf) {
    const int hq = hk * grp + it / ntq;
    const int q0 = q_begin + (it % ntq) * 64;
    const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(Q + (int64_t)b * Sq * qs + (int64_t)hq * D), 0, (int)(((int64_t)(Sq - 1) * qs + D) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(dO + (int64_t)b * Sq * os + (int64_t)hq * D), 0, (int)(((int64_t)(Sq - 1) * os + D) * 2), 0x00020000);
    qt.issue(qrs, (int)((int64_t)q0 * qs * 2), buf, w);
    gt2.issue(grs, (int)((int64_t)q0 * os * 2), buf + TILE, w);
    if (w == 0) {  // per-row stats, 4 bytes per lane (rows past Sq are masked in the math)
      const int q = min(q0 + lane, Sq - 1);
      const int64_t idx = ((int64_t)b * H + hq) * Sq + q;
      __builtin_amdgcn_global_load_lds((const void*)(LSE + idx),
                                       (__attribute__((address_space(3))) void*)(buf + 2 * TILE), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(DELTA + idx),
                                       (__attribute__((address_space(3))) void*)(buf + 2 * TILE + 256), 4, 0, 0);
    }
  };
  constexpr int PER_TILE = 2 * BTile<DP>::PPW;  // DMA instructions per tile per wave (+2 on wave 0)
#pragma unroll
  for (int i = 0; i < LOOK; ++i)
    if (i < total) issue_to(i, smem + i * BUFB);
  auto tile = [&](auto bufc, int it) {
    constexpr int BUF = decltype(bufc)::value;
    const int hq = hk * grp + it / ntq;
    const int q0 = q_begin + (it % ntq) * 64;
    const int bhq = b * H + hq;
    const DropKey dkey = drop_key(seed, (uint32_t)bhq);
    // tile `it` landed (up to LOOK-1 younger tiles may stay in flight), then publish to all
    // waves; wave 0 issues 2 extra DMAs per tile (the row stats)
    if (LOOK >= 3 && it + 2 < total) {
      if (w == 0) attn_wait_vmcnt<2 * (PER_TILE + 2)>(); else attn_wait_vmcnt<2 * PER_TILE>();
    } else if (LOOK >= 2 && it + 1 < total) {
      if (w == 0) attn_wait_vmcnt<PER_TILE + 2>(); else attn_wait_vmcnt<PER_TILE>();
    } else {
      attn_wait_vmcnt<0>();
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // the buffer of tile it-1 is free now: refill it with tile it+LOOK
    if (it + LOOK < total) issue_to(it + LOOK, smem + ((BUF + LOOK) % NBUF) * BUFB);
    const char* qb = smem + BUF * BUFB;
    const char* gb = qb + TILE;
    const float* ls = reinterpret_cast<const float*>(qb + 2 * TILE);
    const float* dl = ls + 64;
    const bool skip = CAUSAL && (k0 + 32 * w > q0 + 63 + shift);  // all of this wave's keys masked
    if (!skip) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // S[q][key] = Q K^T, dP[q][key] = dO V^T   (query rows u*32.. in registers, key on lane)
        f32x16 sacc = {}, pacc = {};
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) {
          const bf16x8 aq = *reinterpret_cast<const bf16x8*>(qb + roff[s] + u * 32 * DP * 2);
          const bf16x8 ag = *reinterpret_cast<const bf16x8*>(gb + roff[s] + u * 32 * DP * 2);
          sacc = mfma32(aq, kf[s], sacc);
          pacc = mfma32(ag, vf[s], pacc);
        }
        f32x16 pm, ds;
        // per-row stats: rows 32u + 8g + 4hl + 0..3 are contiguous -> one 16-byte LDS read
        float4 lsv[4], dlv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          lsv[g] = *reinterpret_cast<const float4*>(ls + 32 * u + 8 * g + 4 * hl);
          dlv[g] = *reinterpret_cast<const float4*>(dl + 32 * u + 8 * g + 4 * hl);
        }
        // masks only where needed: the causal diagonal and query rows past Sq (their
        // stats were clamped); keys past Sk only feed their own unwritten outputs
        const bool edge = (q0 + 64 > Sq) || (CAUSAL && (k0 + 32 * w + 31 > q0 + 32 * u + shift));
        // the element math twice, masked and unmasked, behind one wave-uniform branch: as a
        // per-element select the mask's index compares and cndmasks were issued on every
        // tile (~half of the loop's VALU, profiles/r2_attention_pmc_counters.json)
        // dropout keep bits first (only the mask stays live across the hashes)
        uint32_t keep = 0xffffu;
        if (DROP) {
          keep = 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const uint32_t q = (uint32_t)(q0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hl);
            keep |= (hash_lo(dkey, q * (uint32_t)Sk + (uint32_t)key) >= dthr ? 1u : 0u) << r;
          }
        }
        auto elems = [&](auto masked) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qr = 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hl;
            const int q = q0 + qr;
            const float lv = (&lsv[r >> 2].x)[r & 3], dv_ = (&dlv[r >> 2].x)[r & 3];
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], c, -lv));
            if constexpr (decltype(masked)::value) {
              if (q >= Sq || (CAUSAL && key > q + shift)) p = 0.f;
            }
            float dpv = pacc[r];
            float pd = p;
            if (DROP) {
              const float msk = (keep >> r) & 1u ? dinv : 0.f;
              pd = p * msk;
              dpv = dpv * msk;
            }
            pm[r] = pd;                      // dropped P for dV
            ds[r] = p * (dpv - dv_);         // dS
          }
        };
        if (edge) elems(std::true_type{});
        else elems(std::false_type{});
        // dV^T += dO^T P ;  dK^T += Q^T dS     (A via transposed LDS reads of the row images)
        const bf16x8 pb0 = pack8(pm, 0), pb1 = pack8(pm, 1);
        const bf16x8 db0 = pack8(ds, 0), db1 = pack8(ds, 1);
#pragma unroll
        for (int d = 0; d < DP / 32; ++d) {
          auto tr = [&](const char* img, int jp, int m) {
            return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4*)(img + troff[d][jp] + u * 32 * DP * 2 + 16 * DP * 2 * m));
          };
          dv[d] = mfma32(cat44(tr(gb, 0, 0), tr(gb, 1, 0)), pb0, dv[d]);
          dv[d] = mfma32(cat44(tr(gb, 0, 1), tr(gb, 1, 1)), pb1, dv[d]);
          dk[d] = mfma32(cat44(tr(qb, 0, 0), tr(qb, 1, 0)), db0, dk[d]);
          dk[d] = mfma32(cat44(tr(qb, 0, 1), tr(qb, 1, 1)), db1, dk[d]);
        }
      }
    }
  };
  for (int t0 = 0; t0 < total; t0 += NBUF) {
    tile(std::integral_constant<int, 0>{}, t0);
    if (t0 + 1 < total) tile(std::integral_constant<int, 1>{}, t0 + 1);
    if (t0 + 2 < total) tile(std::integral_constant<int, 2>{}, t0 + 2);
    if (t0 + 3 < total) tile(std::integral_constant<int, 3>{}, t0 + 3);
  }
  // ---- fused bias-gradient column sums of dK (scaled) and dV
  if (CSK != nullptr) {
    __syncthreads();   // the Q / dO ring is free
    float* red = reinterpret_cast<float*>(smem);
    wg_colsum_atomic<DP>(dk, scale, kvalid, red, CSK + (int64_t)hk * D, D);
    __syncthreads();
    wg_colsum_atomic<DP>(dv, 1.f, kvalid, red, CSV + (int64_t)hk * D, D);
  }
  // ---- epilogue: lane = key, registers = d
  if (kvalid) {
    bf16_t* dkrow = dK + ((int64_t)b * Sk + key) * dks + (int64_t)hk * D;
    bf16_t* dvrow = dV + ((int64_t)b * Sk + key) * dvs + (int64_t)hk * D;
#pragma unroll
    for (int d = 0; d < DP / 32; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * d + 8 * g + 4 * hl;
        if (col < D) {
          u16x4 a, bb;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[e] = f2bf(dk[d][4 * g + e] * scale);
            bb[e] = f2bf(dv[d][4 * g + e]);
          }
          *reinterpret_cast<u16x4*>(dkrow + col) = a;
          *reinterpret_cast<u16x4*>(dvrow + col) = bb;
        }
      }
    }
  }
  }
}
