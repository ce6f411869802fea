// The forward kernels of attention.hip (structure: the header comment there): v1
// (attn_fwd_kernel, every head dim), the key-split kernel of short non-causal problems
// (attn_fwd_ks2_kernel) and v2 (attn_fwd2_kernel, the default at d_h <= 64).  Which one a
// problem runs: mp_attn_plan.h.
#pragma once
#include "mp_attn_common.h"

// ==========================================================================================
// forward
// ==========================================================================================
template <int DP, bool CAUSAL, bool DROP>
__global__ void __launch_bounds__(256, DP <= 128 ? 2 : 1) attn_fwd_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs,
    int64_t os, float scale, float p_drop, uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;  // bytes per [64][DP] tile
#define kbuf(i) (smem + (i) * TILE)
#define vbuf(i) (smem + (2 + (i)) * TILE)

  const int nmb = (Sq + 127) / 128;
  // causal: longest-first over the WHOLE grid (workgroups are dispatched in linear id
  // order): every (b, h)'s last query block, then the second to last, ...  Heavy-first
  // within each (b, h) row only interleaved heavy and light blocks and left a tail of
  // late heavy blocks -- causal took as long as full attention at S = 1024
  const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
  const int nbh = (int)gridDim.y;
  const int mb = CAUSAL ? (nmb - 1 - lin / nbh) : (int)blockIdx.x;
  const int bh = CAUSAL ? lin % nbh : (int)blockIdx.y;
  const int b = bh / H, h = bh % H, hk = h / (H / Hkv);
  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: scalar branches
  const int m0 = mb * 128;
  const int qrow = m0 + 32 * w + l32;  // this lane's query
  const bool qvalid = qrow < Sq;
  const bf16_t* Qb = Q + (int64_t)b * Sq * qs + (int64_t)h * D;
  const bf16_t* Kb = K + (int64_t)b * Sk * ks + (int64_t)hk * D;
  const bf16_t* Vb = V + (int64_t)b * Sk * vs + (int64_t)hk * D;

  // Q as the B operand of S^T = K Q^T: lane holds Q[qrow][16s + 8hl + j]
  bf16x8 qf[DP / 16];
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    u16x8 t = gload8(Qb + (int64_t)qrow * qs, 16 * s + 8 * hl, D, qvalid);
    qf[s] = __builtin_bit_cast(bf16x8, t);
  }
  const float c = scale * LOG2E;
  // dropout stream of this (b, h): keys once, 32-bit index q * Sk + key (drop_idx's low word)
  const DropKey dkey = drop_key(seed, (uint32_t)bh);
  const uint32_t dthr = drop_thr(p_drop), qoff = (uint32_t)qrow * (uint32_t)Sk;
  const float dinv = 1.0f / (1.0f - p_drop);
  f32x16 o[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) o[d] = {};
  float m_run = -INFINITY, l_run = 0.f;

  // causal alignment: query i may attend keys <= i + (Sk - Sq)
  const int shift = Sk - Sq;
  int n_end = Sk;
  if (CAUSAL) n_end = min(Sk, m0 + 128 + shift);
  const int ntiles = (n_end + 63) / 64;

  Stage64<DP> kst, vst;
  kst.load(Kb, ks, 0, Sk, D);
  vst.load(Vb, vs, 0, Sk, D);
  kst.store(kbuf(0));
  vst.store(vbuf(0));
  const int wave_last_q = m0 + 32 * w + 31 + shift;

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const int n0 = t * 64;
    if (t + 1 < ntiles) {
      kst.load(Kb, ks, n0 + 64, Sk, D);
      vst.load(Vb, vs, n0 + 64, Sk, D);
    }
    __syncthreads();
    const bool skip = CAUSAL && n0 > wave_last_q;
    if (!skip) {
      const char* kb = kbuf(cur);
      const char* vb = vbuf(cur);
      // ---- S^T = K Q^T (two 32-key sub tiles)
      f32x16 s0 = {}, s1 = {};
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        bf16x8 a0 = lds_row8<DP>(kb, l32, 2 * s + hl);
        bf16x8 a1 = lds_row8<DP>(kb, 32 + l32, 2 * s + hl);
        s0 = mfma32(a0, qf[s], s0);
        s1 = mfma32(a1, qf[s], s1);
      }
      // ---- mask (only tiles that cross the causal diagonal or the key end), tile max on
      // raw scores; p = 2^(s*c - m) is one v_fma + one v_exp (scale folded, log2 units)
      const bool edge = (n0 + 64 > Sk) || (CAUSAL && n0 + 63 > m0 + 32 * w + shift);
      if (edge) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = (r & 3) + 8 * (r >> 2) + 4 * hl;
          const int ka = n0 + kr, kb2 = n0 + 32 + kr;
          if (ka >= Sk || (CAUSAL && ka > qrow + shift)) s0[r] = -INFINITY;
          if (kb2 >= Sk || (CAUSAL && kb2 > qrow + shift)) s1[r] = -INFINITY;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = max3_raw(mx, s0[r], s1[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx * c);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
      // dropout: the 32 keep bits of this lane's scores first (only the bit mask stays live
      // across the hashes: computed beside the probabilities the DP = 128 build spilled)
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
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], c, -m_use));
        float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], c, -m_use));
        rs += p0 + p1;
        if (DROP) {
          p0 = (keep >> r) & 1u ? p0 * dinv : 0.f;
          p1 = (keep >> (16 + r)) & 1u ? p1 * dinv : 0.f;
        }
        s0[r] = p0;
        s1[r] = p1;
      }
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run * alpha + rs;
      m_run = m_new;
#pragma unroll
      for (int d = 0; d < DP / 32; ++d) o[d] *= alpha;
      // ---- O^T += V^T P^T
      const bf16x8 p00 = pack8(s0, 0), p01 = pack8(s0, 1), p10 = pack8(s1, 0), p11 = pack8(s1, 1);
#pragma unroll
      for (int d = 0; d < DP / 32; ++d) {
        const int c0 = 32 * d + 16 * ((lane >> 4) & 1);
        bf16x8 a;
        a = cat44(lds_tr4<DP>(vb, 0 + 4 * hl, c0), lds_tr4<DP>(vb, 8 + 4 * hl, c0));
        o[d] = mfma32(a, p00, o[d]);
        a = cat44(lds_tr4<DP>(vb, 16 + 4 * hl, c0), lds_tr4<DP>(vb, 24 + 4 * hl, c0));
        o[d] = mfma32(a, p01, o[d]);
        a = cat44(lds_tr4<DP>(vb, 32 + 4 * hl, c0), lds_tr4<DP>(vb, 40 + 4 * hl, c0));
        o[d] = mfma32(a, p10, o[d]);
        a = cat44(lds_tr4<DP>(vb, 48 + 4 * hl, c0), lds_tr4<DP>(vb, 56 + 4 * hl, c0));
        o[d] = mfma32(a, p11, o[d]);
      }
    }
    if (t + 1 < ntiles) {
      kst.store(kbuf(cur ^ 1));
      vst.store(vbuf(cur ^ 1));
    }
  }
  // ---- epilogue: O = O^T / l ; LSE
  if (qvalid) {
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    bf16_t* orow = O + ((int64_t)b * Sq + qrow) * os + (int64_t)h * D;
#pragma unroll
    for (int d = 0; d < DP / 32; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * d + 8 * g + 4 * hl;
        if (col < D) {
          u16x4 pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = f2bf(o[d][4 * g + e] * inv);
          *reinterpret_cast<u16x4*>(orow + col) = pk;
        }
      }
    }
    if (hl == 0) LSE[(int64_t)bh * Sq + qrow] = l_run > 0.f ? m_run + log2f(l_run) : INFINITY;
  }
#undef kbuf
#undef vbuf
}

// ==========================================================================================
// forward, short sequences: workgroup = 64 queries, keys split over two wave pairs
// ==========================================================================================
// At the reference's shape (B 8, S 128, non-causal, 4-12 heads) the 128-query workgroups
// above are 32-96 for 256 CUs and every wave walks both 64-key tiles back to back.  Here
// a workgroup owns 64 queries: waves (qs = w & 1: which 32 queries, kh = w >> 1: which key
// tiles -- kh, kh + 2, ...).  Each wave pair streams its own K/V tiles into the same
// swizzled image by LDS-DMA (no staging registers), keeps its own online-softmax state,
// and the kh = 1 waves hand (O^T, m, l) to their kh = 0 partners through LDS at the end:
// twice the workgroups, half the serial tile chain per wave.  Non-causal only.
template <int DP, bool DROP>
__global__ void __launch_bounds__(256, 2) attn_fwd_ks2_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs,
    int64_t os, float scale, float p_drop, uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
  const int bh = (int)blockIdx.y;
  const int b = bh / H, h = bh % H, hk = h / (H / Hkv);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, l32 = lane & 31;
  const int qsub = w & 1, kh = w >> 1;
  const int ntiles = (Sk + 63) / 64;
  const int niter = (ntiles + 1) / 2;   // the same trip count in both pairs (barriers inside)
  // this pair's K / V tiles: double-buffered when it walks more than one tile (S = 128:
  // one tile per pair, 64 KB of LDS in all, as much as the 128-query kernel)
  const int nbuf = niter > 1 ? 2 : 1;
  char* gbase = smem + kh * 2 * nbuf * TILE;
#define kbuf2(i) (gbase + (i) * TILE)
#define vbuf2(i) (gbase + (nbuf + (i)) * TILE)
  const int m0 = (int)blockIdx.x * 64;
  const int qrow = m0 + 32 * qsub + l32;
  const bool qvalid = qrow < Sq;
  const bf16_t* Qb = Q + (int64_t)b * Sq * qs + (int64_t)h * D;
  const bf16_t* Kb = K + (int64_t)b * Sk * ks + (int64_t)hk * D;
  const bf16_t* Vb = V + (int64_t)b * Sk * vs + (int64_t)hk * D;
  bf16x8 qf[DP / 16];
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    u16x8 t = gload8(Qb + (int64_t)qrow * qs, 16 * s + 8 * hl, D, qvalid);
    qf[s] = __builtin_bit_cast(bf16x8, t);
  }
  const float c = scale * LOG2E;
  const DropKey dkey = drop_key(seed, (uint32_t)bh);
  const uint32_t dthr = drop_thr(p_drop), qoff = (uint32_t)qrow * (uint32_t)Sk;
  const float dinv = 1.0f / (1.0f - p_drop);
  f32x16 o[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) o[d] = {};
  float m_run = -INFINITY, l_run = 0.f;
  GTileP<DP> gp;
  gp.init();
  const int wv = __builtin_amdgcn_readfirstlane(qsub);
  gp.issue(Kb, ks, 64 * kh, Sk, D, kbuf2(0), wv);
  gp.issue(Vb, vs, 64 * kh, Sk, D, vbuf2(0), wv);
  for (int it = 0; it < niter; ++it) {
    const int cur = it & 1;
    const int n0 = 64 * (2 * it + kh);
    __syncthreads();   // (waits for this wave's LDS-DMA first: tile `it` is in LDS for the pair)
    if (it + 1 < niter) {   // the next tile into the buffer the pair finished before this barrier
      gp.issue(Kb, ks, n0 + 128, Sk, D, kbuf2(cur ^ 1), wv);
      gp.issue(Vb, vs, n0 + 128, Sk, D, vbuf2(cur ^ 1), wv);
    }
    if (n0 < Sk) {
      const char* kb = kbuf2(cur);
      const char* vb = vbuf2(cur);
      f32x16 s0 = {}, s1 = {};
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        bf16x8 a0 = lds_row8<DP>(kb, l32, 2 * s + hl);
        bf16x8 a1 = lds_row8<DP>(kb, 32 + l32, 2 * s + hl);
        s0 = mfma32(a0, qf[s], s0);
        s1 = mfma32(a1, qf[s], s1);
      }
      if (n0 + 64 > Sk) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = (r & 3) + 8 * (r >> 2) + 4 * hl;
          if (n0 + kr >= Sk) s0[r] = -INFINITY;
          if (n0 + 32 + kr >= Sk) s1[r] = -INFINITY;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = max3_raw(mx, s0[r], s1[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx * c);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
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
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], c, -m_use));
        float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], c, -m_use));
        rs += p0 + p1;
        if (DROP) {
          p0 = (keep >> r) & 1u ? p0 * dinv : 0.f;
          p1 = (keep >> (16 + r)) & 1u ? p1 * dinv : 0.f;
        }
        s0[r] = p0;
        s1[r] = p1;
      }
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run * alpha + rs;
      m_run = m_new;
#pragma unroll
      for (int d = 0; d < DP / 32; ++d) o[d] *= alpha;
      const bf16x8 p00 = pack8(s0, 0), p01 = pack8(s0, 1), p10 = pack8(s1, 0), p11 = pack8(s1, 1);
#pragma unroll
      for (int d = 0; d < DP / 32; ++d) {
        const int c0 = 32 * d + 16 * ((lane >> 4) & 1);
        bf16x8 a;
        a = cat44(lds_tr4<DP>(vb, 0 + 4 * hl, c0), lds_tr4<DP>(vb, 8 + 4 * hl, c0));
        o[d] = mfma32(a, p00, o[d]);
        a = cat44(lds_tr4<DP>(vb, 16 + 4 * hl, c0), lds_tr4<DP>(vb, 24 + 4 * hl, c0));
        o[d] = mfma32(a, p01, o[d]);
        a = cat44(lds_tr4<DP>(vb, 32 + 4 * hl, c0), lds_tr4<DP>(vb, 40 + 4 * hl, c0));
        o[d] = mfma32(a, p10, o[d]);
        a = cat44(lds_tr4<DP>(vb, 48 + 4 * hl, c0), lds_tr4<DP>(vb, 56 + 4 * hl, c0));
        o[d] = mfma32(a, p11, o[d]);
      }
    }
  }
#undef kbuf2
#undef vbuf2
  // the kh = 1 pair hands (O^T, m, l) to the kh = 0 pair
  __syncthreads();
  float* xo = reinterpret_cast<float*>(smem) + qsub * (DP / 32 * 16 * 64 + 128);
  if (kh == 1) {
#pragma unroll
    for (int d = 0; d < DP / 32; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) xo[(d * 16 + r) * 64 + lane] = o[d][r];
    xo[DP / 32 * 16 * 64 + lane] = m_run;
    xo[DP / 32 * 16 * 64 + 64 + lane] = l_run;
  }
  __syncthreads();
  if (kh == 1) return;
  const float m1 = xo[DP / 32 * 16 * 64 + lane], l1 = xo[DP / 32 * 16 * 64 + 64 + lane];
  const float mm = fmaxf(m_run, m1);
  const float mu = mm == -INFINITY ? 0.f : mm;
  const float a0 = __builtin_amdgcn_exp2f(m_run - mu), a1 = __builtin_amdgcn_exp2f(m1 - mu);
  const float l = l_run * a0 + l1 * a1;
#pragma unroll
  for (int d = 0; d < DP / 32; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = o[d][r] * a0 + xo[(d * 16 + r) * 64 + lane] * a1;
  if (qvalid) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    bf16_t* orow = O + ((int64_t)b * Sq + qrow) * os + (int64_t)h * D;
#pragma unroll
    for (int d = 0; d < DP / 32; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = 32 * d + 8 * g + 4 * hl;
        if (col < D) {
          u16x4 pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = f2bf(o[d][4 * g + e] * inv);
          *reinterpret_cast<u16x4*>(orow + col) = pk;
        }
      }
    }
    if (hl == 0) LSE[(int64_t)bh * Sq + qrow] = l > 0.f ? mm + log2f(l) : INFINITY;
  }
}

// ==========================================================================================
// forward v2: paired query blocks, LDS-DMA K/V ring, lazy rescale (the default at d_h 64)
// ==========================================================================================
// Same tile structure as attn_fwd_kernel (4 waves x 32 queries, 64-key tiles, swapped
// S^T = K Q^T with P^T kept in registers), with the per-tile VALU cut and the grid reshaped
// (the forward issued ~18 VALU per MFMA at 0.26 MFMA busy, profiles/r5_attention_pmc.md):
//   * K/V tiles stream through a 3-deep LDS ring by buffer-load-to-LDS DMA (GTile's piece
//     layout; 32-bit per-lane offsets fixed at entry + a scalar per-tile offset; rows past
//     the key end read as zero): two tiles in flight, counted vmcnt, one raw barrier per tile.  v1 staged one
//     tile ahead through registers, so every tile waited out a full load latency (v1 -> v2
//     with register staging kept: 2-4 %; the dQ kernel, on the ring, ran 1.5x v1's MFMA
//     work per tile in less time).
//   * causal / key-end mask: one compare against a per-lane limit and one select per score
//     (the key's in-tile position is a compile-time constant per accumulator register).
//   * cross-half max / sum by v_permlane32_swap instead of an LDS bpermute.
//   * lazy rescale: the subtracted row maximum moves only when a lane's tile maximum exceeds
//     it by more than 2^8 (wave-uniform branch); otherwise O and l are not rescaled (P stays
//     <= 2^8, exact in f32 sums and bf16 products).
//   * causal: one workgroup runs query block nmb-1-p and then block p of the same (b, h), so
//     every workgroup does the same number of tiles (no heavy-first tail); the pairs of one
//     (b, h) sit on one XCD (workgroup id mod 8) next to each other, so their K/V tiles are
//     read while the others still hold them in that XCD's L2.
template <int DP, bool CAUSAL, bool DROP>
__global__ void __launch_bounds__(256, DROP ? 2 : (MP_FWD_NBUF == 2 ? 4 : 3)) attn_fwd2_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs,
    int64_t os, float scale, float p_drop, uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
  constexpr float TAU = 8.f;   // lazy-rescale threshold (log2 units)
  const int nmb = (Sq + 127) / 128;
  const int npair = CAUSAL ? (nmb + 1) / 2 : nmb;   // workgroups per (b, h)
  const int nbh = B * H;
  // workgroup -> (bh, p): the npair workgroups of one bh are consecutive on one XCD
  const int lin = (int)blockIdx.x;
  int bh, p;
  if ((nbh & 7) == 0) {
    const int xcd = lin & 7, j = lin >> 3;
    bh = (j / npair) * 8 + xcd;
    p = j % npair;
  } else {
    bh = lin / npair;
    p = lin % npair;
  }
  const int b = bh / H, h = bh % H, hk = h / (H / Hkv);
  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bf16_t* Qb = Q + (int64_t)b * Sq * qs + (int64_t)h * D;
  // range: through the last valid row's head slice (the launcher keeps it below 2^31)
  const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(K + (int64_t)b * Sk * ks + (int64_t)hk * D), 0, (int)(((int64_t)(Sk - 1) * ks + D) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(V + (int64_t)b * Sk * vs + (int64_t)hk * D), 0, (int)(((int64_t)(Sk - 1) * vs + D) * 2), 0x00020000);
  // K / V ring: NBUF buffers of (K tile, V tile), LOOK tiles in flight
  // ring depth (build-time A/B, MP_FWD_NBUF): 2 = 32 KB of LDS, 4 workgroups per CU (B 64:
  // 190 vs 200 us at 3 = 48 KB, 3 per CU; profiles/r6_attention_v2.md)
  constexpr int NBUF = MP_FWD_NBUF, LOOK = NBUF - 1, BUFB = 2 * TILE;
  static_assert(NBUF == 2 || NBUF == 3, "the tile loop below is unrolled by NBUF");
  constexpr int PER_TILE = 2 * BTile<DP>::PPW;   // DMA instructions per tile per wave
  BTile<DP> kt, vt;
  kt.init(ks, D, w);
  vt.init(vs, D, w);
  const int kstep = (int)(64 * ks * 2), vstep = (int)(64 * vs * 2);
  // per-lane LDS byte offsets of the fragment reads inside a tile (swizzle included; the rows
  // a lane reads 32 / 16 apart share the swizzle, so the rest are immediate offsets):
  //   K rows l32 (+32: +4096) at chunk 2s + hl;  V^T transposed reads of rows 8j + 4hl + q
  //   at column 32d + 16 (lane>>4 & 1) + 4p: j = jp + 2m is voff[d][jp] + 2048 m
  int koff[DP / 16], vtoff[DP / 32][2];
  {
    const int i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) koff[s] = lds_off<DP>(l32, 2 * s + hl);
#pragma unroll
    for (int d = 0; d < DP / 32; ++d)
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int row = 8 * jp + 4 * hl + q, col = 32 * d + 16 * ((lane >> 4) & 1) + 4 * pp;
        vtoff[d][jp] = lds_off<DP>(row, col >> 3) + ((col & 7) << 1);
      }
  }
  auto issue = [&](int t) {
    char* buf = smem + (t % NBUF) * BUFB;
    kt.issue(krs, t * kstep, buf, w);
    vt.issue(vrs, t * vstep, buf + TILE, w);
  };
  const float c = scale * LOG2E;
  const DropKey dkey = drop_key(seed, (uint32_t)bh);
  const uint32_t dthr = drop_thr(p_drop);
  const float dinv = 1.0f / (1.0f - p_drop);
  const int shift = Sk - Sq;
  const u16x8 ones_u = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};   // bf16 1.0
  const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_u);
  const int npass = CAUSAL && (nmb - 1 - p) != p ? 2 : 1;

  for (int pass = 0; pass < npass; ++pass) {
    const int mb = CAUSAL ? (pass == 0 ? nmb - 1 - p : p) : p;
    const int m0 = mb * 128;
    const int qrow = m0 + 32 * w + l32;
    const bool qvalid = qrow < Sq;
    bf16x8 qf[DP / 16];
#pragma unroll
    for (int s = 0; s < DP / 16; ++s)
      qf[s] = __builtin_bit_cast(bf16x8, gload8(Qb + (int64_t)qrow * qs, 16 * s + 8 * hl, D, qvalid));
    const uint32_t qoff = (uint32_t)qrow * (uint32_t)Sk;
    f32x16 o[DP / 32];
#pragma unroll
    for (int d = 0; d < DP / 32; ++d) o[d] = {};
    float m_run = -INFINITY;   // running maximum (log2 units) ...
    float m_sub = 0.f;         // ... and the finite value the probabilities subtract
    f32x16 lsum = {};          // running row sum (every register: this lane's query) ...
    float l_drop = 0.f;        // ... or, with dropout, the pre-mask sum on the VALU
    int n_end = Sk;
    if (CAUSAL) n_end = min(Sk, m0 + 128 + shift);
    const int ntiles = n_end > 0 ? (n_end + 63) / 64 : 0;
    const int wave_last_q = m0 + 32 * w + 31 + shift;
    // per-lane mask limit: a key of in-tile offset k (+4 hl) is kept iff k <= lim - n0
    const int lim0 = (CAUSAL ? min(qrow + shift, Sk - 1) : Sk - 1) - 4 * hl;

    if (pass > 0) {   // every wave has read the previous pass's last tiles
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int i = 0; i < LOOK; ++i)
      if (i < ntiles) issue(i);
    // one tile on ring buffer BUF (a compile-time constant: every LDS address of the tile is
    // an immediate offset, and the refill target (BUF + LOOK) % NBUF too)
    auto tile = [&](auto bufc, int t) {
      constexpr int BUF = decltype(bufc)::value;
      const int n0 = t * 64;
      // tile t landed (the younger one may stay in flight), then publish it to all waves
      if (LOOK >= 2 && t + 1 < ntiles) attn_wait_vmcnt<PER_TILE>();
      else attn_wait_vmcnt<0>();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // every wave is done with tile t-1: its buffer takes tile t+LOOK
      if (t + LOOK < ntiles) {
        char* buf = smem + ((BUF + LOOK) % NBUF) * BUFB;
        kt.issue(krs, (t + LOOK) * kstep, buf, w);
        vt.issue(vrs, (t + LOOK) * vstep, buf + TILE, w);
      }
      const bool skip = CAUSAL && n0 > wave_last_q;
      if (!skip) {
        const char* kb = smem + BUF * BUFB;
        const char* vb = kb + TILE;
        f32x16 s0 = {}, s1 = {};
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) {
          const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(kb + koff[s]);
          const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(kb + koff[s] + 32 * DP * 2);
          s0 = mfma32(a0, qf[s], s0);
          s1 = mfma32(a1, qf[s], s1);
        }
        const bool edge = (n0 + 64 > Sk) || (CAUSAL && n0 + 63 > m0 + 32 * w + shift);
        if (edge) {
          const int lim = lim0 - n0;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            s0[r] = key_of(r) > lim ? -INFINITY : s0[r];
            s1[r] = key_of(r) + 32 > lim ? -INFINITY : s1[r];
          }
        }
        float mx = tile_max32(s0, s1);
        mx = xhalf_max(mx);
        const float mxc = mx * c;
        // lazy rescale: wave-uniform, taken on the first tile and when a maximum jumps
        if (__builtin_amdgcn_ballot_w64(mxc > m_run + TAU)) {
          const float m_new = fmaxf(m_run, mxc);
          const float s_new = m_new == -INFINITY ? 0.f : m_new;
          const float alpha = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_sub - s_new);
#pragma unroll
          for (int d = 0; d < DP / 32; ++d) o[d] *= alpha;
          lsum *= alpha;
          l_drop *= alpha;
          m_run = m_new;
          m_sub = s_new;
        }
        uint32_t keep = 0xffffffffu;
        if (DROP) {
          keep = 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const uint32_t kr = (uint32_t)(n0 + key_of(r) + 4 * hl);
            keep |= (hash_lo(dkey, qoff + kr) >= dthr ? 1u : 0u) << r;
            keep |= (hash_lo(dkey, qoff + kr + 32u) >= dthr ? 1u : 0u) << (16 + r);
          }
        }
        float rs0 = 0.f, rs1 = 0.f;   // dropout: the normaliser sums P BEFORE the mask
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], c, -m_sub));
          float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], c, -m_sub));
          if (DROP) {
            rs0 += p0;
            rs1 += p1;
            p0 = (keep >> r) & 1u ? p0 * dinv : 0.f;
            p1 = (keep >> (16 + r)) & 1u ? p1 * dinv : 0.f;
          }
          s0[r] = p0;
          s1[r] = p1;
        }
        const bf16x8 p00 = pack8(s0, 0), p01 = pack8(s0, 1), p10 = pack8(s1, 0), p11 = pack8(s1, 1);
        if constexpr (DROP) {
          l_drop += xhalf_sum(rs0 + rs1);
        } else {
          // row sums on the matrix cores: ones^T . P^T puts sum_k P[q][k] (of the bf16 P that
          // the PV product uses) in every register of lane q -- 4 MFMAs in place of 32 adds
          // and a cross-half exchange on the VALU, which is the busier pipe here
          lsum = mfma32(ones, p00, lsum);
          lsum = mfma32(ones, p01, lsum);
          lsum = mfma32(ones, p10, lsum);
          lsum = mfma32(ones, p11, lsum);
        }
#pragma unroll
        for (int d = 0; d < DP / 32; ++d) {
          auto tr = [&](int jp, int m) {
            return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4*)(vb + vtoff[d][jp] + 16 * DP * 2 * m));
          };
          o[d] = mfma32(cat44(tr(0, 0), tr(1, 0)), p00, o[d]);
          o[d] = mfma32(cat44(tr(0, 1), tr(1, 1)), p01, o[d]);
          o[d] = mfma32(cat44(tr(0, 2), tr(1, 2)), p10, o[d]);
          o[d] = mfma32(cat44(tr(0, 3), tr(1, 3)), p11, o[d]);
        }
      }
    };
    for (int t0 = 0; t0 < ntiles; t0 += NBUF) {
      tile(std::integral_constant<int, 0>{}, t0);
      if (t0 + 1 < ntiles) tile(std::integral_constant<int, 1>{}, t0 + 1);
      if constexpr (NBUF == 3)
        if (t0 + 2 < ntiles) tile(std::integral_constant<int, 2 % NBUF>{}, t0 + 2);
    }
    const float l_run = DROP ? l_drop : lsum[0];
    if (qvalid) {
      const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
      bf16_t* orow = O + ((int64_t)b * Sq + qrow) * os + (int64_t)h * D;
#pragma unroll
      for (int d = 0; d < DP / 32; ++d) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = 32 * d + 8 * g + 4 * hl;
          if (col < D) {
            u16x4 pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[e] = f2bf(o[d][4 * g + e] * inv);
            *reinterpret_cast<u16x4*>(orow + col) = pk;
          }
        }
      }
      if (hl == 0) LSE[(int64_t)bh * Sq + qrow] = l_run > 0.f ? m_sub + log2f(l_run) : INFINITY;
    }
  }
}
