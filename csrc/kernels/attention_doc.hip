// Document-masked causal flash attention for packed sequences (bf16, gfx950), forward and
// backward, plus the kernel that derives the document bounds from the tokens.
//
// A row of S tokens holds several documents.  Two int32 arrays of B*S entries, token-major:
// doc_start[b*S + i] / doc_end[b*S + i] are the positions, inside sequence b, of the first /
// last token of the document that holds position i.  Key j is visible to query i iff
//   doc_start[i] <= j <= i      (forward, dQ: query on the lane)
//   j <= i <= doc_end[j]        (dK/dV: key on the lane)
//
// The three kernels have the structure of attention.hip's v1 kernels (128 queries or keys per
// workgroup, 64-row tiles, swapped QK^T, LSE in log2 units, delta written by dQ and read by
// dK/dV) with a register-staged two-buffer LDS ring.  The tile loops start and end at the
// documents of the block, read from the device arrays inside the kernel: nothing about the
// boundaries reaches the host or the grid, so a captured graph replays with new boundaries.
// Every bound is clamped as it is loaded (doc_start[i] into [0, i], doc_end[j] into
// [j, S-1]): array contents can change results, never an address.  No atomics.
#include "mp_api.h"
#include "mp_attn_tiles.h"

#include <type_traits>

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ==========================================================================================
// forward: workgroup = 128 queries of one (b, h)
// ==========================================================================================
template <int DP>
__global__ void __launch_bounds__(256, 2) attn_doc_fwd_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
    float* __restrict__ LSE, const int* __restrict__ DS, int B, int S, int H, int Hkv, int D, int64_t qs, int64_t ks,
    int64_t vs, int64_t os, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;  // bytes per [64][DP] tile
#define kbuf(i) (smem + (i) * TILE)
#define vbuf(i) (smem + (2 + (i)) * TILE)
  const int nmb = (S + 127) / 128;
  // longest-first over the whole grid, as the causal v1 kernel
  const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
  const int nbh = (int)gridDim.y;
  const int mb = nmb - 1 - lin / nbh;
  const int bh = lin % nbh;
  const int b = bh / H, h = bh % H, hk = h / (H / Hkv);
  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int m0 = mb * 128;
  const int qrow = m0 + 32 * w + l32;  // this lane's query
  const bool qvalid = qrow < S;
  const bf16_t* Qb = Q + (int64_t)b * S * qs + (int64_t)h * D;
  const bf16_t* Kb = K + (int64_t)b * S * ks + (int64_t)hk * D;
  const bf16_t* Vb = V + (int64_t)b * S * vs + (int64_t)hk * D;
  const int* dsb = DS + (int64_t)b * S;

  // document bounds: this lane's, the block's minimum (its first query: doc_start is
  // non-decreasing) and the wave's first / last valid query (wave-uniform scalars)
  const int ds_q = qvalid ? clampi(dsb[qrow], 0, qrow) : qrow;
  const int t_begin = __builtin_amdgcn_readfirstlane(clampi(dsb[m0], 0, m0)) / 64;
  const int qw0 = m0 + 32 * w, qwl = min(qw0 + 31, S - 1);
  const bool wave_live = qw0 < S;
  const int ds_wfirst = wave_live ? __builtin_amdgcn_readfirstlane(clampi(dsb[qw0], 0, qw0)) : 0;
  const int ds_wlast = wave_live ? __builtin_amdgcn_readfirstlane(clampi(dsb[qwl], 0, qwl)) : 0;

  bf16x8 qf[DP / 16];
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    u16x8 t = gload8(Qb + (int64_t)qrow * qs, 16 * s + 8 * hl, D, qvalid);
    qf[s] = __builtin_bit_cast(bf16x8, t);
  }
  const float c = scale * LOG2E;
  f32x16 o[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) o[d] = {};
  float m_run = -INFINITY, l_run = 0.f;

  const int n_end = min(S, m0 + 128);
  const int ntiles = (n_end + 63) / 64;

  Stage64<DP> kst, vst;
  kst.load(Kb, ks, t_begin * 64, S, D);
  vst.load(Vb, vs, t_begin * 64, S, D);
  kst.store(kbuf(0));
  vst.store(vbuf(0));

  for (int t = t_begin; t < ntiles; ++t) {
    const int cur = (t - t_begin) & 1;
    const int n0 = t * 64;
    if (t + 1 < ntiles) {
      kst.load(Kb, ks, n0 + 64, S, D);
      vst.load(Vb, vs, n0 + 64, S, D);
    }
    __syncthreads();
    // the wave skips tiles above its causal diagonal and tiles that end below the document
    // of its first query
    const bool skip = !wave_live || n0 > qw0 + 31 || n0 + 63 < ds_wfirst;
    if (!skip) {
      const char* kb = kbuf(cur);
      const char* vb = vbuf(cur);
      f32x16 s0 = {}, s1 = {};
#pragma unroll
      for (int s = 0; s < DP / 16; ++s) {
        bf16x8 a0 = lds_row8<DP>(kb, l32, 2 * s + hl);
        bf16x8 a1 = lds_row8<DP>(kb, 32 + l32, 2 * s + hl);
        s0 = mfma32(a0, qf[s], s0);
        s1 = mfma32(a1, qf[s], s1);
      }
      // masks only on tiles that cross the key end, the causal diagonal or the document
      // start of the wave's last valid query (the largest doc_start of the wave)
      const bool edge = (n0 + 64 > S) || (n0 + 63 > qw0) || (n0 < ds_wlast);
      if (edge) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = (r & 3) + 8 * (r >> 2) + 4 * hl;
          const int ka = n0 + kr, kb2 = n0 + 32 + kr;
          if (ka >= S || ka > qrow || ka < ds_q) s0[r] = -INFINITY;
          if (kb2 >= S || kb2 > qrow || kb2 < ds_q) s1[r] = -INFINITY;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = max3_raw(mx, s0[r], s1[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx * c);
      // a lane can pass leading tiles in which it sees nothing: its running maximum is still
      // -inf, and 2^(-inf - 0) = 0 keeps l and O at zero
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], c, -m_use));
        const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], c, -m_use));
        rs += p0 + p1;
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
    if (t + 1 < ntiles) {
      kst.store(kbuf(cur ^ 1));
      vst.store(vbuf(cur ^ 1));
    }
  }
  if (qvalid) {
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    bf16_t* orow = O + ((int64_t)b * S + qrow) * os + (int64_t)h * D;
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
    if (hl == 0) LSE[(int64_t)bh * S + qrow] = l_run > 0.f ? m_run + log2f(l_run) : INFINITY;
  }
#undef kbuf
#undef vbuf
}

// ==========================================================================================
// backward dQ: workgroup = 128 queries of one (b, h) (forward structure); writes delta
// ==========================================================================================
template <int DP>
__global__ void __launch_bounds__(256, DP <= 64 ? 2 : 1) attn_doc_bwd_dq_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const bf16_t* __restrict__ O, const bf16_t* __restrict__ dO, const float* __restrict__ LSE,
    float* __restrict__ DELTA, bf16_t* __restrict__ dQ, const int* __restrict__ DS, int B, int S, int H, int Hkv,
    int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dqs, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
#define kbuf(i) (smem + (i) * TILE)
#define vbuf(i) (smem + (2 + (i)) * TILE)
  const int nmb = (S + 127) / 128;
  const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
  const int nbh = (int)gridDim.y;
  const int mb = nmb - 1 - lin / nbh;
  const int bh = lin % nbh;
  const int b = bh / H, h = bh % H, hk = h / (H / Hkv);
  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int m0 = mb * 128;
  const int qrow = m0 + 32 * w + l32;
  const bool qvalid = qrow < S;
  const bf16_t* Kb = K + (int64_t)b * S * ks + (int64_t)hk * D;
  const bf16_t* Vb = V + (int64_t)b * S * vs + (int64_t)hk * D;
  const int* dsb = DS + (int64_t)b * S;

  const int ds_q = qvalid ? clampi(dsb[qrow], 0, qrow) : qrow;
  const int t_begin = __builtin_amdgcn_readfirstlane(clampi(dsb[m0], 0, m0)) / 64;
  const int qw0 = m0 + 32 * w, qwl = min(qw0 + 31, S - 1);
  const bool wave_live = qw0 < S;
  const int ds_wfirst = wave_live ? __builtin_amdgcn_readfirstlane(clampi(dsb[qw0], 0, qw0)) : 0;
  const int ds_wlast = wave_live ? __builtin_amdgcn_readfirstlane(clampi(dsb[qwl], 0, qwl)) : 0;

  bf16x8 qf[DP / 16], gf[DP / 16];
  const bf16_t* Qrow = Q + ((int64_t)b * S + qrow) * qs + (int64_t)h * D;
  const bf16_t* Grow = dO + ((int64_t)b * S + qrow) * os + (int64_t)h * D;
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    qf[s] = __builtin_bit_cast(bf16x8, gload8(Qrow, 16 * s + 8 * hl, D, qvalid));
    gf[s] = __builtin_bit_cast(bf16x8, gload8(Grow, 16 * s + 8 * hl, D, qvalid));
  }
  const int64_t sidx = (int64_t)bh * S + qrow;
  const float lse = qvalid ? LSE[sidx] : INFINITY;
  // delta = rowsum(dO * O), fused here (each lane holds half of the row's d range)
  float dlt = 0.f;
  {
    const bf16_t* Orow = O + ((int64_t)b * S + qrow) * os + (int64_t)h * D;
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
  f32x16 dq[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) dq[d] = {};
  const int n_end = min(S, m0 + 128);
  const int ntiles = (n_end + 63) / 64;

  Stage64<DP> kst, vst;
  kst.load(Kb, ks, t_begin * 64, S, D);
  vst.load(Vb, vs, t_begin * 64, S, D);
  kst.store(kbuf(0));
  vst.store(vbuf(0));

  for (int t = t_begin; t < ntiles; ++t) {
    const int cur = (t - t_begin) & 1;
    const int n0 = t * 64;
    if (t + 1 < ntiles) {
      kst.load(Kb, ks, n0 + 64, S, D);
      vst.load(Vb, vs, n0 + 64, S, D);
    }
    __syncthreads();
    const bool skip = !wave_live || n0 > qw0 + 31 || n0 + 63 < ds_wfirst;
    if (!skip) {
      const char* kb = kbuf(cur);
      const char* vb = vbuf(cur);
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
      const bool edge = (n0 + 64 > S) || (n0 + 63 > qw0) || (n0 < ds_wlast);
      // masked / unmasked element math behind one wave-uniform branch; invalid query rows
      // have lse = +inf
      auto elems = [&](auto masked) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = (r & 3) + 8 * (r >> 2) + 4 * hl;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int kk = n0 + 32 * half + kr;
            const float sv = half ? s1[r] : s0[r];
            const float dpv = half ? p1[r] : p0[r];
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sv, c, -lse));
            float dsv = p * (dpv - dlt);
            if constexpr (decltype(masked)::value) {
              if (kk >= S || kk > qrow || kk < ds_q) dsv = 0.f;
            }
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
    if (t + 1 < ntiles) {
      kst.store(kbuf(cur ^ 1));
      vst.store(vbuf(cur ^ 1));
    }
  }
  if (qvalid) {
    bf16_t* drow = dQ + ((int64_t)b * S + qrow) * dqs + (int64_t)h * D;
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
#undef kbuf
#undef vbuf
}

// ==========================================================================================
// backward dK / dV: workgroup = 128 keys of one (b, kv-head), key on the MFMA lane; loops
// over the query heads of the group and the query tiles from the block's first key up to
// the document end of its last valid key
// ==========================================================================================
template <int DP>
__global__ void __launch_bounds__(256, DP <= 64 ? 2 : 1) attn_doc_bwd_dkdv_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const bf16_t* __restrict__ dO, const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16_t* __restrict__ dK, bf16_t* __restrict__ dV, const int* __restrict__ DE, int B, int S, int H, int Hkv, int D,
    int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dks, int64_t dvs, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = 64 * DP * 2;
  constexpr int BUFB = 2 * TILE + 512;  // Q, dO, lse[64], delta[64]
  // key block 0 has the longest query range when there is one document: longest-first
  const int lin = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
  const int kblk = lin / (int)gridDim.y;
  const int bhk = lin % (int)gridDim.y;
  const int b = bhk / Hkv, hk = bhk % Hkv;
  const int grp = H / Hkv;
  const int lane = threadIdx.x & 63, hl = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int k0 = kblk * 128;
  const int key = k0 + 32 * w + l32;  // this lane's key (MFMA column)
  const bool kvalid = key < S;
  const int* deb = DE + (int64_t)b * S;

  // document ends: this lane's, the block's maximum (its last valid key: doc_end is
  // non-decreasing) and the wave's first / last valid key
  const int de_k = kvalid ? clampi(deb[key], key, S - 1) : key;
  const int kl = min(k0 + 127, S - 1);
  const int de_blk = __builtin_amdgcn_readfirstlane(clampi(deb[kl], kl, S - 1));
  const int kw0 = k0 + 32 * w, kwl = min(kw0 + 31, S - 1);
  const bool wave_live = kw0 < S;
  const int de_wfirst = wave_live ? __builtin_amdgcn_readfirstlane(clampi(deb[kw0], kw0, S - 1)) : 0;
  const int de_wlast = wave_live ? __builtin_amdgcn_readfirstlane(clampi(deb[kwl], kwl, S - 1)) : 0;

  bf16x8 kf[DP / 16], vf[DP / 16];
  const bf16_t* Krow = K + ((int64_t)b * S + key) * ks + (int64_t)hk * D;
  const bf16_t* Vrow = V + ((int64_t)b * S + key) * vs + (int64_t)hk * D;
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
  const int q_begin = k0;                          // k0 is a multiple of 128
  const int ntq = (de_blk - q_begin) / 64 + 1;     // de_blk >= kl >= k0
  const int total = ntq * grp;

  // register staging of tile `it`: Q and dO rows, and one lse / delta value on threads 0..127
  Stage64<DP> qst, gst;
  float stat = 0.f;
  auto stage = [&](int it) {
    const int hq = hk * grp + it / ntq;
    const int q0 = q_begin + (it % ntq) * 64;
    qst.load(Q + (int64_t)b * S * qs + (int64_t)hq * D, qs, q0, S, D);
    gst.load(dO + (int64_t)b * S * os + (int64_t)hq * D, os, q0, S, D);
    if (threadIdx.x < 128) {  // rows past S are masked in the math: clamp the index
      const int q = min(q0 + (int)(threadIdx.x & 63), S - 1);
      const int64_t idx = ((int64_t)b * H + hq) * S + q;
      stat = threadIdx.x < 64 ? LSE[idx] : DELTA[idx];
    }
  };
  auto commit = [&](char* buf) {
    qst.store(buf);
    gst.store(buf + TILE);
    if (threadIdx.x < 128) reinterpret_cast<float*>(buf + 2 * TILE)[threadIdx.x] = stat;
  };
  stage(0);
  commit(smem);

  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    const int q0 = q_begin + (it % ntq) * 64;
    if (it + 1 < total) stage(it + 1);
    __syncthreads();
    const char* qb = smem + cur * BUFB;
    const char* gb = qb + TILE;
    const float* ls = reinterpret_cast<const float*>(qb + 2 * TILE);
    const float* dl = ls + 64;
    // all of this wave's keys above the tile's last query, or every document of the wave
    // ended before the tile
    const bool skip = !wave_live || kw0 > q0 + 63 || q0 > de_wlast;
    if (!skip) {
      // the two 32-query sub tiles stay a loop: unrolled, their LDS reads are hoisted over each
      // other and, with the staging registers of the next tile live, the kernel spills
#pragma unroll 1
      for (int u = 0; u < 2; ++u) {
        f32x16 sacc = {}, pacc = {};
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) {
          bf16x8 aq = lds_row8<DP>(qb, 32 * u + l32, 2 * s + hl);
          bf16x8 ag = lds_row8<DP>(gb, 32 * u + l32, 2 * s + hl);
          sacc = mfma32(aq, kf[s], sacc);
          pacc = mfma32(ag, vf[s], pacc);
        }
        float4 lsv[4], dlv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          lsv[g] = *reinterpret_cast<const float4*>(ls + 32 * u + 8 * g + 4 * hl);
          dlv[g] = *reinterpret_cast<const float4*>(dl + 32 * u + 8 * g + 4 * hl);
        }
        // masks only where needed: query rows past S, the causal diagonal, and sub tiles
        // that reach past the document end of the wave's first key (the smallest of the wave)
        const bool edge = (q0 + 64 > S) || (kw0 + 31 > q0 + 32 * u) || (q0 + 32 * u + 31 > de_wfirst);
        auto elems = [&](auto masked) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int q = q0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hl;
            const float lv = (&lsv[r >> 2].x)[r & 3], dv_ = (&dlv[r >> 2].x)[r & 3];
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], c, -lv));
            float dsv = p * (pacc[r] - dv_);
            if constexpr (decltype(masked)::value) {
              if (q >= S || key > q || q > de_k) {
                p = 0.f;
                dsv = 0.f;
              }
            }
            sacc[r] = p;      // P for dV
            pacc[r] = dsv;    // dS for dK
          }
        };
        if (edge) elems(std::true_type{});
        else elems(std::false_type{});
        const bf16x8 pb0 = pack8(sacc, 0), pb1 = pack8(sacc, 1);
        const bf16x8 db0 = pack8(pacc, 0), db1 = pack8(pacc, 1);
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
    if (it + 1 < total) commit(smem + (cur ^ 1) * BUFB);
  }
  if (kvalid) {
    bf16_t* dkrow = dK + ((int64_t)b * S + key) * dks + (int64_t)hk * D;
    bf16_t* dvrow = dV + ((int64_t)b * S + key) * dvs + (int64_t)hk * D;
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

// ==========================================================================================
// document bounds from tokens: position i starts a document iff i == 0 or
// tokens[i-1] == eos.  One workgroup per sequence: every thread owns a contiguous chunk,
// the chunk summaries are scanned in LDS (a running maximum of start positions from the
// left, a running minimum of end positions from the right), plain vector stores.
// ==========================================================================================
__global__ void __launch_bounds__(256) doc_bounds_kernel(const int64_t* __restrict__ tok, int64_t eos,
                                                         int* __restrict__ DS, int* __restrict__ DE, int S) {
  __shared__ int smax[256], smin[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t* row = tok + (int64_t)b * S;
  int* ds = DS + (int64_t)b * S;
  int* de = DE + (int64_t)b * S;
  const int per = (S + 255) / 256;
  const int i0 = min(t * per, S), i1 = min(i0 + per, S);
  // chunk summaries: the last start and the first end inside the chunk
  int last_start = -1, first_end = S - 1;
  for (int i = i1 - 1; i >= i0; --i) {
    const bool is_end = (i == S - 1) || row[i] == eos;
    if (is_end) first_end = i;
  }
  for (int i = i0; i < i1; ++i) {
    const bool is_start = (i == 0) || row[i - 1] == eos;
    if (is_start) last_start = i;
  }
  smax[t] = last_start;
  smin[t] = first_end;
  __syncthreads();
  // inclusive scans over the 256 summaries: max from the left, min from the right
  for (int off = 1; off < 256; off <<= 1) {
    const int a = t >= off ? smax[t - off] : -1;
    const int m = t + off < 256 ? smin[t + off] : S - 1;
    __syncthreads();
    smax[t] = max(smax[t], a);
    smin[t] = min(smin[t], m);
    __syncthreads();
  }
  int run_start = t > 0 ? smax[t - 1] : 0;
  for (int i = i0; i < i1; ++i) {
    if ((i == 0) || row[i - 1] == eos) run_start = i;
    ds[i] = run_start;
  }
  int run_end = t < 255 ? smin[t + 1] : S - 1;
  for (int i = i1 - 1; i >= i0; --i) {
    if ((i == S - 1) || row[i] == eos) run_end = i;
    de[i] = run_end;
  }
}

template <int DP>
int launch_doc_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int* ds, int B, int S,
                   int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, float scale,
                   hipStream_t st) {
  const size_t lds = 4 * 64 * DP * 2;
  auto kern = attn_doc_fwd_kernel<DP>;
  if (lds > 64 * 1024) hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  dim3 grid((S + 127) / 128, B * H);
  kern<<<grid, 256, lds, st>>>((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse, ds, B, S, H, Hkv,
                               D, qs, ks, vs, os, scale);
  return (int)hipGetLastError();
}

template <int DP>
int launch_doc_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   float* delta, void* dq, void* dk, void* dv, const int* ds, const int* de, int B, int S, int H,
                   int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dqs, int64_t dks,
                   int64_t dvs, float scale, hipStream_t st) {
  {
    const size_t lds = 4 * 64 * DP * 2;
    auto kern = attn_doc_bwd_dq_kernel<DP>;
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    dim3 grid((S + 127) / 128, B * H);
    kern<<<grid, 256, lds, st>>>((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)o,
                                 (const bf16_t*)dout, lse, delta, (bf16_t*)dq, ds, B, S, H, Hkv, D, qs, ks, vs, os, dqs,
                                 scale);
    const int e = (int)hipGetLastError();
    if (e) return e;
  }
  const size_t lds = 2 * (2 * 64 * DP * 2 + 512);
  auto kern = attn_doc_bwd_dkdv_kernel<DP>;
  if (lds > 64 * 1024) hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  dim3 grid((S + 127) / 128, B * Hkv);
  kern<<<grid, 256, lds, st>>>((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, lse, delta,
                               (bf16_t*)dk, (bf16_t*)dv, de, B, S, H, Hkv, D, qs, ks, vs, os, dks, dvs, scale);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int mp_attn_doc_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int* doc_start,
                               int B, int S, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os,
                               float scale, hipStream_t st) {
  if (H % Hkv) return -1;
  if (D == 64) return launch_doc_fwd<64>(q, k, v, o, lse, doc_start, B, S, H, Hkv, D, qs, ks, vs, os, scale, st);
  if (D == 128) return launch_doc_fwd<128>(q, k, v, o, lse, doc_start, B, S, H, Hkv, D, qs, ks, vs, os, scale, st);
  return -1;
}

extern "C" int mp_attn_doc_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                               const float* lse, float* delta, void* dq, void* dk, void* dv, const int* doc_start,
                               const int* doc_end, int B, int S, int H, int Hkv, int D, int64_t qs, int64_t ks,
                               int64_t vs, int64_t os, int64_t dqs, int64_t dks, int64_t dvs, float scale,
                               hipStream_t st) {
  if (H % Hkv) return -1;
  if (D == 64)
    return launch_doc_bwd<64>(q, k, v, o, dout, lse, delta, dq, dk, dv, doc_start, doc_end, B, S, H, Hkv, D, qs, ks, vs,
                              os, dqs, dks, dvs, scale, st);
  if (D == 128)
    return launch_doc_bwd<128>(q, k, v, o, dout, lse, delta, dq, dk, dv, doc_start, doc_end, B, S, H, Hkv, D, qs, ks,
                               vs, os, dqs, dks, dvs, scale, st);
  return -1;
}

extern "C" int mp_doc_bounds(const int64_t* tokens, int64_t eos, int* doc_start, int* doc_end, int B, int S,
                             hipStream_t st) {
  doc_bounds_kernel<<<B, 256, 0, st>>>(tokens, eos, doc_start, doc_end, S);
  return (int)hipGetLastError();
}
