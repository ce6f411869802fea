// The int8 KV cache ("kv8"), gfx950: the quantising append and the decode / append attention
// kernels that read it.  Siblings of rope_kv_append_kernel (generate.hip), attn_decode_partial
// (attention_decode.hip) and attn_append_partial (attention_append.hip): the same grids, split
// planners, workspaces, combine pass (mp_attn_split.h) and masks, with one cache row in another
// format.
//
// One cache row (one token of one sequence, K or V) of Hkv heads of dim D is W =
// round_up(Hkv * D + 4 * Hkv, 16) bytes:
//   [0, Hkv * D)                  int8 payload, head-major
//   [Hkv * D, Hkv * D + 4 Hkv)    Hkv little-endian f32 scales
//   the rest                      zero padding
// and head h of the row stands for q[d] * scale[h].  The quantiser, all in f32, of the values
// x[0..D) the bf16 cache would have stored:
//   amax = max |x[d]|, scale = amax / 127, inv = amax > 0 ? 127 / amax : 0,
//   q[d] = clamp(rint(x[d] * inv), -127, 127)
// (two correctly rounded divisions per head, a multiplication per element: the bits of
// ops.kv_quantize).  Every stride of a cache is in BYTES here, rows are 16-byte aligned.
//
//  1. rope_kv_append_kv8: per row b * T + t of packed qkv rows at p = pos[b] + t: q rotated in
//     place exactly as rope_kv_append_kernel does; K (rotated with the same rope_rot4 and
//     rounded to bf16 first) and V quantised into k_cache[b, p] / v_cache[b, p].  One head is
//     held by Dh / 16 lanes of a wave, 16 values each (8 of either half of the head); the
//     absolute maximum is a shuffle reduction over those lanes.  Two 8-byte payload stores per
//     lane, one lane per head stores the scale, the lanes after it the zero padding.  A row
//     with active[b] == 0 or t >= counts[b] is not touched; nothing outside the W bytes of a
//     touched row is written.
//  2. attn_decode_partial_kv8: 8 dims per lane as in the bf16 kernel (8-byte loads now), with
//     twice the unroll where the registers allow, so the same bytes are in flight.  The scale
//     enters once per key: s = ks[j] * dot(q, kq[j]), acc += (p * vs[j]) * vq[j], l sums the
//     unscaled p.  Bytes become f32 by a sign-extending byte-select convert (one instruction
//     per element).  The kernel has twice the elements per byte of its bf16 sibling and is
//     bound by VALU issue, not by HBM, so the rest is instruction count: the dims of a lane are
//     held in pairs and multiplied / accumulated with packed f32 operations, the sum over a
//     key's lanes is four DPP adds instead of LDS-path shuffles, and a row is addressed by a
//     uniform base plus a 32-bit byte offset (one sequence's cache must stay below 4 GiB).
//  3. attn_append_partial_kv8: K bytes become bf16 exactly in registers (|q| <= 127 has 7
//     significant bits) and feed the same 32x32x16 bf16 MFMA; ks[j] multiplies row j of the f32
//     S^T accumulator, vs[j] row j of P^T before it is packed to bf16; V is converted before
//     it is staged into the swizzled LDS tile.  A lane loads 16 contiguous bytes of a K row:
//     two k-steps of the MFMA, and Q's fragment reads the matching columns.  The 32 scales of a
//     tile reach the lanes that need them through a small per-wave LDS array.
//
// Lanes past a chunk's end re-read its last valid row (payload and scale), so stale rows never
// reach a register.  No atomics: results are bit-identical from run to run.
#include "mp_api.h"
#include "mp_attn_split.h"
#include "mp_attn_tiles.h"
#include "mp_rope.h"

#include <limits.h>

using namespace mp;

namespace {

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

__device__ __forceinline__ float byte2f(uint32_t w, int e) { return (float)(int8_t)(w >> (8 * e)); }

constexpr int kv8_row_bytes(int Hkv, int D) { return (Hkv * D + 4 * Hkv + 15) / 16 * 16; }

// ------------------------------------------------------------------ the quantising append
// quantise this lane's 16 values of a head held by NL = Dh / 16 lanes: a[0..8) are elements
// [v8 * 8, v8 * 8 + 8) of the first half of the head, a[8..16) the same of the second half
template <int NL>
__device__ __forceinline__ void quant_store(const float (&a)[16], int8_t* __restrict__ row, int head, int v8, int Dh,
                                            int Hkv, int W) {
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(a[e]));
#pragma unroll
  for (int o = 1; o < NL; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const float scale = amax / 127.0f;
  const float inv = amax > 0.f ? 127.0f / amax : 0.f;
  u32x2 lo = {0, 0}, hi = {0, 0};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int q0 = (int)fminf(fmaxf(rintf(a[e] * inv), -127.f), 127.f);
    const int q1 = (int)fminf(fmaxf(rintf(a[8 + e] * inv), -127.f), 127.f);
    lo[e >> 2] |= (uint32_t)(q0 & 0xFF) << (8 * (e & 3));
    hi[e >> 2] |= (uint32_t)(q1 & 0xFF) << (8 * (e & 3));
  }
  int8_t* dst = row + (int64_t)head * Dh + v8 * 8;
  *reinterpret_cast<u32x2*>(dst) = lo;
  *reinterpret_cast<u32x2*>(dst + Dh / 2) = hi;
  const int tail = Hkv * Dh;                         // scales, then up to three zero words
  if (v8 == 0) *reinterpret_cast<float*>(row + tail + 4 * head) = scale;
  else if (head == 0 && tail + 4 * Hkv + 4 * v8 <= W) *reinterpret_cast<uint32_t*>(row + tail + 4 * Hkv + 4 * (v8 - 1)) = 0u;
}

// Work items of one qkv row, each one thread, NL = Dh / 16 per head:
//   rope:  [0, H * NL)        q head h: rotate in place (rope_kv_append_kernel's item)
//   then   [.., + Hkv * NL)   k head h: (rotate,) quantise -> k_cache
//          [.., + Hkv * NL)   v head h: quantise -> v_cache
template <int NL>
__global__ void __launch_bounds__(256) rope_kv_append_kv8_kernel(
    bf16_t* __restrict__ qkv, const float* __restrict__ cs, const float* __restrict__ sn, int8_t* __restrict__ kc,
    int8_t* __restrict__ vc, const int* __restrict__ pos, const uint8_t* __restrict__ active,
    const int* __restrict__ counts, int T, int H, int Hkv, int Smax, int64_t qkv_ld, int64_t k_bs, int64_t k_ts,
    int64_t v_bs, int64_t v_ts, int rope) {
  constexpr int Dh = NL * 16, half = Dh / 2;
  const int n = blockIdx.x;                  // row b * T + t: new token t of sequence b
  const int b = n / T, t = n % T;
  if (active && !active[b]) return;
  if (counts && t >= counts[b]) return;
  int p = pos[b];
  p = p < 0 ? 0 : (p >= Smax ? Smax - 1 : p);
  p = min(p + t, Smax - 1);
  bf16_t* row = qkv + (int64_t)n * qkv_ld;
  const int n_q = rope ? H * NL : 0;
  const int W = kv8_row_bytes(Hkv, Dh);
  const int i = blockIdx.y * 256 + threadIdx.x;
  const float* cr = cs + (int64_t)p * half;
  const float* sr = sn + (int64_t)p * half;
  if (i < n_q) {
    const int h = i / NL, v8 = i % NL;
    bf16_t* x = row + (int64_t)h * Dh + v8 * 8;
    const u16x8 x1 = *reinterpret_cast<const u16x8*>(x);
    const u16x8 x2 = *reinterpret_cast<const u16x8*>(x + half);
    u16x4 a1, a2, b1, b2;
    rope_rot4(u16x4{x1[0], x1[1], x1[2], x1[3]}, u16x4{x2[0], x2[1], x2[2], x2[3]}, cr, sr, v8 * 8, 1.0f, a1, a2);
    rope_rot4(u16x4{x1[4], x1[5], x1[6], x1[7]}, u16x4{x2[4], x2[5], x2[6], x2[7]}, cr, sr, v8 * 8 + 4, 1.0f, b1,
              b2);
    *reinterpret_cast<u16x8*>(x) = u16x8{a1[0], a1[1], a1[2], a1[3], b1[0], b1[1], b1[2], b1[3]};
    *reinterpret_cast<u16x8*>(x + half) = u16x8{a2[0], a2[1], a2[2], a2[3], b2[0], b2[1], b2[2], b2[3]};
    return;
  }
  const int c = i - n_q;
  if (c >= 2 * Hkv * NL) return;             // whole heads: a head's NL lanes leave together
  const bool is_v = c >= Hkv * NL;
  const int hv = (is_v ? c - Hkv * NL : c) / NL, v8 = c % NL;
  const bf16_t* x = row + (int64_t)(H + (is_v ? Hkv : 0) + hv) * Dh + v8 * 8;
  u16x8 x1 = *reinterpret_cast<const u16x8*>(x);
  u16x8 x2 = *reinterpret_cast<const u16x8*>(x + half);
  if (rope && !is_v) {
    u16x4 a1, a2, b1, b2;
    rope_rot4(u16x4{x1[0], x1[1], x1[2], x1[3]}, u16x4{x2[0], x2[1], x2[2], x2[3]}, cr, sr, v8 * 8, 1.0f, a1, a2);
    rope_rot4(u16x4{x1[4], x1[5], x1[6], x1[7]}, u16x4{x2[4], x2[5], x2[6], x2[7]}, cr, sr, v8 * 8 + 4, 1.0f, b1,
              b2);
    x1 = u16x8{a1[0], a1[1], a1[2], a1[3], b1[0], b1[1], b1[2], b1[3]};
    x2 = u16x8{a2[0], a2[1], a2[2], a2[3], b2[0], b2[1], b2[2], b2[3]};
  }
  float a[16];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    a[e] = bf2f(x1[e]);
    a[8 + e] = bf2f(x2[e]);
  }
  int8_t* dst = is_v ? vc + (int64_t)b * v_bs + (int64_t)p * v_ts : kc + (int64_t)b * k_bs + (int64_t)p * k_ts;
  quant_store<NL>(a, dst, hv, v8, Dh, Hkv, W);
}

// ------------------------------------------------------------------------ decode attention
constexpr int kDecodeThreads = 256;                  // 4 waves, one per SIMD
constexpr int kDecodeWaves = kDecodeThreads / MP_WAVE;

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

typedef __attribute__((ext_vector_type(2))) float f32x2;

// v + (v of the lane a DPP control pairs this lane with): one VALU instruction, no LDS traffic
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// sum over the aligned group of LPK = 8 or 16 lanes that hold one key, the same bits in every
// lane of the group: lane ^ 1, lane ^ 2 (quad_perm), then the mirrors of 8 and of 16 lanes
template <int LPK>
__device__ __forceinline__ float key_sum(float v) {
  v = dpp_add<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);       // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);      // row_half_mirror
  if (LPK == 16) v = dpp_add<0x140>(v);   // row_mirror
  return v;
}

// K and V loads in flight per lane: 2 * UNR x (8 B payload + 4 B scale)
template <int REP>
constexpr int decode_unroll() { return REP >= 8 ? 4 : 8; }

template <int D, int REP>
__global__ __launch_bounds__(kDecodeThreads) void attn_decode_partial_kv8(
    const bf16_t* __restrict__ q, const int8_t* __restrict__ kc, const int8_t* __restrict__ vc,
    const int* __restrict__ lens, float* __restrict__ part_o, float* __restrict__ part_ml, int H, int Hkv, int rep,
    int Smax, int chunk, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, float scale_log2) {
  constexpr int LPK = D / 8;          // lanes per key row (8 B each)
  constexpr int KPW = MP_WAVE / LPK;  // keys per wave load instruction
  constexpr int UNR = decode_unroll<REP>();
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z, nsplit = gridDim.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane % LPK, slot = lane / LPK;

  const int len = min(max(lens[b], 0), Smax);
  const int start = split * chunk;
  const int end = min(start + chunk, len);

  // two dims per register pair: the products and sums below are packed f32 operations
  f32x2 qf[REP][4];
  u16x8 qraw[REP];
#pragma unroll
  for (int r = 0; r < REP; ++r)
    qraw[r] = *reinterpret_cast<const u16x8*>(q + (int64_t)b * q_stride + (int64_t)(kvh * rep + min(r, rep - 1)) * D +
                                              sub * 8);
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    const float sc = r < rep ? scale_log2 : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) qf[r][e] = f32x2{bf2f(qraw[r][2 * e]) * sc, bf2f(qraw[r][2 * e + 1]) * sc};
  }

  f32x2 acc[REP][4];
  float m[REP], l[REP];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = f32x2{0.f, 0.f};
  }

  if (start < end) {
    // byte offsets inside one sequence's cache fit 32 bits (the launcher checks): a uniform
    // base plus one 32-bit lane offset per load
    const int8_t* kb = kc + (int64_t)b * k_bs;
    const int8_t* vb = vc + (int64_t)b * v_bs;
    const uint32_t kts = (uint32_t)k_ts, vts = (uint32_t)v_ts;
    const uint32_t poff = kvh * D + sub * 8;             // this lane's payload bytes inside a row
    const uint32_t soff = Hkv * D + 4 * kvh;             // this head's scale inside a row
    const int last = end - 1;
    for (int j0 = start + w * (UNR * KPW); j0 < end; j0 += kDecodeWaves * UNR * KPW) {
      u32x2 kr[UNR], vr[UNR];
      float ks[UNR], vs[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t ro = (uint32_t)min(j0 + u * KPW + slot, last) * kts;
        kr[u] = *reinterpret_cast<const u32x2*>(kb + (ro + poff));
        ks[u] = *reinterpret_cast<const float*>(kb + (ro + soff));
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t ro = (uint32_t)min(j0 + u * KPW + slot, last) * vts;
        vr[u] = *reinterpret_cast<const u32x2*>(vb + (ro + poff));
        vs[u] = *reinterpret_cast<const float*>(vb + (ro + soff));
      }
      float s[UNR][REP];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        f32x2 kf[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) kf[e] = f32x2{byte2f(kr[u][e >> 1], 2 * (e & 1)), byte2f(kr[u][e >> 1], 2 * (e & 1) + 1)};
        const bool valid = j0 + u * KPW + slot < end;
#pragma unroll
        for (int r = 0; r < REP; ++r) {
          f32x2 d2 = qf[r][0] * kf[0];
#pragma unroll
          for (int e = 1; e < 4; ++e) d2 = __builtin_elementwise_fma(qf[r][e], kf[e], d2);
          const float d = key_sum<LPK>(d2[0] + d2[1]);
          s[u][r] = valid ? d * ks[u] : -INFINITY;
        }
      }
      // online softmax, one rescale per UNR keys; p is then scaled by the key's V scale
#pragma unroll
      for (int r = 0; r < REP; ++r) {
        float mn = m[r];
#pragma unroll
        for (int u = 0; u < UNR; ++u) mn = fmaxf(mn, s[u][r]);
        const float ms = mn == -INFINITY ? 0.f : mn;   // nothing valid yet: every weight 0
        const float alpha = exp2_fast(m[r] - ms);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const float p = exp2_fast(s[u][r] - ms);
          ps += p;
          s[u][r] = p * vs[u];
        }
        l[r] = l[r] * alpha + ps;
        m[r] = mn;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        f32x2 vf[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) vf[e] = f32x2{byte2f(vr[u][e >> 1], 2 * (e & 1)), byte2f(vr[u][e >> 1], 2 * (e & 1) + 1)};
#pragma unroll
        for (int r = 0; r < REP; ++r) {
          const f32x2 pv = {s[u][r], s[u][r]};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r][e] = __builtin_elementwise_fma(pv, vf[e], acc[r][e]);
        }
      }
    }
  }

  // merge the key slots of the wave (lanes with the same `sub`)
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    float mw = m[r];
#pragma unroll
    for (int o = LPK; o < MP_WAVE; o <<= 1) mw = fmaxf(mw, __shfl_xor(mw, o, 64));
    const float ms = mw == -INFINITY ? 0.f : mw;
    const float sc = exp2_fast(m[r] - ms);
    float lw = l[r] * sc;
#pragma unroll
    for (int o = LPK; o < MP_WAVE; o <<= 1) lw += __shfl_xor(lw, o, 64);
    l[r] = lw;
    m[r] = mw;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = acc[r][e >> 1][e & 1] * sc;
#pragma unroll
      for (int o = LPK; o < MP_WAVE; o <<= 1) a += __shfl_xor(a, o, 64);
      acc[r][e >> 1][e & 1] = a;
    }
  }

  // merge the waves through LDS (its only use), in wave order
  __shared__ float sh_o[kDecodeWaves][REP][D];
  __shared__ float sh_m[kDecodeWaves][REP];
  __shared__ float sh_l[kDecodeWaves][REP];
  if (slot == 0) {
#pragma unroll
    for (int r = 0; r < REP; ++r) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sh_o[w][r][sub * 8 + e] = acc[r][e >> 1][e & 1];
      if (sub == 0) {
        sh_m[w][r] = m[r];
        sh_l[w][r] = l[r];
      }
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < rep * D; idx += kDecodeThreads) {
    const int r = idx / D, d = idx % D;
    float M = sh_m[0][r];
#pragma unroll
    for (int i = 1; i < kDecodeWaves; ++i) M = fmaxf(M, sh_m[i][r]);
    const float ms = M == -INFINITY ? 0.f : M;
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int i = 0; i < kDecodeWaves; ++i) {
      const float sc = exp2_fast(sh_m[i][r] - ms);
      L += sh_l[i][r] * sc;
      O += sh_o[i][r][d] * sc;
    }
    const int64_t row = ((int64_t)b * H + kvh * rep + r) * nsplit + split;
    part_o[row * D + d] = O;
    if (d == 0) {
      part_ml[row * 2] = M;
      part_ml[row * 2 + 1] = L;
    }
  }
}

template <int D, int REP>
int launch_decode(const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B, int H,
                  int Hkv, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs,
                  int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st) {
  const int rep = H / Hkv;
  const int chunk = (max_len + splits - 1) / splits;
  float* part_o = ws;
  float* part_ml = ws + (int64_t)B * H * splits * D;
  attn_decode_partial_kv8<D, REP><<<dim3(splits, Hkv, B), kDecodeThreads, 0, st>>>(
      (const bf16_t*)q, (const int8_t*)k, (const int8_t*)v, lens, part_o, part_ml, H, Hkv, rep, Smax, chunk, q_stride,
      k_bs, k_ts, v_bs, v_ts, scale * 1.4426950408889634f);
  attn_split_combine<D><<<attn_split_combine_grid(B, H), D, 0, st>>>(part_o, part_ml, (bf16_t*)o, B, H, splits,
                                                                      o_stride);
  return (int)hipGetLastError();
}

template <int D>
int launch_decode_rep(int rep, const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B,
                      int H, int Hkv, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts,
                      int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st) {
#define MP_DECODE_GO(R)                                                                                      \
  return launch_decode<D, R>(q, k, v, lens, o, ws, B, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts, \
                             o_stride, scale, splits, st)
  if (rep == 1) MP_DECODE_GO(1);
  if (rep == 2) MP_DECODE_GO(2);
  if (rep <= 4) MP_DECODE_GO(4);
  MP_DECODE_GO(8);
#undef MP_DECODE_GO
}

// ------------------------------------------------------------------------ append attention
constexpr int kAppendThreads = 256;
constexpr int kAppendWaves = kAppendThreads / MP_WAVE;
constexpr int kQT = 32;                    // query rows (token, head) per workgroup
constexpr int kKT = 32;                    // keys per wave tile

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int DP>
constexpr int append_lds_bytes() {
  constexpr int stage = kAppendWaves * 2 * kKT * DP * 2;           // V tiles, two per wave
  constexpr int merge = kAppendWaves * kQT * (DP + 4) * 4;         // f32 rows, padded
  return stage > merge ? stage : merge;
}

// 8 int8 (two words) -> 8 bf16, exactly
__device__ __forceinline__ u16x8 bytes2bf(uint32_t w0, uint32_t w1) {
  u16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[e] = f2bf(byte2f(w0, e));
    r[4 + e] = f2bf(byte2f(w1, e));
  }
  return r;
}

// this wave's K fragments, V rows and scales of the 32-key tile at j0 (rows clamped to `last`),
// as stored: 16 bytes of a K row are k-steps 2 s and 2 s + 1 of the lane
template <int DP>
struct KV8Regs {
  u32x4 k[DP / 32], v[DP / 32];
  float ks, vs;                 // of key j0 + (lane & 31)
  __device__ __forceinline__ void load(const int8_t* kb, const int8_t* vb, int64_t k_ts, int64_t v_ts, int poff,
                                       int soff, int j0, int last) {
    const int lane = threadIdx.x & 63, l32 = lane & 31, hl = lane >> 5;
    const int8_t* kr = kb + (int64_t)min(j0 + l32, last) * k_ts;
#pragma unroll
    for (int s = 0; s < DP / 32; ++s) k[s] = *reinterpret_cast<const u32x4*>(kr + poff + 32 * s + 16 * hl);
    ks = *reinterpret_cast<const float*>(kr + soff);
    vs = *reinterpret_cast<const float*>(vb + (int64_t)min(j0 + l32, last) * v_ts + soff);
#pragma unroll
    for (int i = 0; i < DP / 32; ++i) {
      const int idx = lane + 64 * i;
      const int r = idx / (DP / 16), c = idx % (DP / 16);
      v[i] = *reinterpret_cast<const u32x4*>(vb + (int64_t)min(j0 + r, last) * v_ts + poff + c * 16);
    }
  }
  // V as bf16 into the swizzled tile, the tile's scales into sc[0 / 1][32]
  __device__ __forceinline__ void store_v(char* lds, float* sc) const {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < DP / 32; ++i) {
      const int idx = lane + 64 * i;
      const int r = idx / (DP / 16), c = idx % (DP / 16);
      *reinterpret_cast<u16x8*>(lds + lds_off<DP>(r, 2 * c)) = bytes2bf(v[i][0], v[i][1]);
      *reinterpret_cast<u16x8*>(lds + lds_off<DP>(r, 2 * c + 1)) = bytes2bf(v[i][2], v[i][3]);
    }
    if (lane < kKT) {
      sc[lane] = ks;
      sc[kKT + lane] = vs;
    }
  }
};

template <int DP>
__global__ __launch_bounds__(kAppendThreads) void attn_append_partial_kv8(
    const bf16_t* __restrict__ q, const int8_t* __restrict__ kc, const int8_t* __restrict__ vc,
    const int* __restrict__ base, const int* __restrict__ counts, float* __restrict__ part_o,
    float* __restrict__ part_ml, int T, int H, int Hkv, int rep, int Smax, int chunk, int nqt, int64_t q_stride,
    int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, float scale_log2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float sh_m[kAppendWaves][kQT];
  __shared__ float sh_l[kAppendWaves][kQT];
  __shared__ __attribute__((aligned(16))) float sh_sc[kAppendWaves][2][2 * kKT];   // per wave and buffer: ks | vs
  constexpr int VT = kKT * DP * 2;  // bytes of one staged V tile
  const int split = blockIdx.x, kvh = blockIdx.y, nsplit = gridDim.x;
  const int b = (int)blockIdx.z / nqt, qt = (int)blockIdx.z % nqt;
  const int lane = threadIdx.x & 63, l32 = lane & 31, hl = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

  const int bs = clampi(base[b], 0, Smax);
  const int cnt = clampi(counts ? counts[b] : T, 0, min(T, Smax - bs));
  const int R = T * rep;
  const int r = qt * kQT + l32;
  const int t = r / rep;
  const int hq = kvh * rep + r % rep;
  const bool rvalid = r < R && t < cnt;
  const int qpos = bs + t;                                  // the last key the row sees
  const int t_first = (qt * kQT) / rep;
  const int t_last = min(min(qt * kQT + kQT - 1, R - 1) / rep, cnt - 1);
  const int kv_end = t_last >= t_first ? bs + t_last + 1 : 0;      // <= bs + cnt <= Smax
  const int start = split * chunk;
  const int end = min(start + chunk, kv_end);

  // k-step s of this lane: columns 32 (s / 2) + 16 hl + 8 (s % 2), K's 16-byte loads in halves
  bf16x8 qf[DP / 16];
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rvalid)
      z = *reinterpret_cast<const u16x8*>(q + ((int64_t)b * T + t) * q_stride + (int64_t)hq * DP + 32 * (s >> 1) +
                                          16 * hl + 8 * (s & 1));
    qf[s] = __builtin_bit_cast(bf16x8, z);
  }
  f32x16 o[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) o[d] = {};
  float m_run = -INFINITY, l_run = 0.f;

  if (start < end) {   // uniform over the workgroup
    const int8_t* kb = kc + (int64_t)b * k_bs;
    const int8_t* vb = vc + (int64_t)b * v_bs;
    const int poff = kvh * DP, soff = Hkv * DP + 4 * kvh;
    const int last = end - 1;
    char* vl = smem + w * 2 * VT;
    KV8Regs<DP> cur, nxt;
    if (start + w * kKT < end) cur.load(kb, vb, k_ts, v_ts, poff, soff, start + w * kKT, last);
    int buf = 0;
    for (int it = start; it < end; it += kAppendWaves * kKT, buf ^= 1) {
      const int j0 = it + w * kKT;
      const bool live = j0 < end;
      if (live) cur.store_v(vl + buf * VT, sh_sc[w][buf]);
      if (j0 + kAppendWaves * kKT < end) nxt.load(kb, vb, k_ts, v_ts, poff, soff, j0 + kAppendWaves * kKT, last);
      __syncthreads();
      if (live) {
        const char* vt = vl + buf * VT;
        const float* sc = sh_sc[w][buf];
        f32x16 s0 = {};
#pragma unroll
        for (int s = 0; s < DP / 32; ++s) {
          s0 = mfma32(__builtin_bit_cast(bf16x8, bytes2bf(cur.k[s][0], cur.k[s][1])), qf[2 * s], s0);
          s0 = mfma32(__builtin_bit_cast(bf16x8, bytes2bf(cur.k[s][2], cur.k[s][3])), qf[2 * s + 1], s0);
        }
        // element e is key j0 + (e & 3) + 8 (e >> 2) + 4 hl: its scales are 4 consecutive floats per e >> 2
        f32x4 ksv[4], vsv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          ksv[g] = *reinterpret_cast<const f32x4*>(sc + 8 * g + 4 * hl);
          vsv[g] = *reinterpret_cast<const f32x4*>(sc + kKT + 8 * g + 4 * hl);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kj = j0 + (e & 3) + 8 * (e >> 2) + 4 * hl;
          s0[e] *= ksv[e >> 2][e & 3];
          if (kj >= end || kj > qpos || !rvalid) s0[e] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s0[e]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx * scale_log2);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        float rs = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[e], scale_log2, -m_use));
          rs += p;
          s0[e] = p * vsv[e >> 2][e & 3];
        }
        rs += __shfl_xor(rs, 32, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
#pragma unroll
        for (int d = 0; d < DP / 32; ++d) o[d] *= alpha;
        const bf16x8 p0 = pack8(s0, 0), p1 = pack8(s0, 1);
#pragma unroll
        for (int d = 0; d < DP / 32; ++d) {
          const int c0 = 32 * d + 16 * ((lane >> 4) & 1);
          bf16x8 a;
          a = cat44(lds_tr4<DP>(vt, 0 + 4 * hl, c0), lds_tr4<DP>(vt, 8 + 4 * hl, c0));
          o[d] = mfma32(a, p0, o[d]);
          a = cat44(lds_tr4<DP>(vt, 16 + 4 * hl, c0), lds_tr4<DP>(vt, 24 + 4 * hl, c0));
          o[d] = mfma32(a, p1, o[d]);
        }
      }
      cur = nxt;
    }
  }

  // merge the four waves through LDS, in wave order (the V tiles are dead)
  __syncthreads();
  constexpr int LD = DP + 4;
  float* sh_o = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int d = 0; d < DP / 32; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4*>(sh_o + ((int64_t)w * kQT + l32) * LD + 32 * d + 8 * g + 4 * hl) =
          f32x4{o[d][4 * g], o[d][4 * g + 1], o[d][4 * g + 2], o[d][4 * g + 3]};
  if (hl == 0) {
    sh_m[w][l32] = m_run;
    sh_l[w][l32] = l_run;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < kQT * DP; idx += kAppendThreads) {
    const int qi = idx / DP, d = idx % DP;
    const int rr = qt * kQT + qi;
    if (rr >= R) break;            // qi grows with idx
    float M = sh_m[0][qi];
#pragma unroll
    for (int i = 1; i < kAppendWaves; ++i) M = fmaxf(M, sh_m[i][qi]);
    const float ms = M == -INFINITY ? 0.f : M;
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int i = 0; i < kAppendWaves; ++i) {
      const float sc = __builtin_amdgcn_exp2f(sh_m[i][qi] - ms);
      L += sh_l[i][qi] * sc;
      O += sh_o[((int64_t)i * kQT + qi) * LD + d] * sc;
    }
    const int64_t row = (((int64_t)b * T + rr / rep) * H + kvh * rep + rr % rep) * nsplit + split;
    part_o[row * DP + d] = O;
    if (d == 0) {
      part_ml[row * 2] = M;
      part_ml[row * 2 + 1] = L;
    }
  }
}

template <int D>
int launch_append(const void* q, const void* k, const void* v, const int* base, const int* counts, void* o, float* ws,
                  int B, int T, int H, int Hkv, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts,
                  int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st) {
  const int rep = H / Hkv;
  const int nqt = (T * rep + kQT - 1) / kQT;
  const int chunk = (max_len + splits - 1) / splits;
  float* part_o = ws;
  float* part_ml = ws + (int64_t)B * T * H * splits * D;
  constexpr int lds = append_lds_bytes<D>();
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)attn_append_partial_kv8<D>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  attn_append_partial_kv8<D><<<dim3(splits, Hkv, B * nqt), kAppendThreads, lds, st>>>(
      (const bf16_t*)q, (const int8_t*)k, (const int8_t*)v, base, counts, part_o, part_ml, T, H, Hkv, rep, Smax, chunk,
      nqt, q_stride, k_bs, k_ts, v_bs, v_ts, scale * LOG2E);
  attn_split_combine<D><<<attn_split_combine_grid(B * T, H), D, 0, st>>>(part_o, part_ml, (bf16_t*)o, B * T, H,
                                                                          splits, o_stride);
  return (int)hipGetLastError();
}

// what every launcher here asks of a pair of int8 caches: 16-byte aligned rows that hold W bytes
bool kv8_strides_ok(const void* k, const void* v, int Hkv, int D, int B, int Smax, int64_t k_bs, int64_t k_ts,
                    int64_t v_bs, int64_t v_ts) {
  const int64_t W = kv8_row_bytes(Hkv, D);
  if (((uintptr_t)k | (uintptr_t)v) % 16 != 0 || (k_bs | k_ts | v_bs | v_ts) % 16 != 0) return false;
  if (k_ts < W || v_ts < W) return false;
  // the attention kernels index one sequence's rows with 32-bit byte offsets
  if ((int64_t)Smax * k_ts > (int64_t)UINT32_MAX || (int64_t)Smax * v_ts > (int64_t)UINT32_MAX) return false;
  return B == 1 || (k_bs >= (int64_t)Smax * k_ts && v_bs >= (int64_t)Smax * v_ts);
}

}  // namespace

// The int8-cache form of mp_rope_kv_append: kc / vc are int8 caches [B, Smax, W] with batch /
// token strides in bytes; qkv_ld in elements.  Returns -1 for an unsupported shape.
extern "C" int mp_rope_kv_append_kv8(void* qkv, const float* cs, const float* sn, void* kc, void* vc, const int* pos,
                                     const uint8_t* active, const int* counts, int B, int T, int H, int Hkv, int Dh,
                                     int Smax, int64_t qkv_ld, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts,
                                     int rope, hipStream_t st) {
  if ((Dh != 64 && Dh != 128) || B < 1 || T < 1 || (int64_t)B * T > INT_MAX || H < 1 || Hkv < 1 || Smax < 1) return -1;
  if (H > 65535 || Hkv > 65535 || qkv_ld % 8 != 0 || (uintptr_t)qkv % 16 != 0) return -1;
  if (rope && (!cs || !sn)) return -1;
  if (!kv8_strides_ok(kc, vc, Hkv, Dh, B, Smax, k_bs, k_ts, v_bs, v_ts)) return -1;
  const int nl = Dh / 16;
  const int items = ((rope ? H : 0) + 2 * Hkv) * nl;
  if ((items + 255) / 256 > 65535) return -1;
  dim3 grid(B * T, (items + 255) / 256);
  if (Dh == 64)
    rope_kv_append_kv8_kernel<4><<<grid, 256, 0, st>>>((bf16_t*)qkv, cs, sn, (int8_t*)kc, (int8_t*)vc, pos, active,
                                                       counts, T, H, Hkv, Smax, qkv_ld, k_bs, k_ts, v_bs, v_ts, rope);
  else
    rope_kv_append_kv8_kernel<8><<<grid, 256, 0, st>>>((bf16_t*)qkv, cs, sn, (int8_t*)kc, (int8_t*)vc, pos, active,
                                                       counts, T, H, Hkv, Smax, qkv_ld, k_bs, k_ts, v_bs, v_ts, rope);
  return (int)hipGetLastError();
}

// The int8-cache form of mp_attn_decode: the same arguments, planner (mp_attn_decode_plan) and
// workspace (mp_attn_decode_ws_floats); k / v are int8 caches [B, Smax, W] whose batch / token
// strides are in bytes (q_stride / o_stride in elements).  Returns -1 for an unsupported shape.
extern "C" int mp_attn_decode_kv8(const void* q, const void* k, const void* v, const int* lens, void* o, float* ws,
                                  int B, int H, int Hkv, int D, int Smax, int max_len, int64_t q_stride, int64_t k_bs,
                                  int64_t k_ts, int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale, int splits,
                                  hipStream_t st) {
  if ((D != 64 && D != 128) || Hkv < 1 || H < 1 || H % Hkv != 0 || H / Hkv > 8) return -1;
  if (B < 1 || B > 65535 || Hkv > 65535 || Smax < 1 || max_len < 1 || max_len > Smax) return -1;
  if (splits == 0) splits = mp_attn_decode_plan(B, Hkv, max_len);
  if (splits < 1 || splits > max_len || splits > kSplitMaxSplits || ws == nullptr) return -1;
  if (q_stride % 8 != 0 || (uintptr_t)q % 16 != 0) return -1;
  if (!kv8_strides_ok(k, v, Hkv, D, B, Smax, k_bs, k_ts, v_bs, v_ts)) return -1;
  const int rep = H / Hkv;
  if (D == 64)
    return launch_decode_rep<64>(rep, q, k, v, lens, o, ws, B, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts,
                                 o_stride, scale, splits, st);
  return launch_decode_rep<128>(rep, q, k, v, lens, o, ws, B, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts,
                                o_stride, scale, splits, st);
}

// The int8-cache form of mp_attn_append (planner mp_attn_append_plan, workspace
// mp_attn_append_ws_floats): cache strides in bytes.  Returns -1 for an unsupported shape.
extern "C" int mp_attn_append_kv8(const void* q, const void* k, const void* v, const int* base, const int* counts,
                                  void* o, float* ws, int B, int T, int H, int Hkv, int D, int Smax, int max_len,
                                  int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts,
                                  int64_t o_stride, float scale, int splits, hipStream_t st) {
  if ((D != 64 && D != 128) || Hkv < 1 || H < 1 || H % Hkv != 0 || H / Hkv > 8) return -1;
  if (B < 1 || T < 1 || Hkv > 65535 || H > 65535 || Smax < 1 || max_len < 1 || max_len > Smax) return -1;
  const int rep = H / Hkv;
  const int64_t nqt = ((int64_t)T * rep + kQT - 1) / kQT;
  if ((int64_t)B * nqt > 65535 || (int64_t)B * T > INT32_MAX) return -1;
  if (splits == 0) splits = mp_attn_append_plan(B, T, Hkv, rep, max_len);
  if (splits < 1 || splits > max_len || splits > kSplitMaxSplits || ws == nullptr || base == nullptr) return -1;
  if (q_stride % 8 != 0 || (uintptr_t)q % 16 != 0) return -1;
  if (!kv8_strides_ok(k, v, Hkv, D, B, Smax, k_bs, k_ts, v_bs, v_ts)) return -1;
  if (D == 64)
    return launch_append<64>(q, k, v, base, counts, o, ws, B, T, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs,
                             v_ts, o_stride, scale, splits, st);
  return launch_append<128>(q, k, v, base, counts, o, ws, B, T, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs,
                            v_ts, o_stride, scale, splits, st);
}
