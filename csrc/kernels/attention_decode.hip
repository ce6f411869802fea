// Single-token (decode) attention over a per-sequence KV cache, bf16, gfx950.
//
// One query row per (sequence, head) against lens[b] cached keys: a memory-bound stream
// over the cache, nothing like the 128-query tiles of attention.hip.  Two launches:
//
//  1. attn_decode_partial, grid (split, Hkv, B), 256 threads.  A workgroup owns one
//     contiguous key chunk [split * chunk, (split + 1) * chunk) of one KV head and serves
//     all rep = H / Hkv query heads of that KV head, so every K/V byte is read once per KV
//     head.  K/V rows go straight from global memory to VGPRs in 16-byte loads (D / 8 lanes
//     per key, 64 / (D / 8) keys per wave instruction), kUnroll K loads and kUnroll V loads
//     are issued before the first use, and nothing is staged through LDS.  The dot products
//     are VALU FMAs in f32; the softmax is online, in exp2 units (q is pre-scaled by
//     scale * log2 e), with one running (max, sum, acc) per key slot of a wave, so the loop
//     has no cross-slot traffic.  The slots of a wave are merged with shuffles and the four
//     waves through LDS once, at the end of the chunk.  The workgroup writes its
//     unnormalised f32 output [D] and its (max, sum) per query head into the workspace.
//  2. attn_split_combine (mp_attn_split.h), grid (H, B), D threads: merges the splits in split
//     order and writes bf16.  No atomics anywhere: results are bit-identical from run to run.
//
// A split that lies wholly beyond lens[b] writes (-inf, 0) and a zero row, which the
// combine ignores.  Keys at positions >= lens[b] never enter a result: a lane whose key
// index is past the end re-reads the chunk's last valid row (an address that is always
// inside the valid part of the cache) and its score is set to -inf, so its weight is an
// exact zero whatever the stale cache rows hold.
#include "mp_api.h"
#include "mp_attn_split.h"

using namespace mp;

namespace {

constexpr int kDecodeThreads = 256;                  // 4 waves, one per SIMD
constexpr int kDecodeWaves = kDecodeThreads / MP_WAVE;
constexpr int kUnroll = 4;                           // K and V loads in flight per lane: 2 * kUnroll x 16 B
// split planner: no chunk shorter than this many keys (below it the per-workgroup merge and
// the combine pass cost more than the extra workgroups bring), and enough workgroups for
// two per CU where the cache is long enough
constexpr int kDecodeMinChunk = 256;
constexpr int kDecodeCUs = 256;
constexpr int kDecodeWgPerCU = 2;
constexpr int kDecodeMaxSplits = kSplitMaxSplits;

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

template <int D, int REP>
__global__ __launch_bounds__(kDecodeThreads) void attn_decode_partial(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ lens, float* __restrict__ part_o, float* __restrict__ part_ml, int H, int rep, int Smax,
    int chunk, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, float scale_log2) {
  constexpr int LPK = D / 8;          // lanes per key row (16 B each)
  constexpr int KPW = MP_WAVE / LPK;  // keys per wave load instruction
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z, nsplit = gridDim.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane % LPK, slot = lane / LPK;

  const int len = min(max(lens[b], 0), Smax);
  const int start = split * chunk;
  const int end = min(start + chunk, len);

  // this lane's 8 dims of every query head of the KV head, pre-scaled to exp2 units
  // (heads r >= rep of a padded REP re-read the last real head and are zeroed: the loads
  // stay unconditional, so all REP of them are in flight together)
  float qf[REP][8];
  u16x8 qraw[REP];
#pragma unroll
  for (int r = 0; r < REP; ++r)
    qraw[r] = *reinterpret_cast<const u16x8*>(q + (int64_t)b * q_stride + (int64_t)(kvh * rep + min(r, rep - 1)) * D +
                                              sub * 8);
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    const float sc = r < rep ? scale_log2 : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[r][e] = bf2f(qraw[r][e]) * sc;
  }

  float acc[REP][8], m[REP], l[REP];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[r][e] = 0.f;
  }

  if (start < end) {
    const bf16_t* kb = kc + (int64_t)b * k_bs + (int64_t)kvh * D + sub * 8;
    const bf16_t* vb = vc + (int64_t)b * v_bs + (int64_t)kvh * D + sub * 8;
    const int last = end - 1;
    for (int j0 = start + w * (kUnroll * KPW); j0 < end; j0 += kDecodeWaves * kUnroll * KPW) {
      u16x8 kr[kUnroll], vr[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int jc = min(j0 + u * KPW + slot, last);
        kr[u] = *reinterpret_cast<const u16x8*>(kb + (int64_t)jc * k_ts);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int jc = min(j0 + u * KPW + slot, last);
        vr[u] = *reinterpret_cast<const u16x8*>(vb + (int64_t)jc * v_ts);
      }
      // scores: partial dot over this lane's 8 dims, summed over the key's LPK lanes
      float s[kUnroll][REP];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        float kf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) kf[e] = bf2f(kr[u][e]);
        const bool valid = j0 + u * KPW + slot < end;
#pragma unroll
        for (int r = 0; r < REP; ++r) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) d = fmaf(qf[r][e], kf[e], d);
#pragma unroll
          for (int o = 1; o < LPK; o <<= 1) d += __shfl_xor(d, o, 64);
          s[u][r] = valid ? d : -INFINITY;
        }
      }
      // online softmax, one rescale per kUnroll keys
      float p[kUnroll][REP];
#pragma unroll
      for (int r = 0; r < REP; ++r) {
        float mn = m[r];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) mn = fmaxf(mn, s[u][r]);
        const float ms = mn == -INFINITY ? 0.f : mn;   // nothing valid yet: every weight 0
        const float alpha = exp2_fast(m[r] - ms);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          p[u][r] = exp2_fast(s[u][r] - ms);
          ps += p[u][r];
        }
        l[r] = l[r] * alpha + ps;
        m[r] = mn;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r][e] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        float vf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) vf[e] = bf2f(vr[u][e]);
#pragma unroll
        for (int r = 0; r < REP; ++r)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][e] = fmaf(p[u][r], vf[e], acc[r][e]);
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
      float a = acc[r][e] * sc;
#pragma unroll
      for (int o = LPK; o < MP_WAVE; o <<= 1) a += __shfl_xor(a, o, 64);
      acc[r][e] = a;
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
      for (int e = 0; e < 8; ++e) sh_o[w][r][sub * 8 + e] = acc[r][e];
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
int launch(const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B, int H, int Hkv,
           int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts,
           int64_t o_stride, float scale, int splits, hipStream_t st) {
  const int rep = H / Hkv;
  const int chunk = (max_len + splits - 1) / splits;
  float* part_o = ws;
  float* part_ml = ws + (int64_t)B * H * splits * D;
  attn_decode_partial<D, REP><<<dim3(splits, Hkv, B), kDecodeThreads, 0, st>>>(
      (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, lens, part_o, part_ml, H, rep, Smax, chunk, q_stride, k_bs,
      k_ts, v_bs, v_ts, scale * 1.4426950408889634f);
  attn_split_combine<D><<<attn_split_combine_grid(B, H), D, 0, st>>>(part_o, part_ml, (bf16_t*)o, B, H, splits,
                                                                      o_stride);
  return (int)hipGetLastError();
}

template <int D>
int launch_rep(int rep, const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B, int H,
               int Hkv, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs,
               int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st) {
#define MP_DECODE_GO(R)                                                                                         \
  return launch<D, R>(q, k, v, lens, o, ws, B, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts, o_stride, \
                      scale, splits, st)
  if (rep == 1) MP_DECODE_GO(1);
  if (rep == 2) MP_DECODE_GO(2);
  if (rep <= 4) MP_DECODE_GO(4);
  MP_DECODE_GO(8);
#undef MP_DECODE_GO
}

}  // namespace

// Number of key splits for B sequences x Hkv KV heads over caches of up to max_len keys:
// enough workgroups for kDecodeWgPerCU per CU, but no chunk shorter than kDecodeMinChunk.
extern "C" int mp_attn_decode_plan(int B, int Hkv, int max_len) {
  if (B < 1 || Hkv < 1 || max_len < 1) return 1;
  const int64_t groups = (int64_t)B * Hkv;
  const int64_t want = (kDecodeCUs * kDecodeWgPerCU + groups - 1) / groups;
  const int64_t cap = max_len / kDecodeMinChunk;
  int64_t s = want < cap ? want : cap;
  if (s > kDecodeMaxSplits) s = kDecodeMaxSplits;
  return s < 1 ? 1 : (int)s;
}

extern "C" int64_t mp_attn_decode_ws_floats(int B, int H, int D, int splits) {
  return (int64_t)B * H * splits * (D + 2);
}

// q [B, H*D] rows (row stride q_stride), k/v caches [B, Smax, Hkv*D] (batch / token strides),
// lens int32 [B] on the device (valid keys per sequence, current token included), o [B, H*D]
// rows.  max_len >= max(lens) sizes the grid; splits: 0 = mp_attn_decode_plan's choice,
// n > 0 forces n (at most min(max_len, 256)); ws holds mp_attn_decode_ws_floats(B, H, D, splits) floats for that count.
// All strides in elements; every q/k/v row must be 16-byte aligned.  Returns -1 for an
// unsupported shape.
extern "C" int mp_attn_decode(const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B,
                              int H, int Hkv, int D, int Smax, int max_len, int64_t q_stride, int64_t k_bs,
                              int64_t k_ts, int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale, int splits,
                              hipStream_t st) {
  if ((D != 64 && D != 128) || Hkv < 1 || H < 1 || H % Hkv != 0 || H / Hkv > 8) return -1;
  if (B < 1 || B > 65535 || Hkv > 65535 || Smax < 1 || max_len < 1 || max_len > Smax) return -1;
  if (splits == 0) splits = mp_attn_decode_plan(B, Hkv, max_len);
  if (splits < 1 || splits > max_len || splits > kDecodeMaxSplits || ws == nullptr) return -1;
  if ((q_stride | k_bs | k_ts | v_bs | v_ts) % 8 != 0) return -1;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 != 0) return -1;
  const int rep = H / Hkv;
  if (D == 64)
    return launch_rep<64>(rep, q, k, v, lens, o, ws, B, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts,
                          o_stride, scale, splits, st);
  return launch_rep<128>(rep, q, k, v, lens, o, ws, B, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts,
                         o_stride, scale, splits, st);
}
