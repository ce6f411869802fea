// Multi-token (append) attention over a per-sequence KV cache, bf16, gfx950.
//
// T new tokens per sequence, already appended to the cache at rows base[b] .. base[b] + T - 1
// (rope_kv_append runs first); query (b, t) sees the keys j <= base[b] + t.  base and counts
// live on the device and are clamped before they become an index: array contents can change
// results, never an address (the rule of attention_doc.hip and attention_decode.hip).
//
// The M rows of the matrix products are the R = T * rep (token, query head of one KV head)
// pairs, token-major (row r = t * rep + head-of-group), in tiles of 32.  Two launches:
//
//  1. attn_append_partial, grid (split, Hkv, B * query tiles), 256 threads.  A workgroup owns
//     one key chunk [split * chunk, (split + 1) * chunk) of one KV head for one query tile;
//     its four waves share the 32 query rows and take every fourth 32-key tile of the chunk,
//     so a cache row is read once per (KV head, query tile).  Per tile a wave computes
//     S^T = K Q^T (mfma 32x32x16 bf16: K rows go from global memory straight into the A
//     fragment, one 16-byte load per lane and k-step, Q is the B fragment and stays in
//     registers), masks with one compare per element (key <= base + t of the lane's row),
//     runs the online softmax in exp2 units with the query on the lane, and feeds the packed
//     P^T accumulator as the B operand of O^T += V^T P^T.  V needs the transposed read: the
//     wave stages its 32 rows into a private, double-buffered swizzled LDS tile
//     (mp_attn_tiles.h) and reads it back with ds_read_b64_tr_b16, as attention.hip does.
//     Loads of the next tile are issued before the current one is used.  The four waves are
//     merged through LDS in wave order and the workgroup writes an unnormalised f32 row plus
//     (max, sum) per query row into the workspace.
//  2. attn_split_combine (mp_attn_split.h), the decode kernel's combine pass with B * T rows:
//     merges the splits in split order and writes bf16.
//
// A query tile stops at the last key its last real token may see, so key tiles above it are
// skipped and a split wholly past it writes (-inf, 0) and zero rows.  Rows t >= counts[b]
// are zero query rows whose every score is masked: they get (-inf, 0), and the combine
// writes an exact zero row for them.  Keys at or beyond base[b] + counts[b] never enter a
// result: a lane whose key index is past the chunk's end re-reads the chunk's last valid row
// (always inside the valid part of the cache), so no stale row reaches a register, and its
// score is -inf.  No atomics: results are bit-identical from run to run.
#include "mp_api.h"
#include "mp_attn_split.h"
#include "mp_attn_tiles.h"

namespace {

constexpr int kAppendThreads = 256;
constexpr int kAppendWaves = kAppendThreads / MP_WAVE;
constexpr int kQT = 32;                    // query rows (token, head) per workgroup
constexpr int kKT = 32;                    // keys per wave tile
constexpr int kAppendMinChunk = 256;       // planner: no chunk under two passes of the four waves
constexpr int kAppendCUs = 256;
constexpr int kAppendWgPerCU = 2;
constexpr int kAppendMaxSplits = kSplitMaxSplits;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int DP>
constexpr int append_lds_bytes() {
  constexpr int stage = kAppendWaves * 2 * kKT * DP * 2;           // V tiles, two per wave
  constexpr int merge = kAppendWaves * kQT * (DP + 4) * 4;         // f32 rows, padded
  return stage > merge ? stage : merge;
}

// this wave's K fragments and V rows of the 32-key tile at j0 (rows clamped to `last`)
template <int DP>
struct KVRegs {
  u16x8 k[DP / 16], v[DP / 16];
  __device__ __forceinline__ void load(const bf16_t* kb, const bf16_t* vb, int64_t k_ts, int64_t v_ts, int j0,
                                       int last) {
    const int lane = threadIdx.x & 63, l32 = lane & 31, hl = lane >> 5;
    const bf16_t* kr = kb + (int64_t)min(j0 + l32, last) * k_ts + 8 * hl;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) k[s] = *reinterpret_cast<const u16x8*>(kr + 16 * s);
#pragma unroll
    for (int i = 0; i < DP / 16; ++i) {
      const int idx = lane + 64 * i;
      const int r = idx / (DP / 8), c = idx % (DP / 8);
      v[i] = *reinterpret_cast<const u16x8*>(vb + (int64_t)min(j0 + r, last) * v_ts + c * 8);
    }
  }
  __device__ __forceinline__ void store_v(char* lds) const {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < DP / 16; ++i) {
      const int idx = lane + 64 * i;
      const int r = idx / (DP / 8), c = idx % (DP / 8);
      *reinterpret_cast<u16x8*>(lds + lds_off<DP>(r, c)) = v[i];
    }
  }
};

template <int DP>
__global__ __launch_bounds__(kAppendThreads) void attn_append_partial(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ base, const int* __restrict__ counts, float* __restrict__ part_o,
    float* __restrict__ part_ml, int T, int H, int rep, int Smax, int chunk, int nqt, int64_t q_stride, int64_t k_bs,
    int64_t k_ts, int64_t v_bs, int64_t v_ts, float scale_log2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float sh_m[kAppendWaves][kQT];
  __shared__ float sh_l[kAppendWaves][kQT];
  constexpr int VT = kKT * DP * 2;  // bytes of one staged V tile
  const int split = blockIdx.x, kvh = blockIdx.y, nsplit = gridDim.x;
  const int b = (int)blockIdx.z / nqt, qt = (int)blockIdx.z % nqt;
  const int lane = threadIdx.x & 63, l32 = lane & 31, hl = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

  const int bs = clampi(base[b], 0, Smax);
  const int cnt = clampi(counts ? counts[b] : T, 0, min(T, Smax - bs));
  const int R = T * rep;
  // this lane's query row: token t, query head hq
  const int r = qt * kQT + l32;
  const int t = r / rep;
  const int hq = kvh * rep + r % rep;
  const bool rvalid = r < R && t < cnt;
  const int qpos = bs + t;                                  // the last key the row sees
  // keys the tile may see: [0, base + its last real token]
  const int t_first = (qt * kQT) / rep;
  const int t_last = min(min(qt * kQT + kQT - 1, R - 1) / rep, cnt - 1);
  const int kv_end = t_last >= t_first ? bs + t_last + 1 : 0;      // <= bs + cnt <= Smax
  const int start = split * chunk;
  const int end = min(start + chunk, kv_end);

  bf16x8 qf[DP / 16];
#pragma unroll
  for (int s = 0; s < DP / 16; ++s) {
    u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rvalid)
      z = *reinterpret_cast<const u16x8*>(q + ((int64_t)b * T + t) * q_stride + (int64_t)hq * DP + 16 * s + 8 * hl);
    qf[s] = __builtin_bit_cast(bf16x8, z);
  }
  f32x16 o[DP / 32];
#pragma unroll
  for (int d = 0; d < DP / 32; ++d) o[d] = {};
  float m_run = -INFINITY, l_run = 0.f;

  if (start < end) {   // uniform over the workgroup
    const bf16_t* kb = kc + (int64_t)b * k_bs + (int64_t)kvh * DP;
    const bf16_t* vb = vc + (int64_t)b * v_bs + (int64_t)kvh * DP;
    const int last = end - 1;
    char* vl = smem + w * 2 * VT;
    KVRegs<DP> cur, nxt;
    if (start + w * kKT < end) cur.load(kb, vb, k_ts, v_ts, start + w * kKT, last);
    int buf = 0;
    for (int it = start; it < end; it += kAppendWaves * kKT, buf ^= 1) {
      const int j0 = it + w * kKT;
      const bool live = j0 < end;
      if (live) cur.store_v(vl + buf * VT);
      if (j0 + kAppendWaves * kKT < end) nxt.load(kb, vb, k_ts, v_ts, j0 + kAppendWaves * kKT, last);
      __syncthreads();
      if (live) {
        const char* vt = vl + buf * VT;
        f32x16 s0 = {};
#pragma unroll
        for (int s = 0; s < DP / 16; ++s) s0 = mfma32(__builtin_bit_cast(bf16x8, cur.k[s]), qf[s], s0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kj = j0 + (e & 3) + 8 * (e >> 2) + 4 * hl;
          if (kj >= end || kj > qpos || !rvalid) s0[e] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s0[e]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx * scale_log2);
        // nothing visible yet: the running maximum is still -inf, and 2^(-inf - 0) = 0 keeps
        // l and O at zero
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        float rs = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[e], scale_log2, -m_use));
          rs += p;
          s0[e] = p;
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
int launch(const void* q, const void* k, const void* v, const int* base, const int* counts, void* o, float* ws, int B,
           int T, int H, int Hkv, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs,
           int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st) {
  const int rep = H / Hkv;
  const int nqt = (T * rep + kQT - 1) / kQT;
  const int chunk = (max_len + splits - 1) / splits;
  float* part_o = ws;
  float* part_ml = ws + (int64_t)B * T * H * splits * D;
  constexpr int lds = append_lds_bytes<D>();
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)attn_append_partial<D>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  attn_append_partial<D><<<dim3(splits, Hkv, B * nqt), kAppendThreads, lds, st>>>(
      (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, base, counts, part_o, part_ml, T, H, rep, Smax, chunk, nqt,
      q_stride, k_bs, k_ts, v_bs, v_ts, scale * LOG2E);
  attn_split_combine<D><<<attn_split_combine_grid(B * T, H), D, 0, st>>>(part_o, part_ml, (bf16_t*)o, B * T, H,
                                                                          splits, o_stride);
  return (int)hipGetLastError();
}

}  // namespace

// Number of key splits for B sequences x T new tokens x Hkv KV heads of rep query heads each
// over caches of up to max_len keys: the decode planner's rule with one group per
// (sequence, KV head, query tile): enough workgroups for kAppendWgPerCU per CU, but no chunk
// shorter than kAppendMinChunk.
extern "C" int mp_attn_append_plan(int B, int T, int Hkv, int rep, int max_len) {
  if (B < 1 || T < 1 || Hkv < 1 || rep < 1 || max_len < 1) return 1;
  const int64_t nqt = ((int64_t)T * rep + kQT - 1) / kQT;
  const int64_t groups = (int64_t)B * Hkv * nqt;
  const int64_t want = (kAppendCUs * kAppendWgPerCU + groups - 1) / groups;
  const int64_t cap = max_len / kAppendMinChunk;
  int64_t s = want < cap ? want : cap;
  if (s > kAppendMaxSplits) s = kAppendMaxSplits;
  return s < 1 ? 1 : (int)s;
}

extern "C" int64_t mp_attn_append_ws_floats(int B, int T, int H, int D, int splits) {
  return (int64_t)B * T * H * splits * (D + 2);
}

// q/o [B*T, H*D] rows (row strides q_stride / o_stride; row b*T + t is new token t of
// sequence b), k/v caches [B, Smax, Hkv*D] (batch / token strides), base int32 [B] on the
// device (valid cache rows before this call), counts int32 [B] on the device or null (= T):
// how many of the row's T tokens are real.  The new tokens' K/V rows are already in the cache
// at base[b] + t.  max_len >= max(base + counts) sizes the grid; splits: 0 =
// mp_attn_append_plan's choice, n > 0 forces n (at most min(max_len, 256)); ws holds
// mp_attn_append_ws_floats(B, T, H, D, splits) floats for that count.  All strides in
// elements; every q/k/v row must be 16-byte aligned.  Returns -1 for an unsupported shape.
extern "C" int mp_attn_append(const void* q, const void* k, const void* v, const int* base, const int* counts, void* o,
                              float* ws, int B, int T, int H, int Hkv, int D, int Smax, int max_len, int64_t q_stride,
                              int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale,
                              int splits, hipStream_t st) {
  if ((D != 64 && D != 128) || Hkv < 1 || H < 1 || H % Hkv != 0 || H / Hkv > 8) return -1;
  if (B < 1 || T < 1 || Hkv > 65535 || H > 65535 || Smax < 1 || max_len < 1 || max_len > Smax) return -1;
  const int rep = H / Hkv;
  const int64_t nqt = ((int64_t)T * rep + kQT - 1) / kQT;
  if ((int64_t)B * nqt > 65535 || (int64_t)B * T > INT32_MAX) return -1;
  if (splits == 0) splits = mp_attn_append_plan(B, T, Hkv, rep, max_len);
  if (splits < 1 || splits > max_len || splits > kAppendMaxSplits || ws == nullptr || base == nullptr) return -1;
  if ((q_stride | k_bs | k_ts | v_bs | v_ts) % 8 != 0) return -1;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 != 0) return -1;
  if (D == 64)
    return launch<64>(q, k, v, base, counts, o, ws, B, T, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts,
                      o_stride, scale, splits, st);
  return launch<128>(q, k, v, base, counts, o, ws, B, T, H, Hkv, Smax, max_len, q_stride, k_bs, k_ts, v_bs, v_ts,
                     o_stride, scale, splits, st);
}
