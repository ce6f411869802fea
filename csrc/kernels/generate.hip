// Kernels of the ragged, host-value-free decode step (models/generate.py), gfx950.  Every
// position comes from device memory and is clamped before it becomes an address: array
// contents may change results, never an address (the rule of attention_doc.hip).
//
//   embed_pos       out[b, :] = wte[idx[b], :] (+ wpe[pos[b], :]): embed_fwd at S = 1 with a
//                   per-row device position.  One wave per row, 16-byte vectors.
//   rope_kv_append  per row b * T + t (new token t of sequence b) of packed
//                   [B * T, (H + 2 Hkv) Dh] qkv rows, at p = pos[b] + t: q rotated in place
//                   at p (rope_rot4 of mp_rope.h, the arithmetic of rope_kernel, so the
//                   bits are those of rope at pos_offset = p); k rotated into
//                   k_cache[b, p, :] (the qkv row keeps the unrotated k); v copied to
//                   v_cache[b, p, :].  rope = 0: the two appends alone.  A row with
//                   active[b] == 0 or t >= counts[b] is left alone altogether.  One thread per 16-byte vector
//                   (rotations: a 16-byte vector of each half); replaces one rope and two
//                   copy launches per layer.
//   sample          one 1024-thread workgroup per row of logits [B, Vp] (bf16 or f32, row
//                   stride ld): greedy / temperature / top-k / top-p / inverse-CDF draw from
//                   u[b], with a done mask and a stop token.  z_j = logit_j / temperature in
//                   f32 over j < V only.
//
// sample, storage and passes.  Thread t owns the contiguous block [t * chunk, (t + 1) * chunk)
// of the row, chunk a multiple of 8, read as 16-byte (bf16) / 2 x 16-byte (f32) vectors.  A
// row of up to 144 KiB (bf16: V <= 73728, so GPT-2's 100 KB; f32: V <= 36864) is copied once,
// as stored, into the workgroup's LDS and every pass reads that copy; a larger row (Llama-3's
// 128256 columns, or GPT-2 logits in f32) is re-read from global memory on every pass and
// stays in L2 / the CU's vector cache between passes.  z is recomputed from the stored logit
// on every pass (the same division each time).  Thresholds are found without sorting, by
// building the order-preserving 32-bit key of z from the top, one hexadecimal digit per
// pass: the 15 candidate keys of a digit are counted (or their masses summed) together:
//   greedy (temperature == 0)   1 pass  (argmax, ties to the lowest index)
//   max                         1 pass
//   top-k threshold t_k         8 counting passes   (0 < top_k < V only)
//   top-p threshold t_p         1 + 8 mass passes   (top_p < 1 only)
//   draw                        2 passes (block sums + scan, then the search in the owner's block)
// so 3 passes for plain temperature sampling and at most 20 with both filters.  Every sum is
// sequential inside a thread's block, then a fixed shuffle tree over the wave and a fixed
// sequential sum over the 16 waves: bit-identical from run to run.  No atomics.
#include "mp_api.h"
#include "mp_common.h"
#include "mp_rope.h"

#include <limits.h>

using namespace mp;

// ------------------------------------------------------------------------------ embed_pos
template <typename T>
__global__ void __launch_bounds__(256) embed_pos_kernel(const int64_t* __restrict__ idx, const int* __restrict__ pos,
                                                        const T* __restrict__ wte, const T* __restrict__ wpe,
                                                        T* __restrict__ out, int B, int D, int n_tok, int n_pos) {
  using IO = IO8<T>;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  int64_t tok = idx[b];
  tok = tok < 0 ? 0 : (tok >= n_tok ? n_tok - 1 : tok);
  const T* src = wte + (size_t)tok * D;
  const T* psrc = nullptr;
  if (wpe) {
    int p = pos[b];
    p = p < 0 ? 0 : (p >= n_pos ? n_pos - 1 : p);
    psrc = wpe + (size_t)p * D;
  }
  T* dst = out + (size_t)b * D;
  for (int c = lane; c < D / 8; c += 64) {
    typename IO::Raw v = IO::load(src + c * 8);
    if (psrc) {
      const typename IO::Raw p = IO::load(psrc + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) IO::set(v, e, IO::get(v, e) + IO::get(p, e));
    }
    IO::store(dst + c * 8, v);
  }
}

extern "C" int mp_embed_pos(const int64_t* idx, const int* pos, const void* wte, const void* wpe, void* out, int B,
                            int D, int n_tok, int n_pos, int f32, hipStream_t st) {
  if (D % 8 || B < 1 || n_tok < 1 || (wpe && n_pos < 1)) return -1;
  if (f32)
    embed_pos_kernel<float><<<(B + 3) / 4, 256, 0, st>>>(idx, pos, (const float*)wte, (const float*)wpe, (float*)out,
                                                         B, D, n_tok, n_pos);
  else
    embed_pos_kernel<bf16_t><<<(B + 3) / 4, 256, 0, st>>>(idx, pos, (const bf16_t*)wte, (const bf16_t*)wpe,
                                                          (bf16_t*)out, B, D, n_tok, n_pos);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------- rope_kv_append
// Work items of one sequence, each one thread:
//   rope:   [0, H * h8)                    q head h, vector i of each half: rotate in place
//           [.., + Hkv * h8)               k head h, vector i of each half: rotate -> k_cache
//           [.., + Hkv * 2 h8)             v vectors -> v_cache
//   plain:  [0, Hkv * 2 h8)                k vectors -> k_cache, then the same of v
// with h8 = Dh / 16 vectors per half head.
__global__ void __launch_bounds__(256) rope_kv_append_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ cs,
                                                             const float* __restrict__ sn, bf16_t* __restrict__ kc,
                                                             bf16_t* __restrict__ vc, const int* __restrict__ pos,
                                                             const uint8_t* __restrict__ active,
                                                             const int* __restrict__ counts, int T, int H, int Hkv,
                                                             int Dh, int Smax, int64_t qkv_ld, int64_t k_bs,
                                                             int64_t k_ts, int64_t v_bs, int64_t v_ts, int rope) {
  const int n = blockIdx.x;                  // row b * T + t: new token t of sequence b
  const int b = n / T, t = n % T;
  if (active && !active[b]) return;
  if (counts && t >= counts[b]) return;
  int p = pos[b];
  p = p < 0 ? 0 : (p >= Smax ? Smax - 1 : p);
  p = min(p + t, Smax - 1);
  const int half = Dh / 2, h8 = half / 8;
  bf16_t* row = qkv + (int64_t)n * qkv_ld;
  bf16_t* krow = kc + (int64_t)b * k_bs + (int64_t)p * k_ts;
  bf16_t* vrow = vc + (int64_t)b * v_bs + (int64_t)p * v_ts;
  const int n_rot = rope ? (H + Hkv) * h8 : 0;
  const int n_kcopy = rope ? 0 : Hkv * 2 * h8;
  const int n_vcopy = Hkv * 2 * h8;
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i < n_rot) {
    const int h = i / h8, v8 = i % h8;       // h < H: a q head, else k head h - H
    const bf16_t* src = row + (int64_t)h * Dh + v8 * 8;
    bf16_t* dst = h < H ? row + (int64_t)h * Dh + v8 * 8 : krow + (int64_t)(h - H) * Dh + v8 * 8;
    const u16x8 x1 = *reinterpret_cast<const u16x8*>(src);
    const u16x8 x2 = *reinterpret_cast<const u16x8*>(src + half);
    const float* cr = cs + (int64_t)p * half;
    const float* sr = sn + (int64_t)p * half;
    u16x4 a1, a2, b1, b2;
    rope_rot4(u16x4{x1[0], x1[1], x1[2], x1[3]}, u16x4{x2[0], x2[1], x2[2], x2[3]}, cr, sr, v8 * 8, 1.0f, a1, a2);
    rope_rot4(u16x4{x1[4], x1[5], x1[6], x1[7]}, u16x4{x2[4], x2[5], x2[6], x2[7]}, cr, sr, v8 * 8 + 4, 1.0f, b1,
              b2);
    *reinterpret_cast<u16x8*>(dst) = u16x8{a1[0], a1[1], a1[2], a1[3], b1[0], b1[1], b1[2], b1[3]};
    *reinterpret_cast<u16x8*>(dst + half) = u16x8{a2[0], a2[1], a2[2], a2[3], b2[0], b2[1], b2[2], b2[3]};
    return;
  }
  int c = i - n_rot;
  if (c < n_kcopy) {
    *reinterpret_cast<u16x8*>(krow + c * 8) = *reinterpret_cast<const u16x8*>(row + (int64_t)H * Dh + c * 8);
    return;
  }
  c -= n_kcopy;
  if (c < n_vcopy)
    *reinterpret_cast<u16x8*>(vrow + c * 8) = *reinterpret_cast<const u16x8*>(row + (int64_t)(H + Hkv) * Dh + c * 8);
}

extern "C" int mp_rope_kv_append(void* qkv, const float* cs, const float* sn, void* kc, void* vc, const int* pos,
                                 const uint8_t* active, const int* counts, int B, int T, int H, int Hkv, int Dh,
                                 int Smax, int64_t qkv_ld, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts,
                                 int rope, hipStream_t st) {
  if ((Dh != 64 && Dh != 128) || B < 1 || T < 1 || (int64_t)B * T > INT_MAX || H < 1 || Hkv < 1 || Smax < 1) return -1;
  if (rope && (!cs || !sn)) return -1;
  const int h8 = Dh / 16;
  const int items = rope ? (H + Hkv) * h8 + Hkv * 2 * h8 : 2 * Hkv * 2 * h8;
  if ((items + 255) / 256 > 65535) return -1;
  dim3 grid(B * T, (items + 255) / 256);
  rope_kv_append_kernel<<<grid, 256, 0, st>>>((bf16_t*)qkv, cs, sn, (bf16_t*)kc, (bf16_t*)vc, pos, active, counts, T, H,
                                              Hkv, Dh, Smax, qkv_ld, k_bs, k_ts, v_bs, v_ts, rope);
  return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------- sample
#define SAMPLE_NT 1024

// The order-preserving key of an f32 z (-0 folded into +0) is its bit pattern u with the sign
// bit set when z >= 0 and all bits flipped when z < 0: a < b  <=>  key(a) < key(b).  The
// thresholds are built as keys, digit by digit, and compared as floats: key_floor(k) is the
// value a key stands for, z >= key_floor(k)  <=>  key(z) >= k for every non-NaN z.  Keys at
// or below key(-inf) (the negative-NaN patterns) admit everything; keys above key(+inf) come
// back as NaN, which no z reaches.
__device__ __forceinline__ float key_floor(uint32_t k) {
  if (k <= 0x007FFFFFu) return -INFINITY;
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// a value every thread of the workgroup computed alike, moved to a scalar register
__device__ __forceinline__ uint32_t uniform_u(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform_f(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the 15 per-thread partials of one digit -> 15 block-wide sums in every thread, in a fixed
// order (shuffle tree over the wave, then the 16 waves one after the other)
// (the sums over the waves are real loops: unrolled, their 240 LDS reads would all be in
// flight at once and push the row's registers into scratch)
__device__ __forceinline__ float wave_sum_any(float v) { return wave_sum(v); }
__device__ __forceinline__ int wave_sum_any(int v) { return wave_sum_i(v); }
template <typename V>
__device__ __forceinline__ void block_sum15(V (&v)[15], V* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 15; ++i) v[i] = wave_sum_any(v[i]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 15; ++i) red[w * 15 + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 15; ++i) {
    V t = 0;
#pragma unroll 1
    for (int x = 0; x < 16; ++x) t += red[x * 15 + i];
    v[i] = t;
  }
}

// block-wide integer reductions over SAMPLE_NT threads; op: 0 sum, 1 min, 2 max
template <int OP>
__device__ __forceinline__ int block_red_i(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o, 64);
    v = OP == 0 ? v + t : (OP == 1 ? min(v, t) : max(v, t));
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int i = 1; i < SAMPLE_NT / 64; ++i) r = OP == 0 ? r + red[i] : (OP == 1 ? min(r, red[i]) : max(r, red[i]));
  return r;
}

static_assert(SAMPLE_NT == 1024, "block_sum15 and the scan assume 16 waves");

// The thread's block [j0, j1) of the row (global memory, or the workgroup's LDS copy).
// each(f) calls f(j, z_j) in index order; slots at j >= V count as z = -inf (no mass, never
// above a threshold a real z decides), and f checks j < V where a slot's index matters.
template <typename T>
struct SampleRow {
  const T* row;
  int V, j0, j1;
  float temperature;

  __device__ __forceinline__ float zval(float x) const {
    return (temperature > 0.f ? x / temperature : x) + 0.0f;      // -0 folded into +0
  }
  template <typename F>
  __device__ __forceinline__ void each(F&& f) const {
    for (int c = j0; c < j1; c += 8) {
      const typename IO8<T>::Raw r = IO8<T>::load(row + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) f(c + e, c + e < V ? zval(IO8<T>::get(r, e)) : -INFINITY);
    }
  }
};

// STAGE: the launcher gave vend * sizeof(T) bytes of dynamic LDS for the row
template <typename T, bool STAGE>
__global__ void __launch_bounds__(SAMPLE_NT) sample_kernel(const T* __restrict__ logits, int64_t ld,
                                                           const float* __restrict__ u, uint8_t* __restrict__ done,
                                                           int64_t* __restrict__ out, int V, float temperature,
                                                           int top_k, float top_p, int stop_token, int pad_token) {
  extern __shared__ __attribute__((aligned(16))) unsigned char staged[];
  __shared__ float redf[16 * 15];
  __shared__ int redi[16 * 15];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  if (done && done[b]) {   // uniform over the workgroup
    if (tid == 0) out[b] = pad_token;
    return;
  }
  const int chunk = (((V + SAMPLE_NT - 1) / SAMPLE_NT) + 7) & ~7;
  const int vend = (V + 7) & ~7;   // <= Vp: Vp is a multiple of 8
  SampleRow<T> R;
  R.row = logits + (int64_t)b * ld;
  if (STAGE) {     // one coalesced read of the row; every pass then reads the LDS copy
    T* copy = reinterpret_cast<T*>(staged);
    for (int c = tid * 8; c < vend; c += SAMPLE_NT * 8) IO8<T>::store(copy + c, IO8<T>::load(R.row + c));
    __syncthreads();
    R.row = copy;
  }
  R.V = V;
  R.j0 = min(tid * chunk, vend);
  R.j1 = min(R.j0 + chunk, vend);
  R.temperature = temperature;
  int token;

  if (temperature == 0.f) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    R.each([&](int j, float z) {
      if (j < V && (z > bv || bi == INT_MAX)) {
        bv = z;
        bi = j;
      }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    __syncthreads();
    if (lane == 0) {
      redf[wv] = bv;
      redi[wv] = bi;
    }
    __syncthreads();
    bv = redf[0];
    bi = redi[0];
    for (int i = 1; i < SAMPLE_NT / 64; ++i) {
      const float ov = redf[i];
      const int oi = redi[i];
      if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    token = bi;
  } else {
    // max of z
    float m = -INFINITY;
    R.each([&](int, float z) { m = fmaxf(m, z); });
    m = uniform_f(block_max<SAMPLE_NT>(m, redf));
    // top-k: the largest key t with |{key >= t}| >= k is the k-th largest key; one
    // hexadecimal digit of t per pass (the counts fall as the digit rises)
    uint32_t thr = 0;
    if (top_k > 0 && top_k < V) {
      for (int sh = 28; sh >= 0; sh -= 4) {
        float cf[15];
        int n[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) {
          cf[i] = key_floor(thr | ((uint32_t)(i + 1) << sh));
          n[i] = 0;
        }
        R.each([&](int, float z) {
#pragma unroll
          for (int i = 0; i < 15; ++i) n[i] += z >= cf[i] ? 1 : 0;
        });
        block_sum15(n, redi);
        uint32_t d = 0;
#pragma unroll
        for (int i = 0; i < 15; ++i) d = n[i] >= top_k ? (uint32_t)(i + 1) : d;
        thr = uniform_u(thr | (d << sh));
      }
    }
    // top-p over the kept set: the largest key t whose mass {key >= t} is >= top_p * W
    if (top_p < 1.f) {
      const float tkf = key_floor(thr);
      float s = 0.f;
      R.each([&](int, float z) { s += z >= tkf ? __expf(z - m) : 0.f; });
      const float need = uniform_f(top_p * block_sum<SAMPLE_NT>(s, redf));
      const uint32_t tk = thr;
      uint32_t t = 0;
      for (int sh = 28; sh >= 0; sh -= 4) {
        float cf[15], a[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) {
          const uint32_t cand = t | ((uint32_t)(i + 1) << sh);
          cf[i] = key_floor(cand > tk ? cand : tk);
          a[i] = 0.f;
        }
        R.each([&](int, float z) {
          const float w = __expf(z - m);
#pragma unroll
          for (int i = 0; i < 15; ++i) a[i] += z >= cf[i] ? w : 0.f;
        });
        block_sum15(a, redf);
        uint32_t d = 0;
#pragma unroll
        for (int i = 0; i < 15; ++i) d = a[i] >= need ? (uint32_t)(i + 1) : d;
        t = uniform_u(t | (d << sh));
      }
      thr = t > tk ? t : tk;
    }
    // draw: block sums, exclusive scan over the threads in index order, search in the block
    const float thrf = key_floor(thr);
    float s = 0.f;
    int last = -1;
    R.each([&](int j, float z) {
      if (j < V && z >= thrf) {
        s += __expf(z - m);
        last = j;
      }
    });
    float inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    float excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 0.f;
    __syncthreads();
    if (lane == 63) redf[wv] = inc;
    __syncthreads();
    float base = 0.f, W = 0.f;
    for (int i = 0; i < SAMPLE_NT / 64; ++i) {
      if (i == wv) base = W;
      W += redf[i];
    }
    const float target = u[b] * W;
    float run = base + excl;
    int found = INT_MAX;
    R.each([&](int j, float z) {
      if (j < V && z >= thrf) {
        run += __expf(z - m);
        if (run > target && found == INT_MAX) found = j;
      }
    });
    found = block_red_i<1>(found, redi);
    last = block_red_i<2>(last, redi);
    token = found != INT_MAX ? found : last;
  }
  token = token < 0 ? 0 : (token >= V ? V - 1 : token);
  if (tid == 0) {
    out[b] = token;
    if (done && token == stop_token) done[b] = 1;
  }
}

extern "C" int mp_sample(const void* logits, int64_t ld, const float* u, uint8_t* done, int64_t* out, int B, int V,
                         int Vp, float temperature, int top_k, float top_p, int stop_token, int pad_token, int f32,
                         hipStream_t st) {
  if (B < 1 || V < 1 || V > Vp || Vp % 8 || ld < Vp || ld % (f32 ? 4 : 8)) return -1;
  if (!(temperature >= 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f)) return -1;
  if (temperature > 0.f && !u) return -1;
  // the row goes to LDS when it fits beside the reduction buffers (144 KiB of the 160)
  const size_t bytes = (size_t)((V + 7) & ~7) * (f32 ? 4 : 2);
  const bool stage = bytes <= 144 * 1024;
  const auto launch = [&](auto kern, auto* row) {
    if (stage && bytes > 48 * 1024)
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    kern<<<B, SAMPLE_NT, stage ? bytes : 0, st>>>(row, ld, u, done, out, V, temperature, top_k, top_p, stop_token,
                                                  pad_token);
  };
  if (f32) {
    if (stage) launch(sample_kernel<float, true>, (const float*)logits);
    else launch(sample_kernel<float, false>, (const float*)logits);
  } else {
    if (stage) launch(sample_kernel<bf16_t, true>, (const bf16_t*)logits);
    else launch(sample_kernel<bf16_t, false>, (const bf16_t*)logits);
  }
  return (int)hipGetLastError();
}
