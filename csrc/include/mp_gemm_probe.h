// Engines with recorded null results, built only with MP_PROBE_ENGINES (tools/build_ext.py
// --variant probes -D MP_PROBE_ENGINES): stream-K gemm7 (cfg 14), gemm4 (cfg 7 / 100 + G) and
// gemm5 (cfg 8).  gemm7 runs its whole rounds on gemm3: include mp_gemm_pingpong.h first.
#pragma once

#include "mp_gemm_core.h"
#include "mp_gemm_pingpong.h"
#include "mp_gemm_plan.h"

namespace g2 {

// ---------------------------------------------------------------------------------------
// gemm7: the PARTIAL round of a 256x256 NT GEMM split over all CUs -- a pipeline rank's
// 8K-32K-token microbatches are 96-384 tiles of 256x256 for N = 768, i.e. 0.4-1.5 rounds of
// 256 CUs (profiles/r5_gemm7_*).  The host runs the whole rounds as a plain gemm3 launch on
// the leading rows and this kernel on the remaining tail rows (mp_gemm2, cfg 14).
//
// The tail's tiles are split into 8 XCD groups (consecutive tile ids; block b runs on XCD
// b % 8) and each of a group's c tiles into S K-chunks: the group's workgroup l (b = x + 8 l,
// in dispatch order) computes chunk j = l / c of tile l % c.  Workgroups of one chunk index
// walk the same K range of neighbouring tiles at the same time, so A panels are shared in
// the XCD's L2 (a stream-K walk that staggers K offsets across the tiles of one row band
// measured 2.4x slower: the A panel is re-read from HBM per tile).  Chunks 0..S-2 publish
// f32 partials; the last chunk's workgroup owns the tile: it absorbs the others (they were
// dispatched before it, hold a CU or are done -- no deadlock even when other kernels occupy
// CUs) and runs the fused epilogue.
//
// Hand-off (cdna guide §6 Guideline 16, R1): the partial is staged through LDS like the
// epilogue and stored row-major with sc1 (write-through) 16-byte buffer stores, every wave
// drains vmcnt, workgroup barrier, one agent-scope 8-byte flag store of a 64-bit tag; the
// owner's thread 0 polls the flags (bounded: a lost hand-off sets an error word instead of
// hanging), clears them, takes one agent-scope acquire, barrier, and the epilogue adds the
// partials (plain loads) to the LDS-staged accumulator before the fused epilogue.  So every flag is back to 0 when a launch ends and no
// memset node is needed before the next (one measured 5.3 us per call): a fresh workspace
// from the caching allocator can only hold the tag by a 2^-64 accident.
// ---------------------------------------------------------------------------------------
#ifndef MP_G7_SC1
#define MP_G7_SC1 0   // 1: partials by sc1 write-through buffer stores (no release fence)
#endif
constexpr int SK_SLOT = 256 * 256;          // floats per partial tile
constexpr int SK_FLAGS = 2 * 256 + 16;      // 256 64-bit flags + the error word (floats of workspace)
constexpr int SK_ERR = 2 * 256;             // error word (as a 32-bit index)
constexpr unsigned long long SK_TAG = 0x7FF7A5A55A5AC3C3ull;   // a NaN payload: never f32 data

__device__ __forceinline__ void g7_mainloop(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, int M, int N,
                                            int64_t lda, int64_t ldb, int m0, int n0, int kt0, int nk, char* smem,
                                            f32x4 (&acc)[8][4]) {
  constexpr int HALF = 128 * 128;
  constexpr int BUF = 4 * HALF;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / 4, wc = wave % 4;
  const int lr = lane >> 3;
  const int lc = (lane & 7) ^ swzq(8 * (wave & 1) + lr);
  const bf16_t* pa[2];
  const bf16_t* pb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int ra = m0 + 128 * j + 8 * wave + lr;
    ra = ra < M ? ra : M - 1;
    int rb = n0 + 64 * ((wave >> 2) + 2 * j) + 8 * (wave & 3) + lr;
    rb = rb < N ? rb : N - 1;
    pa[j] = A + (int64_t)ra * lda + (int64_t)kt0 * BK + lc * 8;
    pb[j] = B + (int64_t)rb * ldb + (int64_t)kt0 * BK + lc * 8;
  }
  const bool a1_ok0 = m0 + 64 + 8 * wave + lr < M, a1_ok1 = m0 + 192 + 8 * wave + lr < M;
  const bool b1_ok0 = n0 + 64 * (wave >> 2) + 32 + 8 * (wave & 3) + lr < N;
  const bool b1_ok1 = n0 + 64 * ((wave >> 2) + 2) + 32 + 8 * (wave & 3) + lr < N;
  const int64_t a1_off0 = a1_ok0 ? 64 * lda : 0, a1_off1 = a1_ok1 ? 64 * lda : 0;
  const int64_t b1_off0 = b1_ok0 ? 32 * ldb : 0, b1_off1 = b1_ok1 ? 32 * ldb : 0;
  auto issue = [&](int h, int kt) {
    char* img = smem + (kt & 1) * BUF + (h == 0 ? 0 : h == 3 ? HALF : h == 1 ? 2 * HALF : 3 * HALF);
    const int64_t dk = (int64_t)kt * BK;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bf16_t* src;
      if (h == 0) src = pa[j] + dk;
      else if (h == 3) src = pa[j] + dk + (j ? a1_off1 : a1_off0);
      else if (h == 1) src = pb[j] + dk;
      else src = pb[j] + dk + (j ? b1_off1 : b1_off0);
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (__attribute__((address_space(3))) void*)(img + (wave + 8 * j) * 1024), 16, 0,
                                       0);
    }
  };
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{};
  issue(0, 0);
  issue(1, 0);
  issue(2, 0);
  issue(3, 0);
  if (nk > 1) {
    issue(0, 1);
    issue(1, 1);
    wait_vmcnt<8>();
  } else {
    wait_vmcnt<4>();
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // stagger the wave rows by one barrier
  asm volatile("" ::: "memory");

  bf16x8 af[4][2], b0[2][2], b1[2][2];
  const int q = lane >> 4;
  const int rA = wr * 64 + (lane & 15);
  const int rB = wc * 32 + (lane & 15);
  auto fq = [&](const char* img, int row, int st) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(img + row * 128 + 16 * ((4 * st + q) ^ swzq(row)));
  };
#define G7_MFMA(R0, BF, C0)                                                              \
  __builtin_amdgcn_sched_barrier(0);                                                     \
  __builtin_amdgcn_s_setprio(1);                                                         \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_)                                       \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                       \
  _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                       \
    acc[R0 + i_][C0 + j_] = mfma16(af[i_][s_], BF[j_][s_], acc[R0 + i_][C0 + j_]);       \
  __builtin_amdgcn_s_setprio(0);                                                         \
  __builtin_amdgcn_sched_barrier(0);
#define G7_BAR()                          \
  asm volatile("" ::: "memory");          \
  __builtin_amdgcn_s_barrier();           \
  asm volatile("" ::: "memory");
  for (int t = 0; t < nk; ++t) {
    const char* buf = smem + (t & 1) * BUF;
    const bool steady = t + 2 < nk;
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i][s_] = fq(buf, rA + 16 * i, s_);
#pragma unroll
      for (int j = 0; j < 2; ++j) b0[j][s_] = fq(buf + 2 * HALF, rB + 16 * j, s_);
    }
    if (t + 1 < nk) issue(2, t + 1);
    if (steady) wait_vmcnt<8>(); else wait_vmcnt<0>();
    G7_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G7_MFMA(0, b0, 0);
    G7_BAR();
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int j = 0; j < 2; ++j) b1[j][s_] = fq(buf + 3 * HALF, rB + 16 * j, s_);
    if (t + 1 < nk) issue(3, t + 1);
    if (steady) wait_vmcnt<8>(); else wait_vmcnt<0>();
    G7_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G7_MFMA(0, b1, 2);
    G7_BAR();
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i][s_] = fq(buf + HALF, rA + 16 * i, s_);
    if (steady) issue(0, t + 2);
    G7_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    G7_MFMA(4, b0, 0);
    G7_BAR();
    if (steady) {
      issue(1, t + 2);
      wait_vmcnt<8>();
    } else {
      wait_vmcnt<0>();
    }
    G7_BAR();
    G7_MFMA(4, b1, 2);
    G7_BAR();
  }
#undef G7_MFMA
#undef G7_BAR
  if (wr == 0) __builtin_amdgcn_s_barrier();  // re-align the staggered wave rows
  __syncthreads();
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// a contributor's partial tile -> its slot, row-major [256][256] f32: staged through LDS one
// wave-row group at a time exactly like the epilogue (so the accumulators die as they are
// staged), then sc1 (write-through) 16-byte buffer stores; every wave drains them, a
// barrier, one agent-scope flag store
template <class StageF>
__device__ __forceinline__ void g7_publish(const StageF& stage, char* smem, int wr, float* slot,
                                           unsigned long long* flag) {
  constexpr int RG = 128, CP = 256 + 4;
  float* ct = reinterpret_cast<float*>(smem);
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(slot, 0, SK_SLOT * 4, 0x00020000);
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if (wr == pass) stage(ct, CP);
    __syncthreads();
    for (int idx = threadIdx.x; idx < RG * 64; idx += NT) {
      const int row = idx >> 6, c4 = (idx & 63) * 4;
      const float4 v = *reinterpret_cast<const float4*>(ct + row * CP + c4);
#if MP_G7_SC1
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), r, ((pass * RG + row) * 256 + c4) * 4, 0,
                                             16 /* sc1 */);
#else
      *reinterpret_cast<float4*>(slot + (pass * RG + row) * 256 + c4) = v;   // into this XCD's L2
#endif
    }
    __syncthreads();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its stores
  __syncthreads();
  if (threadIdx.x == 0) {
#if !MP_G7_SC1
    // plain stores: one agent-scope release writes the XCD L2's dirty lines back (the
    // cdna guide's split-K recipe: fence, then an explicit wait, then the signal)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __hip_atomic_store(flag, SK_TAG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the owner waits for its contributors' flags (thread 0, bounded poll), clears them for the
// next launch, and makes their partials visible to this CU: one agent-scope acquire (drops
// this CU's L1) before a barrier; the epilogue then reads them with plain loads
__device__ __forceinline__ void g7_await(unsigned long long* flags, int first, int step, int n, unsigned* err) {
  if (threadIdx.x == 0) {
    for (int p = 0; p < n; ++p) {
      unsigned long long* f = flags + first + p * step;
      unsigned spins = 0;
      while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != SK_TAG) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > (1u << 24)) {     // ~0.5 s: a lost hand-off ends the kernel, flagged
          __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
      __hip_atomic_store(f, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}

template <int EPI>
__global__ void __launch_bounds__(NT, 1) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm7_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, bf16_t* __restrict__ C,
             const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
             float* __restrict__ colsum, float* __restrict__ ws, int M, int N, int K, int64_t lda, int64_t ldb,
             int64_t ldc, int64_t ldr, int64_t ldx, float alpha, float p_drop, uint64_t seed, int S, int tile0) {
  if (p_drop > 0.f) seed = step_seed(seed);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  // the tail tiles [tile0, T) of the whole output in row-major tile order (full-matrix
  // indices: the fused dropout's mask index is the element of the whole output)
  const int gn = (N + 255) / 256, T = ((M + 255) / 256) * gn - tile0;
  const int kt = K / BK;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / 4, wn = (wave % 4) * 64;
  unsigned long long* flags = reinterpret_cast<unsigned long long*>(ws);
  float* part = ws + SK_FLAGS;
  // XCD group x owns tiles [t0, t1) (c of them); workgroup l of the group takes chunk
  // l / c of tile l % c, so one chunk index walks the same K range of neighbouring tiles
  const int x = b & 7, l = b >> 3;
  const int t0 = (int)((int64_t)x * T / 8), t1 = (int)((int64_t)(x + 1) * T / 8);
  const int c = t1 - t0;
  if (c <= 0 || l >= c * S) return;
  const int ti = l % c, j = l / c;
  const int k0 = (int)((int64_t)j * kt / S), k1 = (int)((int64_t)(j + 1) * kt / S);
  const int tile = tile0 + t0 + ti;
  const int m0 = (tile / gn) * 256, n0 = (tile % gn) * 256;
  f32x4 acc[8][4];
  g7_mainloop(A, B, M, N, lda, ldb, m0, n0, k0, k1 - k0, smem, acc);
  if (j < S - 1) {   // contributor: partial + flag
    g7_publish(Stage16<8, 4>{acc, wn, lane}, smem, wr, part + (int64_t)b * SK_SLOT, flags + b);
    return;
  }
  // owner (the last chunk): the lower chunks of this tile were dispatched before it
  g7_await(flags, x + 8 * ti, 8 * c, S - 1, reinterpret_cast<unsigned*>(ws) + SK_ERR);
  epilogue<256, 256, 2, 4, EPI, false, NT, true>(Stage16<8, 4>{acc, wn, lane}, smem, m0, n0, wr, C, bias, R, AUX,
                                       colsum, M, N, ldc, ldr, ldx, alpha, 1, p_drop, seed,
                                       part + (int64_t)(x + 8 * ti) * SK_SLOT,
                                       (int64_t)8 * c * SK_SLOT, S - 1);
}

template <int EPI>
static int launch7(const void* A, const void* B, void* C, const void* bias, const void* R, void* X, float* colsum,
                   float* ws, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx,
                   float alpha, float p_drop, uint64_t seed, hipStream_t st) {
  Plan7 pl{};
  if (!plan7(M, N, K, PlanEnv::process(), &pl) || ws == nullptr) return -1;
  constexpr int LDS_MAIN = 2 * 4 * 128 * 128;
  constexpr int EPI_BYTES = 128 * (256 + 4) * 4;
  constexpr int LDS = LDS_MAIN > EPI_BYTES ? LDS_MAIN : EPI_BYTES;
  if (pl.dp > 0) {   // the whole rounds: the ping-pong engine on the first dp tiles (row-major)
    const int rc = launch3<EPI, false, true>(A, B, C, bias, R, X, colsum, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, 1,
                                             p_drop, seed, st, pl.dp);
    if (rc != 0) return rc;
  }
  auto kern = gemm7_kernel<EPI>;
  static bool attr = false;
  lds_attr_once(attr, (const void*)kern, LDS);
  // the tail tiles [dp, T)
  const int cmax = (pl.tail + 7) / 8;
  kern<<<dim3(8 * cmax * pl.S), NT, LDS, st>>>((const bf16_t*)A, (const bf16_t*)B, (bf16_t*)C, (const bf16_t*)bias,
                                               (const bf16_t*)R, (bf16_t*)X, colsum, ws, M, N, K, lda, ldb, ldc, ldr,
                                               ldx, alpha, p_drop, seed, pl.S, pl.dp);
  return (int)hipGetLastError();
}

// gemm4 / gemm5: probe engines with recorded null results (profiles/r2_probes.md).
// ---------------------------------------------------------------------------------------
// gemm4: persistent 256x256 NT GEMM (gemm3's 16x16x32 phase schedule) whose C write is
// deferred into the NEXT tile's main loop.
//
// At K = 768 about a third of a gemm3 launch is the C write of each tile wave: all 256
// CUs store their 128 KiB at the same moment while the matrix cores idle
// (profiles/r2_probes.md "fixed vs per-K-tile cost"; hipBLASLt pays the same).  Here one
// workgroup per CU walks tiles vb = blockIdx.x + k * gridDim.x (same XCD for every k); a
// finished tile is packed to bf16 in registers (64 VGPRs, epilogue applied) and its 32
// 8-byte stores per lane go out one per phase during the first 8 K-tiles of the next
// tile, so HBM drains C while the MFMAs run.  The last tile is written after the loop.
//
// Operand roles are swapped by the host: the kernel computes D = A B^T with A = the
// weight [N][K] and B = the activations [M][K], and writes D transposed into the
// row-major C[M][N].  A lane's 16x16x32 accumulator holds 4 consecutive D rows = 4
// consecutive C columns: one 8-byte store, one 8-byte bias load.
//
// vmcnt: stores retire through the same in-order counter as the half-tile DMA, so every
// counted wait of gemm3 grows by the stores issued after its target half-tile (derivation
// at the waits; the drain phases keep vmcnt(0)).
// ---------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

__device__ __forceinline__ void wait_vm_rt(int n) {
  switch (n) {   // wave-uniform n: scalar branch to the immediate form
    case 8: wait_vmcnt<8>(); break;
    case 9: wait_vmcnt<9>(); break;
    case 10: wait_vmcnt<10>(); break;
    case 11: wait_vmcnt<11>(); break;
    case 12: wait_vmcnt<12>(); break;
    default: wait_vmcnt<0>(); break;
  }
}

__device__ __forceinline__ uint32_t pack_bf2(float a, float b) {
  return (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
}

template <int EPI>
__global__ void __launch_bounds__(NT, 1) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm4_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, bf16_t* __restrict__ C,
             const bf16_t* __restrict__ bias, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
             float alpha) {
  static_assert(EPI == EPI_NONE || EPI == EPI_BIAS, "gemm4 epilogues: none, bias");
  constexpr int BM = 256, BN = 256, WN = 4;
  constexpr int HALF = 128 * 128;
  constexpr int BUF = 4 * HALF;
  constexpr int SK = MP_G4_SR;   // K-tiles that carry the previous tile's deferred rows (one store per phase)
  constexpr int SR = MP_G4_SR;   // accumulator row blocks deferred (the other 8 - SR are stored at the tile end)
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  const int nwg = gm * gn;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int lr = lane >> 3;
  const int lc = (lane & 7) ^ swzq(8 * (wave & 1) + lr);
  const int q = lane >> 4;
  const int nk = K / BK;
  const int rA = wr * 64 + (lane & 15);
  const int rB = wc * 32 + (lane & 15);

  // previous tile: stash[i][j] = D rows pm0 + 128 wr + 16 (i + shifts) + 4 q .. +3 at
  // column pn0 + 64 wc + 16 j + (lane & 15); rows leave through stash[0] (shift())
  u32x2 stash[SR][4];
  int pm0 = 0, pn0 = 0;
  bool has_prev = false;
  auto put = [&](int j, int srow) {
    const int r = pm0 + wr * 128 + 16 * srow + 4 * q;
    const int c = pn0 + 64 * wc + 16 * j + (lane & 15);
    if (r < M && c < N) __builtin_nontemporal_store(stash[0][j], reinterpret_cast<u32x2*>(C + (int64_t)c * ldc + r));
  };
  auto shift = [&]() {
#pragma unroll
    for (int i = 0; i < SR - 1; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) stash[i][j] = stash[i + 1][j];
  };

#define G4_MFMA(R0, BF, C0)                                                              \
  __builtin_amdgcn_sched_barrier(0);                                                     \
  __builtin_amdgcn_s_setprio(1);                                                         \
  _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_)                                       \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                       \
  _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                       \
    acc[R0 + i_][C0 + j_] = mfma16(af[i_][s_], BF[j_][s_], acc[R0 + i_][C0 + j_]);       \
  __builtin_amdgcn_s_setprio(0);                                                         \
  __builtin_amdgcn_sched_barrier(0);
#define G4_BAR()                          \
  asm volatile("" ::: "memory");          \
  __builtin_amdgcn_s_barrier();           \
  asm volatile("" ::: "memory");

#pragma unroll 1
  for (int vb = blockIdx.x; vb < nwg; vb += gridDim.x) {
    const int wg = xcd_remap(vb, nwg);
    constexpr int GROUP = MP_G3_GROUP;
    const int group = wg / (GROUP * gn);
    const int first_m = group * GROUP;
    const int gsz = min(gm - first_m, GROUP);
    const int tm = first_m + (wg % (GROUP * gn)) % gsz;
    const int tn = (wg % (GROUP * gn)) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const bf16_t* pa[2];
    const bf16_t* pb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int ra = m0 + 128 * j + 8 * wave + lr;
      ra = ra < M ? ra : M - 1;
      int rb = n0 + 64 * ((wave >> 2) + 2 * j) + 8 * (wave & 3) + lr;
      rb = rb < N ? rb : N - 1;
      pa[j] = A + (int64_t)ra * lda + lc * 8;
      pb[j] = B + (int64_t)rb * ldb + lc * 8;
    }
    const bool a1_ok0 = m0 + 64 + 8 * wave + lr < M, a1_ok1 = m0 + 192 + 8 * wave + lr < M;
    const bool b1_ok0 = n0 + 64 * (wave >> 2) + 32 + 8 * (wave & 3) + lr < N;
    const bool b1_ok1 = n0 + 64 * ((wave >> 2) + 2) + 32 + 8 * (wave & 3) + lr < N;
    const int64_t a1_off0 = a1_ok0 ? 64 * lda : 0, a1_off1 = a1_ok1 ? 64 * lda : 0;
    const int64_t b1_off0 = b1_ok0 ? 32 * ldb : 0, b1_off1 = b1_ok1 ? 32 * ldb : 0;

    auto issue = [&](int h, int kt) {
      char* img = smem + (kt & 1) * BUF + (h == 0 ? 0 : h == 3 ? HALF : h == 1 ? 2 * HALF : 3 * HALF);
      const int64_t dk = (int64_t)kt * BK;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16_t* src;
        if (h == 0) src = pa[j] + dk;
        else if (h == 3) src = pa[j] + dk + (j ? a1_off1 : a1_off0);
        else if (h == 1) src = pb[j] + dk;
        else src = pb[j] + dk + (j ? b1_off1 : b1_off0);
        __builtin_amdgcn_global_load_lds((const void*)src,
                                         (__attribute__((address_space(3))) void*)(img + (wave + 8 * j) * 1024), 16,
                                         0, 0);
      }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{};

    issue(0, 0);
    issue(1, 0);
    issue(2, 0);
    issue(3, 0);
    if (nk > 1) {
      issue(0, 1);
      issue(1, 1);
      wait_vmcnt<8>();
    } else {
      wait_vmcnt<4>();
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();  // stagger the wave rows by one barrier
    asm volatile("" ::: "memory");

    bf16x8 af[4][2], b0[2][2], b1[2][2];
    auto fq = [&](const char* img, int row, int st) -> bf16x8 {
      return *reinterpret_cast<const bf16x8*>(img + row * 128 + 16 * ((4 * st + q) ^ swzq(row)));
    };

#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
      const char* buf = smem + (t & 1) * BUF;
      const bool steady = t + 2 < nk;
      // sc: this K-tile's four phases each store one stash entry right after their wait;
      // sp: the previous K-tile's did
      const int sc = (has_prev && t < SK) ? 1 : 0;
      const int sp = (has_prev && t >= 1 && t - 1 < SK) ? 1 : 0;
      // ---- phase 1: A0 x B0.  Target B1(t), issued in phase 1 of t-1 (t = 0: prologue);
      // younger: 4 half-tiles (8 ops) + the 4 stores of K-tile t-1
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_) {
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i][s_] = fq(buf, rA + 16 * i, s_);
#pragma unroll
        for (int j = 0; j < 2; ++j) b0[j][s_] = fq(buf + 2 * HALF, rB + 16 * j, s_);
      }
      if (t + 1 < nk) issue(2, t + 1);
      wait_vm_rt(steady ? 8 + 4 * sp : 0);
      G4_BAR();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (sc) put(0, t);
      G4_MFMA(0, b0, 0);
      G4_BAR();
      // ---- phase 2: A0 x B1.  Target A1(t) (phase 2 of t-1); younger: 8 DMA ops, the
      // stores of phases 2-4 of t-1 and of phase 1 of t
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
        for (int j = 0; j < 2; ++j) b1[j][s_] = fq(buf + 3 * HALF, rB + 16 * j, s_);
      if (t + 1 < nk) issue(3, t + 1);
      wait_vm_rt(steady ? 8 + 3 * sp + sc : 0);
      G4_BAR();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (sc) put(1, t);
      G4_MFMA(0, b1, 2);
      G4_BAR();
      // ---- phase 3: A1 x B0; refill A0 of this buffer for K-tile t+2
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i][s_] = fq(buf + HALF, rA + 16 * i, s_);
      if (steady) issue(0, t + 2);
      G4_BAR();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (sc) put(2, t);
      G4_MFMA(4, b0, 0);
      G4_BAR();
      // ---- phase 4: A1 x B1; refill B0.  Target B0(t+1) (phase 4 of t-1; t = 0: the last
      // prologue issue); younger: 8 DMA ops, the store of phase 4 of t-1, phases 1-3 of t
      if (steady) {
        issue(1, t + 2);
        wait_vm_rt(8 + sp + 3 * sc);
      } else {
        wait_vmcnt<0>();
      }
      G4_BAR();
      if (sc) put(3, t);
      G4_MFMA(4, b1, 2);
      G4_BAR();
      if (sc) shift();
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();  // re-align the staggered wave rows
    __syncthreads();
    // short K (< SK K-tiles): the rest of the previous tile
    if (has_prev) {
#pragma unroll 1
      for (int s = nk; s < SK; ++s) {
        put(0, s);
        put(1, s);
        put(2, s);
        put(3, s);
        shift();
      }
    }
    // this tile: alpha (+ bias) -> bf16; row blocks SR.. stored now, 0..SR-1 deferred
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = m0 + wr * 128 + 16 * i + 4 * q;
      u32x2 bz = {0u, 0u};
      if constexpr (EPI == EPI_BIAS) bz = *reinterpret_cast<const u32x2*>(bias + (r < M ? r : 0));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] * alpha;
        if constexpr (EPI == EPI_BIAS) {
          v[0] += __uint_as_float(bz[0] << 16);
          v[1] += __uint_as_float(bz[0] & 0xffff0000u);
          v[2] += __uint_as_float(bz[1] << 16);
          v[3] += __uint_as_float(bz[1] & 0xffff0000u);
        }
        const u32x2 o = u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        if (i < SR) {
          stash[i < SR ? i : 0][j] = o;
        } else {
          const int c = n0 + 64 * wc + 16 * j + (lane & 15);
          if (r < M && c < N) __builtin_nontemporal_store(o, reinterpret_cast<u32x2*>(C + (int64_t)c * ldc + r));
        }
      }
    }
    pm0 = m0;
    pn0 = n0;
    has_prev = true;
  }
#undef G4_MFMA
#undef G4_BAR
  if (has_prev) {
#pragma unroll 1
    for (int s = 0; s < SK; ++s) {
      put(0, s);
      put(1, s);
      put(2, s);
      put(3, s);
      shift();
    }
  }
}

// C[M][N] (bf16, row stride ldc) = alpha * X[M][K] W[N][K]^T (+ bias[N]) on gemm4
// (kernel space: D = W X^T, Mk = N, Nk = M); one workgroup per CU once the tiles
// outnumber the CUs
template <int EPI>
static int launch4(const void* X, const void* W, void* C, const void* bias, int M, int N, int K, int64_t ldx,
                   int64_t ldw, int64_t ldc, float alpha, int grid_override, hipStream_t st) {
  constexpr int LDS = 2 * 4 * 128 * 128;
  auto kern = gemm4_kernel<EPI>;
  static bool attr = false;
  lds_attr_once(attr, (const void*)kern, LDS);
  const int nwg = ((N + 255) / 256) * ((M + 255) / 256);
  int grid = nwg < 256 ? nwg : 256;
  if (grid_override > 0) grid = grid_override < nwg ? grid_override : nwg;   // tests: several tiles per workgroup
  kern<<<grid, NT, LDS, st>>>((const bf16_t*)W, (const bf16_t*)X, (bf16_t*)C, (const bf16_t*)bias, N, M, K, ldw,
                              ldx, ldc, alpha);
  return (int)hipGetLastError();
}


// ---------------------------------------------------------------------------------------
// gemm5 (probe, opt-in: 0.7-0.8x gemm3, profiles/r2_probes.md): 256x256 NT with 4 waves, ONE wave per SIMD (512 registers: a 128x128
// accumulator per wave in 256 AGPRs), instead of gemm3's 8 waves in ping-pong pairs.
// Per K-tile (BK = 64) a wave reads 32 KiB of fragments (gemm3: 24 KiB x 8 waves) and
// issues 128 MFMAs; fragments are register double-buffered by 32-deep k-step, so the
// ds_reads of the next k-step (and the next K-tile's DMA) interleave with the current
// k-step's MFMAs (sched_group_barrier).  2 LDS buffers, one barrier per K-tile.
// ---------------------------------------------------------------------------------------
template <int EPI>
__global__ void __launch_bounds__(256, 1) __attribute__((amdgpu_waves_per_eu(1, 1)))
gemm5_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, void* __restrict__ Cv,
             const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R, bf16_t* __restrict__ AUX,
             float* __restrict__ WS, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr,
             int64_t ldx, float alpha, float p_drop, uint64_t seed) {
  if (p_drop > 0.f) seed = step_seed(seed);
  constexpr int BM = 256, BN = 256, NTH5 = 256;
  constexpr int IMG = 256 * 128;          // one operand image: 256 rows x 64 k (128 B rows)
  constexpr int BUF = 2 * IMG;            // A | B
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int gm = (M + BM - 1) / BM, gn = (N + BN - 1) / BN;
  const int nwg = gm * gn;
  const int wg = xcd_remap((int)blockIdx.x, nwg);
  constexpr int GROUP = MP_G3_GROUP;
  const int group = wg / (GROUP * gn);
  const int first_m = group * GROUP;
  const int gsz = min(gm - first_m, GROUP);
  const int tm = first_m + (wg % (GROUP * gn)) % gsz;
  const int tn = (wg % (GROUP * gn)) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int nk = K / BK;

  // DMA: 64 pieces of 1 KiB per K-tile (A rows 0..255 = pieces 0..31, B = 32..63); wave w
  // issues pieces w, w + 4, ..., each lane 16 bytes: image row 8 p' + (lane >> 3), physical
  // chunk lane & 7 <- logical chunk (lane & 7) ^ swzq(row)
  const int lr = lane >> 3;
  const bf16_t* src[16];
  int dst[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int piece = wave + 4 * u;                  // 0..63
    const bool isb = piece >= 32;
    const int prow = (piece & 31) * 8 + lr;          // image row
    const int lc = (lane & 7) ^ swzq(prow);
    int gr = (isb ? n0 : m0) + prow;
    const int lim = isb ? N : M;
    gr = gr < lim ? gr : lim - 1;
    src[u] = (isb ? B : A) + (int64_t)gr * (isb ? ldb : lda) + lc * 8;
    dst[u] = (isb ? IMG : 0) + (piece & 31) * 1024;
  }
  auto issue = [&](int kt) {
    char* base = smem + (kt & 1) * BUF;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      __builtin_amdgcn_global_load_lds((const void*)(src[u] + (int64_t)kt * BK),
                                       (__attribute__((address_space(3))) void*)(base + dst[u]), 16, 0, 0);
  };
  auto fq = [&](const char* img, int row, int st) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(img + row * 128 + 16 * ((4 * st + q) ^ swzq(row)));
  };

  f32x4 acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{};

  const int rA = wr * 128 + (lane & 15), rB = wc * 128 + (lane & 15);
  bf16x8 a0[8], b0[8], a1[8], b1[8];

  issue(0);
  if (nk > 1) issue(1);
  if (nk > 1) wait_vmcnt<16>(); else wait_vmcnt<0>();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a0[i] = fq(smem, rA + 16 * i, 0);
    b0[i] = fq(smem + IMG, rB + 16 * i, 0);
  }

#pragma unroll 1
  for (int t = 0; t < nk; ++t) {
    const char* buf = smem + (t & 1) * BUF;
    // (A) k-step 0 MFMAs; the k-step 1 fragments of this K-tile load meanwhile
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a1[i] = fq(buf, rA + 16 * i, 1);
      b1[i] = fq(buf + IMG, rB + 16 * i, 1);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = mfma16(a0[i], b0[j], acc[i][j]);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
    }
    // (B) every wave done reading this buffer, the next K-tile landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // (C, D) DMA of K-tile t+2 into this buffer; k-step 1 MFMAs while the next K-tile's
    // k-step 0 fragments load
    if (t + 2 < nk) issue(t + 2);
    const char* nbuf = smem + ((t + 1) & 1) * BUF;
    if (t + 1 < nk) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        a0[i] = fq(nbuf, rA + 16 * i, 0);
        b0[i] = fq(nbuf + IMG, rB + 16 * i, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = mfma16(a1[i], b1[j], acc[i][j]);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  epilogue<BM, BN, 2, 2, EPI, false, NTH5>(Stage16<8, 8>{acc, wc * 128, lane}, smem, m0, n0, wr, Cv, bias, R, AUX,
                                           WS, M, N, ldc, ldr, ldx, alpha, 1, p_drop, seed);
}

template <int EPI>
static int launch5(const void* A, const void* B, void* C, const void* bias, const void* R, void* X, float* ws, int M,
                   int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int64_t ldx, float alpha,
                   float p_drop, uint64_t seed, hipStream_t st) {
  constexpr int LDS_MAIN = 2 * 2 * 256 * 128;
  constexpr int EPI_BYTES = 128 * (256 + 4) * 4;
  constexpr int LDS = LDS_MAIN > EPI_BYTES ? LDS_MAIN : EPI_BYTES;
  auto kern = gemm5_kernel<EPI>;
  static bool attr = false;
  lds_attr_once(attr, (const void*)kern, LDS);
  const int nwg = ((M + 255) / 256) * ((N + 255) / 256);
  kern<<<nwg, 256, LDS, st>>>((const bf16_t*)A, (const bf16_t*)B, C, (const bf16_t*)bias, (const bf16_t*)R,
                              (bf16_t*)X, ws, M, N, K, lda, ldb, ldc, ldr, ldx, alpha, p_drop, seed);
  return (int)hipGetLastError();
}

}  // namespace g2
