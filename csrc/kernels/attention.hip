// Flash attention forward / backward for gfx950 (bf16 in, f32 accumulate, MFMA 32x32x16).
// SURVEY §2.5 K4 (self + cross attention, causal / non-causal, head dims 64..256,
// GQA, in-kernel counter-based dropout regenerated in the backward).
//
// Layout: q/k/v/o are token-major rows ([B*S, row_stride] bf16), head h at column h*D,
// i.e. exactly what the fused QKV projection writes and the output projection reads:
// no transposes or head-major copies anywhere.  LSE is kept per (b, h, query) in log2
// units (lse2 = m + log2(l)) for the backward.
//
// Forward (one workgroup = 4 waves = 128 queries of one (b, h); 64-key tiles):
//   * "swapped" QK^T: each wave computes S^T = K . Q^T so the QUERY is on the MFMA lane and
//     the 32 keys of a 32x32 tile are in its registers: the row max / row sum are
//     in-lane (+1 cross-half shuffle), and the online-softmax rescale of O is a per-lane
//     scalar because O is also kept transposed (O^T = V^T . P^T).
//   * P^T never leaves registers: the S^T accumulator is already the B operand of
//     V^T . P^T (k order permuted, see cdna guide §3); V^T fragments come from
//     ds_read_b64_tr_b16 hardware-transposed LDS reads.
//   * K and V tiles are register-staged into a double-buffered LDS ring (loads for tile
//     j+1 issued before computing tile j, written after), XOR-swizzled in 16-byte chunks
//     so both the b128 row reads (K) and the transposed reads (V) are bank-conflict free.
//   * causal: heavy query blocks launch first; per-wave skip of fully masked tiles.
// Backward = two deterministic kernels (no f32 atomics):
//   dkdv: one workgroup = 128 keys of one (b, kv-head), loops over all query heads of the
//         group (GQA) and all query tiles; key on the MFMA lane so P and dS are directly
//         the B operands of dV^T += dO^T P and dK^T += Q^T dS.
//   dq:   one workgroup = 128 queries (forward structure), recomputes P^T and dP^T and
//         accumulates dQ^T += K^T dS^T.
//
// This file is the translation unit: the launchers and the C API.  The kernels are in
// csrc/include: mp_attn_fwd.h, mp_attn_bwd_dkdv.h, mp_attn_bwd_dq.h, mp_attn_bwd_short.h, over
// the helpers of mp_attn_common.h and mp_attn_tiles.h (the LDS tile image, MFMA / pack
// wrappers and Stage64, shared with attention_doc.hip).  Which kernel a problem runs, on
// which grid and with how much LDS, is decided by mp_attn_plan.h.
#include "mp_api.h"
#include "mp_common.h"

#include <type_traits>

using namespace mp;

#include "mp_attn_plan.h"
#include "mp_attn_fwd.h"
#include "mp_attn_bwd_dkdv.h"
#include "mp_attn_bwd_dq.h"
#include "mp_attn_bwd_short.h"

// ==========================================================================================
// launchers: one switch on the planned kernel; grid and LDS bytes are the plan's
// ==========================================================================================
// more than 64 KiB of dynamic LDS is announced per kernel; per launch, since the key-split
// forward's size varies by call.  For the kernels that can need it at some head dim (v1,
// key-split, short); the d_h 64 v2 / v3 kernels have always launched without.
static void allow_lds(const void* kern, size_t lds) {
  if (lds > 64 * 1024) (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

template <int DP, bool CAUSAL, bool DROP>
static int launch_fwd(const attn::Launch& L, const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* o, float* lse,
                      int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os,
                      float scale, float p, uint64_t seed, hipStream_t st) {
  const auto run = [&](auto kern, bool big_lds) {
    if (big_lds) allow_lds((const void*)kern, L.lds);
    kern<<<dim3(L.gx, L.gy), 256, L.lds, st>>>(q, k, v, o, lse, B, Sq, Sk, H, Hkv, D, qs, ks, vs, os, scale, p, seed);
    return (int)hipGetLastError();
  };
  switch (L.kernel) {
    case attn::K_KS2:
      if constexpr (!CAUSAL && DP <= 128) return run(attn_fwd_ks2_kernel<DP, DROP>, true);
      break;
    case attn::K_FWD2:
      if constexpr (DP == 64) return run(attn_fwd2_kernel<DP, CAUSAL, DROP>, false);
      break;
    case attn::K_FWD1:
      return run(attn_fwd_kernel<DP, CAUSAL, DROP>, true);
    default:
      break;
  }
  return -1;   // a plan that names a kernel this instantiation does not hold
}

template <int DP, bool CAUSAL, bool DROP>
static int launch_bwd(const attn::BwdPlan& P, const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* o,
                      const bf16_t* dout, const float* lse, float* delta, bf16_t* dq, bf16_t* dk, bf16_t* dv, int B,
                      int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os,
                      int64_t dqs, int64_t dks, int64_t dvs, float scale, float p, uint64_t seed, float* csq,
                      float* csk, float* csv, hipStream_t st) {
  for (int i = 0; i < P.n; ++i) {
    const attn::Launch& L = P.l[i];
    const dim3 grid(L.gx, L.gy);
    const auto run_dq = [&](auto kern, bool big_lds) {
      if (big_lds) allow_lds((const void*)kern, L.lds);
      kern<<<grid, 256, L.lds, st>>>(q, k, v, o, dout, lse, delta, dq, B, Sq, Sk, H, Hkv, D, qs, ks, vs, os, dqs, scale,
                                     p, seed, csq);
    };
    const auto run_dkdv = [&](auto kern, bool big_lds) {
      if (big_lds) allow_lds((const void*)kern, L.lds);
      kern<<<grid, 256, L.lds, st>>>(q, k, v, dout, lse, delta, dk, dv, B, Sq, Sk, H, Hkv, D, qs, ks, vs, os, dks, dvs,
                                     scale, p, seed, csk, csv);
    };
    bool held = false;   // this instantiation holds the planned kernel
    switch (L.kernel) {
      case attn::K_SHORT:
        if constexpr (!CAUSAL && DP <= 128) {
          auto kern = attn_bwd_short_kernel<DP, DROP>;
          allow_lds((const void*)kern, L.lds);
          kern<<<grid, 256, L.lds, st>>>(q, k, v, o, dout, lse, dq, dk, dv, B, Sq, Sk, H, D, qs, ks, vs, os, dqs, dks,
                                         dvs, scale, p, seed, csq, csk, csv);
          held = true;
        }
        break;
      case attn::K_DQ1:
        run_dq(attn_bwd_dq_kernel<DP, CAUSAL, DROP>, true);
        held = true;
        break;
      case attn::K_DQ2:
      case attn::K_DQ3:
        if constexpr (DP == 64) {
          if (L.kernel == attn::K_DQ3) run_dq(attn_bwd_dq23_kernel<DP, CAUSAL, DROP, true>, false);
          else run_dq(attn_bwd_dq23_kernel<DP, CAUSAL, DROP, false>, false);
          held = true;
        }
        break;
      case attn::K_DKDV1:
        run_dkdv(attn_bwd_dkdv_kernel<DP, CAUSAL, DROP>, true);
        held = true;
        break;
      case attn::K_DKDV2:
      case attn::K_DKDV3:
        if constexpr (DP == 64) {
          if (L.kernel == attn::K_DKDV3) run_dkdv(attn_bwd_dkdv23_kernel<DP, CAUSAL, DROP, true>, false);
          else run_dkdv(attn_bwd_dkdv23_kernel<DP, CAUSAL, DROP, false>, false);
          held = true;
        }
        break;
      default:
        break;
    }
    if (!held) return -1;
  }
  return (int)hipGetLastError();
}

// f(dp, causal, drop) with the three as integral constants: the instantiation of a launcher
template <class F>
static int with_instance(int DP, bool causal, bool drop, F&& f) {
  const auto flags = [&](auto dp) {
    if (causal) return drop ? f(dp, std::true_type{}, std::true_type{}) : f(dp, std::true_type{}, std::false_type{});
    return drop ? f(dp, std::false_type{}, std::true_type{}) : f(dp, std::false_type{}, std::false_type{});
  };
  switch (DP) {
    case 64: return flags(std::integral_constant<int, 64>{});
    case 128: return flags(std::integral_constant<int, 128>{});
    case 256: return flags(std::integral_constant<int, 256>{});
    default: return -1;
  }
}

extern "C" int mp_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int Sq, int Sk,
                           int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int causal,
                           float scale, float p_drop, uint64_t seed, hipStream_t st) {
  const bool drop = p_drop > 0.f;
  const attn::Launch L = attn::plan_attn_fwd(B, Sq, Sk, H, Hkv, D, ks, vs, causal != 0, drop, attn::AttnEnv::process());
  if (L.kernel == attn::K_NONE) return -1;
  return with_instance(L.dp, causal != 0, drop, [&](auto dp, auto c, auto d) {
    return launch_fwd<decltype(dp)::value, decltype(c)::value, decltype(d)::value>(
        L, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse, B, Sq, Sk, H, Hkv, D, qs, ks, vs, os,
        scale, p_drop, seed, st);
  });
}

extern "C" int mp_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                           const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int Sq,
                           int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dqs,
                           int64_t dks, int64_t dvs, int causal, float scale, float p_drop, uint64_t seed,
                           float* csq, float* csk, float* csv, hipStream_t st) {
  if ((csq == nullptr) != (csk == nullptr) || (csk == nullptr) != (csv == nullptr)) return -1;
  const bool drop = p_drop > 0.f;
  const attn::BwdPlan P =
      attn::plan_attn_bwd(B, Sq, Sk, H, Hkv, D, qs, ks, vs, os, causal != 0, drop, attn::AttnEnv::process());
  if (P.n == 0) return -1;
  return with_instance(P.l[0].dp, causal != 0, drop, [&](auto dp, auto c, auto d) {
    return launch_bwd<decltype(dp)::value, decltype(c)::value, decltype(d)::value>(
        P, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)o, (const bf16_t*)dout, lse, delta,
        (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, B, Sq, Sk, H, Hkv, D, qs, ks, vs, os, dqs, dks, dvs, scale, p_drop, seed,
        csq, csk, csv, st);
  });
}

MP_DROP_STEP_SETTER(mp_set_drop_step_attn)
