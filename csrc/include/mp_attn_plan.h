// The host-side launch plan of the training attention (attention.hip): which of its ten kernels
// a problem runs, with which grid and how much dynamic LDS, as a pure function of the problem
// and the MIPIPE_ATTN_* switches (AttnEnv).  Plain C++17 with no HIP header: the launchers of
// attention.hip switch on it, and the Python binding attn_plan reports it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

// ring depths of the LDS-DMA kernels (build-time A/B: tools/build_ext.py --variant ... -D ...):
// forward v2's K / V ring (2 = 32 KB of LDS, 4 workgroups per CU; 3 = 48 KB, 3 per CU) and
// dK/dV v1's Q / dO ring at d_h <= 128 (4 buffers keep 3 tiles in flight)
#ifndef MP_FWD_NBUF
#define MP_FWD_NBUF 2
#endif
#ifndef MP_DKDV_NBUF
#define MP_DKDV_NBUF 4
#endif

namespace attn {

// The kernels.  attn_plan reports them by name, and tests, tools and recorded paths spell the
// names, so they are fixed.
enum Kernel : int {
  K_NONE = -1,   // no kernel takes the problem (head dim, H % Hkv)
  K_FWD1,        // attn_fwd_kernel: register-staged K / V, every head dim
  K_KS2,         // attn_fwd_ks2_kernel: key-split forward of short non-causal problems
  K_FWD2,        // attn_fwd2_kernel: paired query blocks, LDS-DMA ring (d_h <= 64)
  K_DQ1,         // attn_bwd_dq_kernel
  K_DQ2,         // attn_bwd_dq23_kernel, one query block per workgroup (A/B arm)
  K_DQ3,         //   paired causal query blocks on one XCD (the default at d_h <= 64)
  K_DKDV1,       // attn_bwd_dkdv_kernel
  K_DKDV2,       // attn_bwd_dkdv23_kernel, one key block per workgroup (A/B arm)
  K_DKDV3,       //   paired causal key blocks on one XCD (the default at d_h <= 64)
  K_SHORT,       // attn_bwd_short_kernel: dQ and dK/dV of a short non-causal problem in one launch
};

inline const char* kernel_name(Kernel k) {
  switch (k) {
    case K_FWD1: return "fwd1";
    case K_KS2: return "ks2";
    case K_FWD2: return "fwd2";
    case K_DQ1: return "dq1";
    case K_DQ2: return "dq2";
    case K_DQ3: return "dq3";
    case K_DKDV1: return "dkdv1";
    case K_DKDV2: return "dkdv2";
    case K_DKDV3: return "dkdv3";
    case K_SHORT: return "short";
    default: return "none";
  }
}

// Every MIPIPE_ATTN_* switch, with its default.
struct AttnEnv {
  bool fwd1 = false;        // MIPIPE_ATTN_FWD=1: forward v1 at d_h <= 64 too (A/B)
  int dq = 3;               // MIPIPE_ATTN_BWD_DQ=1 / 2: dQ v1 / v2; anything else: v3
  int dkdv = 3;             // MIPIPE_ATTN_BWD_DKDV=1 / 2: dK/dV v1 / v2; anything else: v3
  bool ks2 = true;          // MIPIPE_ATTN_KS2=0: no key-split forward
  bool bwd_short = true;    // MIPIPE_ATTN_BWD_SHORT=0: the two-kernel backward for short problems too

  static constexpr const char* NAMES[] = {"MIPIPE_ATTN_FWD", "MIPIPE_ATTN_BWD_DQ", "MIPIPE_ATTN_BWD_DKDV",
                                          "MIPIPE_ATTN_KS2", "MIPIPE_ATTN_BWD_SHORT"};

  static bool known(const char* name) {
    for (const char* n : NAMES)
      if (!strcmp(n, name)) return true;
    return false;
  }

  // get(name) -> the value's C string, or nullptr where the name is not set
  template <class Get>
  static AttnEnv parse(Get&& get) {
    const auto unless0 = [&](const char* n) { const char* e = get(n); return !(e && e[0] == '0'); };
    const auto version = [&](const char* n) {
      const char* e = get(n);
      return (e && e[0] == '1') ? 1 : ((e && e[0] == '2') ? 2 : 3);
    };
    AttnEnv v;
    const char* f = get("MIPIPE_ATTN_FWD");
    v.fwd1 = f && f[0] == '1';
    v.dq = version("MIPIPE_ATTN_BWD_DQ");
    v.dkdv = version("MIPIPE_ATTN_BWD_DKDV");
    v.ks2 = unless0("MIPIPE_ATTN_KS2");
    v.bwd_short = unless0("MIPIPE_ATTN_BWD_SHORT");
    return v;
  }

  // the process environment, read once
  static const AttnEnv& process() {
    static const AttnEnv env = parse([](const char* n) { return (const char*)getenv(n); });
    return env;
  }
};

// One kernel launch (256 threads per workgroup): the head dim the kernel is instantiated for,
// the grid and the dynamic LDS bytes.
struct Launch {
  Kernel kernel = K_NONE;
  int dp = 0;
  unsigned gx = 1, gy = 1;
  size_t lds = 0;
};

struct BwdPlan {
  int n = 0;     // 0: no kernel takes the problem; 1: short; 2: dQ, then dK/dV
  Launch l[2];
};

// head dim padded to the instantiated 64 / 128 / 256; -1: not supported
inline int pick_dp(int D) { return D <= 64 ? 64 : (D <= 128 ? 128 : (D <= 256 ? 256 : -1)); }
inline bool supported(int H, int Hkv, int D) { return pick_dp(D) >= 0 && D % 8 == 0 && H % Hkv == 0; }

// the LDS-DMA kernels address a (b, head)'s rows by 32-bit buffer offsets: S rows (+ the
// tiles issued past the end) of `stride` bf16 must stay below 2^31 bytes
inline bool narrow(int S, int64_t stride) { return (int64_t)(S + 128) * stride * 2 < (1ll << 31); }

// LDS of attn_bwd_short_kernel: max over the roles' tiles and hand-off areas
constexpr size_t short_bwd_lds(int DP) {
  const size_t tile = 64 * DP * 2;
  const size_t dq_tiles = 4 * tile;
  const size_t dkdv_tiles = 2 * ((DP > 128 ? 2 : 3) * tile + 512);
  const size_t xq = 2 * (DP / 32) * 16 * 64 * 4;
  const size_t xkv = 2 * xq;
  const size_t red = 4 * DP * 4;
  size_t m = dq_tiles;
  m = dkdv_tiles > m ? dkdv_tiles : m;
  m = xq > m ? xq : m;
  m = xkv > m ? xkv : m;
  m = red > m ? red : m;
  return m;
}

inline Launch plan_attn_fwd(int B, int Sq, int Sk, int H, int Hkv, int D, int64_t ks, int64_t vs, bool causal,
                            bool drop, const AttnEnv& env) {
  (void)drop;   // selects the instantiation, never the kernel
  if (!supported(H, Hkv, D)) return {};
  const int DP = pick_dp(D);
  const int nmb = (Sq + 127) / 128;
  // short non-causal problems (fewer 128-query blocks than CUs): the key-split kernel, whose
  // wave pairs double-buffer their K / V tiles when they walk more than one
  if (!causal && DP <= 128 && env.ks2 && (int64_t)nmb * B * H < 256) {
    const int niter = ((Sk + 63) / 64 + 1) / 2;
    return {K_KS2, DP, (unsigned)((Sq + 63) / 64), (unsigned)(B * H), (size_t)(niter > 1 ? 8 : 4) * 64 * DP * 2};
  }
  // v2 (default at d_h 64; d_h 128 / 256 spill at 3 waves per SIMD); MIPIPE_ATTN_FWD=1 selects v1 (A/B)
  if (DP == 64 && !env.fwd1 && narrow(Sk, ks) && narrow(Sk, vs)) {
    const int npair = causal ? (nmb + 1) / 2 : nmb;
    return {K_FWD2, DP, (unsigned)(npair * B * H), 1u, (size_t)MP_FWD_NBUF * 2 * 64 * 64 * 2};
  }
  return {K_FWD1, DP, (unsigned)nmb, (unsigned)(B * H), (size_t)4 * 64 * DP * 2};
}

inline BwdPlan plan_attn_bwd(int B, int Sq, int Sk, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs,
                             int64_t os, bool causal, bool drop, const AttnEnv& env) {
  (void)drop;
  BwdPlan p;
  if (!supported(H, Hkv, D)) return p;
  const int DP = pick_dp(D);
  const int nmb = (Sq + 127) / 128, nkb = (Sk + 127) / 128;
  // short non-causal problems: dQ and dK/dV in one launch (MIPIPE_ATTN_BWD_SHORT=0: the
  // two-kernel path, for A/B; d_h 256: the role-merged register file spills)
  if (!causal && DP <= 128 && env.bwd_short && Sq <= 128 && Sk <= 128 && H == Hkv) {
    p.n = 1;
    p.l[0] = {K_SHORT, DP, (unsigned)((Sq + 63) / 64 + (Sk + 63) / 64), (unsigned)(B * H), short_bwd_lds(DP)};
    return p;
  }
  p.n = 2;
  // dQ.  v3 (paired query blocks on one XCD) by default: +0.35 % on the step over v2 (2
  // same-box runs each); MIPIPE_ATTN_BWD_DQ=2 / 1 select v2 / v1
  if (DP == 64 && env.dq != 1 && narrow(Sk, ks) && narrow(Sk, vs)) {
    const size_t lds = (size_t)4 * 2 * 64 * DP * 2;
    if (env.dq == 3) p.l[0] = {K_DQ3, DP, (unsigned)((causal ? (nmb + 1) / 2 : nmb) * B * H), 1u, lds};
    else p.l[0] = {K_DQ2, DP, (unsigned)nmb, (unsigned)(B * H), lds};
  } else {
    p.l[0] = {K_DQ1, DP, (unsigned)nmb, (unsigned)(B * H), (size_t)(DP <= 128 ? 4 : 2) * 2 * 64 * DP * 2};
  }
  // dK/dV.  v3 (paired key blocks on one XCD) by default: +0.4 % on the step over v2 (2
  // same-box runs each, profiles/r6_attention_v2.md); MIPIPE_ATTN_BWD_DKDV=2 / 1 select v2 / v1
  if (DP == 64 && env.dkdv != 1 && narrow(Sq, qs) && narrow(Sq, os)) {
    const size_t lds = (size_t)4 * (2 * 64 * DP * 2 + 512);
    if (env.dkdv == 3) p.l[1] = {K_DKDV3, DP, (unsigned)((causal ? (nkb + 1) / 2 : nkb) * B * Hkv), 1u, lds};
    else p.l[1] = {K_DKDV2, DP, (unsigned)nkb, (unsigned)(B * Hkv), lds};
  } else {
    p.l[1] = {K_DKDV1, DP, (unsigned)nkb, (unsigned)(B * Hkv),
              (size_t)(DP <= 128 ? MP_DKDV_NBUF : 2) * (2 * 64 * DP * 2 + 512)};
  }
  return p;
}

}  // namespace attn
