// The host-side planner of the bf16 GEMM engines of gemm2.hip: which engine (cfg) and which
// split-K factor a problem runs with, as a pure function of the problem, the forced
// configuration and the MIPIPE_* switches (PlanEnv).  Plain C++17 with no HIP header: the
// Python binding plans with it, sizes the workspace and hands cfg / split to mp_gemm2.
#pragma once

#include <cstdlib>
#include <cstring>

namespace g2 {

// The engine numbers: gemm2_plan reports them, force_cfg takes them and tests, tools and
// recorded paths ("cfg5.s1") spell them, so the values are fixed.
enum Cfg : int {
  CFG_UNAVAILABLE = -1,   // a forced engine that this build does not hold
  CFG_T256x256 = 0,       // 2-stage tiles (gemm2_kernel): 256x256 (2x4 waves)
  CFG_T256x192 = 1,       //   256x192 (4x2)
  CFG_T256x128 = 2,       //   256x128 (4x2)
  CFG_T128x128 = 3,       //   128x128 (2x4)
  CFG_PP_M32 = 4,         // ping-pong gemm3, NT, 32x32x16 MFMAs
  CFG_PP_M16 = 5,         // ping-pong gemm3, NT, 16x16x32 MFMAs
  CFG_PP_TT = 6,          // ping-pong gemm3, TT dW (f32 accumulate)
  CFG_G4 = 7,             // probe: persistent deferred-store gemm4 (100 + G: on G workgroups)
  CFG_G5 = 8,             // probe: 4-wave glds gemm5
  CFG_G6 = 9,             // ping-pong 256x192 gemm6
  CFG_S64x64 = 10,        // small-tile gemms, NT
  CFG_S64x32 = 11,
  CFG_S32x32 = 12,
  CFG_S_TT = 13,          // small-tile gemms, TT dW 64x64
  CFG_SK = 14,            // probe: stream-K gemm7
  CFG_G8 = 15,            // register-staged 256x192 gemm8, PGR 2
  CFG_G8_PGR3 = 16,       //   PGR 3
};

constexpr int PLAN_BK = 64;   // the engines' K-tile (g2::BK)

// Every MIPIPE_* switch that the planner or a launcher reads, with its default.
struct PlanEnv {
  bool gemm3 = true;        // MIPIPE_GEMM3=0: no ping-pong engine for NT problems
  bool m16 = true;          // MIPIPE_GEMM_M16=0: the 32x32x16-MFMA builds (gemm3 cfg 4, gemm2 tiles)
  bool m16t = false;        // MIPIPE_GEMM_M16T=1: 16x16x32 MFMAs in the gemm2 tiles for transposed operands too
  bool gemm6 = false;       // MIPIPE_GEMM6=1
  bool gemm3t = true;       // MIPIPE_GEMM3T=0: dW GEMMs stay on the 2-stage TT tiles
  bool small = true;        // MIPIPE_GEMM_SMALL=0: no small-tile engine
  int small_minwg = 256;    // MIPIPE_GEMMS_MINWG: workgroups the small engine aims for
  int gemm8 = 0;            // MIPIPE_GEMM8: 0 off, 1 wherever cfg 5 would run unsplit, 2 ("auto") by its model
  int dw_maxsplit = 32;     // MIPIPE_DW_MAXSPLIT: cap on the f32-accumulate split-K factor
  int dw_group_split = 0;   // MIPIPE_DW_GROUP_SPLIT: > 0 sets the grouped dW launch's split
  bool gemm5 = false;       // MIPIPE_GEMM5=1 (probe builds)
  bool gemm_sk = false;     // MIPIPE_GEMM_SK=1 (probe builds)
  bool gemm4 = false;       // MIPIPE_GEMM4=1 (probe builds; read by mp_gemm2)
  int gemm7_s = 0;          // MIPIPE_GEMM7_S: >= 1 sets gemm7's chunks per tail tile (A/B probes)

  static constexpr const char* NAMES[] = {
      "MIPIPE_GEMM3", "MIPIPE_GEMM_M16", "MIPIPE_GEMM_M16T", "MIPIPE_GEMM6", "MIPIPE_GEMM3T",
      "MIPIPE_GEMM_SMALL", "MIPIPE_GEMMS_MINWG", "MIPIPE_GEMM8", "MIPIPE_DW_MAXSPLIT", "MIPIPE_DW_GROUP_SPLIT",
      "MIPIPE_GEMM5", "MIPIPE_GEMM_SK", "MIPIPE_GEMM4", "MIPIPE_GEMM7_S"};

  static bool known(const char* name) {
    for (const char* n : NAMES)
      if (!strcmp(n, name)) return true;
    return false;
  }

  // get(name) -> the value's C string, or nullptr where the name is not set
  template <class Get>
  static PlanEnv parse(Get&& get) {
    const auto unless0 = [&](const char* n) { const char* e = get(n); return !(e && e[0] == '0'); };
    const auto if1 = [&](const char* n) { const char* e = get(n); return e && e[0] == '1'; };
    const auto positive = [&](const char* n, int dflt) {   // non-positive: the default
      const char* e = get(n);
      const int v = e ? atoi(e) : dflt;
      return v > 0 ? v : dflt;
    };
    const auto number = [&](const char* n) { const char* e = get(n); return e ? atoi(e) : 0; };
    PlanEnv v;
    v.gemm3 = unless0("MIPIPE_GEMM3");
    v.m16 = unless0("MIPIPE_GEMM_M16");
    v.m16t = if1("MIPIPE_GEMM_M16T");
    v.gemm6 = if1("MIPIPE_GEMM6");
    v.gemm3t = unless0("MIPIPE_GEMM3T");
    v.small = unless0("MIPIPE_GEMM_SMALL");
    v.small_minwg = positive("MIPIPE_GEMMS_MINWG", 256);
    const char* e8 = get("MIPIPE_GEMM8");
    v.gemm8 = (e8 && e8[0] == '1') ? 1 : ((e8 && e8[0] == 'a') ? 2 : 0);
    v.dw_maxsplit = positive("MIPIPE_DW_MAXSPLIT", 32);
    v.dw_group_split = number("MIPIPE_DW_GROUP_SPLIT");
    v.gemm5 = if1("MIPIPE_GEMM5");
    v.gemm_sk = if1("MIPIPE_GEMM_SK");
    v.gemm4 = if1("MIPIPE_GEMM4");
    v.gemm7_s = number("MIPIPE_GEMM7_S");
    return v;
  }

  // the process environment, read once
  static const PlanEnv& process() {
    static const PlanEnv env = parse([](const char* n) { return (const char*)getenv(n); });
    return env;
  }
};

struct Plan {
  int cfg;
  int split;
};

struct TileCfg {
  int bm, bn;
  float eff;  // relative efficiency of the tile shape (bigger tiles reuse more)
};
// indexed by CFG_T256x256 .. CFG_T128x128
static const TileCfg CFGS[4] = {{256, 256, 1.00f}, {256, 192, 0.96f}, {256, 128, 0.90f}, {128, 128, 0.72f}};

inline int tiles256(int M, int N) { return ((M + 255) / 256) * ((N + 255) / 256); }

// the 2-stage tile and split-K factor of a problem
inline Plan choose(int M, int N, int K, bool acc, bool outer, const PlanEnv& env) {
  // minimise modelled time = (#rounds of CU slots) x (per-item k-loop + epilogue) / tile efficiency;
  // padded tiles are charged like real ones, so quantisation and padding waste both count
  int best = 3, best_split = 1;
  float best_t = 3.0e38f;
  const int kt = K / PLAN_BK;
  for (int c = 0; c < 4; ++c) {
    const int cus = 256;
    const int slots = c == 3 ? 2 * cus : cus;  // 128x128 tiles fit two workgroups per CU
    if (outer && CFGS[c].bn == 192) continue;  // outer-contig images need power-of-two widths
    const int tiles = ((M + CFGS[c].bm - 1) / CFGS[c].bm) * ((N + CFGS[c].bn - 1) / CFGS[c].bn);
    const float area = (float)(CFGS[c].bm * CFGS[c].bn) / (256.f * 256.f) * (c == 3 ? 2.f : 1.f);
    // bf16 outputs split too (f32 slabs + one reduce pass that applies the epilogue):
    // small-M problems (1024-token microbatches) otherwise fill 24-48 of 256 CUs
    const int acc_max = kt / 4 < env.dw_maxsplit ? kt / 4 : env.dw_maxsplit;
    const int max_split = acc ? acc_max : (kt / 3 < 8 ? kt / 3 : 8);
    for (int s = 1; s <= (max_split > 1 ? max_split : 1); ++s) {
      const int work = tiles * s;
      const int rounds = (work + slots - 1) / slots;
      const int kper = (kt + s - 1) / s;
      // f32 slab store (+ the reduce pass for bf16 outputs) vs a direct store, in k-tile units
      const float epi = s > 1 ? (acc ? 6.f : 8.f) : 2.f;
      const float t = rounds * (kper + epi + 2.f) * area / CFGS[c].eff;  // +2: prologue fill
      if (t < best_t * 0.999f) {
        best_t = t;
        best = c;
        best_split = s;
      }
    }
  }
  return {best, best_split};
}

// The common split-K factor of a grouped dW launch (gemm3_tt_grouped_kernel) of `tiles`
// 256x256 tiles over kt K-tiles.  The K-loop work does not depend on S; the slab traffic
// (2 x S x 256 KiB per tile) and the reduce pass grow with it.  So: the SMALLEST S whose
// tiles * S workgroups fill their ceil(tiles * S / 256) rounds of CUs to >= 80 % (S = 1, no
// slabs at all, where the tiles alone do), at >= 4 K-tiles per workgroup and within
// MIPIPE_DW_MAXSPLIT; where no S gets there, the best-filling one.  GPT-2 small's layer
// (108 tiles): S = 2, 216 workgroups.  force > 0 (or MIPIPE_DW_GROUP_SPLIT) sets S, clamped
// to the K-tiles.
inline int choose_group_split(int tiles, int kt, int force, const PlanEnv& env) {
  if (force <= 0) force = env.dw_group_split;
  if (force > 0) return force < kt ? force : (kt > 0 ? kt : 1);
  const int smax = kt / 4 < env.dw_maxsplit ? kt / 4 : env.dw_maxsplit;
  int best = 1;
  float best_fill = 0.f;
  for (int s = 1; s <= (smax > 1 ? smax : 1); ++s) {
    const int work = tiles * s, rounds = (work + 255) / 256;
    const float fill = (float)work / (float)(rounds * 256);
    if (fill >= 0.8f) return s;
    if (fill > best_fill) {
      best_fill = fill;
      best = s;
    }
  }
  return best;
}

// plan of the split-tail engine (gemm7): 0 if it should not be used for this grid, else 1 with
// the tiles of the leading data-parallel rounds (dp, row-major, run by gemm3), the tail tiles
// and the chunks per tail tile (S)
constexpr int SK_MAX_G = 256;
struct Plan7 {
  int dp, tail, S;
};
inline int plan7(int M, int N, int K, const PlanEnv& env, Plan7* out) {
  const int G = SK_MAX_G, q = G / 8;
  const int T = tiles256(M, N);
  const int kt = K / PLAN_BK;
  if (T < 64 || T % G == 0 || kt < 4) return 0;
  const int dp = (T / G) * G, tail = T - dp;
  const int cmax = (tail + 7) / 8;                  // tail tiles of the fullest XCD group
  // modelled k-iteration units: a tile costs kt + 3 (prologue fill, C write); a chunked
  // tail tile ceil(kt / S) + 3, plus 2 per partial its owner reads (256 KiB at the
  // cross-XCD rate) and 1 for the contributors' publish; + 2 for a second launch
  const float plain = (float)((T + G - 1) / G) * (kt + 3);
  const float lead = (float)(dp / G) * (kt + 3) + (dp > 0 ? 2.f : 0.f);
  float best = 3.0e38f;
  int bestS = 0;
  for (int S = 2; S * cmax <= q && S <= 8; ++S) {
    const float t = lead + (float)((kt + S - 1) / S) + 3.f + 2.f * (S - 1) + 1.f;
    if (t < best) {
      best = t;
      bestS = S;
    }
  }
  if (env.gemm7_s >= 1 && env.gemm7_s * cmax <= q) bestS = env.gemm7_s, best = 0.f;   // A/B probes
  if (bestS == 0 || best > 0.95f * plain) return 0;
  out->dp = dp;
  out->tail = tail;
  out->S = bestS;
  return 1;
}

// short problems (fewer than 64 tiles of 256x256, K <= 4096: with a long K the big split-K
// plan wins) go to the small-tile engine: one launch, no split-K
inline bool is_short(int M, int N, int K) { return tiles256(M, N) < 64 && K <= 4096; }

// the small NT tile that still gives MIPIPE_GEMMS_MINWG workgroups
inline int small_nt_cfg(int M, int N, const PlanEnv& env) {
  const int w64 = ((M + 63) / 64) * ((N + 63) / 64);
  const int w6432 = ((M + 63) / 64) * ((N + 31) / 32);
  return w64 >= env.small_minwg ? CFG_S64x64 : (w6432 >= env.small_minwg ? CFG_S64x32 : CFG_S32x32);
}

// whole rounds of 256 CUs that a 256 x bn grid takes
inline float rounds256(int M, int N, int bn) {
  return (float)((((M + 255) / 256) * ((N + bn - 1) / bn) + 255) / 256);
}

// NT (both operands K-contiguous), no forced configuration: forward and dX GEMMs (bf16
// output) and the rare NT f32-accumulate
inline Plan plan_nt(int M, int N, int K, bool acc, const PlanEnv& env, bool probes_built) {
  // short-token bf16-output problems (few 256-row tiles): the small-tile engine
  // (MIPIPE_GEMM_SMALL=0 disables; MIPIPE_GEMMS_MINWG = workgroups to aim for)
  if (!acc && env.small && is_short(M, N, K)) return {small_nt_cfg(M, N, env), 1};
  Plan p = choose(M, N, K, acc, false, env);
  // the ping-pong 256x256 engine (MIPIPE_GEMM3=0 disables; MIPIPE_GEMM_M16=0 selects its
  // 32x32x16-MFMA build).  16x16x32 MFMAs hold a higher clock under load
  // (MI355X_MICROARCH.md DVFS item 7): the M16 ping-pong engine beat the 256x192 / 256x128
  // gemm2 tiles on every measured NT shape, including grids of fewer tiles than CUs
  // (N = 768: 27.5 vs 30.8 us), so it also takes their unsplit problems from 96 tiles up
  if (env.gemm3) {
    if (p.cfg == CFG_T256x256) p.cfg = env.m16 ? CFG_PP_M16 : CFG_PP_M32;
    else if (env.m16 && p.split == 1 && tiles256(M, N) >= 96) p.cfg = CFG_PP_M16;
  }
  // Opt-in engines take over where gemm3's M16 build would run without split-K; the first
  // that applies wins
  if (p.cfg == CFG_PP_M16 && p.split == 1) {
    const float r256 = rounds256(M, N, 256);
    // the 256x192 ping-pong engine (gemm6) where its grid fills whole rounds of 256 CUs
    // better than 256x256 does on a multi-round grid: modelled time = rounds x tile area /
    // tile efficiency, 0.84 measured (profiles/r4_gemm6_tail_probe.txt: N = 768 at 32K
    // tokens 2 rounds x 0.89 vs 2 rounds with the second half empty, +3-7 %; 12 MFMAs per
    // phase against gemm3's 16 under the same barriers cost 16 % per tile, so 4.5-round
    // grids and one-round grids stay on gemm3).  Opt-in (MIPIPE_GEMM6=1; force_cfg 9 selects
    // it): inside the step it lost -- 946K vs 973K tok/s with 2 lanes, 929K vs 933K with one,
    // at the PP > 1 per-rank work (r4_gemm6_tail_probe.txt) -- the lanes already fill the
    // half-empty round that it fixes, and it pays its lower per-tile rate everywhere
    if (env.gemm6 && tiles256(M, N) > 256 && rounds256(M, N, 192) * (0.75f / 0.84f) < 0.97f * r256) {
      p.cfg = CFG_G6;
    } else if (probes_built && env.gemm5 && !acc) {
      // the 4-wave / one-wave-per-SIMD 256x256 NT engine (gemm5 probe, MIPIPE_GEMM5=1)
      p.cfg = CFG_G5;
    } else if (env.gemm8 == 1 ||
               (env.gemm8 == 2 && !acc && rounds256(M, N, 192) * (0.75f / 0.9f) < 0.97f * r256)) {
      // the four-wave register-staged 256x192 NT engine (gemm8): MIPIPE_GEMM8=1 always,
      // MIPIPE_GEMM8=auto where its 256x192 grid fills whole rounds of 256 CUs better than
      // 256x256 does: modelled time = rounds x tile area / tile efficiency, 0.9 measured per
      // 256x192 tile against gemm3's 256x256 (profiles/r6_gemm8_engine.md: standalone, the
      // 16K-token N = 768 / 2304 grids run 1.11-1.15x gemm3 and the 64K-token grids
      // 0.88-0.95x).  Off by default: inside the step (2 lanes, 16K-token microbatches) auto
      // measured 910K vs 942K tok/s -- the second lane already fills gemm3's partial rounds,
      // and gemm8 pays its lower per-tile rate
      return {CFG_G8, 1};
    }
  }
  // the stream-K engine (gemm7) where the 256x256 grid is not whole rounds of 256 CUs: it
  // replaces the ping-pong engine's partial rounds and the bf16-output split-K slabs (f32
  // slab round trip through HBM + a reduce pass) of the gemm2 tiles alike.
  // Opt-in (MIPIPE_GEMM_SK=1): measured null -- on the all-tail M = 8192 grids the split
  // tail (S = 2) takes 37 vs 23.5 us at K = 768 and 60 vs 55 us at K = 3072; the hand-off of
  // a 256x256 f32 partial (LDS staging + 256 KiB out and back in, sc1 or plain + release
  // alike) costs about what the halved K loop saves (profiles/r5_gemm7_split_tail_null.txt)
  // Probe-only: a timed-out partial hand-off cannot be reported to the host, so
  // cfg 14 is reachable only in the A/B probe build (tools/build_ext.py --variant probes
  // -D MP_PROBE_ENGINES), where test_gemm7_stream_k checks it
  Plan7 pl{};
  if (probes_built && env.gemm_sk && !acc && p.cfg != CFG_G5 && plan7(M, N, K, env, &pl) > 0) return {CFG_SK, 1};
  return p;
}

// TT (both operands k-major), no forced configuration: the weight-gradient GEMMs (f32
// accumulate) and the rare TT bf16 output, which keeps the 2-stage tiles with their split-K
inline Plan plan_tt(int M, int N, int K, bool acc, const PlanEnv& env) {
  const bool dw_ok = acc && M % 8 == 0 && N % 8 == 0;
  // short-token dW GEMMs: the small engine's TT build, 64x64 tiles, no split-K (the slabs +
  // reduce pass cost as much as the GEMM here)
  if (dw_ok && env.small && is_short(M, N, K)) return {CFG_S_TT, 1};
  Plan p = choose(M, N, K, acc, true, env);
  // the TT build of the ping-pong engine: 256x256 tiles, split-K f32 accumulate
  // (MIPIPE_GEMM3T=0 keeps the 2-stage gemm2 TT engine)
  if (p.cfg == CFG_T256x256 && dw_ok && env.gemm3t) p.cfg = CFG_PP_TT;
  return p;
}

// A forced configuration (force_cfg >= 0): tests and probes.  Engines that cannot run the
// problem's layout fall back to a 2-stage tile, they do not fail.
inline Plan plan_forced(int M, int N, int K, bool transA, bool transB, bool acc, int force, const PlanEnv& env,
                        bool probes_built) {
  const bool nt = !transA && !transB, tt = transA && transB, outer = transA || transB;
  // 7: the persistent deferred-store engine (gemm4); 100 + G: gemm4 on a grid of G
  // workgroups (tests drive several tiles per workgroup through small problems); 8: gemm5;
  // 14: gemm7 wherever plan7 accepts the grid.  All three only in probe builds
  if (force == CFG_G4 || force >= 100) return {probes_built ? CFG_G4 : CFG_UNAVAILABLE, 1};
  if (force == CFG_G5) return {probes_built ? CFG_G5 : CFG_UNAVAILABLE, 1};
  if (force == CFG_SK && !probes_built) return {CFG_UNAVAILABLE, 1};
  // the split-K factor stays the tile model's; a mixed-layout bf16 output has no split-K
  // path (bf16-output split-K runs the f32-accumulate instantiation, NT or TT, into slabs)
  int split = choose(M, N, K, acc, outer, env).split;
  if (!acc && transA != transB) split = 1;
  // (the planner used to end with "bf16 output, split > 1, cfg 4 / 5 and transA: cfg 0"; no
  // path reached it, transposed operands never hold cfg 4 / 5)
  if (force < CFG_G4) {   // 0-3: a 2-stage tile; 4-6: the ping-pong builds, where the layout is theirs
    int cfg = force;
    if (cfg == CFG_PP_TT && !(tt && acc)) cfg = CFG_T256x256;
    if ((cfg == CFG_PP_M32 || cfg == CFG_PP_M16) && outer) cfg = CFG_T256x256;
    if (cfg == CFG_T256x192 && outer) cfg = CFG_T256x128;   // outer-contig images need power-of-two widths
    return {cfg, split};
  }
  if (force == CFG_G6) return {outer ? CFG_T256x256 : CFG_G6, 1};
  // force >= 10.  Odd but kept: the starting point is a placeholder 256x256 tile at the tile
  // model's split, and the unforced short-problem rule still applies to NT problems.  So a
  // forced engine that does not take the problem (13 on an NT problem, 15 on a TT one, any
  // number in 17..99) answers cfg 0 -- or a small NT tile -- not the unforced plan.
  if (nt) {
    if (env.small && force <= CFG_S32x32) return {force, 1};
    if (force == CFG_G8 || force == CFG_G8_PGR3) return {force, 1};
    Plan7 pl{};
    if (force == CFG_SK && !acc && plan7(M, N, K, env, &pl) > 0) return {CFG_SK, 1};
    if (env.small && !acc && is_short(M, N, K)) return {small_nt_cfg(M, N, env), 1};
  }
  if (force == CFG_S_TT && tt && acc && env.small && M % 8 == 0 && N % 8 == 0) return {CFG_S_TT, 1};
  return {CFG_T256x256, split};
}

// Engine and split-K factor for C[M,N] (+)= op(A) op(B).  probes_built: the build holds the
// probe engines (MP_PROBE_ENGINES); without them cfg 7 / 8 / 14 are never planned and
// forcing one answers CFG_UNAVAILABLE.
inline Plan plan_gemm(int M, int N, int K, bool transA, bool transB, bool acc, int force_cfg, const PlanEnv& env,
                      bool probes_built) {
  if (force_cfg >= 0) return plan_forced(M, N, K, transA, transB, acc, force_cfg, env, probes_built);
  if (!transA && !transB) return plan_nt(M, N, K, acc, env, probes_built);
  if (transA && transB) return plan_tt(M, N, K, acc, env);
  // mixed layouts: the 2-stage tiles (never 256x192); bf16 outputs without split-K
  Plan p = choose(M, N, K, acc, true, env);
  if (!acc) p.split = 1;
  return p;
}

}  // namespace g2
