// Bindings of the bf16 GEMMs (gemm.hip, gemm2.hip and its grouped weight-gradient launches),
// the transposes beside them (elementwise.hip) and the skinny-M GEMV (gemv_skinny.hip).
#include "common.h"
#include "mp_gemm_plan.h"
#include "mp_gemv_plan.h"

namespace mipipe_bind {
namespace {

// ---- host-side argument checks: every tensor a kernel will touch is looked at before any
// launch, and the message names the argument

// a 2-D operand of 16-byte row accesses: on `ref`'s GPU, dtype dt, unit inner stride, rows and
// base 16-byte aligned (per = elements per 16 bytes)
void gemm_operand(const char* fn, const char* name, const torch::Tensor& t, torch::ScalarType dt,
                  const torch::Tensor& ref) {
  TORCH_CHECK(t.is_cuda(), fn, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.get_device() == ref.get_device(), fn, ": ", name, " is on another device than A");
  TORCH_CHECK(t.scalar_type() == dt, fn, ": ", name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2, fn, ": ", name, " must be 2-D, got ", t.dim(), " dimensions");
  TORCH_CHECK(t.size(0) > 0 && t.size(1) > 0, fn, ": ", name, " is empty");
  TORCH_CHECK(t.stride(1) == 1, fn, ": ", name, " needs a unit inner stride");
  const int64_t per = dt == torch::kFloat32 ? 4 : 8;
  TORCH_CHECK(aligned16(t) && (t.size(0) == 1 || t.stride(0) % per == 0), fn, ": ", name,
              " rows must be 16-byte aligned (base address and row stride)");
}

// the tensors of gemm / gemm2 against the epilogue that reads or writes them
void gemm_args(const char* fn, const torch::Tensor& A, const torch::Tensor& B, const torch::Tensor& C,
               const c10::optional<torch::Tensor>& bias, const c10::optional<torch::Tensor>& residual,
               const c10::optional<torch::Tensor>& aux, bool transA, bool transB, int64_t epi, bool accum) {
  TORCH_CHECK(A.is_cuda(), fn, ": A must be on the GPU");
  gemm_operand(fn, "A", A, torch::kBFloat16, A);
  gemm_operand(fn, "B", B, torch::kBFloat16, A);
  TORCH_CHECK(!accum || C.scalar_type() == torch::kFloat32, fn, ": accumulate needs f32 C");
  gemm_operand(fn, "C", C, accum ? torch::kFloat32 : torch::kBFloat16, A);
  const int64_t M = C.size(0), N = C.size(1), K = transA ? A.size(0) : A.size(1);
  TORCH_CHECK(M <= INT_MAX && N <= INT_MAX && K <= INT_MAX, fn, ": M, N, K must fit 32 bits");
  TORCH_CHECK((transA ? A.size(1) : A.size(0)) == M, fn, ": A/M mismatch");
  TORCH_CHECK((transB ? B.size(0) : B.size(1)) == K && (transB ? B.size(1) : B.size(0)) == N, fn, ": B mismatch");
  TORCH_CHECK(epi >= 0 && epi <= 7, fn, ": epilogue ", epi, " outside 0..7");
  const bool need_bias = epi >= 1 && epi <= 4, need_res = epi == 4 || epi == 5, need_aux = epi == 2 || epi == 3 || epi >= 6;
  if (need_bias) {
    TORCH_CHECK(bias.has_value(), fn, ": epilogue ", epi, " needs bias");
    TORCH_CHECK(bias->is_cuda() && bias->get_device() == A.get_device(), fn, ": bias must be on A's GPU");
    TORCH_CHECK(bias->scalar_type() == torch::kBFloat16, fn, ": bias must be bf16, got ", bias->scalar_type());
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == N && aligned16(*bias), fn,
                ": bias must be a contiguous 16-byte aligned [N] tensor, N = ", N, ", got ", bias->numel(), " elements");
  }
  const auto row_input = [&](const c10::optional<torch::Tensor>& t, const char* name) {
    TORCH_CHECK(t.has_value(), fn, ": epilogue ", epi, " needs ", name);
    gemm_operand(fn, name, *t, torch::kBFloat16, A);
    TORCH_CHECK(t->size(0) == M && t->size(1) == N, fn, ": ", name, " must be [M, N] = [", M, ", ", N, "]");
  };
  if (need_res) row_input(residual, "residual");
  if (need_aux) row_input(aux, "aux");
}

// C[M,N] (+)= alpha * op(A) @ op(B) with fused epilogue.
//   A: [M,K] row-major (transA=0) or [K,M] (transA=1); B: [N,K] (transB=0, "NT") or [K,N] (transB=1)
void gemm(torch::Tensor A, torch::Tensor B, torch::Tensor C, c10::optional<torch::Tensor> bias,
          c10::optional<torch::Tensor> residual, c10::optional<torch::Tensor> aux, bool transA, bool transB,
          int64_t epilogue, bool accum, double alpha) {
  gemm_args("gemm", A, B, C, bias, residual, aux, transA, transB, epilogue, accum);
  const int M = C.size(0), N = C.size(1);
  const int K = transA ? A.size(0) : A.size(1);
  check(mp_gemm(A.data_ptr(), B.data_ptr(), C.data_ptr(), ptr_or_null(bias), ptr_or_null(residual), mptr_or_null(aux),
                M, N, K, A.stride(0), B.stride(0), C.stride(0), residual.has_value() ? residual->stride(0) : 0,
                aux.has_value() ? aux->stride(0) : 0, transA, transB, epilogue, accum, (float)alpha, cur_stream()),
        "gemm");
}

// What the v2 GEMM will run (mp_gemm_plan.h).  env: the planner switches by name over their
// defaults; none: the process environment, read once.
g2::Plan gemm2_plan(int64_t M, int64_t N, int64_t K, bool transA, bool transB, bool accum, int64_t force_cfg,
                    const std::optional<PlanEnvDict>& env) {
  return g2::plan_gemm((int)M, (int)N, (int)K, transA, transB, accum, (int)force_cfg,
                       parse_env<g2::PlanEnv>("gemm2_plan", "a planner switch", env),
                       mp_gemm2_has_probe_engines() != 0);
}

// v2 engine (8 waves, glds staging).
// returns 1 if done, 0 if the combination is not provided by v2 (caller uses gemm()),
// 2 if done WITHOUT the requested fused column sums (caller sums separately)
int64_t gemm2(torch::Tensor A, torch::Tensor B, torch::Tensor C, c10::optional<torch::Tensor> bias,
              c10::optional<torch::Tensor> residual, c10::optional<torch::Tensor> aux, bool transA, bool transB,
              int64_t epilogue, bool accum, double alpha, int64_t force_cfg, c10::optional<torch::Tensor> colsum,
              double p_drop, int64_t seed) {
  gemm_args("gemm2", A, B, C, bias, residual, aux, transA, transB, epilogue, accum);
  const int M = C.size(0), N = C.size(1);
  const int K = transA ? A.size(0) : A.size(1);
  TORCH_CHECK(!colsum.has_value() || (colsum->is_cuda() && colsum->get_device() == A.get_device() &&
                                      colsum->scalar_type() == torch::kFloat32 && colsum->is_contiguous() &&
                                      colsum->numel() >= N),
              "gemm2: colsum must be a contiguous f32 [N] tensor on A's GPU");
  TORCH_CHECK(p_drop >= 0.0 && p_drop < 1.0, "gemm2: p_drop ", p_drop, " outside [0, 1)");
  if (p_drop > 0.0) {
    TORCH_CHECK(epilogue == 2 || epilogue == 3 || epilogue == 6 || epilogue == 7, "gemm2: p_drop with epilogue ",
                epilogue, ", which takes no dropout");
    // the mask index is row * ldc + column: act_fwd / act_bwd regenerate it for a contiguous output
    TORCH_CHECK(C.is_contiguous(), "gemm2: p_drop needs a contiguous C");
  }
  // split-K slabs (plain stores + one reduce pass instead of f32 atomics), or the stream-K
  // engine's flags + partial tiles: from the caching allocator on the current stream (graph
  // captures take it from their private pool), so concurrent streams never share one
  const g2::Plan plan = gemm2_plan(M, N, K, transA, transB, accum, force_cfg, std::nullopt);
  torch::Tensor ws;
  const int64_t ws_n = mp_gemm2_ws_floats(plan.cfg, plan.split, M, N, K);
  if (ws_n > 0) ws = torch::empty({ws_n}, C.options().dtype(torch::kFloat32));
  const auto run = [&](float* colsum_ptr) {
    return mp_gemm2(A.data_ptr(), B.data_ptr(), C.data_ptr(), ptr_or_null(bias), ptr_or_null(residual),
                    mptr_or_null(aux), M, N, K, A.stride(0), B.stride(0), C.stride(0),
                    residual.has_value() ? residual->stride(0) : 0, aux.has_value() ? aux->stride(0) : 0, transA,
                    transB, epilogue, accum, (float)alpha, plan.cfg, plan.split, (int)force_cfg,
                    ws.defined() ? ws.data_ptr<float>() : nullptr, colsum_ptr, (float)p_drop, (uint64_t)seed,
                    cur_stream());
  };
  int rc = run(colsum.has_value() ? colsum->data_ptr<float>() : nullptr);
  const bool no_colsum = rc == -3;
  if (no_colsum) rc = run(nullptr);
  if (rc == -2 || rc == -1) return 0;
  check(rc, "gemm2");
  return no_colsum ? 2 : 1;
}

// The operand arrays of a grouped weight-gradient launch, C[i] (f32 [N_i, K_i]) += alpha *
// dy[i]^T x[i] with dy [T_i, N_i], x [T_i, K_i] bf16 of unit inner stride: the launcher's
// (M, N, K) of problem i is (N_i, K_i, T_i).
struct DwGroup {
  const void* A[8];
  const void* B[8];
  float* C[8];
  int M[8], N[8], K[8];
  int64_t lda[8], ldb[8], ldc[8];
  void set(const char* fn, int i, const torch::Tensor& dy, const torch::Tensor& x, const torch::Tensor& c,
           const torch::Tensor& ref) {
    gemm_operand(fn, "dy", dy, torch::kBFloat16, ref);
    gemm_operand(fn, "x", x, torch::kBFloat16, ref);
    gemm_operand(fn, "C", c, torch::kFloat32, ref);
    A[i] = dy.data_ptr(), B[i] = x.data_ptr(), C[i] = c.data_ptr<float>();
    M[i] = (int)dy.size(1), N[i] = (int)x.size(1), K[i] = (int)dy.size(0);
    lda[i] = dy.stride(0), ldb[i] = x.stride(0), ldc[i] = c.stride(0);
  }
};

// one launch of 64x64 tiles
void gemm_tt_grouped(std::vector<torch::Tensor> dy, std::vector<torch::Tensor> x, std::vector<torch::Tensor> C,
                     double alpha) {
  const int n = (int)dy.size();
  TORCH_CHECK(n == (int)x.size() && n == (int)C.size() && n >= 1 && n <= 8, "gemm_tt_grouped: 1..8 problems");
  TORCH_CHECK(dy[0].is_cuda(), "gemm_tt_grouped: dy must be on the GPU");
  DwGroup g;
  for (int i = 0; i < n; ++i) {
    g.set("gemm_tt_grouped", i, dy[i], x[i], C[i], dy[0]);
    TORCH_CHECK(dy[i].size(0) == x[i].size(0) && C[i].size(0) == dy[i].size(1) && C[i].size(1) == x[i].size(1),
                "gemm_tt_grouped: shape mismatch");
  }
  check(mp_gemm_tt_grouped(n, g.A, g.B, g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc, (float)alpha, cur_stream()),
        "gemm_tt_grouped");
}

// long token counts: ONE token count T for the group, in one launch of 256x256 tiles at a
// common split-K factor (split = 0: the planner's; > 0: forced, clamped to T / 64) plus one
// reduce launch when that factor is > 1.  Returns the factor used.
int64_t gemm_dw_grouped(std::vector<torch::Tensor> dy, std::vector<torch::Tensor> x, std::vector<torch::Tensor> C,
                        double alpha, int64_t split) {
  const char* fn = "gemm_dw_grouped";
  const int n = (int)dy.size();
  TORCH_CHECK(n == (int)x.size() && n == (int)C.size() && n >= 1 && n <= 8, fn, ": 1..8 problems");
  TORCH_CHECK(split >= 0 && split <= INT_MAX, fn, ": split ", split, " must be >= 0");
  TORCH_CHECK(dy[0].is_cuda(), fn, ": dy must be on the GPU");
  const int64_t T = dy[0].dim() == 2 ? dy[0].size(0) : 0;
  DwGroup g;
  for (int i = 0; i < n; ++i) {
    g.set(fn, i, dy[i], x[i], C[i], dy[0]);
    TORCH_CHECK(dy[i].size(0) == T && x[i].size(0) == T, fn, ": every dy and x needs the same token count T = ", T,
                ", problem ", i, " has ", dy[i].size(0), " and ", x[i].size(0));
    TORCH_CHECK(C[i].size(0) == dy[i].size(1) && C[i].size(1) == x[i].size(1), fn, ": C[", i, "] must be [",
                dy[i].size(1), ", ", x[i].size(1), "]");
    TORCH_CHECK(dy[i].size(1) % 8 == 0 && x[i].size(1) % 8 == 0, fn, ": problem ", i, ": M = ", dy[i].size(1),
                " and N = ", x[i].size(1), " must be multiples of 8");
    TORCH_CHECK(dy[i].size(1) <= INT_MAX && x[i].size(1) <= INT_MAX, fn, ": M, N must fit 32 bits");
  }
  TORCH_CHECK(T % 64 == 0 && T <= INT_MAX, fn, ": T = ", T, " must be a multiple of 64");
  // split-K slabs from the caching allocator on the current stream (graph captures take
  // them from their private pool), as gemm2() does
  int64_t ws_n = 0;
  const int S = mp_gemm3_tt_grouped_plan(n, g.M, g.N, (int)T, (int)split, &ws_n);
  torch::Tensor ws;
  if (ws_n > 0) ws = torch::empty({ws_n}, C[0].options().dtype(torch::kFloat32));
  check(mp_gemm3_tt_grouped(n, g.A, g.B, g.C, g.M, g.N, (int)T, g.lda, g.ldb, g.ldc, (float)alpha, S,
                            ws.defined() ? ws.data_ptr<float>() : nullptr, cur_stream()),
        fn);
  return S;
}

void transpose(torch::Tensor in, torch::Tensor out) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda() && in.get_device() == out.get_device(), "transpose: in and out must be on one GPU");
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 && out.scalar_type() == torch::kBFloat16, "transpose: in and out must be bf16");
  TORCH_CHECK(in.dim() == 2 && out.dim() == 2 && in.stride(1) == 1 && out.stride(1) == 1, "transpose: 2-D rows");
  TORCH_CHECK(in.size(0) > 0 && in.size(1) > 0, "transpose: in is empty");
  TORCH_CHECK(out.size(0) == in.size(1) && out.size(1) == in.size(0), "transpose: shape");
  check(mp_transpose(in.data_ptr(), out.data_ptr(), in.size(0), in.size(1), in.stride(0), out.stride(0),
                     cur_stream()),
        "transpose");
}

// every W^T copy of an arena in one launch: desc int64 [n, 4] = (src off, dst off, R, C),
// tile0 int32 [n] = first 64x64 tile of each matrix
void transpose_batched(torch::Tensor src, torch::Tensor dst, torch::Tensor desc, torch::Tensor tile0,
                       int64_t total_tiles) {
  TORCH_CHECK(desc.scalar_type() == torch::kInt64 && tile0.scalar_type() == torch::kInt32 && desc.is_cuda() &&
                  tile0.is_cuda() && desc.size(0) == tile0.size(0),
              "transpose_batched: bad descriptors");
  check(mp_transpose_batched(src.data_ptr(), dst.data_ptr(), desc.data_ptr<int64_t>(), tile0.data_ptr<int>(),
                             (int)desc.size(0), (int)total_tiles, cur_stream()),
        "transpose_batched");
}

// y[M, N] = epi(x[M, K] @ What^T), M <= 16 (csrc/kernels/gemv_skinny.hip): w int8 [N, K] with scale f32 [N],
// w uint8 [N, K / 2] (packed 4-bit) with scale f32 [K / 128, N], or w bf16 [N, K] without.  No allocation, no
// synchronisation.
void gemv_skinny(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> scale, torch::Tensor y,
                 c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> residual, bool gelu,
                 int64_t force_split) {
  // x / y / residual: bf16 rows of any stride
  auto rows = [](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.dim() == 2 && t.stride(1) == 1 &&
                    (t.size(0) == 1 || t.stride(0) >= t.size(1)),
                name, " must be bf16 GPU rows [M, cols] with a unit inner stride");
  };
  rows(x, "gemv_skinny: x");
  rows(y, "gemv_skinny: y");
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.is_contiguous(), "gemv_skinny: w must be a contiguous [N, K] GPU matrix");
  const bool w8 = w.scalar_type() == torch::kInt8, w4 = w.scalar_type() == torch::kUInt8;
  TORCH_CHECK(w8 || w4 || w.scalar_type() == torch::kBFloat16, "gemv_skinny: w must be int8, uint8 (packed 4-bit) or bf16, got ",
              w.scalar_type());
  TORCH_CHECK((w8 || w4) == scale.has_value(), "gemv_skinny: int8 and 4-bit weights take a scale, bf16 weights none");
  const int code = w4 ? 0 : w8 ? 1 : 2;
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= gemv::MAX_M, "gemv_skinny: M = ", M, " outside [1, ", gemv::MAX_M, "]");
  TORCH_CHECK(w.size(1) * (w4 ? 2 : 1) == K && y.size(0) == M && y.size(1) == N, "gemv_skinny: shapes x ", x.sizes(), " w ",
              w.sizes(), " y ", y.sizes());
  TORCH_CHECK(gemv::plan(N, K, code, (int)force_split).rows != 0, "gemv_skinny: N = ", N, ", K = ", K,
              ", force_split = ", force_split, " is not supported (K a multiple of 32, of 128 for 4-bit weights; "
              "force_split <= 16)");
  TORCH_CHECK(aligned16(w), "gemv_skinny: w must be 16-byte aligned");
  if (w8) {
    req(*scale, torch::kFloat32, "gemv_skinny: scale");
    TORCH_CHECK(scale->numel() == N && scale->is_contiguous(), "gemv_skinny: scale must hold N contiguous values");
  }
  if (w4) {
    req(*scale, torch::kFloat32, "gemv_skinny: scale");
    TORCH_CHECK(scale->dim() == 2 && scale->size(0) == K / gemv::KSTEP && scale->size(1) == N && scale->is_contiguous(),
                "gemv_skinny: the scale of 4-bit weights must be contiguous [K / 128, N]");
  }
  if (bias.has_value()) {
    req(*bias, torch::kBFloat16, "gemv_skinny: bias");
    TORCH_CHECK(bias->numel() == N && bias->is_contiguous(), "gemv_skinny: bias must hold N contiguous values");
  }
  TORCH_CHECK(!gelu || bias.has_value(), "gemv_skinny: the GELU epilogue needs a bias");
  TORCH_CHECK(!gelu || !residual.has_value(), "gemv_skinny: no residual behind GELU");
  int64_t ldr = 0;
  if (residual.has_value()) {
    rows(*residual, "gemv_skinny: residual");
    TORCH_CHECK(residual->size(0) == M && residual->size(1) == N, "gemv_skinny: residual must be [M, N]");
    ldr = residual->stride(0);
  }
  check(mp_gemv_skinny(w.data_ptr(), code != 2 ? scale->data_ptr<float>() : nullptr, code, x.data_ptr(), y.data_ptr(),
                       ptr_or_null(bias), ptr_or_null(residual), (int)M, (int)N, (int)K, x.stride(0), y.stride(0), ldr,
                       gelu ? 1 : 0, (int)force_split, cur_stream()),
        "gemv_skinny");
}

// q int8 [N, K] with scale [N], or q uint8 [N, K / 2] (packed 4-bit) with scale [K / 128, N]
void dequant_w8(torch::Tensor q, torch::Tensor scale, torch::Tensor out) {
  req(scale, torch::kFloat32, "dequant_w8: scale");
  req(out, torch::kBFloat16, "dequant_w8: out");
  if (q.scalar_type() == torch::kUInt8) {
    req(q, torch::kUInt8, "dequant_w8: q");
    TORCH_CHECK(q.dim() == 2 && q.is_contiguous() && out.is_contiguous() && out.numel() == 2 * q.numel(),
                "dequant_w8: packed 4-bit q [N, K / 2] and out [N, K], both contiguous");
    const int64_t N = q.size(0), K = 2 * q.size(1);
    TORCH_CHECK(K >= 128 && K % 128 == 0, "dequant_w8: K = ", K, " must be a multiple of 128 for 4-bit weights");
    TORCH_CHECK(scale.is_contiguous() && scale.dim() == 2 && scale.size(0) == K / 128 && scale.size(1) == N,
                "dequant_w8: the scale of 4-bit weights must be contiguous [K / 128, N]");
    check(mp_dequant_w4(q.data_ptr(), scale.data_ptr<float>(), out.data_ptr(), N, K, cur_stream()), "dequant_w8 (4-bit)");
    return;
  }
  req(q, torch::kInt8, "dequant_w8: q");
  TORCH_CHECK(q.dim() == 2 && q.is_contiguous() && out.is_contiguous() && out.numel() == q.numel() &&
                  scale.is_contiguous() && scale.numel() == q.size(0),
              "dequant_w8: q [N, K], scale [N], out [N, K], all contiguous");
  TORCH_CHECK(q.size(1) % 16 == 0, "dequant_w8: K = ", q.size(1), " must be a multiple of 16");
  check(mp_dequant_w8(q.data_ptr(), scale.data_ptr<float>(), out.data_ptr(), q.size(0), q.size(1), cur_stream()),
        "dequant_w8");
}

}  // namespace

void register_gemm(py::module& m) {
  m.def("gemm", &gemm);
  m.def("gemm2", &gemm2, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("bias"), py::arg("residual"), py::arg("aux"),
        py::arg("transA"), py::arg("transB"), py::arg("epilogue"), py::arg("accum"), py::arg("alpha"),
        py::arg("force_cfg"), py::arg("colsum"), py::arg("p_drop") = 0.0, py::arg("seed") = 0);
  m.def("gemm2_plan", [](int64_t M, int64_t N, int64_t K, bool transA, bool transB, bool accum, int64_t force_cfg,
                         std::optional<PlanEnvDict> env) {
    const g2::Plan p = gemm2_plan(M, N, K, transA, transB, accum, force_cfg, env);
    return std::make_tuple(p.cfg, p.split);
  }, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("transA"), py::arg("transB"), py::arg("accum"),
     py::arg("force_cfg"), py::arg("env") = py::none(),
     "engine config + split-K factor the v2 GEMM picks (14: stream-K gemm7); env: the MIPIPE_* planner "
     "switches as a dict over their defaults instead of the process environment");
  m.def("gemm2_has_probe_engines", []() { return mp_gemm2_has_probe_engines() != 0; });
  m.def("gemm_tt_grouped", &gemm_tt_grouped, py::arg("dy"), py::arg("x"), py::arg("C"), py::arg("alpha") = 1.0);
  m.def("gemm_dw_grouped", &gemm_dw_grouped, py::arg("dy"), py::arg("x"), py::arg("C"), py::arg("alpha") = 1.0,
        py::arg("split") = 0);
  m.def("transpose", &transpose);
  m.def("transpose_batched", &transpose_batched);
  m.def("gemv_skinny", &gemv_skinny, py::arg("x"), py::arg("w"), py::arg("scale"), py::arg("y"), py::arg("bias"),
        py::arg("residual"), py::arg("gelu") = false, py::arg("force_split") = 0);
  m.def("dequant_w8", &dequant_w8);
  m.def("gemv_plan", [](int64_t N, int64_t K, int64_t wbytes, int64_t force_split) {
    const gemv::Plan p = gemv::plan(N, K, (int)wbytes, (int)force_split);
    TORCH_CHECK(p.rows != 0, "gemv_plan: N = ", N, ", K = ", K, ", wbytes = ", wbytes, ", force_split = ", force_split,
                " is not supported");
    return std::make_tuple(p.rows, p.ksplit);
  }, py::arg("N"), py::arg("K"), py::arg("wbytes"), py::arg("force_split") = 0,
     "(weight rows per workgroup, K-splits = waves per workgroup) of the skinny-M kernel");
}

}  // namespace mipipe_bind
