// Bindings of gemm_f32.hip: the f32 MFMA GEMMs of the reference-precision path.
#include "common.h"

namespace mipipe_bind {
namespace {

// the f32 GEMM operands: on one GPU, f32, 2-D, non-empty
void gemm_f32_args(const char* fn, const torch::Tensor& A, const torch::Tensor& B, const torch::Tensor& C,
                   const c10::optional<torch::Tensor>& bias) {
  const torch::Tensor* ts[3] = {&A, &B, &C};
  const char* names[3] = {"A", "B", "C"};
  for (int i = 0; i < 3; ++i) {
    TORCH_CHECK(ts[i]->is_cuda(), fn, ": ", names[i], " must be on the GPU");
    TORCH_CHECK(ts[i]->get_device() == A.get_device(), fn, ": ", names[i], " is on another device than A");
    TORCH_CHECK(ts[i]->scalar_type() == torch::kFloat32, fn, ": ", names[i], " must be f32, got ", ts[i]->scalar_type());
    TORCH_CHECK(ts[i]->dim() == 2, fn, ": ", names[i], " must be 2-D, got ", ts[i]->dim(), " dimensions");
    TORCH_CHECK(ts[i]->size(0) > 0 && ts[i]->size(1) > 0, fn, ": ", names[i], " is empty");
  }
  if (bias.has_value())
    TORCH_CHECK(bias->is_cuda() && bias->get_device() == A.get_device() && bias->scalar_type() == torch::kFloat32, fn,
                ": bias must be an f32 tensor on A's GPU");
}

// Which stride of a 2-D operand is 1: *unit_first = 1 when it is dimension `first`, 0 when it
// is the other one; *ld = the stride of the dimension that is not.  `first` is tested first, so
// it also decides the answer for a [K,1] or [1,N] operand, whose strides can both be 1.
// False when neither stride is 1.
bool f32_layout(const torch::Tensor& t, int first, int* unit_first, int64_t* ld) {
  if (t.stride(first) == 1) { *unit_first = 1; *ld = t.stride(1 - first); }
  else if (t.stride(1 - first) == 1) { *unit_first = 0; *ld = t.stride(first); }
  else return false;
  return true;
}

// f32 MFMA GEMM: C (+)= alpha * A @ B (+ bias); A [M,K], B [K,N] 2-D views with either inner
// stride 1; returns 1 if done, 0 if the layout is not supported (caller falls back)
int64_t gemm_f32(torch::Tensor A, torch::Tensor B, torch::Tensor C, c10::optional<torch::Tensor> bias, double alpha,
                 bool accumulate) {
  gemm_f32_args("gemm_f32", A, B, C, bias);
  const int M = A.size(0), K = A.size(1), N = B.size(1);
  TORCH_CHECK(B.size(0) == K && C.size(0) == M && C.size(1) == N, "gemm_f32: shape mismatch");
  int a_kc, b_nc;  // this launcher names B by its N-contiguous layout: stride(1) is tested first
  int64_t lda, ldb;
  if (C.stride(1) != 1 || !f32_layout(A, 1, &a_kc, &lda) || !f32_layout(B, 1, &b_nc, &ldb)) return 0;
  if (bias.has_value()) TORCH_CHECK(bias->is_contiguous() && bias->numel() == N, "gemm_f32: bias [N]");
  const int rc = mp_gemm_f32(A.data_ptr<float>(), B.data_ptr<float>(), C.data_ptr<float>(),
                             bias.has_value() ? bias->data_ptr<float>() : nullptr, M, N, K, lda, a_kc, ldb, b_nc,
                             C.stride(0), (float)alpha, accumulate ? 1 : 0, cur_stream());
  if (rc == -1) return 0;
  check(rc, "gemm_f32");
  return 1;
}

// f32 GEMM with fused epilogues (gemm_f32.hip mp_gemm_f32_ex): C = epi(alpha * A @ B (+ C)).
// A [M,K], B [K,N] 2-D views with either inner stride 1 (a transposed view of an [N,K]
// weight is the K-contiguous B); C row-major.  epi: 0 none, 1 bias, 2 bias+ReLU(+dropout,
// pre-activation -> X), 3 residual R, 4 bias+residual, 5 dReLU(R = pre-activation) x mask.
// Returns 1 if done, 0 if the layout is not supported.
int64_t gemm_f32_ex(torch::Tensor A, torch::Tensor B, torch::Tensor C, c10::optional<torch::Tensor> bias,
                    c10::optional<torch::Tensor> R, c10::optional<torch::Tensor> X, int64_t epi, double alpha,
                    bool accumulate, double p_drop, int64_t seed, int64_t force_ks) {
  gemm_f32_args("gemm_f32_ex", A, B, C, bias);
  TORCH_CHECK(epi >= 0 && epi <= 5, "gemm_f32_ex: epi ", epi, " outside 0..5");
  TORCH_CHECK(p_drop >= 0.0 && p_drop < 1.0, "gemm_f32_ex: p_drop ", p_drop, " outside [0, 1)");
  TORCH_CHECK(p_drop == 0.0 || epi == 2 || epi == 5, "gemm_f32_ex: p_drop with epi ", epi, ", which takes no dropout");
  const int M = A.size(0), K = A.size(1), N = B.size(1);
  TORCH_CHECK(B.size(0) == K && C.size(0) == M && C.size(1) == N, "gemm_f32_ex: shape mismatch");
  int a_kc, b_kc;  // this launcher names B by its K-contiguous layout: stride(0) is tested first
  int64_t lda, ldb;
  if (C.stride(1) != 1 || !f32_layout(A, 1, &a_kc, &lda) || !f32_layout(B, 0, &b_kc, &ldb)) return 0;
  const bool need_bias = epi == 1 || epi == 2 || epi == 4, need_r = epi >= 3, need_x = epi == 2;
  TORCH_CHECK(!need_bias || (bias.has_value() && bias->is_contiguous() && bias->numel() == N), "gemm_f32_ex: bias [N]");
  // R / X: returns the row stride
  const auto rows_mn = [&](const c10::optional<torch::Tensor>& t, const char* name) {
    TORCH_CHECK(t.has_value() && t->is_cuda() && t->get_device() == A.get_device() &&
                    t->scalar_type() == torch::kFloat32 && t->dim() == 2 && t->stride(1) == 1 && t->size(0) == M &&
                    t->size(1) == N, "gemm_f32_ex: ", name, " must be [M,N] f32 rows on A's GPU");
    return t->stride(0);
  };
  const int64_t ldr = need_r ? rows_mn(R, "R") : 0, ldx = need_x ? rows_mn(X, "X") : 0;
  // split-K slabs from the caching allocator (inside a graph capture: the graph's pool)
  const int64_t ws_n = mp_gemm_f32_ws_elems(M, N, K, (int)force_ks);
  torch::Tensor ws;
  if (ws_n > 0) ws = torch::empty({ws_n}, A.options());
  const int rc = mp_gemm_f32_ex(A.data_ptr<float>(), B.data_ptr<float>(), C.data_ptr<float>(),
                                need_bias ? bias->data_ptr<float>() : nullptr, need_r ? R->data_ptr<float>() : nullptr,
                                need_x ? X->data_ptr<float>() : nullptr, M, N, K, lda, a_kc, ldb, b_kc, C.stride(0), ldr,
                                ldx, (int)epi, (float)alpha, accumulate ? 1 : 0, (float)p_drop, (uint64_t)seed,
                                (int)force_ks, ws_n > 0 ? ws.data_ptr<float>() : nullptr, cur_stream());
  if (rc == -1) return 0;
  check(rc, "gemm_f32_ex");
  return 1;
}

}  // namespace

void register_gemm_f32(py::module& m) {
  m.def("gemm_f32", &gemm_f32);
  m.def("gemm_f32_ex", &gemm_f32_ex, py::arg("A"), py::arg("B"), py::arg("C"), py::arg("bias"), py::arg("R"),
        py::arg("X"), py::arg("epi") = 0, py::arg("alpha") = 1.0, py::arg("accumulate") = false,
        py::arg("p_drop") = 0.0, py::arg("seed") = 0, py::arg("force_ks") = 0);
  m.def("gemm_f32_plan", [](int64_t M, int64_t N, int64_t K, int64_t force_ks) {
    int split = 1, sk_grid = 0, sk_chunk = 0;
    const int big = mp_gemm_f32_plan((int)M, (int)N, (int)K, (int)force_ks, &split, &sk_grid, &sk_chunk);
    return std::make_tuple(big != 0, split, sk_grid, sk_chunk);
  }, "what gemm_f32_ex will run: (128x128 engine, split-K factor, stream-K workgroups, K-tile pairs per workgroup)");
  m.def("gemm_f32_set_lanes", &mp_gemm_f32_set_lanes);
}

}  // namespace mipipe_bind
