// Bindings of the training attention: attention.hip (bf16), attention_f32.hip and the
// document-masked attention_doc.hip, plus the launch plan of mp_attn_plan.h.
#include "common.h"
#include "mp_attn_plan.h"

namespace mipipe_bind {
namespace {

// Argument checks of attn_fwd / attn_bwd, all before any launch: the kernels index raw
// pointers by (B, S, heads, D) and the row strides, so a tensor of another dtype or a smaller
// one would be read or written past its end.
void attn_check_dims(int64_t B, int64_t Sq, int64_t Sk, int64_t H, int64_t Hkv, int64_t D) {
  TORCH_CHECK(B > 0 && Sq > 0 && Sk > 0 && H > 0 && Hkv > 0, "attn: B, Sq, Sk, H, Hkv must be positive (got ", B, ", ",
              Sq, ", ", Sk, ", ", H, ", ", Hkv, ")");
  TORCH_CHECK(H % Hkv == 0, "attn: H = ", H, " is not a multiple of Hkv = ", Hkv);
  TORCH_CHECK(D > 0 && D % 8 == 0, "attn: head_dim ", D, " is not a positive multiple of 8");
  TORCH_CHECK(B * std::max(Sq, Sk) <= INT32_MAX && std::max(H, Hkv) * D <= INT32_MAX, "attn: problem too large");
}

// a token-major [>= rows, >= cols] view of dtype `dt` with a unit inner stride
void attn_check_rows(const torch::Tensor& t, torch::ScalarType dt, int64_t rows, int64_t cols, const char* name) {
  TORCH_CHECK(t.is_cuda(), "attn: ", name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, "attn: ", name, " has dtype ", t.scalar_type(), ", q has ", dt,
              " (q, k, v, o, dout, dq, dk, dv share one dtype)");
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, "attn: ", name, " must be a 2-D token-major view with unit inner stride");
  TORCH_CHECK(t.size(0) >= rows && t.size(1) >= cols, "attn: ", name, " is [", t.size(0), ", ", t.size(1),
              "], needs at least [", rows, ", ", cols, "]");
  TORCH_CHECK(rows == 1 || t.stride(0) >= cols, "attn: ", name, " rows overlap (row stride ", t.stride(0), " < ", cols, ")");
}

// a contiguous f32 vector of at least n elements (lse, delta)
void attn_check_vec(const torch::Tensor& t, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() >= n, "attn: ", name,
              " must be a contiguous f32 GPU tensor of at least B*H*Sq = ", n, " elements");
}

// q/k/v/o are [B*S, stride] row views (token-major), heads at h*D inside a row.
void attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o, torch::Tensor lse, int64_t B,
              int64_t Sq, int64_t Sk, int64_t H, int64_t Hkv, int64_t D, bool causal, double scale, double p,
              int64_t seed) {
  attn_check_dims(B, Sq, Sk, H, Hkv, D);
  const torch::ScalarType dt = q.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kFloat32, "attn: bf16 or f32");
  attn_check_rows(q, dt, B * Sq, H * D, "q");
  attn_check_rows(k, dt, B * Sk, Hkv * D, "k");
  attn_check_rows(v, dt, B * Sk, Hkv * D, "v");
  attn_check_rows(o, dt, B * Sq, H * D, "o");
  attn_check_vec(lse, B * H * Sq, "lse");
  if (dt == torch::kFloat32) {
    // f32 flash attention (attention_f32.hip): the reference-precision path
    check(mp_attn_f32_fwd(q.data_ptr<float>(), k.data_ptr<float>(), v.data_ptr<float>(), o.data_ptr<float>(),
                          lse.data_ptr<float>(), B, Sq, Sk, H, Hkv, D, q.stride(0), k.stride(0), v.stride(0),
                          o.stride(0), causal, (float)scale, (float)p, (uint64_t)seed, cur_stream()),
          "attn_f32_fwd");
    return;
  }
  check(mp_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), B, Sq, Sk, H, Hkv,
                    D, q.stride(0), k.stride(0), v.stride(0), o.stride(0), causal, (float)scale, (float)p,
                    (uint64_t)seed, cur_stream()),
        "attn_fwd");
}

void attn_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o, torch::Tensor dout,
              torch::Tensor lse, torch::Tensor delta, torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
              int64_t B, int64_t Sq, int64_t Sk, int64_t H, int64_t Hkv, int64_t D, bool causal,
              double scale, double p, int64_t seed, c10::optional<torch::Tensor> dbias) {
  attn_check_dims(B, Sq, Sk, H, Hkv, D);
  const torch::ScalarType dt = q.scalar_type();
  TORCH_CHECK(dt == torch::kBFloat16 || dt == torch::kFloat32, "attn: bf16 or f32");
  attn_check_rows(q, dt, B * Sq, H * D, "q");
  attn_check_rows(k, dt, B * Sk, Hkv * D, "k");
  attn_check_rows(v, dt, B * Sk, Hkv * D, "v");
  attn_check_rows(o, dt, B * Sq, H * D, "o");
  attn_check_rows(dout, dt, B * Sq, H * D, "dout");
  attn_check_rows(dq, dt, B * Sq, H * D, "dq");
  attn_check_rows(dk, dt, B * Sk, Hkv * D, "dk");
  attn_check_rows(dv, dt, B * Sk, Hkv * D, "dv");
  attn_check_vec(lse, B * H * Sq, "lse");
  attn_check_vec(delta, B * H * Sq, "delta");
  TORCH_CHECK(o.stride(0) == dout.stride(0), "o and dout must share a row stride");
  if (dt == torch::kFloat32) {
    TORCH_CHECK(!dbias.has_value(), "attn_bwd f32: no fused bias sums");
    check(mp_attn_f32_bwd(q.data_ptr<float>(), k.data_ptr<float>(), v.data_ptr<float>(), o.data_ptr<float>(),
                          dout.data_ptr<float>(), lse.data_ptr<float>(), delta.data_ptr<float>(), dq.data_ptr<float>(),
                          dk.data_ptr<float>(), dv.data_ptr<float>(), B, Sq, Sk, H, Hkv, D, q.stride(0), k.stride(0),
                          v.stride(0), o.stride(0), dq.stride(0), dk.stride(0), dv.stride(0), causal, (float)scale,
                          (float)p, (uint64_t)seed, cur_stream()),
          "attn_f32_bwd");
    return;
  }
  // dbias: f32 [(H + 2 Hkv) D] QKV bias gradient, accumulated by the kernels (q | k | v)
  float* cs = nullptr;
  if (dbias.has_value()) {
    TORCH_CHECK(dbias->is_cuda() && dbias->scalar_type() == torch::kFloat32 && dbias->is_contiguous() &&
                    dbias->numel() == (H + 2 * Hkv) * D,
                "attn_bwd: dbias must be a contiguous f32 [(H + 2 Hkv) D] tensor");
    cs = dbias->data_ptr<float>();
  }
  check(mp_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(), lse.data_ptr<float>(),
                    delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B,
                    Sq, Sk, H, Hkv, D, q.stride(0), k.stride(0), v.stride(0), o.stride(0), dq.stride(0), dk.stride(0),
                    dv.stride(0), causal, (float)scale, (float)p, (uint64_t)seed, cs,
                    cs ? cs + H * D : nullptr, cs ? cs + (H + Hkv) * D : nullptr, cur_stream()),
        "attn_bwd");
}

// Document-masked causal attention (attention_doc.hip).  All checks before any launch.
void attn_doc_check_common(const torch::Tensor& q, int64_t B, int64_t S, int64_t H, int64_t Hkv, int64_t D,
                           bool causal, double p) {
  attn_check_dims(B, S, S, H, Hkv, D);
  TORCH_CHECK(causal, "attn_doc: the document mask is causal only");
  TORCH_CHECK(p == 0.0, "attn_doc: no dropout (p_drop = ", p, ")");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn_doc: bf16 tensors only (q has ", q.scalar_type(), ")");
  TORCH_CHECK(D == 64 || D == 128, "attn_doc: head_dim ", D, " is not supported (64 or 128)");
}

// 16-byte rows (the kernels move 8 bf16 at a time) whose offsets inside one sequence fit 32 bits
void attn_doc_check_rows(const torch::Tensor& t, int64_t B, int64_t S, int64_t cols, const char* name) {
  attn_check_rows(t, torch::kBFloat16, B * S, cols, name);
  TORCH_CHECK(aligned16(t) && (B * S == 1 || t.stride(0) % 8 == 0), "attn_doc: ", name,
              " rows must be 16-byte aligned (row stride ", t.stride(0), ")");
  TORCH_CHECK((S + 128) * t.stride(0) * 2 < (int64_t(1) << 31), "attn_doc: ", name, " row stride ", t.stride(0),
              " is too large for S = ", S);
}

void attn_doc_check_bounds(const torch::Tensor& t, const torch::Tensor& q, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == q.device(), "attn_doc: ", name, " must be on q's device");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, "attn_doc: ", name, " must be int32 (got ", t.scalar_type(), ")");
  TORCH_CHECK(t.is_contiguous(), "attn_doc: ", name, " must be contiguous");
  TORCH_CHECK(t.numel() == n, "attn_doc: ", name, " has ", t.numel(), " entries, needs B*S = ", n);
}

void attn_doc_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o, torch::Tensor lse,
                  torch::Tensor doc_start, int64_t B, int64_t S, int64_t H, int64_t Hkv, int64_t D, bool causal,
                  double scale, double p) {
  attn_doc_check_common(q, B, S, H, Hkv, D, causal, p);
  attn_doc_check_rows(q, B, S, H * D, "q");
  attn_doc_check_rows(k, B, S, Hkv * D, "k");
  attn_doc_check_rows(v, B, S, Hkv * D, "v");
  attn_doc_check_rows(o, B, S, H * D, "o");
  attn_check_vec(lse, B * H * S, "lse");
  attn_doc_check_bounds(doc_start, q, B * S, "doc_start");
  check(mp_attn_doc_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                        doc_start.data_ptr<int>(), B, S, H, Hkv, D, q.stride(0), k.stride(0), v.stride(0), o.stride(0),
                        (float)scale, cur_stream()),
        "attn_doc_fwd");
}

void attn_doc_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o, torch::Tensor dout,
                  torch::Tensor lse, torch::Tensor delta, torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                  torch::Tensor doc_start, torch::Tensor doc_end, int64_t B, int64_t S, int64_t H, int64_t Hkv,
                  int64_t D, bool causal, double scale, double p) {
  attn_doc_check_common(q, B, S, H, Hkv, D, causal, p);
  attn_doc_check_rows(q, B, S, H * D, "q");
  attn_doc_check_rows(k, B, S, Hkv * D, "k");
  attn_doc_check_rows(v, B, S, Hkv * D, "v");
  attn_doc_check_rows(o, B, S, H * D, "o");
  attn_doc_check_rows(dout, B, S, H * D, "dout");
  attn_doc_check_rows(dq, B, S, H * D, "dq");
  attn_doc_check_rows(dk, B, S, Hkv * D, "dk");
  attn_doc_check_rows(dv, B, S, Hkv * D, "dv");
  attn_check_vec(lse, B * H * S, "lse");
  attn_check_vec(delta, B * H * S, "delta");
  TORCH_CHECK(o.stride(0) == dout.stride(0), "o and dout must share a row stride");
  attn_doc_check_bounds(doc_start, q, B * S, "doc_start");
  attn_doc_check_bounds(doc_end, q, B * S, "doc_end");
  check(mp_attn_doc_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(), lse.data_ptr<float>(),
                        delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), doc_start.data_ptr<int>(),
                        doc_end.data_ptr<int>(), B, S, H, Hkv, D, q.stride(0), k.stride(0), v.stride(0), o.stride(0),
                        dq.stride(0), dk.stride(0), dv.stride(0), (float)scale, cur_stream()),
        "attn_doc_bwd");
}

// tokens: contiguous int64 [B, S] on the GPU -> (doc_start, doc_end), int32 [B*S]; no host sync
std::vector<torch::Tensor> doc_bounds(torch::Tensor tokens, int64_t eos) {
  TORCH_CHECK(tokens.is_cuda() && tokens.scalar_type() == torch::kInt64 && tokens.dim() == 2 && tokens.is_contiguous(),
              "doc_bounds: tokens must be a contiguous int64 [B, S] GPU tensor");
  const int64_t B = tokens.size(0), S = tokens.size(1);
  TORCH_CHECK(B > 0 && S > 0 && B * S <= INT32_MAX, "doc_bounds: bad shape [", B, ", ", S, "]");
  auto opt = torch::TensorOptions().dtype(torch::kInt32).device(tokens.device());
  torch::Tensor ds = torch::empty({B * S}, opt), de = torch::empty({B * S}, opt);
  check(mp_doc_bounds(tokens.data_ptr<int64_t>(), eos, ds.data_ptr<int>(), de.data_ptr<int>(), (int)B, (int)S,
                      cur_stream()),
        "doc_bounds");
  return {ds, de};
}

// What attn_fwd / attn_bwd will launch for a bf16 problem (mp_attn_plan.h): {"fwd": launch,
// "bwd": [launch, ...]}, a launch being {"kernel", "dp", "grid", "lds"}.  env: the
// MIPIPE_ATTN_* switches by name over their defaults; none: the process environment.
py::dict attn_plan(int64_t B, int64_t Sq, int64_t Sk, int64_t H, int64_t Hkv, int64_t D, int64_t qs, int64_t ks,
                   int64_t vs, int64_t os, bool causal, bool drop, const std::optional<PlanEnvDict>& env) {
  TORCH_CHECK(B > 0 && Sq > 0 && Sk > 0 && H > 0 && Hkv > 0 && D > 0, "attn_plan: sizes must be positive");
  const attn::AttnEnv e = parse_env<attn::AttnEnv>("attn_plan", "an attention switch", env);
  const attn::Launch f = attn::plan_attn_fwd((int)B, (int)Sq, (int)Sk, (int)H, (int)Hkv, (int)D, ks, vs, causal, drop, e);
  const attn::BwdPlan b =
      attn::plan_attn_bwd((int)B, (int)Sq, (int)Sk, (int)H, (int)Hkv, (int)D, qs, ks, vs, os, causal, drop, e);
  TORCH_CHECK(f.kernel != attn::K_NONE && b.n > 0, "attn_plan: no kernel for D = ", D, ", H = ", H, ", Hkv = ", Hkv,
              " (D a multiple of 8 up to 256, H a multiple of Hkv)");
  const auto launch = [](const attn::Launch& l) {
    py::dict d;
    d["kernel"] = attn::kernel_name(l.kernel);
    d["dp"] = l.dp;
    d["grid"] = py::make_tuple(l.gx, l.gy);
    d["lds"] = l.lds;
    return d;
  };
  py::list bwd;
  for (int i = 0; i < b.n; ++i) bwd.append(launch(b.l[i]));
  py::dict out;
  out["fwd"] = launch(f);
  out["bwd"] = bwd;
  return out;
}

}  // namespace

void register_attention(py::module& m) {
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_doc_fwd", &attn_doc_fwd);
  m.def("attn_doc_bwd", &attn_doc_bwd);
  m.def("doc_bounds", &doc_bounds);
  m.def("attn_plan", &attn_plan, py::arg("B"), py::arg("Sq"), py::arg("Sk"), py::arg("H"), py::arg("Hkv"), py::arg("D"),
        py::arg("qs"), py::arg("ks"), py::arg("vs"), py::arg("os"), py::arg("causal"), py::arg("drop"),
        py::arg("env") = py::none(),
        "kernels, grids and LDS bytes the bf16 attention launches; env: the MIPIPE_ATTN_* switches as a dict over "
        "their defaults instead of the process environment");
}

}  // namespace mipipe_bind
