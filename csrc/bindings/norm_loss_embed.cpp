// Bindings of norm.hip, xent.hip and embedding.hip: normalisation (+ fused residual add /
// dropout), the cross-entropy loss and the token / position embedding.
#include "common.h"

namespace mipipe_bind {
namespace {

void norm_fwd(bool rms, torch::Tensor a, c10::optional<torch::Tensor> b, torch::Tensor w,
              c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> s_out, torch::Tensor y,
              c10::optional<torch::Tensor> mean, torch::Tensor rstd, double eps, double p, int64_t seed) {
  const int f32 = storage(a, "a");
  const auto dt = a.scalar_type();
  req(a, dt, "a");
  req(y, dt, "y");
  req(w, dt, "w");
  if (b.has_value()) req(*b, dt, "b");
  if (bias.has_value()) req(*bias, dt, "bias");
  if (s_out.has_value()) req(*s_out, dt, "s_out");
  req(rstd, torch::kFloat32, "rstd");
  const int D = a.size(-1);
  const int rows = a.numel() / D;
  TORCH_CHECK(!b.has_value() || (s_out.has_value() && b->numel() == a.numel()), "b needs s_out");
  TORCH_CHECK(rms || mean.has_value(), "LayerNorm needs mean");
  TORCH_CHECK(rstd.numel() >= rows && w.numel() == D, "bad norm shapes");
  check(mp_norm_fwd(f32, rms, a.data_ptr(), ptr_or_null(b), w.data_ptr(), ptr_or_null(bias), mptr_or_null(s_out),
                    y.data_ptr(), mean.has_value() ? mean->data_ptr<float>() : nullptr, rstd.data_ptr<float>(), rows,
                    D, (float)eps, (float)p, (uint64_t)seed, cur_stream()),
        "norm_fwd");
}

// returns 0, or -3 when the requested fused column sums are not available for this shape
// (the caller then sums separately); other failures raise
int64_t norm_bwd(bool rms, torch::Tensor dy, torch::Tensor s, torch::Tensor w, c10::optional<torch::Tensor> mean,
                 torch::Tensor rstd, c10::optional<torch::Tensor> dres, torch::Tensor ds,
                 c10::optional<torch::Tensor> dbranch, torch::Tensor dw, c10::optional<torch::Tensor> dbias, double p,
                 int64_t seed, c10::optional<torch::Tensor> cs_res, c10::optional<torch::Tensor> cs_ds) {
  const int f32 = storage(dy, "dy");
  const auto dt = dy.scalar_type();
  req(dy, dt, "dy");
  req(s, dt, "s");
  req(ds, dt, "ds");
  req(w, dt, "w");
  if (dres.has_value()) req(*dres, dt, "dres");
  if (dbranch.has_value()) req(*dbranch, dt, "dbranch");
  req(dw, torch::kFloat32, "dw");
  const int D = dy.size(-1);
  const int rows = dy.numel() / D;
  TORCH_CHECK(s.numel() == dy.numel() && ds.numel() == dy.numel() && dw.numel() == D, "bad norm_bwd shapes");
  // per-block partial column sums (two-stage reduction instead of contended atomics)
  const int64_t pe = mp_norm_bwd_part_elems(rows, D);
  torch::Tensor part;
  if (pe > 0) part = torch::empty({pe}, dy.options().dtype(torch::kFloat32));
  const auto run = [&](float* csr, float* css) {
    return mp_norm_bwd(f32, rms, dy.data_ptr(), s.data_ptr(), w.data_ptr(),
                       mean.has_value() ? mean->data_ptr<float>() : nullptr, rstd.data_ptr<float>(),
                       ptr_or_null(dres), ds.data_ptr(), mptr_or_null(dbranch), dw.data_ptr<float>(),
                       dbias.has_value() ? dbias->data_ptr<float>() : nullptr, csr, css, rows, D, (float)p,
                       (uint64_t)seed, part.defined() ? part.data_ptr<float>() : nullptr, cur_stream());
  };
  const int rc = run(cs_res.has_value() ? cs_res->data_ptr<float>() : nullptr,
                     cs_ds.has_value() ? cs_ds->data_ptr<float>() : nullptr);
  if (rc == -3) {
    // the launcher refused before launching anything: the backward itself still has to run,
    // without the fused sums (the caller adds them in separate passes)
    check(run(nullptr, nullptr), "norm_bwd");
    return -3;
  }
  check(rc, "norm_bwd");
  return 0;
}

void xent(torch::Tensor logits, torch::Tensor target, torch::Tensor loss, int64_t V, double grad_scale,
          int64_t ignore_index, bool write_grad) {
  const int f32 = storage(logits, "logits");
  req(logits, logits.scalar_type(), "logits");
  req(target, torch::kInt64, "target");
  req(loss, torch::kFloat32, "loss");
  const int Vp = logits.size(-1);
  const int T = logits.numel() / Vp;
  TORCH_CHECK(target.numel() == T && loss.numel() == T, "bad xent shapes");
  check(mp_xent_fwd_bwd(logits.data_ptr(), target.data_ptr<int64_t>(), loss.data_ptr<float>(), T, V, Vp,
                        (float)grad_scale, ignore_index, write_grad, f32, cur_stream()),
        "xent");
}

void embed_fwd(torch::Tensor idx, torch::Tensor wte, c10::optional<torch::Tensor> wpe, torch::Tensor out, int64_t S,
               int64_t pos_offset) {
  req(idx, torch::kInt64, "idx");
  const int f32 = storage(out, "out");
  req(out, out.scalar_type(), "out");
  req(wte, out.scalar_type(), "wte");
  if (wpe.has_value()) req(*wpe, out.scalar_type(), "wpe");
  const int D = wte.size(1);
  const int T = idx.numel();
  TORCH_CHECK(wte.dim() == 2 && out.numel() == (int64_t)T * D, "bad embed shapes");
  if (wpe.has_value()) req_pos_table(*wpe, D, T, S, pos_offset, "wpe");
  check(mp_embed_fwd(idx.data_ptr<int64_t>(), wte.data_ptr(), ptr_or_null(wpe), out.data_ptr(), T, S, D, pos_offset,
                     f32, cur_stream()),
        "embed_fwd");
}

void embed_bwd(torch::Tensor idx, torch::Tensor dout, torch::Tensor dwte, c10::optional<torch::Tensor> dwpe,
               int64_t S, int64_t pos_offset) {
  req(idx, torch::kInt64, "idx");
  req(dwte, torch::kFloat32, "dwte");
  const int f32 = storage(dout, "dout");
  req(dout, dout.scalar_type(), "dout");
  const int D = dwte.size(-1);
  const int T = idx.numel();
  TORCH_CHECK(dout.numel() == (int64_t)T * D, "bad embed_bwd shapes");
  if (dwpe.has_value()) {
    req(*dwpe, torch::kFloat32, "dwpe");
    req_pos_table(*dwpe, D, T, S, pos_offset, "dwpe");
  }
  check(mp_embed_bwd(idx.data_ptr<int64_t>(), dout.data_ptr(), dwte.data_ptr<float>(),
                     dwpe.has_value() ? dwpe->data_ptr<float>() : nullptr, T, S, D, pos_offset, f32, cur_stream()),
        "embed_bwd");
}

}  // namespace

void register_norm_loss_embed(py::module& m) {
  m.def("norm_fwd", &norm_fwd);
  m.def("norm_bwd", &norm_bwd);
  m.def("xent", &xent);
  m.def("embed_fwd", &embed_fwd);
  m.def("embed_bwd", &embed_bwd);
}

}  // namespace mipipe_bind
