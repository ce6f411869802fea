// Bindings of elementwise.hip and optim.hip: activations, column sums, SwiGLU, RoPE, the
// gradient-lane merge, the optimizer and the dropout step counter.
#include "common.h"

namespace mipipe_bind {
namespace {

// g0 += sum(lanes); lanes zeroed (1..3 extra f32 lane buffers of g0's size); with
// `sumsq` (f32 [1]) also *sumsq += |merged g0|^2 in the same pass
void lane_merge(torch::Tensor g0, std::vector<torch::Tensor> lanes, c10::optional<torch::Tensor> sumsq) {
  TORCH_CHECK(lanes.size() >= 1 && lanes.size() <= 3, "lane_merge: 1..3 lane buffers");
  req(g0, torch::kFloat32, "g0");
  float* p[3] = {nullptr, nullptr, nullptr};
  for (size_t i = 0; i < lanes.size(); ++i) {
    req(lanes[i], torch::kFloat32, "lane");
    TORCH_CHECK(lanes[i].numel() == g0.numel(), "lane_merge: size mismatch");
    p[i] = lanes[i].data_ptr<float>();
  }
  if (sumsq.has_value()) req(*sumsq, torch::kFloat32, "sumsq");
  check(mp_lane_merge(g0.data_ptr<float>(), p[0], p[1], p[2], g0.numel(),
                      sumsq.has_value() ? sumsq->data_ptr<float>() : nullptr, cur_stream()),
        "lane_merge");
}

void sumsq(torch::Tensor g, torch::Tensor out) {
  req(g, torch::kFloat32, "g");
  reqn(out, torch::kFloat32, 1, "out");
  check(mp_sumsq(g.data_ptr<float>(), g.numel(), out.data_ptr<float>(), cur_stream()), "sumsq");
}

// contiguous tensor <- 0 with hipMemsetAsync on the current stream (graph-capturable)
void zero_(torch::Tensor t) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "zero_: contiguous GPU tensor");
  TORCH_CHECK(hipMemsetAsync(t.data_ptr(), 0, t.numel() * t.element_size(), cur_stream()) == hipSuccess, "zero_");
}

// out (f32 scalar) = scale * sum(x): one workgroup, deterministic
void scaled_sum(torch::Tensor x, double scale, torch::Tensor out) {
  req(x, torch::kFloat32, "x");
  req(out, torch::kFloat32, "out");
  check(mp_scaled_sum(x.data_ptr<float>(), x.numel(), (float)scale, out.data_ptr<float>(), cur_stream()),
        "scaled_sum");
}

void adamw(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, c10::optional<torch::Tensor> w16,
           int64_t n_decay, double lr, double b1, double b2, double eps, double wd, int64_t step,
           c10::optional<torch::Tensor> sumsq_buf, double max_norm, double grad_scale, bool zero_grad) {
  req(p, torch::kFloat32, "p");
  req(g, torch::kFloat32, "g");
  reqn(m, torch::kFloat32, p.numel(), "m");
  reqn(v, torch::kFloat32, p.numel(), "v");
  if (w16.has_value()) reqn(*w16, torch::kBFloat16, p.numel(), "w16");
  if (sumsq_buf.has_value()) reqn(*sumsq_buf, torch::kFloat32, 1, "sumsq_buf");
  TORCH_CHECK(g.numel() == p.numel(), "bad adamw shapes");
  check(mp_adamw(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), mptr_or_null(w16),
                 p.numel(), n_decay, (float)lr, (float)b1, (float)b2, (float)eps, (float)wd, (int)step,
                 sumsq_buf.has_value() ? sumsq_buf->data_ptr<float>() : nullptr, (float)max_norm, (float)grad_scale,
                 zero_grad, cur_stream()),
        "adamw");
}

void cast_f32_bf16(torch::Tensor src, torch::Tensor dst) {
  req(src, torch::kFloat32, "src");
  reqn(dst, torch::kBFloat16, src.numel(), "dst");
  check(mp_cast_f32_bf16(src.data_ptr<float>(), dst.data_ptr(), src.numel(), cur_stream()), "cast");
}

void act_fwd(torch::Tensor a, torch::Tensor g, int64_t act, double p, int64_t seed) {
  req(a, torch::kBFloat16, "a");
  reqn(g, torch::kBFloat16, a.numel(), "g");
  check(mp_act_fwd(a.data_ptr(), g.data_ptr(), a.numel(), act, (float)p, (uint64_t)seed, cur_stream()), "act_fwd");
}

void act_bwd(torch::Tensor dg, torch::Tensor a, torch::Tensor da, c10::optional<torch::Tensor> dbias, int64_t act,
             double p, int64_t seed) {
  req(dg, torch::kBFloat16, "dg");
  const int cols = dg.size(-1);
  const int rows = dg.numel() / cols;
  reqn(a, torch::kBFloat16, dg.numel(), "a");
  reqn(da, torch::kBFloat16, dg.numel(), "da");
  if (dbias.has_value()) reqn(*dbias, torch::kFloat32, cols, "dbias");
  const int64_t pe = dbias.has_value() ? mp_colsum_part_elems(rows, cols) : 0;
  torch::Tensor part;
  if (pe > 0) part = torch::empty({pe}, dg.options().dtype(torch::kFloat32));
  check(mp_act_bwd(dg.data_ptr(), a.data_ptr(), da.data_ptr(), dbias.has_value() ? dbias->data_ptr<float>() : nullptr,
                   rows, cols, act, (float)p, (uint64_t)seed, part.defined() ? part.data_ptr<float>() : nullptr,
                   cur_stream()),
        "act_bwd");
}

void colsum(torch::Tensor x, torch::Tensor dbias) {
  const int f32 = storage(x, "x");
  req(x, x.scalar_type(), "x");
  req(dbias, torch::kFloat32, "dbias");
  const int cols = x.size(-1);
  const int rows = x.numel() / cols;
  const int64_t pe = mp_colsum_part_elems(rows, cols);
  torch::Tensor part;
  if (pe > 0) part = torch::empty({pe}, x.options().dtype(torch::kFloat32));
  check(mp_colsum(x.data_ptr(), dbias.data_ptr<float>(), rows, cols, part.defined() ? part.data_ptr<float>() : nullptr,
                  f32, cur_stream()),
        "colsum");
}

void swiglu_fwd(torch::Tensor gu, torch::Tensor y) {
  const int F = y.size(-1);
  req(y, torch::kBFloat16, "y");
  reqn(gu, torch::kBFloat16, 2 * y.numel(), "gu");
  TORCH_CHECK(gu.size(-1) == 2 * F, "swiglu_fwd: gu rows must be gate | up of 2 F columns");
  check(mp_swiglu_fwd(gu.data_ptr(), y.data_ptr(), y.numel() / F, F, cur_stream()), "swiglu_fwd");
}

void swiglu_bwd(torch::Tensor gu, torch::Tensor dy, torch::Tensor dgu) {
  const int F = dy.size(-1);
  req(dy, torch::kBFloat16, "dy");
  reqn(gu, torch::kBFloat16, 2 * dy.numel(), "gu");
  reqn(dgu, torch::kBFloat16, 2 * dy.numel(), "dgu");
  TORCH_CHECK(gu.size(-1) == 2 * F, "swiglu_bwd: gu rows must be gate | up of 2 F columns");
  check(mp_swiglu_bwd(gu.data_ptr(), dy.data_ptr(), dgu.data_ptr(), dy.numel() / F, F, cur_stream()), "swiglu_bwd");
}

void rope(torch::Tensor qkv, torch::Tensor cs, torch::Tensor sn, int64_t S, int64_t H, int64_t Hkv, int64_t Dh,
          int64_t pos_offset, bool inverse) {
  TORCH_CHECK(H >= 1 && Hkv >= 1 && Dh >= 8 && Dh % 8 == 0, "rope: bad head counts / head_dim");
  const int64_t width = (H + 2 * Hkv) * Dh;
  req(qkv, torch::kBFloat16, "qkv");
  TORCH_CHECK(qkv.numel() % width == 0, "rope: qkv must hold whole [(H + 2 Hkv) Dh] rows");
  const int T = qkv.numel() / width;
  req(cs, torch::kFloat32, "cos");
  req(sn, torch::kFloat32, "sin");
  req_pos_table(cs, Dh / 2, T, S, pos_offset, "cos");
  req_pos_table(sn, Dh / 2, T, S, pos_offset, "sin");
  check(mp_rope(qkv.data_ptr(), cs.data_ptr<float>(), sn.data_ptr<float>(), T, S, H, Hkv, Dh, pos_offset, inverse,
                cur_stream()),
        "rope");
}

// training-step counter the dropout kernels mix into their seeds (mp_common.h
// step_seed): stream-ordered, issued before a step's first replay, never captured
void set_dropout_step(int64_t step) {
  const uint64_t v = (uint64_t)step;
  check(mp_set_drop_step_attn(v, cur_stream()), "set_drop_step");
  check(mp_set_drop_step_attn_f32(v, cur_stream()), "set_drop_step");
  check(mp_set_drop_step_gemm_f32(v, cur_stream()), "set_drop_step");
  check(mp_set_drop_step_elem(v, cur_stream()), "set_drop_step");
  check(mp_set_drop_step_norm(v, cur_stream()), "set_drop_step");
  check(mp_set_drop_step_gemm(v, cur_stream()), "set_drop_step");
}

}  // namespace

void register_elementwise_optim(py::module& m) {
  m.def("act_fwd", &act_fwd);
  m.def("act_bwd", &act_bwd);
  m.def("colsum", &colsum);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope", &rope);
  m.def("lane_merge", &lane_merge, py::arg("g0"), py::arg("lanes"), py::arg("sumsq") = py::none());
  m.def("sumsq", &sumsq);
  m.def("scaled_sum", &scaled_sum);
  m.def("zero_", &zero_);
  m.def("adamw", &adamw);
  m.def("cast_f32_bf16", &cast_f32_bf16);
  m.def("set_dropout_step", &set_dropout_step);
}

}  // namespace mipipe_bind
