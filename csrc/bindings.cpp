// Python bindings of the mipipe HIP kernels (torch tensors in, launches on the current
// HIP stream).  Kernels live in csrc/kernels/*.hip behind plain C launchers so only
// this file pays for the torch headers.  No hipify: written against HIP directly.
#include <climits>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <optional>
#include <string>

#include "mp_attn_plan.h"
#include "mp_gemm_plan.h"
#include "mp_gemv_plan.h"

extern "C" {
int mp_norm_fwd(int f32, int rms, const void* a, const void* b, const void* w, const void* bias, void* s_out, void* y,
                float* mean, float* rstd, int rows, int D, float eps, float p, uint64_t seed, hipStream_t st);
int mp_norm_bwd(int f32, int rms, const void* dy, const void* s, const void* w, const float* mean, const float* rstd,
                const void* dres, void* ds, void* dbranch, float* dw, float* dbias, float* cs_res, float* cs_ds,
                int rows, int D, float p, uint64_t seed, float* part, hipStream_t st);
int64_t mp_norm_bwd_part_elems(int rows, int D);
int64_t mp_colsum_part_elems(int rows, int cols);
int mp_xent_fwd_bwd(void* logits, const int64_t* target, float* loss, int T, int V, int Vp, float grad_scale,
                    int64_t ignore_index, int write_grad, int f32, hipStream_t st);
int mp_embed_fwd(const int64_t* idx, const void* wte, const void* wpe, void* out, int T, int S, int D, int pos_offset,
                 int f32, hipStream_t st);
int mp_embed_bwd(const int64_t* idx, const void* dout, float* dwte, float* dwpe, int T, int S, int D, int pos_offset,
                 int f32, hipStream_t st);
int mp_sumsq(const float* g, int64_t n, float* out, hipStream_t st);
int mp_scaled_sum(const float* x, int64_t n, float scale, float* out, hipStream_t st);
int mp_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int64_t lda,
                int a_kc, int64_t ldb, int b_nc, int64_t ldc, float alpha, int accumulate, hipStream_t st);
int mp_gemm_f32_ex(const float* A, const float* B, float* C, const float* bias, const float* R, float* X, int M, int N,
                   int K, int64_t lda, int a_kc, int64_t ldb, int b_kc, int64_t ldc, int64_t ldr, int64_t ldx, int epi,
                   float alpha, int accumulate, float p_drop, uint64_t seed, int force_split, float* ws,
                   hipStream_t st);
int64_t mp_gemm_f32_ws_elems(int M, int N, int K, int force_split);
int mp_gemm_f32_plan(int M, int N, int K, int force_split, int* split, int* sk_grid, int* sk_chunk);
int mp_lane_merge(float* g0, float* g1, float* g2, float* g3, int64_t n, float* sumsq, hipStream_t st);
int mp_adamw(float* p, float* g, float* m, float* v, void* w16, int64_t n, int64_t n_decay, float lr, float b1,
             float b2, float eps, float wd, int step, const float* sumsq, float max_norm, float grad_scale,
             int zero_grad, hipStream_t st);
int mp_cast_f32_bf16(const float* src, void* dst, int64_t n, hipStream_t st);
int mp_act_fwd(const void* a, void* g, int64_t n, int act, float p, uint64_t seed, hipStream_t st);
int mp_act_bwd(const void* dg, const void* a, void* da, float* dbias, int rows, int cols, int act, float p,
               uint64_t seed, float* part, hipStream_t st);
int mp_colsum(const void* x, float* dbias, int rows, int cols, float* part, int f32, hipStream_t st);
int mp_swiglu_fwd(const void* gu, void* y, int T, int F, hipStream_t st);
int mp_swiglu_bwd(const void* gu, const void* dy, void* dgu, int T, int F, hipStream_t st);
int mp_rope(void* qkv, const float* cs, const float* sn, int T, int S, int H, int Hkv, int Dh, int pos_offset,
            int inverse, hipStream_t st);
int mp_embed_pos(const int64_t* idx, const int* pos, const void* wte, const void* wpe, void* out, int B, int D,
                 int n_tok, int n_pos, int f32, hipStream_t st);
int mp_rope_kv_append(void* qkv, const float* cs, const float* sn, void* kc, void* vc, const int* pos,
                      const uint8_t* active, const int* counts, int B, int T, int H, int Hkv, int Dh, int Smax,
                      int64_t qkv_ld, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, int rope, hipStream_t st);
int mp_sample(const void* logits, int64_t ld, const float* u, uint8_t* done, int64_t* out, int B, int V, int Vp,
              float temperature, int top_k, float top_p, int stop_token, int pad_token, int f32, hipStream_t st);
int mp_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int Sq, int Sk, int H,
                int Hkv, int D, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int causal,
                float scale, float p_drop, uint64_t seed, hipStream_t st);
int mp_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                float* delta, void* dq, void* dk, void* dv, int B, int Sq, int Sk, int H, int Hkv, int D,
                int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int64_t dq_stride,
                int64_t dk_stride, int64_t dv_stride, int causal, float scale, float p_drop, uint64_t seed,
                float* csq, float* csk, float* csv, hipStream_t st);
int mp_attn_doc_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int* doc_start, int B,
                    int S, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, float scale,
                    hipStream_t st);
int mp_attn_doc_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    float* delta, void* dq, void* dk, void* dv, const int* doc_start, const int* doc_end, int B, int S,
                    int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dqs, int64_t dks,
                    int64_t dvs, float scale, hipStream_t st);
int mp_doc_bounds(const int64_t* tokens, int64_t eos, int* doc_start, int* doc_end, int B, int S, hipStream_t st);
int mp_attn_decode(const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B, int H,
                   int Hkv, int D, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs,
                   int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st);
int mp_attn_decode_plan(int B, int Hkv, int max_len);
int64_t mp_attn_decode_ws_floats(int B, int H, int D, int splits);
int mp_attn_append(const void* q, const void* k, const void* v, const int* base, const int* counts, void* o, float* ws,
                   int B, int T, int H, int Hkv, int D, int Smax, int max_len, int64_t q_stride, int64_t k_bs,
                   int64_t k_ts, int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st);
int mp_attn_append_plan(int B, int T, int Hkv, int rep, int max_len);
int64_t mp_attn_append_ws_floats(int B, int T, int H, int D, int splits);
int mp_attn_f32_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Sq, int Sk, int H,
                    int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int causal, float scale,
                    float p_drop, uint64_t seed, hipStream_t st);
int mp_attn_f32_bwd(const float* q, const float* k, const float* v, const float* o, const float* dout,
                    const float* lse, float* delta, float* dq, float* dk, float* dv, int B, int Sq, int Sk, int H,
                    int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dqs, int64_t dks,
                    int64_t dvs, int causal, float scale, float p_drop, uint64_t seed, hipStream_t st);
int mp_set_drop_step_attn_f32(uint64_t v, hipStream_t st);
int mp_set_drop_step_gemm_f32(uint64_t v, hipStream_t st);
int mp_gemm_f32_set_lanes(int lanes);
int mp_transpose(const void* in, void* out, int R, int C, int64_t ldi, int64_t ldo, hipStream_t st);
int mp_transpose_batched(const void* src, void* dst, const int64_t* desc, const int* tile0, int n, int total_tiles,
                         hipStream_t st);
int mp_set_drop_step_attn(uint64_t v, hipStream_t st);
int mp_set_drop_step_elem(uint64_t v, hipStream_t st);
int mp_set_drop_step_norm(uint64_t v, hipStream_t st);
int mp_set_drop_step_gemm(uint64_t v, hipStream_t st);
int mp_gemm2(const void* A, const void* B, void* C, const void* bias, const void* residual, void* aux, int M, int N,
             int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ld_res, int64_t ld_aux, int transA, int transB,
             int epilogue, int c_f32_accum, float alpha, int cfg, int split, int force_cfg, float* ws, float* colsum,
             float p_drop, uint64_t seed, hipStream_t st);
int64_t mp_gemm2_ws_floats(int cfg, int split, int M, int N, int K);
int mp_gemm2_has_probe_engines();
int mp_gemm_tt_grouped(int n, const void* const* A, const void* const* B, float* const* C, const int* M, const int* N,
                       const int* K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc, float alpha,
                       hipStream_t st);
int mp_gemm3_tt_grouped_plan(int n, const int* M, const int* N, int K, int force_split, int64_t* ws_floats);
int mp_gemm3_tt_grouped(int n, const void* const* A, const void* const* B, float* const* C, const int* M, const int* N,
                        int K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc, float alpha, int S, float* ws,
                        hipStream_t st);
int mp_probe_spin(unsigned* flag, unsigned expect, int64_t timeout_us, unsigned* result, hipStream_t waiter);
int mp_probe_set(unsigned* flag, unsigned value, hipStream_t setter);
int mp_probe_clock_khz();
int mp_gemm(const void* A, const void* B, void* C, const void* bias, const void* residual, void* aux, int M, int N,
            int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ld_res, int64_t ld_aux, int transA, int transB,
            int epilogue, int c_f32_accum, float alpha, hipStream_t st);
int mp_gemv_skinny(const void* w, const float* scale, int wbytes, const void* x, void* y, const void* bias,
                   const void* res, int M, int N, int K, int64_t ldx, int64_t ldy, int64_t ldr, int gelu,
                   int force_split, hipStream_t st);
int mp_dequant_w8(const void* q, const float* scale, void* out, int64_t N, int64_t K, hipStream_t st);
}

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check(int rc, const char* what) { TORCH_CHECK(rc == 0, "mipipe kernel ", what, " failed with code ", rc); }

const void* ptr_or_null(const c10::optional<torch::Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }

// storage dtype of the normalisation / loss / embedding kernels: bf16, or f32 (the
// reference-precision path); returns 1 for f32
int storage(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32, name,
              " must be bf16 or f32, got ", t.scalar_type());
  return t.scalar_type() == torch::kFloat32 ? 1 : 0;
}
void* mptr_or_null(const c10::optional<torch::Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }

void req(const torch::Tensor& t, torch::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == dt, name, " has wrong dtype ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// req + the element count the launcher will index
void reqn(const torch::Tensor& t, torch::ScalarType dt, int64_t n, const char* name) {
  req(t, dt, name);
  TORCH_CHECK(t.numel() == n, name, " has ", t.numel(), " elements, expected ", n);
}

// a [rows, width] position table (wpe / dwpe, RoPE cos / sin): token t reads row
// t % S + pos_offset, so rows 0 .. min(T, S) + pos_offset - 1 must exist
void req_pos_table(const torch::Tensor& t, int64_t width, int64_t T, int64_t S, int64_t pos_offset,
                   const char* name) {
  TORCH_CHECK(S >= 1 && pos_offset >= 0, name, ": S must be >= 1 and pos_offset >= 0");
  const int64_t need = std::min(T, S) + pos_offset;
  TORCH_CHECK(t.dim() == 2 && t.size(1) == width && t.size(0) >= need, name, " must be [>= ", need, ", ", width,
              "] (min(T, S) + pos_offset rows), got ", t.sizes());
}

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

// Argument checks of attn_fwd / attn_bwd, all before any launch: the kernels index raw
// pointers by (B, S, heads, D) and the row strides, so a tensor of another dtype or a smaller
// one would be read or written past its end.
static void attn_check_dims(int64_t B, int64_t Sq, int64_t Sk, int64_t H, int64_t Hkv, int64_t D) {
  TORCH_CHECK(B > 0 && Sq > 0 && Sk > 0 && H > 0 && Hkv > 0, "attn: B, Sq, Sk, H, Hkv must be positive (got ", B, ", ",
              Sq, ", ", Sk, ", ", H, ", ", Hkv, ")");
  TORCH_CHECK(H % Hkv == 0, "attn: H = ", H, " is not a multiple of Hkv = ", Hkv);
  TORCH_CHECK(D > 0 && D % 8 == 0, "attn: head_dim ", D, " is not a positive multiple of 8");
  TORCH_CHECK(B * std::max(Sq, Sk) <= INT32_MAX && std::max(H, Hkv) * D <= INT32_MAX, "attn: problem too large");
}

// a token-major [>= rows, >= cols] view of dtype `dt` with a unit inner stride
static void attn_check_rows(const torch::Tensor& t, torch::ScalarType dt, int64_t rows, int64_t cols,
                            const char* name) {
  TORCH_CHECK(t.is_cuda(), "attn: ", name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, "attn: ", name, " has dtype ", t.scalar_type(), ", q has ", dt,
              " (q, k, v, o, dout, dq, dk, dv share one dtype)");
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, "attn: ", name, " must be a 2-D token-major view with unit inner stride");
  TORCH_CHECK(t.size(0) >= rows && t.size(1) >= cols, "attn: ", name, " is [", t.size(0), ", ", t.size(1),
              "], needs at least [", rows, ", ", cols, "]");
  TORCH_CHECK(rows == 1 || t.stride(0) >= cols, "attn: ", name, " rows overlap (row stride ", t.stride(0), " < ", cols, ")");
}

// a contiguous f32 vector of at least n elements (lse, delta)
static void attn_check_vec(const torch::Tensor& t, int64_t n, const char* name) {
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
static void attn_doc_check_common(const torch::Tensor& q, int64_t B, int64_t S, int64_t H, int64_t Hkv, int64_t D,
                                  bool causal, double p) {
  attn_check_dims(B, S, S, H, Hkv, D);
  TORCH_CHECK(causal, "attn_doc: the document mask is causal only");
  TORCH_CHECK(p == 0.0, "attn_doc: no dropout (p_drop = ", p, ")");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attn_doc: bf16 tensors only (q has ", q.scalar_type(), ")");
  TORCH_CHECK(D == 64 || D == 128, "attn_doc: head_dim ", D, " is not supported (64 or 128)");
}

// 16-byte rows (the kernels move 8 bf16 at a time) whose offsets inside one sequence fit 32 bits
static void attn_doc_check_rows(const torch::Tensor& t, int64_t B, int64_t S, int64_t cols, const char* name) {
  attn_check_rows(t, torch::kBFloat16, B * S, cols, name);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && (B * S == 1 || t.stride(0) % 8 == 0),
              "attn_doc: ", name, " rows must be 16-byte aligned (row stride ", t.stride(0), ")");
  TORCH_CHECK((S + 128) * t.stride(0) * 2 < (int64_t(1) << 31), "attn_doc: ", name, " row stride ", t.stride(0),
              " is too large for S = ", S);
}

static void attn_doc_check_bounds(const torch::Tensor& t, const torch::Tensor& q, int64_t n, const char* name) {
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

// Decode attention (attention_decode.hip): one query row per sequence against its KV cache.
// q/o: [B, H*D] row views; k_cache/v_cache: [B, Smax, Hkv*D] views with unit inner stride;
// lens: int32 [B] on the device (valid keys per sequence); max_len >= max(lens) sizes the
// grid; splits: 0 = planner, n > 0 forces n.  Returns the split count used.
int64_t attn_decode(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor lens,
                    torch::Tensor o, int64_t H, int64_t Hkv, int64_t D, int64_t max_len, double scale,
                    int64_t splits) {
  req(lens, torch::kInt32, "lens");
  for (const torch::Tensor* t : {&q, &k_cache, &v_cache, &o})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16, "attn_decode: q/k_cache/v_cache/o must be bf16 GPU tensors");
  TORCH_CHECK(q.dim() == 2 && o.dim() == 2 && q.stride(1) == 1 && o.stride(1) == 1, "attn_decode: q/o are [B, H*D] rows");
  TORCH_CHECK(k_cache.dim() == 3 && v_cache.dim() == 3 && k_cache.stride(2) == 1 && v_cache.stride(2) == 1,
              "attn_decode: caches are [B, Smax, Hkv*D] with a unit inner stride");
  const int64_t B = q.size(0), Smax = k_cache.size(1);
  TORCH_CHECK(D == 64 || D == 128, "attn_decode: head_dim ", D, " is not supported (64 or 128)");
  TORCH_CHECK(Hkv >= 1 && H >= 1 && H % Hkv == 0 && H / Hkv <= 8,
              "attn_decode: H = ", H, ", Hkv = ", Hkv, " is not supported (H % Hkv == 0, H / Hkv <= 8)");
  TORCH_CHECK(q.size(1) == H * D && o.size(0) == B && o.size(1) == H * D, "attn_decode: q/o shape");
  TORCH_CHECK(k_cache.size(0) == B && v_cache.size(0) == B && v_cache.size(1) == Smax &&
                  k_cache.size(2) == Hkv * D && v_cache.size(2) == Hkv * D, "attn_decode: cache shape");
  TORCH_CHECK(lens.numel() == B, "attn_decode: lens must hold one length per sequence");
  TORCH_CHECK(max_len >= 1 && max_len <= Smax, "attn_decode: max_len ", max_len, " outside [1, ", Smax, "]");
  TORCH_CHECK(splits >= 0 && splits <= max_len && splits <= 256, "attn_decode: splits ", splits,
              " outside [0, min(max_len, 256)]");
  TORCH_CHECK(B >= 1 && B <= 65535 && Hkv <= 65535, "attn_decode: batch / KV heads exceed the grid");
  const auto aligned = [](const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; };
  TORCH_CHECK(aligned(q) && aligned(k_cache) && aligned(v_cache) && q.stride(0) % 8 == 0 &&
                  k_cache.stride(0) % 8 == 0 && k_cache.stride(1) % 8 == 0 && v_cache.stride(0) % 8 == 0 &&
                  v_cache.stride(1) % 8 == 0,
              "attn_decode: q / cache rows must be 16-byte aligned");
  const int ns = splits > 0 ? (int)splits : mp_attn_decode_plan((int)B, (int)Hkv, (int)max_len);
  // per-split partial outputs + (max, sum): from the caching allocator on the current stream
  torch::Tensor ws = torch::empty({mp_attn_decode_ws_floats((int)B, (int)H, (int)D, ns)},
                                  q.options().dtype(torch::kFloat32));
  check(mp_attn_decode(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), lens.data_ptr<int>(), o.data_ptr(),
                       ws.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)D, (int)Smax, (int)max_len, q.stride(0),
                       k_cache.stride(0), k_cache.stride(1), v_cache.stride(0), v_cache.stride(1), o.stride(0),
                       (float)scale, ns, cur_stream()),
        "attn_decode");
  return ns;
}

// Append attention (attention_append.hip): T new tokens per sequence, already in the cache at
// rows base[b] + t, each attending causally over the cache.  q/o: [B*T, H*D] row views;
// base: int32 [B] on the device (valid rows before the call); counts: int32 [B] (optional,
// real tokens per sequence); max_len >= max(base + counts) sizes the grid.  Returns the split
// count used.
int64_t attn_append(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor base,
                    c10::optional<torch::Tensor> counts, torch::Tensor o, int64_t T, int64_t H, int64_t Hkv, int64_t D,
                    int64_t max_len, double scale, int64_t splits) {
  req(base, torch::kInt32, "base");
  if (counts.has_value()) req(*counts, torch::kInt32, "counts");
  for (const torch::Tensor* t : {&q, &k_cache, &v_cache, &o})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16, "attn_append: q/k_cache/v_cache/o must be bf16 GPU tensors");
  TORCH_CHECK(q.dim() == 2 && o.dim() == 2 && q.stride(1) == 1 && o.stride(1) == 1, "attn_append: q/o are [B*T, H*D] rows");
  TORCH_CHECK(k_cache.dim() == 3 && v_cache.dim() == 3 && k_cache.stride(2) == 1 && v_cache.stride(2) == 1,
              "attn_append: caches are [B, Smax, Hkv*D] with a unit inner stride");
  const int64_t B = k_cache.size(0), Smax = k_cache.size(1);
  TORCH_CHECK(D == 64 || D == 128, "attn_append: head_dim ", D, " is not supported (64 or 128)");
  TORCH_CHECK(Hkv >= 1 && H >= 1 && H % Hkv == 0 && H / Hkv <= 8,
              "attn_append: H = ", H, ", Hkv = ", Hkv, " is not supported (H % Hkv == 0, H / Hkv <= 8)");
  TORCH_CHECK(T >= 1 && B >= 1 && B * T <= INT_MAX && q.size(0) == B * T && o.size(0) == B * T,
              "attn_append: q/o must hold B * T = ", B * T, " rows");
  TORCH_CHECK(q.size(1) == H * D && o.size(1) == H * D, "attn_append: q/o shape");
  TORCH_CHECK(v_cache.size(0) == B && v_cache.size(1) == Smax && k_cache.size(2) == Hkv * D &&
                  v_cache.size(2) == Hkv * D, "attn_append: cache shape");
  TORCH_CHECK(base.is_contiguous() && base.numel() == B, "attn_append: base must hold one length per sequence");
  for (const torch::Tensor* t : {&k_cache, &v_cache, &o, &base})
    TORCH_CHECK(t->get_device() == q.get_device(), "attn_append: every tensor must be on q's GPU");
  TORCH_CHECK(!counts.has_value() || counts->get_device() == q.get_device(), "attn_append: counts must be on q's GPU");
  TORCH_CHECK(!counts.has_value() || (counts->is_contiguous() && counts->numel() == B),
              "attn_append: counts must hold one count per sequence");
  TORCH_CHECK(max_len >= 1 && max_len <= Smax, "attn_append: max_len ", max_len, " outside [1, ", Smax, "]");
  TORCH_CHECK(splits >= 0 && splits <= max_len && splits <= 256, "attn_append: splits ", splits,
              " outside [0, min(max_len, 256)]");
  const int64_t rep = H / Hkv;
  TORCH_CHECK(B * ((T * rep + 31) / 32) <= 65535 && Hkv <= 65535 && H <= 65535,
              "attn_append: batch x query tiles / heads exceed the grid");
  const auto aligned = [](const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; };
  TORCH_CHECK(aligned(q) && aligned(k_cache) && aligned(v_cache) && q.stride(0) % 8 == 0 &&
                  k_cache.stride(0) % 8 == 0 && k_cache.stride(1) % 8 == 0 && v_cache.stride(0) % 8 == 0 &&
                  v_cache.stride(1) % 8 == 0,
              "attn_append: q / cache rows must be 16-byte aligned");
  const int ns = splits > 0 ? (int)splits : mp_attn_append_plan((int)B, (int)T, (int)Hkv, (int)rep, (int)max_len);
  torch::Tensor ws = torch::empty({mp_attn_append_ws_floats((int)B, (int)T, (int)H, (int)D, ns)},
                                  q.options().dtype(torch::kFloat32));
  check(mp_attn_append(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), base.data_ptr<int>(),
                       counts.has_value() ? counts->data_ptr<int>() : nullptr, o.data_ptr(), ws.data_ptr<float>(),
                       (int)B, (int)T, (int)H, (int)Hkv, (int)D, (int)Smax, (int)max_len, q.stride(0),
                       k_cache.stride(0), k_cache.stride(1), v_cache.stride(0), v_cache.stride(1), o.stride(0),
                       (float)scale, ns, cur_stream()),
        "attn_append");
  return ns;
}

// ---- the ragged decode step (generate.hip): every position is read from device memory
// a contiguous [B] vector of dtype dt on `ref`'s GPU (pos, active, u, done, out)
void gen_vec(const char* fn, const char* name, const torch::Tensor& t, torch::ScalarType dt, int64_t B,
             const torch::Tensor& ref) {
  TORCH_CHECK(t.is_cuda() && t.get_device() == ref.get_device(), fn, ": ", name, " must be on the GPU of ",
              "the other arguments");
  TORCH_CHECK(t.scalar_type() == dt, fn, ": ", name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous() && t.numel() == B, fn, ": ", name, " must be contiguous with one element per ",
              "sequence (", B, "), got ", t.numel());
}

bool gen_aligned(const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

// out[b, :] = wte[idx[b], :] (+ wpe[pos[b], :]); pos: int32 [B] on the device
void embed_pos(torch::Tensor idx, torch::Tensor pos, torch::Tensor wte, c10::optional<torch::Tensor> wpe,
               torch::Tensor out) {
  const int f32 = storage(out, "out");
  const auto dt = out.scalar_type();
  req(out, dt, "out");
  req(wte, dt, "wte");
  TORCH_CHECK(wte.dim() == 2 && wte.size(0) >= 1 && wte.size(0) <= INT_MAX && wte.size(1) % 8 == 0,
              "embed_pos: wte must be [vocab, D] with D a multiple of 8");
  const int64_t D = wte.size(1), B = idx.numel();
  TORCH_CHECK(B >= 1 && B <= INT_MAX && out.numel() == B * D, "embed_pos: out must be [B, D]");
  TORCH_CHECK(wte.get_device() == out.get_device(), "embed_pos: wte is on another device than out");
  gen_vec("embed_pos", "idx", idx, torch::kInt64, B, out);
  gen_vec("embed_pos", "positions", pos, torch::kInt32, B, out);
  int64_t n_pos = 0;
  if (wpe.has_value()) {
    req(*wpe, dt, "wpe");
    TORCH_CHECK(wpe->dim() == 2 && wpe->size(1) == D && wpe->size(0) >= 1 && wpe->size(0) <= INT_MAX &&
                    wpe->get_device() == out.get_device(), "embed_pos: wpe must be [positions, D] on out's device");
    n_pos = wpe->size(0);
  }
  check(mp_embed_pos(idx.data_ptr<int64_t>(), pos.data_ptr<int>(), wte.data_ptr(), ptr_or_null(wpe), out.data_ptr(),
                     (int)B, (int)D, (int)wte.size(0), (int)n_pos, f32, cur_stream()),
        "embed_pos");
}

// qkv: [B * T, (H + 2 Hkv) Dh] rows (T tokens per sequence, row b * T + t at position
// pos[b] + t); caches: [B, Smax, Hkv * Dh] views; pos: int32 [B]; active: uint8 [B]
// (optional); counts: int32 [B] (optional: only rows t < counts[b] are touched).  The RoPE
// tables must cover every position the clamp can produce: Smax rows.
void rope_kv_append(torch::Tensor qkv, c10::optional<torch::Tensor> cs, c10::optional<torch::Tensor> sn,
                    torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor pos,
                    c10::optional<torch::Tensor> active, int64_t H, int64_t Hkv, int64_t Dh, bool rope, int64_t T,
                    c10::optional<torch::Tensor> counts) {
  const char* fn = "rope_kv_append";
  TORCH_CHECK(Dh == 64 || Dh == 128, fn, ": head_dim ", Dh, " is not supported (64 or 128)");
  TORCH_CHECK(H >= 1 && Hkv >= 1 && H <= 65535 && Hkv <= 65535, fn, ": bad head counts");
  for (const torch::Tensor* t : {&qkv, &k_cache, &v_cache}) {
    TORCH_CHECK(t->is_cuda() && t->get_device() == qkv.get_device(), fn, ": qkv / k_cache / v_cache must be on one GPU");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16, fn, ": qkv / k_cache / v_cache must be bf16, got ",
                t->scalar_type());
  }
  const int64_t width = (H + 2 * Hkv) * Dh;
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == width && qkv.stride(1) == 1, fn, ": qkv must be [B, (H + 2 Hkv) Dh] rows");
  TORCH_CHECK(T >= 1 && qkv.size(0) >= T && qkv.size(0) % T == 0 && qkv.size(0) <= INT_MAX, fn, ": qkv must hold B * T rows");
  const int64_t B = qkv.size(0) / T, rows = qkv.size(0);
  TORCH_CHECK(B >= 1 && B <= 65535, fn, ": batch outside [1, 65535]");
  TORCH_CHECK(k_cache.dim() == 3 && v_cache.dim() == 3 && k_cache.stride(2) == 1 && v_cache.stride(2) == 1,
              fn, ": caches are [B, Smax, Hkv*Dh] with a unit inner stride");
  const int64_t Smax = k_cache.size(1);
  TORCH_CHECK(k_cache.size(0) == B && v_cache.size(0) == B && v_cache.size(1) == Smax && Smax >= 1 &&
                  Smax <= INT_MAX && k_cache.size(2) == Hkv * Dh && v_cache.size(2) == Hkv * Dh, fn, ": cache shape");
  TORCH_CHECK(gen_aligned(qkv) && gen_aligned(k_cache) && gen_aligned(v_cache) && (rows == 1 || qkv.stride(0) % 8 == 0) &&
                  k_cache.stride(0) % 8 == 0 && k_cache.stride(1) % 8 == 0 && v_cache.stride(0) % 8 == 0 &&
                  v_cache.stride(1) % 8 == 0, fn, ": qkv / cache rows must be 16-byte aligned");
  TORCH_CHECK(rows == 1 || qkv.stride(0) >= width, fn, ": qkv rows overlap");
  TORCH_CHECK(k_cache.stride(1) >= Hkv * Dh && v_cache.stride(1) >= Hkv * Dh &&
                  (B == 1 || (k_cache.stride(0) >= Smax * k_cache.stride(1) && v_cache.stride(0) >= Smax * v_cache.stride(1))),
              fn, ": cache rows overlap");
  gen_vec(fn, "pos", pos, torch::kInt32, B, qkv);
  if (active.has_value()) gen_vec(fn, "active", *active, torch::kUInt8, B, qkv);
  if (counts.has_value()) gen_vec(fn, "counts", *counts, torch::kInt32, B, qkv);
  const float* cp = nullptr;
  const float* sp = nullptr;
  if (rope) {
    TORCH_CHECK(cs.has_value() && sn.has_value(), fn, ": rope needs the cos / sin tables");
    for (const torch::Tensor* t : {&*cs, &*sn}) {
      req(*t, torch::kFloat32, "cos / sin");
      TORCH_CHECK(t->get_device() == qkv.get_device(), fn, ": cos / sin are on another device than qkv");
      TORCH_CHECK(t->dim() == 2 && t->size(1) == Dh / 2 && t->size(0) >= Smax, fn, ": cos / sin must be [>= Smax = ",
                  Smax, ", ", Dh / 2, "], got ", t->sizes());
    }
    cp = cs->data_ptr<float>();
    sp = sn->data_ptr<float>();
  }
  check(mp_rope_kv_append(qkv.data_ptr(), cp, sp, k_cache.data_ptr(), v_cache.data_ptr(), pos.data_ptr<int>(),
                          active.has_value() ? active->data_ptr<uint8_t>() : nullptr,
                          counts.has_value() ? counts->data_ptr<int>() : nullptr, (int)B, (int)T, (int)H, (int)Hkv,
                          (int)Dh, (int)Smax, qkv.stride(0), k_cache.stride(0), k_cache.stride(1), v_cache.stride(0),
                          v_cache.stride(1), rope ? 1 : 0, cur_stream()),
        fn);
}

// logits: [B, Vp] rows (bf16 or f32, any 16-byte aligned row stride >= Vp); u: f32 [B];
// done: uint8 [B] (optional, read and written); out: int64 [B]
void sample(torch::Tensor logits, int64_t V, torch::Tensor u, double temperature, int64_t top_k, double top_p,
            c10::optional<torch::Tensor> done, int64_t stop_token, int64_t pad_token, torch::Tensor out) {
  const char* fn = "sample";
  TORCH_CHECK(logits.is_cuda(), fn, ": logits must be on the GPU");
  const int f32 = storage(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.size(0) >= 1 && logits.size(1) >= 1,
              fn, ": logits must be [B, Vp] rows with a unit inner stride");
  const int64_t B = logits.size(0), Vp = logits.size(1), per = f32 ? 4 : 8;
  TORCH_CHECK(B <= INT_MAX && Vp <= INT_MAX && Vp % 8 == 0, fn, ": Vp = ", Vp, " must be a multiple of 8");
  TORCH_CHECK(V >= 1 && V <= Vp, fn, ": vocab ", V, " outside [1, Vp = ", Vp, "]");
  const int64_t ld = B == 1 ? std::max<int64_t>(Vp, logits.stride(0) - logits.stride(0) % per) : logits.stride(0);
  TORCH_CHECK(gen_aligned(logits) && ld % per == 0 && ld >= Vp, fn, ": logits rows must be 16-byte aligned and disjoint");
  TORCH_CHECK(temperature >= 0.0, fn, ": temperature ", temperature, " must be >= 0");
  TORCH_CHECK(top_k >= 0 && top_k <= INT_MAX, fn, ": top_k ", top_k, " must be >= 0");
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, fn, ": top_p ", top_p, " outside (0, 1]");
  TORCH_CHECK(stop_token >= -1 && stop_token <= INT_MAX && pad_token >= 0 && pad_token <= INT_MAX,
              fn, ": stop_token / pad_token out of range");
  gen_vec(fn, "u", u, torch::kFloat32, B, logits);
  gen_vec(fn, "out", out, torch::kInt64, B, logits);
  if (done.has_value()) gen_vec(fn, "done", *done, torch::kUInt8, B, logits);
  check(mp_sample(logits.data_ptr(), ld, u.data_ptr<float>(), done.has_value() ? done->data_ptr<uint8_t>() : nullptr,
                  out.data_ptr<int64_t>(), (int)B, (int)V, (int)Vp, (float)temperature, (int)top_k, (float)top_p,
                  (int)stop_token, (int)pad_token, f32, cur_stream()),
        fn);
}

// ---- host-side argument checks of the GEMM bindings: every tensor a kernel will touch is
// looked at before any launch, and the message names the argument
bool aligned16(const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

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
using PlanEnvDict = std::map<std::string, std::string>;
// y[M, N] = epi(x[M, K] @ What^T), M <= 16 (csrc/kernels/gemv_skinny.hip): w int8 [N, K] with scale f32 [N],
// or w bf16 [N, K] without.  No allocation, no synchronisation.
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
  const bool w8 = w.scalar_type() == torch::kInt8;
  TORCH_CHECK(w8 || w.scalar_type() == torch::kBFloat16, "gemv_skinny: w must be int8 or bf16, got ", w.scalar_type());
  TORCH_CHECK(w8 == scale.has_value(), "gemv_skinny: int8 weights take a scale, bf16 weights none");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= gemv::MAX_M, "gemv_skinny: M = ", M, " outside [1, ", gemv::MAX_M, "]");
  TORCH_CHECK(w.size(1) == K && y.size(0) == M && y.size(1) == N, "gemv_skinny: shapes x ", x.sizes(), " w ", w.sizes(), " y ", y.sizes());
  TORCH_CHECK(gemv::plan(N, K, w8 ? 1 : 2, (int)force_split).rows != 0, "gemv_skinny: N = ", N, ", K = ", K,
              ", force_split = ", force_split, " is not supported (K a multiple of 32, force_split <= 16)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0, "gemv_skinny: w must be 16-byte aligned");
  if (w8) {
    req(*scale, torch::kFloat32, "gemv_skinny: scale");
    TORCH_CHECK(scale->numel() == N && scale->is_contiguous(), "gemv_skinny: scale must hold N contiguous values");
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
  check(mp_gemv_skinny(w.data_ptr(), w8 ? scale->data_ptr<float>() : nullptr, w8 ? 1 : 2, x.data_ptr(), y.data_ptr(),
                       ptr_or_null(bias), ptr_or_null(residual), (int)M, (int)N, (int)K, x.stride(0), y.stride(0), ldr,
                       gelu ? 1 : 0, (int)force_split, cur_stream()),
        "gemv_skinny");
}

void dequant_w8(torch::Tensor q, torch::Tensor scale, torch::Tensor out) {
  req(q, torch::kInt8, "dequant_w8: q");
  req(scale, torch::kFloat32, "dequant_w8: scale");
  req(out, torch::kBFloat16, "dequant_w8: out");
  TORCH_CHECK(q.dim() == 2 && q.is_contiguous() && out.is_contiguous() && out.numel() == q.numel() &&
                  scale.is_contiguous() && scale.numel() == q.size(0),
              "dequant_w8: q [N, K], scale [N], out [N, K], all contiguous");
  TORCH_CHECK(q.size(1) % 16 == 0, "dequant_w8: K = ", q.size(1), " must be a multiple of 16");
  check(mp_dequant_w8(q.data_ptr(), scale.data_ptr<float>(), out.data_ptr(), q.size(0), q.size(1), cur_stream()),
        "dequant_w8");
}

g2::Plan gemm2_plan(int64_t M, int64_t N, int64_t K, bool transA, bool transB, bool accum, int64_t force_cfg,
                    const std::optional<PlanEnvDict>& env) {
  g2::PlanEnv parsed;
  if (env.has_value()) {
    for (const auto& kv : *env)
      TORCH_CHECK(g2::PlanEnv::known(kv.first.c_str()), "gemm2_plan: ", kv.first, " is not a planner switch");
    parsed = g2::PlanEnv::parse([&](const char* name) {
      const auto it = env->find(name);
      return it == env->end() ? (const char*)nullptr : it->second.c_str();
    });
  }
  return g2::plan_gemm((int)M, (int)N, (int)K, transA, transB, accum, (int)force_cfg,
                       env.has_value() ? parsed : g2::PlanEnv::process(), mp_gemm2_has_probe_engines() != 0);
}

// What attn_fwd / attn_bwd will launch for a bf16 problem (mp_attn_plan.h): {"fwd": launch,
// "bwd": [launch, ...]}, a launch being {"kernel", "dp", "grid", "lds"}.  env: the
// MIPIPE_ATTN_* switches by name over their defaults; none: the process environment.
pybind11::dict attn_plan(int64_t B, int64_t Sq, int64_t Sk, int64_t H, int64_t Hkv, int64_t D, int64_t qs, int64_t ks,
                         int64_t vs, int64_t os, bool causal, bool drop, const std::optional<PlanEnvDict>& env) {
  TORCH_CHECK(B > 0 && Sq > 0 && Sk > 0 && H > 0 && Hkv > 0 && D > 0, "attn_plan: sizes must be positive");
  attn::AttnEnv parsed;
  if (env.has_value()) {
    for (const auto& kv : *env)
      TORCH_CHECK(attn::AttnEnv::known(kv.first.c_str()), "attn_plan: ", kv.first, " is not an attention switch");
    parsed = attn::AttnEnv::parse([&](const char* name) {
      const auto it = env->find(name);
      return it == env->end() ? (const char*)nullptr : it->second.c_str();
    });
  }
  const attn::AttnEnv& e = env.has_value() ? parsed : attn::AttnEnv::process();
  const attn::Launch f = attn::plan_attn_fwd((int)B, (int)Sq, (int)Sk, (int)H, (int)Hkv, (int)D, ks, vs, causal, drop, e);
  const attn::BwdPlan b =
      attn::plan_attn_bwd((int)B, (int)Sq, (int)Sk, (int)H, (int)Hkv, (int)D, qs, ks, vs, os, causal, drop, e);
  TORCH_CHECK(f.kernel != attn::K_NONE && b.n > 0, "attn_plan: no kernel for D = ", D, ", H = ", H, ", Hkv = ", Hkv,
              " (D a multiple of 8 up to 256, H a multiple of Hkv)");
  const auto launch = [](const attn::Launch& l) {
    pybind11::dict d;
    d["kernel"] = attn::kernel_name(l.kernel);
    d["dp"] = l.dp;
    d["grid"] = pybind11::make_tuple(l.gx, l.gy);
    d["lds"] = l.lds;
    return d;
  };
  pybind11::list bwd;
  for (int i = 0; i < b.n; ++i) bwd.append(launch(b.l[i]));
  pybind11::dict out;
  out["fwd"] = launch(f);
  out["bwd"] = bwd;
  return out;
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

// grouped weight-gradient GEMMs: C[i] (f32 [N_i, K_i]) += alpha * dy[i]^T x[i]
// (dy [T_i, N_i], x [T_i, K_i] bf16, unit inner stride) in one launch of 64x64 tiles
void gemm_tt_grouped(std::vector<torch::Tensor> dy, std::vector<torch::Tensor> x, std::vector<torch::Tensor> C,
                     double alpha) {
  const int n = (int)dy.size();
  TORCH_CHECK(n == (int)x.size() && n == (int)C.size() && n >= 1 && n <= 8, "gemm_tt_grouped: 1..8 problems");
  const void* A[8];
  const void* B[8];
  float* Cp[8];
  int M[8], N[8], K[8];
  int64_t lda[8], ldb[8], ldc[8];
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(dy[0].is_cuda(), "gemm_tt_grouped: dy must be on the GPU");
    gemm_operand("gemm_tt_grouped", "dy", dy[i], torch::kBFloat16, dy[0]);
    gemm_operand("gemm_tt_grouped", "x", x[i], torch::kBFloat16, dy[0]);
    gemm_operand("gemm_tt_grouped", "C", C[i], torch::kFloat32, dy[0]);
    TORCH_CHECK(dy[i].size(0) == x[i].size(0) && C[i].size(0) == dy[i].size(1) && C[i].size(1) == x[i].size(1),
                "gemm_tt_grouped: shape mismatch");
    A[i] = dy[i].data_ptr();
    B[i] = x[i].data_ptr();
    Cp[i] = C[i].data_ptr<float>();
    M[i] = (int)dy[i].size(1);
    N[i] = (int)x[i].size(1);
    K[i] = (int)dy[i].size(0);
    lda[i] = dy[i].stride(0);
    ldb[i] = x[i].stride(0);
    ldc[i] = C[i].stride(0);
  }
  check(mp_gemm_tt_grouped(n, A, B, Cp, M, N, K, lda, ldb, ldc, (float)alpha, cur_stream()), "gemm_tt_grouped");
}

// grouped long-token weight-gradient GEMMs: C[i] (f32 [N_i, K_i]) += alpha * dy[i]^T x[i]
// (dy [T, N_i], x [T, K_i] bf16, unit inner stride, ONE token count T for the group) in one
// launch of 256x256 tiles at a common split-K factor (split = 0: the planner's; > 0: forced,
// clamped to T / 64) plus one reduce launch when that factor is > 1.  Returns the factor used.
int64_t gemm_dw_grouped(std::vector<torch::Tensor> dy, std::vector<torch::Tensor> x, std::vector<torch::Tensor> C,
                        double alpha, int64_t split) {
  const char* fn = "gemm_dw_grouped";
  const int n = (int)dy.size();
  TORCH_CHECK(n == (int)x.size() && n == (int)C.size() && n >= 1 && n <= 8, fn, ": 1..8 problems");
  TORCH_CHECK(split >= 0 && split <= INT_MAX, fn, ": split ", split, " must be >= 0");
  const void* A[8];
  const void* B[8];
  float* Cp[8];
  int M[8], N[8];
  int64_t lda[8], ldb[8], ldc[8];
  TORCH_CHECK(dy[0].is_cuda(), fn, ": dy must be on the GPU");
  const int64_t T = dy[0].dim() == 2 ? dy[0].size(0) : 0;
  for (int i = 0; i < n; ++i) {
    gemm_operand(fn, "dy", dy[i], torch::kBFloat16, dy[0]);
    gemm_operand(fn, "x", x[i], torch::kBFloat16, dy[0]);
    gemm_operand(fn, "C", C[i], torch::kFloat32, dy[0]);
    TORCH_CHECK(dy[i].size(0) == T && x[i].size(0) == T, fn, ": every dy and x needs the same token count T = ", T,
                ", problem ", i, " has ", dy[i].size(0), " and ", x[i].size(0));
    TORCH_CHECK(C[i].size(0) == dy[i].size(1) && C[i].size(1) == x[i].size(1), fn, ": C[", i, "] must be [",
                dy[i].size(1), ", ", x[i].size(1), "]");
    TORCH_CHECK(dy[i].size(1) % 8 == 0 && x[i].size(1) % 8 == 0, fn, ": problem ", i, ": M = ", dy[i].size(1),
                " and N = ", x[i].size(1), " must be multiples of 8");
    TORCH_CHECK(dy[i].size(1) <= INT_MAX && x[i].size(1) <= INT_MAX, fn, ": M, N must fit 32 bits");
    A[i] = dy[i].data_ptr();
    B[i] = x[i].data_ptr();
    Cp[i] = C[i].data_ptr<float>();
    M[i] = (int)dy[i].size(1);
    N[i] = (int)x[i].size(1);
    lda[i] = dy[i].stride(0);
    ldb[i] = x[i].stride(0);
    ldc[i] = C[i].stride(0);
  }
  TORCH_CHECK(T % 64 == 0 && T <= INT_MAX, fn, ": T = ", T, " must be a multiple of 64");
  // split-K slabs from the caching allocator on the current stream (graph captures take
  // them from their private pool), as gemm2() does
  int64_t ws_n = 0;
  const int S = mp_gemm3_tt_grouped_plan(n, M, N, (int)T, (int)split, &ws_n);
  torch::Tensor ws;
  if (ws_n > 0) ws = torch::empty({ws_n}, C[0].options().dtype(torch::kFloat32));
  check(mp_gemm3_tt_grouped(n, A, B, Cp, M, N, (int)T, lda, ldb, ldc, (float)alpha, S,
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

// A private HIP stream (not from torch's round-robin pool, whose streams other users --
// graph capture, process groups -- may also be handed).  Never destroyed: it lives as
// long as the process, like the streams it is used beside.  priority: 0 = default,
// -1 = the device's highest.
int64_t create_stream(int64_t device, int64_t priority) {
  int cur = 0;
  TORCH_CHECK(hipGetDevice(&cur) == hipSuccess, "hipGetDevice");
  TORCH_CHECK(hipSetDevice((int)device) == hipSuccess, "hipSetDevice");
  int lo = 0, hi = 0;
  TORCH_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess, "priority range");
  hipStream_t s = nullptr;
  const hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority < 0 ? hi : lo);
  hipSetDevice(cur);
  TORCH_CHECK(e == hipSuccess, "hipStreamCreateWithPriority: ", hipGetErrorString(e));
  return reinterpret_cast<int64_t>(s);
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

// hardware-queue probe (csrc/kernels/probe.hip, parallel/queues.py): enqueue the bounded
// spinner on stream `waiter` / the flag store on stream `setter` (raw HIP stream handles;
// 0 = the current stream).  flag: int32 [1], result: int32 [2] device tensors.
void probe_spin(torch::Tensor flag, int64_t expect, int64_t timeout_us, torch::Tensor result, int64_t waiter) {
  req(flag, torch::kInt32, "flag");
  req(result, torch::kInt32, "result");
  TORCH_CHECK(result.numel() >= 2 && timeout_us > 0 && timeout_us <= 2000000, "probe_spin: result[2], timeout <= 2 s");
  hipStream_t s = waiter ? reinterpret_cast<hipStream_t>(waiter) : cur_stream();
  check(mp_probe_spin(reinterpret_cast<unsigned*>(flag.data_ptr()), (unsigned)expect, timeout_us,
                      reinterpret_cast<unsigned*>(result.data_ptr()), s),
        "probe_spin");
}

void probe_set(torch::Tensor flag, int64_t value, int64_t setter) {
  req(flag, torch::kInt32, "flag");
  hipStream_t s = setter ? reinterpret_cast<hipStream_t>(setter) : cur_stream();
  check(mp_probe_set(reinterpret_cast<unsigned*>(flag.data_ptr()), (unsigned)value, s), "probe_set");
}

}  // namespace

namespace mipipe_comm {
void register_rccl(pybind11::module& m);
}
namespace mipipe_runtime {
void register_runner(pybind11::module& m);
}

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

// f32 MFMA GEMM: C (+)= alpha * A @ B (+ bias); A [M,K], B [K,N] 2-D views with either inner
// stride 1; returns 1 if done, 0 if the layout is not supported (caller falls back)
int64_t gemm_f32(torch::Tensor A, torch::Tensor B, torch::Tensor C, c10::optional<torch::Tensor> bias, double alpha,
                 bool accumulate) {
  gemm_f32_args("gemm_f32", A, B, C, bias);
  const int M = A.size(0), K = A.size(1), N = B.size(1);
  TORCH_CHECK(B.size(0) == K && C.size(0) == M && C.size(1) == N, "gemm_f32: shape mismatch");
  if (C.stride(1) != 1) return 0;
  int a_kc, b_nc;
  int64_t lda, ldb;
  if (A.stride(1) == 1) { a_kc = 1; lda = A.stride(0); }
  else if (A.stride(0) == 1) { a_kc = 0; lda = A.stride(1); }
  else return 0;
  if (B.stride(1) == 1) { b_nc = 1; ldb = B.stride(0); }
  else if (B.stride(0) == 1) { b_nc = 0; ldb = B.stride(1); }
  else return 0;
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
  if (C.stride(1) != 1) return 0;
  int a_kc, b_kc;
  int64_t lda, ldb;
  if (A.stride(1) == 1) { a_kc = 1; lda = A.stride(0); }
  else if (A.stride(0) == 1) { a_kc = 0; lda = A.stride(1); }
  else return 0;
  if (B.stride(0) == 1) { b_kc = 1; ldb = B.stride(1); }
  else if (B.stride(1) == 1) { b_kc = 0; ldb = B.stride(0); }
  else return 0;
  const bool need_bias = epi == 1 || epi == 2 || epi == 4, need_r = epi >= 3, need_x = epi == 2;
  TORCH_CHECK(!need_bias || (bias.has_value() && bias->is_contiguous() && bias->numel() == N), "gemm_f32_ex: bias [N]");
  int64_t ldr = 0, ldx = 0;
  if (need_r) {
    TORCH_CHECK(R.has_value() && R->is_cuda() && R->get_device() == A.get_device() &&
                    R->scalar_type() == torch::kFloat32 && R->dim() == 2 && R->stride(1) == 1 &&
                    R->size(0) == M && R->size(1) == N, "gemm_f32_ex: R must be [M,N] f32 rows on A's GPU");
    ldr = R->stride(0);
  }
  if (need_x) {
    TORCH_CHECK(X.has_value() && X->is_cuda() && X->get_device() == A.get_device() &&
                    X->scalar_type() == torch::kFloat32 && X->dim() == 2 && X->stride(1) == 1 &&
                    X->size(0) == M && X->size(1) == N, "gemm_f32_ex: X must be [M,N] f32 rows on A's GPU");
    ldx = X->stride(0);
  }
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

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  mipipe_comm::register_rccl(m);
  mipipe_runtime::register_runner(m);
  m.doc() = "mipipe gfx950 HIP kernels";
  m.def("norm_fwd", &norm_fwd);
  m.def("norm_bwd", &norm_bwd);
  m.def("xent", &xent);
  m.def("embed_fwd", &embed_fwd);
  m.def("embed_bwd", &embed_bwd);
  m.def("sumsq", &sumsq);
  m.def("scaled_sum", &scaled_sum);
  m.def("zero_", &zero_);
  m.def("gemm_f32", &gemm_f32);
  m.def("gemm_f32_set_lanes", &mp_gemm_f32_set_lanes);
  m.def("gemm_f32_ex", &gemm_f32_ex, pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("C"), pybind11::arg("bias"),
        pybind11::arg("R"), pybind11::arg("X"), pybind11::arg("epi") = 0, pybind11::arg("alpha") = 1.0,
        pybind11::arg("accumulate") = false, pybind11::arg("p_drop") = 0.0, pybind11::arg("seed") = 0,
        pybind11::arg("force_ks") = 0);
  m.def("adamw", &adamw);
  m.def("cast_f32_bf16", &cast_f32_bf16);
  m.def("act_fwd", &act_fwd);
  m.def("act_bwd", &act_bwd);
  m.def("colsum", &colsum);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope", &rope);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_doc_fwd", &attn_doc_fwd);
  m.def("attn_doc_bwd", &attn_doc_bwd);
  m.def("doc_bounds", &doc_bounds);
  m.def("attn_decode", &attn_decode, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("lens"), pybind11::arg("o"), pybind11::arg("H"), pybind11::arg("Hkv"), pybind11::arg("D"),
        pybind11::arg("max_len"), pybind11::arg("scale"), pybind11::arg("splits") = 0);
  m.def("attn_decode_plan", [](int64_t B, int64_t Hkv, int64_t max_len) {
    return mp_attn_decode_plan((int)B, (int)Hkv, (int)max_len);
  }, "key splits the decode attention picks for B sequences x Hkv KV heads over max_len keys");
  m.def("embed_pos", &embed_pos);
  m.def("attn_append", &attn_append, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("base"), pybind11::arg("counts"), pybind11::arg("o"), pybind11::arg("T"), pybind11::arg("H"),
        pybind11::arg("Hkv"), pybind11::arg("D"), pybind11::arg("max_len"), pybind11::arg("scale"),
        pybind11::arg("splits") = 0);
  m.def("attn_append_plan", [](int64_t B, int64_t T, int64_t Hkv, int64_t rep, int64_t max_len) {
    return mp_attn_append_plan((int)B, (int)T, (int)Hkv, (int)rep, (int)max_len);
  }, "key splits the append attention picks for B sequences x T tokens x Hkv KV heads of rep query heads over max_len keys");
  m.def("rope_kv_append", &rope_kv_append, pybind11::arg("qkv"), pybind11::arg("cos"), pybind11::arg("sin"),
        pybind11::arg("k_cache"), pybind11::arg("v_cache"), pybind11::arg("pos"), pybind11::arg("active"),
        pybind11::arg("H"), pybind11::arg("Hkv"), pybind11::arg("Dh"), pybind11::arg("rope"), pybind11::arg("T") = 1,
        pybind11::arg("counts") = pybind11::none());
  m.def("sample", &sample);
  m.def("gemm", &gemm);
  m.def("lane_merge", &lane_merge, pybind11::arg("g0"), pybind11::arg("lanes"), pybind11::arg("sumsq") = pybind11::none());
  m.def("gemm_tt_grouped", &gemm_tt_grouped, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("C"),
        pybind11::arg("alpha") = 1.0);
  m.def("gemm_dw_grouped", &gemm_dw_grouped, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("C"),
        pybind11::arg("alpha") = 1.0, pybind11::arg("split") = 0);
  m.def("gemm2", &gemm2, pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("C"), pybind11::arg("bias"),
        pybind11::arg("residual"), pybind11::arg("aux"), pybind11::arg("transA"), pybind11::arg("transB"),
        pybind11::arg("epilogue"), pybind11::arg("accum"), pybind11::arg("alpha"), pybind11::arg("force_cfg"),
        pybind11::arg("colsum"), pybind11::arg("p_drop") = 0.0, pybind11::arg("seed") = 0);
  m.def("transpose", &transpose);
  m.def("set_dropout_step", &set_dropout_step);
  m.def("create_stream", &create_stream, pybind11::arg("device"), pybind11::arg("priority") = 0);
  m.def("transpose_batched", &transpose_batched);
  m.def("probe_spin", &probe_spin, pybind11::arg("flag"), pybind11::arg("expect"), pybind11::arg("timeout_us"),
        pybind11::arg("result"), pybind11::arg("waiter") = 0);
  m.def("probe_set", &probe_set, pybind11::arg("flag"), pybind11::arg("value"), pybind11::arg("setter") = 0);
  m.def("probe_clock_khz", []() { return mp_probe_clock_khz(); });
  m.def("gemm2_plan", [](int64_t M, int64_t N, int64_t K, bool transA, bool transB, bool accum, int64_t force_cfg,
                         std::optional<PlanEnvDict> env) {
    const g2::Plan p = gemm2_plan(M, N, K, transA, transB, accum, force_cfg, env);
    return std::make_tuple(p.cfg, p.split);
  }, pybind11::arg("M"), pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("transA"), pybind11::arg("transB"),
     pybind11::arg("accum"), pybind11::arg("force_cfg"), pybind11::arg("env") = pybind11::none(),
     "engine config + split-K factor the v2 GEMM picks (14: stream-K gemm7); env: the MIPIPE_* planner "
     "switches as a dict over their defaults instead of the process environment");
  m.def("attn_plan", &attn_plan, pybind11::arg("B"), pybind11::arg("Sq"), pybind11::arg("Sk"), pybind11::arg("H"),
        pybind11::arg("Hkv"), pybind11::arg("D"), pybind11::arg("qs"), pybind11::arg("ks"), pybind11::arg("vs"),
        pybind11::arg("os"), pybind11::arg("causal"), pybind11::arg("drop"), pybind11::arg("env") = pybind11::none(),
        "kernels, grids and LDS bytes the bf16 attention launches; env: the MIPIPE_ATTN_* switches as a dict over "
        "their defaults instead of the process environment");
  m.def("gemm_f32_plan", [](int64_t M, int64_t N, int64_t K, int64_t force_ks) {
    int split = 1, sk_grid = 0, sk_chunk = 0;
    const int big = mp_gemm_f32_plan((int)M, (int)N, (int)K, (int)force_ks, &split, &sk_grid, &sk_chunk);
    return std::make_tuple(big != 0, split, sk_grid, sk_chunk);
  }, "what gemm_f32_ex will run: (128x128 engine, split-K factor, stream-K workgroups, K-tile pairs per workgroup)");
  m.def("gemv_skinny", &gemv_skinny, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("scale"), pybind11::arg("y"),
        pybind11::arg("bias"), pybind11::arg("residual"), pybind11::arg("gelu") = false, pybind11::arg("force_split") = 0);
  m.def("dequant_w8", &dequant_w8);
  m.def("gemv_plan", [](int64_t N, int64_t K, int64_t wbytes, int64_t force_split) {
    const gemv::Plan p = gemv::plan(N, K, (int)wbytes, (int)force_split);
    TORCH_CHECK(p.rows != 0, "gemv_plan: N = ", N, ", K = ", K, ", wbytes = ", wbytes, ", force_split = ", force_split,
                " is not supported");
    return std::make_tuple(p.rows, p.ksplit);
  }, pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("wbytes"), pybind11::arg("force_split") = 0,
     "(weight rows per workgroup, K-splits = waves per workgroup) of the skinny-M kernel");
  m.def("gemm2_has_probe_engines", []() { return mp_gemm2_has_probe_engines() != 0; });
}
