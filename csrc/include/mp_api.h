// The C ABI between the kernel objects (csrc/kernels/*.hip) and the Python bindings
// (csrc/bindings/*.cpp), declared once.  Every .hip includes this header, so a definition whose
// parameter list drifts from it is a compile error (conflicting types for a C-linkage function)
// instead of garbage on the GPU.  Declarations only: nothing a device compile turns into code.
// Launchers return 0 or a HIP error code; other return values are noted per function.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

extern "C" {
// ---- norm.hip.  f32 != 0: every tensor but mean / rstd in f32, else bf16.  mp_norm_bwd
// returns -3, before launching anything, when the fused column sums are not available.
int mp_norm_fwd(int f32, int rms, const void* a, const void* b, const void* w, const void* bias, void* s_out, void* y,
                float* mean, float* rstd, int rows, int D, float eps, float p, uint64_t seed, hipStream_t st);
int mp_norm_bwd(int f32, int rms, const void* dy, const void* s, const void* w, const float* mean, const float* rstd,
                const void* dres, void* ds, void* dbranch, float* dw, float* dbias, float* cs_res, float* cs_ds,
                int rows, int D, float p, uint64_t seed, float* part, hipStream_t st);
int64_t mp_norm_bwd_part_elems(int rows, int D);  // f32 elements of `part` (0: atomics only)
int mp_set_drop_step_norm(uint64_t v, hipStream_t st);
// ---- xent.hip
int mp_xent_fwd_bwd(void* logits, const int64_t* target, float* loss, int T, int V, int Vp, float grad_scale,
                    int64_t ignore_index, int write_grad, int f32, hipStream_t st);
// ---- embedding.hip
int mp_embed_fwd(const int64_t* idx, const void* wte, const void* wpe, void* out, int T, int S, int D, int pos_offset,
                 int f32, hipStream_t st);
int mp_embed_bwd(const int64_t* idx, const void* dout, float* dwte, float* dwpe, int T, int S, int D, int pos_offset,
                 int f32, hipStream_t st);
// ---- optim.hip
int mp_sumsq(const float* g, int64_t n, float* out, hipStream_t st);
int mp_scaled_sum(const float* x, int64_t n, float scale, float* out, hipStream_t st);
int mp_lane_merge(float* g0, float* g1, float* g2, float* g3, int64_t n, float* sumsq, hipStream_t st);
int mp_adamw(float* p, float* g, float* m, float* v, void* w16, int64_t n, int64_t n_decay, float lr, float b1,
             float b2, float eps, float wd, int step, const float* sumsq, float max_norm, float grad_scale,
             int zero_grad, hipStream_t st);
int mp_cast_f32_bf16(const float* src, void* dst, int64_t n, hipStream_t st);
// ---- elementwise.hip
int mp_act_fwd(const void* a, void* g, int64_t n, int act, float p, uint64_t seed, hipStream_t st);
int mp_act_bwd(const void* dg, const void* a, void* da, float* dbias, int rows, int cols, int act, float p,
               uint64_t seed, float* part, hipStream_t st);
int mp_colsum(const void* x, float* dbias, int rows, int cols, float* part, int f32, hipStream_t st);
int64_t mp_colsum_part_elems(int rows, int cols);  // f32 elements of `part` (0: atomics only)
int mp_swiglu_fwd(const void* gu, void* y, int T, int F, hipStream_t st);
int mp_swiglu_bwd(const void* gu, const void* dy, void* dgu, int T, int F, hipStream_t st);
int mp_rope(void* qkv, const float* cs, const float* sn, int T, int S, int H, int Hkv, int Dh, int pos_offset,
            int inverse, hipStream_t st);
int mp_transpose(const void* in, void* out, int R, int C, int64_t ldi, int64_t ldo, hipStream_t st);
int mp_transpose_batched(const void* src, void* dst, const int64_t* desc, const int* tile0, int n, int total_tiles,
                         hipStream_t st);
int mp_set_drop_step_elem(uint64_t v, hipStream_t st);
// ---- gemm.hip
int mp_gemm(const void* A, const void* B, void* C, const void* bias, const void* residual, void* aux, int M, int N,
            int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ld_res, int64_t ld_aux, int transA, int transB,
            int epilogue, int c_f32_accum, float alpha, hipStream_t st);
// ---- gemm2.hip.  mp_gemm2 returns -1 / -2 when v2 does not provide the combination and -3,
// before launching anything, when it cannot add the requested column sums.
int mp_gemm2(const void* A, const void* B, void* C, const void* bias, const void* residual, void* aux, int M, int N,
             int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ld_res, int64_t ld_aux, int transA, int transB,
             int epilogue, int c_f32_accum, float alpha, int cfg, int split, int force_cfg, float* ws, float* colsum,
             float p_drop, uint64_t seed, hipStream_t st);
int64_t mp_gemm2_ws_floats(int cfg, int split, int M, int N, int K);
int mp_gemm2_has_probe_engines();
int mp_gemm_tt_grouped(int n, const void* const* A, const void* const* B, float* const* C, const int* M, const int* N,
                       const int* K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc, float alpha,
                       hipStream_t st);
// returns the common split-K factor; *ws_floats: the slabs mp_gemm3_tt_grouped then needs
int mp_gemm3_tt_grouped_plan(int n, const int* M, const int* N, int K, int force_split, int64_t* ws_floats);
int mp_gemm3_tt_grouped(int n, const void* const* A, const void* const* B, float* const* C, const int* M, const int* N,
                        int K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc, float alpha, int S, float* ws,
                        hipStream_t st);
int mp_set_drop_step_gemm(uint64_t v, hipStream_t st);
// ---- gemv_skinny.hip
int mp_gemv_skinny(const void* w, const float* scale, int wbytes, const void* x, void* y, const void* bias,
                   const void* res, int M, int N, int K, int64_t ldx, int64_t ldy, int64_t ldr, int gelu,
                   int force_split, hipStream_t st);
int mp_dequant_w8(const void* q, const float* scale, void* out, int64_t N, int64_t K, hipStream_t st);
int mp_dequant_w4(const void* q, const float* scale, void* out, int64_t N, int64_t K, hipStream_t st);
// ---- gemm_f32.hip.  a_kc / b_kc / b_nc: which stride of the operand is 1 (K- or N-contiguous);
// both GEMMs return -1 for a layout they do not provide.
int mp_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int64_t lda,
                int a_kc, int64_t ldb, int b_nc, int64_t ldc, float alpha, int accumulate, hipStream_t st);
int mp_gemm_f32_ex(const float* A, const float* B, float* C, const float* bias, const float* R, float* X, int M, int N,
                   int K, int64_t lda, int a_kc, int64_t ldb, int b_kc, int64_t ldc, int64_t ldr, int64_t ldx, int epi,
                   float alpha, int accumulate, float p_drop, uint64_t seed, int force_split, float* ws,
                   hipStream_t st);
int64_t mp_gemm_f32_ws_elems(int M, int N, int K, int force_split);
int mp_gemm_f32_plan(int M, int N, int K, int force_split, int* split, int* sk_grid, int* sk_chunk);
int mp_gemm_f32_set_lanes(int lanes);  // returns the CUs the split-K planner now plans for
int mp_set_drop_step_gemm_f32(uint64_t v, hipStream_t st);
// ---- attention.hip
int mp_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int Sq, int Sk, int H,
                int Hkv, int D, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int causal,
                float scale, float p_drop, uint64_t seed, hipStream_t st);
int mp_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                float* delta, void* dq, void* dk, void* dv, int B, int Sq, int Sk, int H, int Hkv, int D,
                int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int64_t dq_stride,
                int64_t dk_stride, int64_t dv_stride, int causal, float scale, float p_drop, uint64_t seed,
                float* csq, float* csk, float* csv, hipStream_t st);
int mp_set_drop_step_attn(uint64_t v, hipStream_t st);
// ---- attention_f32.hip
int mp_attn_f32_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Sq, int Sk, int H,
                    int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int causal, float scale,
                    float p_drop, uint64_t seed, hipStream_t st);
int mp_attn_f32_bwd(const float* q, const float* k, const float* v, const float* o, const float* dout,
                    const float* lse, float* delta, float* dq, float* dk, float* dv, int B, int Sq, int Sk, int H,
                    int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dqs, int64_t dks,
                    int64_t dvs, int causal, float scale, float p_drop, uint64_t seed, hipStream_t st);
int mp_set_drop_step_attn_f32(uint64_t v, hipStream_t st);
// ---- attention_doc.hip
int mp_attn_doc_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int* doc_start, int B,
                    int S, int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, float scale,
                    hipStream_t st);
int mp_attn_doc_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                    float* delta, void* dq, void* dk, void* dv, const int* doc_start, const int* doc_end, int B, int S,
                    int H, int Hkv, int D, int64_t qs, int64_t ks, int64_t vs, int64_t os, int64_t dqs, int64_t dks,
                    int64_t dvs, float scale, hipStream_t st);
int mp_doc_bounds(const int64_t* tokens, int64_t eos, int* doc_start, int* doc_end, int B, int S, hipStream_t st);
// ---- attention_decode.hip.  *_plan: key splits the planner picks; *_ws_floats: the f32
// workspace (per-split partial outputs + max / sum) of that many splits.
int mp_attn_decode(const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B, int H,
                   int Hkv, int D, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts, int64_t v_bs,
                   int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st);
int mp_attn_decode_plan(int B, int Hkv, int max_len);
int64_t mp_attn_decode_ws_floats(int B, int H, int D, int splits);
// ---- attention_append.hip
int mp_attn_append(const void* q, const void* k, const void* v, const int* base, const int* counts, void* o, float* ws,
                   int B, int T, int H, int Hkv, int D, int Smax, int max_len, int64_t q_stride, int64_t k_bs,
                   int64_t k_ts, int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st);
int mp_attn_append_plan(int B, int T, int Hkv, int rep, int max_len);
int64_t mp_attn_append_ws_floats(int B, int T, int H, int D, int splits);
// ---- attention_kv8.hip.  The int8 KV cache: a row of Hkv heads of dim D is
// round_up(Hkv * D + 4 * Hkv, 16) bytes (int8 payload, Hkv f32 scales, zero padding).  The
// arguments of the three launchers above that they stand in for, with the caches' batch / token
// strides in bytes; planners and workspaces are those of the bf16 kernels.
int mp_attn_decode_kv8(const void* q, const void* k, const void* v, const int* lens, void* o, float* ws, int B, int H,
                       int Hkv, int D, int Smax, int max_len, int64_t q_stride, int64_t k_bs, int64_t k_ts,
                       int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale, int splits, hipStream_t st);
int mp_attn_append_kv8(const void* q, const void* k, const void* v, const int* base, const int* counts, void* o,
                       float* ws, int B, int T, int H, int Hkv, int D, int Smax, int max_len, int64_t q_stride,
                       int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, int64_t o_stride, float scale,
                       int splits, hipStream_t st);
int mp_rope_kv_append_kv8(void* qkv, const float* cs, const float* sn, void* kc, void* vc, const int* pos,
                          const uint8_t* active, const int* counts, int B, int T, int H, int Hkv, int Dh, int Smax,
                          int64_t qkv_ld, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, int rope,
                          hipStream_t st);
// ---- generate.hip
int mp_embed_pos(const int64_t* idx, const int* pos, const void* wte, const void* wpe, void* out, int B, int D,
                 int n_tok, int n_pos, int f32, hipStream_t st);
int mp_rope_kv_append(void* qkv, const float* cs, const float* sn, void* kc, void* vc, const int* pos,
                      const uint8_t* active, const int* counts, int B, int T, int H, int Hkv, int Dh, int Smax,
                      int64_t qkv_ld, int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, int rope, hipStream_t st);
int mp_sample(const void* logits, int64_t ld, const float* u, uint8_t* done, int64_t* out, int B, int V, int Vp,
              float temperature, int top_k, float top_p, int stop_token, int pad_token, int f32, hipStream_t st);
// ---- probe.hip.  flag / result: device buffers of >= 1 / 2 words
int mp_probe_spin(unsigned* flag, unsigned expect, int64_t timeout_us, unsigned* result, hipStream_t waiter);
int mp_probe_set(unsigned* flag, unsigned value, hipStream_t setter);
int mp_probe_clock_khz();
}
