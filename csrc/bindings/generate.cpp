// Bindings of generation: decode and append attention over a KV cache (attention_decode.hip,
// attention_append.hip) and the ragged decode step (generate.hip), whose positions are all
// read from device memory.
#include "common.h"

namespace mipipe_bind {
namespace {

// bytes of one int8 cache row (attention_kv8.hip): payload, Hkv f32 scales, padding to 16
int64_t kv8_row_bytes(int64_t Hkv, int64_t D) { return (Hkv * D + 4 * Hkv + 15) / 16 * 16; }

// The KV-cache geometry every kernel here indexes: k_cache / v_cache are [B, Smax, Hkv*D] views
// with a unit inner stride and 16-byte aligned base, batch and token strides.  `q_aligned`: the
// same of the caller's query rows (`qname`), a conjunct of the one alignment message; `d`: the
// head dim's name in the caller's messages.  `kv8`: the caches are int8 rows of
// kv8_row_bytes(Hkv, D) bytes (attention_kv8.hip) instead.  Returns Smax.
int64_t kv_cache_args(const char* fn, const char* qname, bool q_aligned, const char* d, const torch::Tensor& k_cache,
                      const torch::Tensor& v_cache, int64_t B, int64_t Hkv, int64_t D, bool kv8 = false) {
  TORCH_CHECK(k_cache.dim() == 3 && v_cache.dim() == 3 && k_cache.stride(2) == 1 && v_cache.stride(2) == 1, fn,
              ": caches are [B, Smax, Hkv*", d, "] with a unit inner stride");
  const int64_t Smax = k_cache.size(1);
  const int64_t width = kv8 ? kv8_row_bytes(Hkv, D) : Hkv * D, per = kv8 ? 16 : 8;     // elements per 16 bytes
  TORCH_CHECK(k_cache.size(0) == B && v_cache.size(0) == B && v_cache.size(1) == Smax && k_cache.size(2) == width &&
                  v_cache.size(2) == width, fn, kv8 ? ": cache shape (int8 rows are round_up(Hkv*D + 4*Hkv, 16) bytes)"
                                                    : ": cache shape");
  TORCH_CHECK(q_aligned && aligned16(k_cache) && aligned16(v_cache) && k_cache.stride(0) % per == 0 &&
                  k_cache.stride(1) % per == 0 && v_cache.stride(0) % per == 0 && v_cache.stride(1) % per == 0,
              fn, ": ", qname, " / cache rows must be 16-byte aligned");
  // the int8 kernels index the rows of one sequence with 32-bit byte offsets
  TORCH_CHECK(!kv8 || (Smax * k_cache.stride(1) <= (int64_t)UINT32_MAX && Smax * v_cache.stride(1) <= (int64_t)UINT32_MAX),
              fn, ": one sequence of an int8 cache must stay below 4 GiB");
  return Smax;
}

// the caches of an attention call: both bf16, or both int8 (the kv8 format); true for int8
bool kv_cache_is_kv8(const char* fn, const torch::Tensor& k_cache, const torch::Tensor& v_cache) {
  for (const torch::Tensor* t : {&k_cache, &v_cache})
    TORCH_CHECK(t->is_cuda() && (t->scalar_type() == torch::kBFloat16 || t->scalar_type() == torch::kChar), fn,
                ": q/k_cache/v_cache/o must be bf16 GPU tensors (or both caches int8)");
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(), fn, ": k_cache and v_cache must share a dtype");
  return k_cache.scalar_type() == torch::kChar;
}

// Decode attention (attention_decode.hip): one query row per sequence against its KV cache.
// q/o: [B, H*D] row views; k_cache/v_cache: [B, Smax, Hkv*D] views with unit inner stride;
// lens: int32 [B] on the device (valid keys per sequence); max_len >= max(lens) sizes the
// grid; splits: 0 = planner, n > 0 forces n.  Returns the split count used.
int64_t attn_decode(torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor lens,
                    torch::Tensor o, int64_t H, int64_t Hkv, int64_t D, int64_t max_len, double scale,
                    int64_t splits) {
  req(lens, torch::kInt32, "lens");
  for (const torch::Tensor* t : {&q, &o})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16, "attn_decode: q/k_cache/v_cache/o must be bf16 GPU tensors");
  const bool kv8 = kv_cache_is_kv8("attn_decode", k_cache, v_cache);
  TORCH_CHECK(q.dim() == 2 && o.dim() == 2 && q.stride(1) == 1 && o.stride(1) == 1, "attn_decode: q/o are [B, H*D] rows");
  TORCH_CHECK(D == 64 || D == 128, "attn_decode: head_dim ", D, " is not supported (64 or 128)");
  TORCH_CHECK(Hkv >= 1 && H >= 1 && H % Hkv == 0 && H / Hkv <= 8,
              "attn_decode: H = ", H, ", Hkv = ", Hkv, " is not supported (H % Hkv == 0, H / Hkv <= 8)");
  const int64_t B = q.size(0);
  TORCH_CHECK(q.size(1) == H * D && o.size(0) == B && o.size(1) == H * D, "attn_decode: q/o shape");
  const int64_t Smax =
      kv_cache_args("attn_decode", "q", aligned16(q) && q.stride(0) % 8 == 0, "D", k_cache, v_cache, B, Hkv, D, kv8);
  TORCH_CHECK(lens.numel() == B, "attn_decode: lens must hold one length per sequence");
  TORCH_CHECK(max_len >= 1 && max_len <= Smax, "attn_decode: max_len ", max_len, " outside [1, ", Smax, "]");
  TORCH_CHECK(splits >= 0 && splits <= max_len && splits <= 256, "attn_decode: splits ", splits,
              " outside [0, min(max_len, 256)]");
  TORCH_CHECK(B >= 1 && B <= 65535 && Hkv <= 65535, "attn_decode: batch / KV heads exceed the grid");
  const int ns = splits > 0 ? (int)splits : mp_attn_decode_plan((int)B, (int)Hkv, (int)max_len);
  // per-split partial outputs + (max, sum): from the caching allocator on the current stream
  torch::Tensor ws = torch::empty({mp_attn_decode_ws_floats((int)B, (int)H, (int)D, ns)},
                                  q.options().dtype(torch::kFloat32));
  // int8 caches: the same arguments (strides of an int8 tensor are bytes) to the kv8 kernel
  check((kv8 ? mp_attn_decode_kv8 : mp_attn_decode)(
            q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), lens.data_ptr<int>(), o.data_ptr(),
            ws.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)D, (int)Smax, (int)max_len, q.stride(0),
            k_cache.stride(0), k_cache.stride(1), v_cache.stride(0), v_cache.stride(1), o.stride(0), (float)scale, ns,
            cur_stream()),
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
  for (const torch::Tensor* t : {&q, &o})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16, "attn_append: q/k_cache/v_cache/o must be bf16 GPU tensors");
  const bool kv8 = kv_cache_is_kv8("attn_append", k_cache, v_cache);
  TORCH_CHECK(q.dim() == 2 && o.dim() == 2 && q.stride(1) == 1 && o.stride(1) == 1, "attn_append: q/o are [B*T, H*D] rows");
  TORCH_CHECK(D == 64 || D == 128, "attn_append: head_dim ", D, " is not supported (64 or 128)");
  TORCH_CHECK(Hkv >= 1 && H >= 1 && H % Hkv == 0 && H / Hkv <= 8,
              "attn_append: H = ", H, ", Hkv = ", Hkv, " is not supported (H % Hkv == 0, H / Hkv <= 8)");
  // the batch is the cache's here: q / o hold B * T rows
  const int64_t B = k_cache.dim() == 3 ? k_cache.size(0) : 0;
  const int64_t Smax =
      kv_cache_args("attn_append", "q", aligned16(q) && q.stride(0) % 8 == 0, "D", k_cache, v_cache, B, Hkv, D, kv8);
  TORCH_CHECK(T >= 1 && B >= 1 && B * T <= INT_MAX && q.size(0) == B * T && o.size(0) == B * T,
              "attn_append: q/o must hold B * T = ", B * T, " rows");
  TORCH_CHECK(q.size(1) == H * D && o.size(1) == H * D, "attn_append: q/o shape");
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
  const int ns = splits > 0 ? (int)splits : mp_attn_append_plan((int)B, (int)T, (int)Hkv, (int)rep, (int)max_len);
  torch::Tensor ws = torch::empty({mp_attn_append_ws_floats((int)B, (int)T, (int)H, (int)D, ns)},
                                  q.options().dtype(torch::kFloat32));
  check((kv8 ? mp_attn_append_kv8 : mp_attn_append)(
            q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), base.data_ptr<int>(),
            counts.has_value() ? counts->data_ptr<int>() : nullptr, o.data_ptr(), ws.data_ptr<float>(), (int)B, (int)T,
            (int)H, (int)Hkv, (int)D, (int)Smax, (int)max_len, q.stride(0), k_cache.stride(0), k_cache.stride(1),
            v_cache.stride(0), v_cache.stride(1), o.stride(0), (float)scale, ns, cur_stream()),
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
  // int8 caches (both): the quantising append of attention_kv8.hip
  const bool kv8 = k_cache.scalar_type() == torch::kChar && v_cache.scalar_type() == torch::kChar;
  for (const torch::Tensor* t : {&qkv, &k_cache, &v_cache}) {
    TORCH_CHECK(t->is_cuda() && t->get_device() == qkv.get_device(), fn, ": qkv / k_cache / v_cache must be on one GPU");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16 || (kv8 && t != &qkv), fn,
                ": qkv / k_cache / v_cache must be bf16 (or both caches int8), got ", t->scalar_type());
  }
  const int64_t width = (H + 2 * Hkv) * Dh;
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == width && qkv.stride(1) == 1, fn, ": qkv must be [B, (H + 2 Hkv) Dh] rows");
  TORCH_CHECK(T >= 1 && qkv.size(0) >= T && qkv.size(0) % T == 0 && qkv.size(0) <= INT_MAX, fn, ": qkv must hold B * T rows");
  const int64_t B = qkv.size(0) / T, rows = qkv.size(0);
  TORCH_CHECK(B >= 1 && B <= 65535, fn, ": batch outside [1, 65535]");
  const int64_t Smax = kv_cache_args(fn, "qkv", aligned16(qkv) && (rows == 1 || qkv.stride(0) % 8 == 0), "Dh", k_cache,
                                     v_cache, B, Hkv, Dh, kv8);
  TORCH_CHECK(Smax >= 1 && Smax <= INT_MAX, fn, ": cache shape");
  // the kernel writes qkv and both caches: no two rows of one may overlap
  TORCH_CHECK(rows == 1 || qkv.stride(0) >= width, fn, ": qkv rows overlap");
  const int64_t row_elems = kv8 ? kv8_row_bytes(Hkv, Dh) : Hkv * Dh;
  TORCH_CHECK(k_cache.stride(1) >= row_elems && v_cache.stride(1) >= row_elems &&
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
  // qkv's row stride as the kernels index it (a single row may have any)
  const int64_t qkv_ld = rows == 1 ? width : qkv.stride(0);
  check((kv8 ? mp_rope_kv_append_kv8 : mp_rope_kv_append)(
            qkv.data_ptr(), cp, sp, k_cache.data_ptr(), v_cache.data_ptr(), pos.data_ptr<int>(),
            active.has_value() ? active->data_ptr<uint8_t>() : nullptr,
            counts.has_value() ? counts->data_ptr<int>() : nullptr, (int)B, (int)T, (int)H, (int)Hkv, (int)Dh,
            (int)Smax, kv8 ? qkv_ld : qkv.stride(0), k_cache.stride(0), k_cache.stride(1), v_cache.stride(0),
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
  TORCH_CHECK(aligned16(logits) && ld % per == 0 && ld >= Vp, fn, ": logits rows must be 16-byte aligned and disjoint");
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

}  // namespace

void register_generate(py::module& m) {
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("lens"), py::arg("o"),
        py::arg("H"), py::arg("Hkv"), py::arg("D"), py::arg("max_len"), py::arg("scale"), py::arg("splits") = 0);
  m.def("attn_decode_plan", [](int64_t B, int64_t Hkv, int64_t max_len) {
    return mp_attn_decode_plan((int)B, (int)Hkv, (int)max_len);
  }, "key splits the decode attention picks for B sequences x Hkv KV heads over max_len keys");
  m.def("attn_append", &attn_append, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("base"),
        py::arg("counts"), py::arg("o"), py::arg("T"), py::arg("H"), py::arg("Hkv"), py::arg("D"), py::arg("max_len"),
        py::arg("scale"), py::arg("splits") = 0);
  m.def("attn_append_plan", [](int64_t B, int64_t T, int64_t Hkv, int64_t rep, int64_t max_len) {
    return mp_attn_append_plan((int)B, (int)T, (int)Hkv, (int)rep, (int)max_len);
  }, "key splits the append attention picks for B sequences x T tokens x Hkv KV heads of rep query heads over max_len keys");
  m.def("embed_pos", &embed_pos);
  m.def("rope_kv_append", &rope_kv_append, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("pos"), py::arg("active"), py::arg("H"), py::arg("Hkv"), py::arg("Dh"),
        py::arg("rope"), py::arg("T") = 1, py::arg("counts") = py::none());
  m.def("sample", &sample);
}

}  // namespace mipipe_bind
