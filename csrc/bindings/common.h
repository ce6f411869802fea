// Shared by the binding files (csrc/bindings/*.cpp): torch tensors in, launches on the current
// HIP stream.  Kernels live in csrc/kernels/*.hip behind the plain C launchers of mp_api.h.
// Helpers are inline: a binding is a handful of checks and one launch, called per token.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <map>
#include <optional>
#include <string>

#include "mp_api.h"

namespace py = pybind11;

namespace mipipe_bind {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check(int rc, const char* what) { TORCH_CHECK(rc == 0, "mipipe kernel ", what, " failed with code ", rc); }

inline const void* ptr_or_null(const c10::optional<torch::Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }
inline void* mptr_or_null(const c10::optional<torch::Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }

// storage dtype of the normalisation / loss / embedding kernels: bf16, or f32 (the
// reference-precision path); returns 1 for f32
inline int storage(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32, name,
              " must be bf16 or f32, got ", t.scalar_type());
  return t.scalar_type() == torch::kFloat32 ? 1 : 0;
}

inline void req(const torch::Tensor& t, torch::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == dt, name, " has wrong dtype ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// req + the element count the launcher will index
inline void reqn(const torch::Tensor& t, torch::ScalarType dt, int64_t n, const char* name) {
  req(t, dt, name);
  TORCH_CHECK(t.numel() == n, name, " has ", t.numel(), " elements, expected ", n);
}

// a [rows, width] position table (wpe / dwpe, RoPE cos / sin): token t reads row
// t % S + pos_offset, so rows 0 .. min(T, S) + pos_offset - 1 must exist
inline void req_pos_table(const torch::Tensor& t, int64_t width, int64_t T, int64_t S, int64_t pos_offset,
                          const char* name) {
  TORCH_CHECK(S >= 1 && pos_offset >= 0, name, ": S must be >= 1 and pos_offset >= 0");
  const int64_t need = std::min(T, S) + pos_offset;
  TORCH_CHECK(t.dim() == 2 && t.size(1) == width && t.size(0) >= need, name, " must be [>= ", need, ", ", width,
              "] (min(T, S) + pos_offset rows), got ", t.sizes());
}

// the base address of 16-byte (8 bf16 / 4 f32) vector accesses
inline bool aligned16(const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

// The switches of a planner (g2::PlanEnv, attn::AttnEnv) by name over their defaults; none:
// the process environment, read once.  `what`: "a planner switch", "an attention switch".
using PlanEnvDict = std::map<std::string, std::string>;
template <class Env>
Env parse_env(const char* fn, const char* what, const std::optional<PlanEnvDict>& env) {
  if (!env.has_value()) return Env::process();
  for (const auto& kv : *env) TORCH_CHECK(Env::known(kv.first.c_str()), fn, ": ", kv.first, " is not ", what);
  return Env::parse([&](const char* name) {
    const auto it = env->find(name);
    return it == env->end() ? (const char*)nullptr : it->second.c_str();
  });
}

}  // namespace mipipe_bind
