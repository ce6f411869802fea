// The Python module: every binding file, the native RCCL engine and the stage runner register
// their own names.  No hipify: written against HIP directly.
#include <pybind11/pybind11.h>

namespace mipipe_bind {
void register_norm_loss_embed(pybind11::module& m);
void register_elementwise_optim(pybind11::module& m);
void register_gemm(pybind11::module& m);
void register_gemm_f32(pybind11::module& m);
void register_attention(pybind11::module& m);
void register_generate(pybind11::module& m);
void register_runtime_misc(pybind11::module& m);
}  // namespace mipipe_bind
namespace mipipe_comm {
void register_rccl(pybind11::module& m);
}
namespace mipipe_runtime {
void register_runner(pybind11::module& m);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "mipipe gfx950 HIP kernels";
  mipipe_comm::register_rccl(m);
  mipipe_runtime::register_runner(m);
  mipipe_bind::register_norm_loss_embed(m);
  mipipe_bind::register_elementwise_optim(m);
  mipipe_bind::register_gemm(m);
  mipipe_bind::register_gemm_f32(m);
  mipipe_bind::register_attention(m);
  mipipe_bind::register_generate(m);
  mipipe_bind::register_runtime_misc(m);
}
