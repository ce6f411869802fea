// Bindings that serve the runtime, not a model: private HIP streams and the hardware-queue
// probe (probe.hip, parallel/queues.py).
#include "common.h"

namespace mipipe_bind {
namespace {

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

// Enqueue the bounded spinner on stream `waiter` / the flag store on stream `setter` (raw HIP
// stream handles; 0 = the current stream).  flag: int32 [1], result: int32 [2] device tensors.
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

void register_runtime_misc(py::module& m) {
  m.def("create_stream", &create_stream, py::arg("device"), py::arg("priority") = 0);
  m.def("probe_spin", &probe_spin, py::arg("flag"), py::arg("expect"), py::arg("timeout_us"), py::arg("result"),
        py::arg("waiter") = 0);
  m.def("probe_set", &probe_set, py::arg("flag"), py::arg("value"), py::arg("setter") = 0);
  m.def("probe_clock_khz", []() { return mp_probe_clock_khz(); });
}

}  // namespace mipipe_bind
