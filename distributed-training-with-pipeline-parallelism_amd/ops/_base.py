"""What every op family shares: the loader of ``_C.so``, the activation / epilogue codes and
the CPU helpers more than one family uses.  Imports no other module of the package.

``_EXT`` is the one place the loaded extension lives: :func:`load_ext` and :func:`_ext` read it
on every call, so whoever needs to stand in for the extension (a call counter, a test) rebinds
``_base._EXT`` and every family sees it, however it imported ``_ext``."""
from __future__ import annotations

import importlib.util
import os
from typing import Optional

import torch

__all__ = ["ACT", "EPI_NONE", "EPI_BIAS", "EPI_BIAS_GELU", "EPI_BIAS_RELU", "EPI_BIAS_RES", "EPI_RES", "EPI_DGELU",
           "EPI_DRELU", "LOG2E", "load_ext", "ext_available"]

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXT = None
_EXT_ERR: Optional[str] = None

ACT = {"none": 0, "gelu_tanh": 1, "gelu": 1, "relu": 2}
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RELU, EPI_BIAS_RES, EPI_RES, EPI_DGELU, EPI_DRELU = range(8)
LOG2E = 1.4426950408889634


def load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    # MIPIPE_EXT_VARIANT=name loads _C_<name>.so: a build of the same sources with extra
    # compile-time defines (tools/build_ext.py --variant), for in-process A/B of kernel variants
    variant = os.environ.get("MIPIPE_EXT_VARIANT", "")
    path = os.path.join(_PKG_DIR, f"_C_{variant}.so" if variant else "_C.so")
    if not os.path.exists(path):
        _EXT_ERR = f"{path} not found (build it with: python tools/build_ext.py)"
        return None
    try:
        import torch  # noqa: F401  (libtorch must be loaded first)
        spec = importlib.util.spec_from_file_location("mipipe._C", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _EXT = mod
    except Exception as e:  # pragma: no cover - depends on build
        _EXT_ERR = f"failed to load {path}: {e}"
    return _EXT


def ext_available() -> bool:
    return load_ext() is not None


def _ext():
    e = load_ext()
    if e is None:
        raise RuntimeError(f"mipipe HIP extension unavailable on a GPU tensor: {_EXT_ERR}")
    return e


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _cpu_dropout_mask(shape, p, seed, device):
    g = torch.Generator(device="cpu").manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    keep = (torch.rand(shape, generator=g) >= p).float() / (1.0 - p)
    return keep.to(device)


def _act_cpu(x, act):
    if ACT[act] == 1:
        return torch.nn.functional.gelu(x, approximate="tanh")
    if ACT[act] == 2:
        return torch.relu(x)
    return x


def _act_grad_cpu(x, act):
    if ACT[act] == 1:
        k0, k1 = 0.7978845608028654, 0.044715
        u = k0 * (x + k1 * x ** 3)
        t = torch.tanh(u)
        return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k0 * (1 + 3 * k1 * x * x)
    if ACT[act] == 2:
        return (x > 0).float()
    return torch.ones_like(x)
