"""Weight-only quantised linear layers on the skinny-M kernel (csrc/kernels/gemv_skinny.hip,
csrc/bindings/quant.cpp).  The formats differ in a handful of functions and numbers, held in
``QUANT_FORMATS``; the skinny call and the any-M linear are one code path over that table."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Tuple

import torch

from ._base import _act_cpu, _ext, _gpu
from .gemm import linear

__all__ = ["SKINNY_MAX_M", "W8_SKINNY_MAX_M", "W4_GROUP", "QUANT_FORMATS", "quantize_w8", "quantize_w4", "dequant_w8",
           "dequant_w4", "gemv_plan", "linear_skinny", "linear_skinny_w4", "linear_w8", "linear_w4", "linear_q"]

SKINNY_MAX_M = 16
# linear_w8 runs the skinny kernel up to this many rows and dequantises above.  16 = one call
# of the kernel; looping it over 16-row blocks has not been measured against the
# dequantising route (tools/w8_time.py prints both, profiles/r12_w8_decode.md)
W8_SKINNY_MAX_M = 16
W4_GROUP = 128


def gemv_plan(N: int, K: int, wbytes: int, force_split: int = 0) -> Tuple[int, int]:
    """(weight rows per workgroup, K-splits) of the skinny kernel for an [N, K] weight of
    ``wbytes`` bytes per element (1: int8, 2: bf16; the code 0: packed 4-bit with group
    scales, which needs ``K % 128 == 0``): csrc/include/mp_gemv_plan.h.  Needs the built
    extension, not a GPU."""
    return tuple(_ext().gemv_plan(int(N), int(K), int(wbytes), int(force_split)))


# int8: one f32 scale per output row (bf16 weights without a scale run the same kernel)
def quantize_w8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Symmetric per-output-row int8 quantisation of a 2-D weight ``w [N, K]`` (bf16 or f32):
    ``scale[n] = max_k |w[n, k]| / 127`` (f32) and ``q[n, k] = clamp(round_half_even(w[n, k] /
    scale[n]), -127, 127)`` (int8, [N, K] row-major: the tensor the kernel reads).  A row of
    zeros gets scale 0 and q 0.  The effective weight is ``q * scale``.  Pure tensor code, the
    same on every device."""
    if w.dim() != 2:
        raise ValueError("quantize_w8: w must be [N, K]")
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    # a tensor divisor: dividing by a Python scalar is a multiplication by its reciprocal on
    # the GPU, an ulp away from the CPU's quotient in some rows
    scale = amax / torch.full_like(amax, 127.0)
    safe = torch.where(scale > 0, scale, torch.ones_like(scale))
    q = torch.round(wf / safe[:, None]).clamp_(-127, 127).to(torch.int8)
    return q.contiguous(), scale.contiguous()


def _w8_check(name, x, w, scale):
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"{name}: x [M, K] and w [N, K] needed, got {tuple(x.shape)} and {tuple(w.shape)}")
    if (w.dtype == torch.int8) != (scale is not None):
        raise ValueError(f"{name}: int8 weights take a scale, other weights none")


def _w8_matmul_cpu(x, w, scale):
    y = x.float() @ w.float().t()
    return y if scale is None else y * scale.float()


def dequant_w8(q: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (q * scale) rounded to out's dtype (bf16 on the GPU): the effective weight."""
    if out is None:
        out = torch.empty(q.shape, device=q.device, dtype=torch.bfloat16 if _gpu(q) else torch.float32)
    if _gpu(q):
        _ext().dequant_w8(q, scale, out)
    else:
        out.copy_((q.float() * scale.float()[:, None]).to(out.dtype))
    return out


# int4g128: 4-bit weights with one f32 scale per 128-element group of K, on the same kernel
def quantize_w4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Symmetric 4-bit quantisation of a 2-D weight ``w [N, K]`` (bf16 or f32) with one scale
    per 128-element group of K (``K % 128 == 0``, else ValueError) -> ``(q4, scale)``:

    * ``scale[g, n] = max_{k in [128 g, 128 g + 128)} |w[n, k]| / 7``, f32 ``[K / 128, N]``
      contiguous (group-major: the four output rows a lane of the kernel owns are 16
      contiguous bytes).  A group of zeros has scale 0 and q 0.
    * ``q[n, k] = clamp(round_half_even(w[n, k] / scale[k // 128, n]), -7, 7)``.
    * ``q4`` is uint8 ``[N, K / 2]`` row-major: byte ``b`` of a row holds ``q[n, 2 b] + 8`` in
      its low nibble and ``q[n, 2 b + 1] + 8`` in its high nibble.  Nibble 0 is never written
      here, but every consumer decodes all 16 values as ``nibble - 8``, so it means -8.

    The effective weight is ``What[n, k] = q[n, k] * scale[k // 128, n]``.  Pure tensor code,
    the same values on every device."""
    if w.dim() != 2:
        raise ValueError("quantize_w4: w must be [N, K]")
    N, K = w.shape
    if K < W4_GROUP or K % W4_GROUP != 0:
        raise ValueError(f"quantize_w4: K = {K} must be a multiple of {W4_GROUP}")
    wf = w.detach().float().reshape(N, K // W4_GROUP, W4_GROUP)
    amax = wf.abs().amax(dim=2)                                     # [N, G]
    # a tensor divisor, as in quantize_w8: the same quotient on the CPU and the GPU
    scale = amax / torch.full_like(amax, 7.0)
    safe = torch.where(scale > 0, scale, torch.ones_like(scale))
    q = torch.round(wf / safe[:, :, None]).clamp_(-7, 7).to(torch.int16).reshape(N, K) + 8
    q4 = (q[:, 0::2] | (q[:, 1::2] << 4)).to(torch.uint8)
    return q4.contiguous(), scale.t().contiguous()


def _w4_check(name, x, q4, scale):
    if q4.dtype != torch.uint8 or q4.dim() != 2 or x.dim() != 2 or x.shape[1] != 2 * q4.shape[1]:
        raise ValueError(f"{name}: x [M, K] and packed uint8 q4 [N, K / 2] needed, got {tuple(x.shape)} and "
                         f"{q4.dtype} {tuple(q4.shape)}")
    N, K = q4.shape[0], 2 * q4.shape[1]
    if K % W4_GROUP != 0:
        raise ValueError(f"{name}: K = {K} must be a multiple of {W4_GROUP}")
    if scale is None or scale.dim() != 2 or tuple(scale.shape) != (K // W4_GROUP, N):
        raise ValueError(f"{name}: scale must be [K / 128, N] = [{K // W4_GROUP}, {N}]")


def _w4_unpack(q4: torch.Tensor) -> torch.Tensor:
    """q [N, K] f32 of packed nibbles: nibble - 8, all 16 values"""
    b = q4.to(torch.int16)
    return (torch.stack((b & 15, b >> 4), dim=2).reshape(q4.shape[0], -1) - 8).float()


def _w4_matmul_cpu(x, q4, scale):
    """sum_g scale[g, n] * (sum_{k in g} x[m, k] q[n, k]) in f32: the kernel's order of scaling"""
    M, K = x.shape
    N, G = q4.shape[0], K // W4_GROUP
    part = torch.einsum("mgk,ngk->mng", x.float().reshape(M, G, W4_GROUP), _w4_unpack(q4).reshape(N, G, W4_GROUP))
    return (part * scale.float().t()[None]).sum(dim=2)


def dequant_w4(q4: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [N, K] = (q * scale per group) rounded to out's dtype (bf16 on the GPU): the
    effective weight of :func:`quantize_w4`'s format."""
    N, K = q4.shape[0], 2 * q4.shape[1]
    if q4.dtype != torch.uint8 or K % W4_GROUP != 0 or tuple(scale.shape) != (K // W4_GROUP, N):
        raise ValueError(f"dequant_w4: packed uint8 q4 [N, K / 2] with K % 128 == 0 and scale [K / 128, N] needed, got "
                         f"{q4.dtype} {tuple(q4.shape)} and {tuple(scale.shape)}")
    if out is None:
        out = torch.empty(N, K, device=q4.device, dtype=torch.bfloat16 if _gpu(q4) else torch.float32)
    if _gpu(q4):
        _ext().dequant_w8(q4, scale, out)
    else:
        out.copy_((_w4_unpack(q4) * scale.float().t().repeat_interleave(W4_GROUP, dim=1)).to(out.dtype))
    return out


# One entry per format, holding what differs: the operand check (name, x, q, scale); x @ What^T in f32 on the CPU,
# scaled in the kernel's order; quantize and dequant; the K multiple a matrix needs to be stored (k_format) and to be
# read by the skinny kernel (k_skinny); the names its errors carry and where the skinny kernel's M bound points
_Format = namedtuple("_Format", "check matmul_cpu quantize dequant k_format k_skinny skinny linear any_m")
QUANT_FORMATS = {
    "int8": _Format(_w8_check, _w8_matmul_cpu, quantize_w8, dequant_w8, 1, 32,
                    "linear_skinny", "linear_w8", "linear_w8 / linear take any M"),
    "int4g128": _Format(_w4_check, _w4_matmul_cpu, quantize_w4, dequant_w4, W4_GROUP, W4_GROUP,
                        "linear_skinny_w4", "linear_w4", "linear_w4 takes any M"),
}


def _checked(name, f, x, q, scale, bias, act, residual, out):
    f.check(name, x, q, scale)
    if act not in ("none", "gelu", "gelu_tanh"):
        raise ValueError(f"{name}: activation {act!r} is not supported (none, gelu_tanh)")
    if act != "none" and (bias is None or residual is not None):
        raise ValueError(f"{name}: activation epilogue needs a bias and no residual")
    if out is None:
        out = torch.empty(x.shape[0], q.shape[0], device=x.device, dtype=x.dtype)
    return x.shape[0], q.shape[0], x.shape[1], out


def _linear_cpu(f, x, q, scale, bias, act, residual, out):
    y = f.matmul_cpu(x, q, scale)
    if bias is not None:
        y = y + bias.float()
    if act != "none":
        y = _act_cpu(y.to(x.dtype).float(), act)
    if residual is not None:
        y = y + residual.float()
    return out.copy_(y.to(out.dtype))


def _skinny(f, x, q, scale, bias, act, residual, out, force_split, checked=None):
    M, N, K, out = checked or _checked(f.skinny, f, x, q, scale, bias, act, residual, out)
    if M < 1 or M > SKINNY_MAX_M:
        raise ValueError(f"{f.skinny}: M = {M} outside [1, {SKINNY_MAX_M}] ({f.any_m})")
    if K % f.k_skinny != 0:
        raise ValueError(f"{f.skinny}: K = {K} must be a multiple of {f.k_skinny}")
    if not _gpu(x):
        return _linear_cpu(f, x, q, scale, bias, act, residual, out)
    _ext().gemv_skinny(x, q, scale, out, bias, residual, act != "none", int(force_split))
    return out


def linear_q(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, fmt: str, bias: Optional[torch.Tensor] = None,
             act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`linear_w8` / :func:`linear_w4` by the name of the format, a key of ``QUANT_FORMATS``."""
    f = QUANT_FORMATS[fmt]
    M, N, K, out = _checked(f.linear, f, x, q, scale, bias, act, residual, out)
    if not _gpu(x):
        return _linear_cpu(f, x, q, scale, bias, act, residual, out)
    if M <= W8_SKINNY_MAX_M and K % f.k_skinny == 0:
        return _skinny(f, x, q, scale, bias, act, residual, out, 0, checked=(M, N, K, out))
    if scratch is None:
        scratch = torch.empty(N * K, device=x.device, dtype=torch.bfloat16)
    if scratch.dtype != torch.bfloat16 or scratch.numel() < N * K or not scratch.is_contiguous():
        raise ValueError(f"{f.linear}: scratch must be contiguous bf16 with at least {N * K} elements")
    w = f.dequant(q, scale, scratch.view(-1)[: N * K].view(N, K))
    return linear(x, w, bias, act=act, residual=residual, out=out)[0]


def linear_skinny(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                  bias: Optional[torch.Tensor] = None, act: str = "none", residual: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, force_split: int = 0) -> torch.Tensor:
    """y = act(x @ What^T + bias) (+ residual) for at most 16 rows of x, streaming the weight
    matrix once.  ``w`` [N, K] is int8 with ``scale`` f32 [N] (What = w * scale, the scale
    applied in f32 after the accumulation) or bf16 without.  ``x`` / ``out`` / ``residual`` are
    bf16 rows of any stride; K must be a multiple of 32.  GELU rounds the pre-activation to
    bf16 first, as :func:`linear` does.  Row m of the result does not depend on the number of
    rows or on the other rows.  ``force_split``: the K-split of the plan, for tests.  No host
    synchronisation and, given ``out``, no allocation.  Returns y."""
    return _skinny(QUANT_FORMATS["int8"], x, w, scale, bias, act, residual, out, force_split)


def linear_w8(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
              act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`linear` over int8 weights ``q`` [N, K] with ``scale`` [N], any number of rows.
    Up to ``W8_SKINNY_MAX_M`` rows: the skinny kernel on ``q`` itself.  More rows (a prefill):
    ``q * scale`` is written as bf16 into ``scratch`` (at least N * K elements; allocated
    here if None) and the training GEMM runs on that.  Returns y."""
    return linear_q(x, q, scale, "int8", bias, act, residual, out, scratch)


def linear_skinny_w4(x: torch.Tensor, q4: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
                     act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     force_split: int = 0) -> torch.Tensor:
    """:func:`linear_skinny` over int4g128 weights (:func:`quantize_w4`): ``q4`` uint8
    [N, K / 2], ``scale`` f32 [K / 128, N], at most 16 rows of x.  Each group's f32 sum is
    multiplied by its scale in f32 and the groups are added in f32.  Everything else --
    strides, GELU rounding, row independence, ``force_split``, no synchronisation, no
    allocation given ``out`` -- is as in :func:`linear_skinny`.  Returns y."""
    return _skinny(QUANT_FORMATS["int4g128"], x, q4, scale, bias, act, residual, out, force_split)


def linear_w4(x: torch.Tensor, q4: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
              act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`linear` over int4g128 weights, any number of rows.  Up to ``W8_SKINNY_MAX_M``
    rows: the skinny kernel on ``q4`` itself.  More rows (a prefill): the effective weight is
    written as bf16 into ``scratch`` (at least N * K elements; allocated here if None) and
    the training GEMM runs on that.  Returns y."""
    return linear_q(x, q4, scale, "int4g128", bias, act, residual, out, scratch)
