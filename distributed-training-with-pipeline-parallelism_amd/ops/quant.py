"""Weight-only quantised linear layers on the skinny-M kernel (csrc/kernels/gemv_skinny.hip,
csrc/bindings/quant.cpp).  The formats differ in a handful of functions and numbers, held in
``QUANT_FORMATS`` and ``MX_FORMATS`` (found by :func:`quant_format`); the skinny call and the any-M
linear are one code path over those tables."""
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
# of the kernel.  Looping it over 16-row blocks and the 64-row kernel behind rows64=True are
# both measured against the dequantising route by tools/w8_time.py (profiles/r15_rows64.md);
# the default route is unchanged
W8_SKINNY_MAX_M = 16
W4_GROUP = 128
# rows of one call of the 64-row sibling (csrc/kernels/gemv_rows64.hip): linear_skinny64, and
# linear_q(rows64=True) between W8_SKINNY_MAX_M and this.  A name of this module only
SKINNY64_MAX_M = 64


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


# mxfp4: OCP MXFP4 -- e2m1 elements with one e8m0 (power-of-two) scale per 32 k -- on the skinny kernel (MX4Fmt of gemv_skinny.hip).  Names of
# this module only
MX_GROUP = 32
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mx4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """OCP MXFP4 quantisation of a 2-D weight ``w [N, K]`` (bf16 or f32, ``K % 128 == 0``, else
    ValueError) -> ``(q4, scale)``, all arithmetic in f32, per group of 32 k:

    * ``scale`` uint8 ``[N, K / 32]``: byte ``e`` stands for ``2^(e - 127)`` (e8m0).  With ``amax``
      the group's largest magnitude, ``E = floor(log2(amax)) - 2`` (from ``torch.frexp``; 2 is
      the exponent of e2m1's largest value, 6) clamped to [-127, 127] and the byte is
      ``E + 127``.  A group of zeros gets byte 0 and codes 0; byte 255 (NaN) is never written.
    * each element is ``w / 2^E`` rounded to the nearest e2m1 magnitude (0, 0.5, 1, 1.5, 2, 3,
      4, 6), ties to the even code, above 6 to 6.  A code is sign << 3 | index of the magnitude;
      a value that rounds to 0 gets code 0 (code 8, -0, is never written; consumers read it as 0).
    * ``q4`` uint8 ``[N, K / 2]``: byte ``b`` of a row holds element ``2 b`` in its low nibble and
      ``2 b + 1`` in its high one (the order of ``torch.float4_e2m1fn_x2``).

    The effective weight is ``What[n, k] = e2m1(code[n, k]) * 2^(scale[n, k // 32] - 127)``.
    Pure tensor code, the same values on every device."""
    if w.dim() != 2:
        raise ValueError("quantize_mx4: w must be [N, K]")
    N, K = w.shape
    if K < W4_GROUP or K % W4_GROUP != 0:
        raise ValueError(f"quantize_mx4: K = {K} must be a multiple of {W4_GROUP}")
    wf = w.detach().float().reshape(N, K // MX_GROUP, MX_GROUP)
    amax = wf.abs().amax(dim=2)
    E = (torch.frexp(amax)[1].to(torch.int32) - 3).clamp_(-127, 127)       # amax = m 2^ex, m in [0.5, 1)
    E = torch.where(amax > 0, E, torch.full_like(E, -127))
    # 2^-E built from its bits (E <= 125 for any finite f32 amax, so the exponent field stays in
    # [2, 254]): an exact power of two on every device, and so is the product
    a = (wf * ((127 - E) << 23).view(torch.float32)[:, :, None]).abs()
    # the seven midpoints between neighbouring magnitudes; a tie goes to the even code, so the
    # midpoints below an even code are included (>=) and those above one are not (>)
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    code = (code | (((wf < 0) & (code > 0)).to(torch.uint8) << 3)).reshape(N, K)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous(), (E + 127).to(torch.uint8).contiguous()


def _mx4_check(name, x, q4, scale):
    if q4.dtype != torch.uint8 or q4.dim() != 2 or x.dim() != 2 or x.shape[1] != 2 * q4.shape[1]:
        raise ValueError(f"{name}: x [M, K] and packed uint8 q4 [N, K / 2] needed, got {tuple(x.shape)} and "
                         f"{q4.dtype} {tuple(q4.shape)}")
    N, K = q4.shape[0], 2 * q4.shape[1]
    if K % W4_GROUP != 0:
        raise ValueError(f"{name}: K = {K} must be a multiple of {W4_GROUP}")
    if scale is None or scale.dtype != torch.uint8 or tuple(scale.shape) != (N, K // MX_GROUP):
        raise ValueError(f"{name}: scale must be uint8 [N, K / 32] = [{N}, {K // MX_GROUP}]")


def _mx4_what(q4, scale):
    """f32 [N, K]: e2m1(code) * 2^(byte - 127), exact (2^-127 is an f32 subnormal; byte 255 is NaN)"""
    lut = torch.tensor(_E2M1 + (0.0,) + tuple(-v for v in _E2M1[1:]), device=q4.device)
    e8 = torch.tensor([2.0 ** (e - 127) for e in range(255)] + [float("nan")], device=q4.device)
    b = q4.to(torch.int64)
    val = lut[torch.stack((b & 15, b >> 4), dim=2).reshape(q4.shape[0], -1)]
    return val * e8[scale.to(torch.int64)].repeat_interleave(MX_GROUP, dim=1)


def _mx4_matmul_cpu(x, q4, scale):
    return x.float() @ _mx4_what(q4, scale).t()


def dequant_mx4(q4: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [N, K] = the effective weight of :func:`quantize_mx4`'s format in out's dtype (bf16 on
    the GPU, where one v_cvt_scalef32_pk_bf16_fp4 makes two elements).  Exact while the value
    is a normal bf16 (scale bytes in [2, 250]); a zero may carry code 8's sign."""
    N, K = q4.shape[0], 2 * q4.shape[1]
    if q4.dtype != torch.uint8 or K % W4_GROUP != 0 or scale.dtype != torch.uint8 or \
            tuple(scale.shape) != (N, K // MX_GROUP):
        raise ValueError(f"dequant_mx4: packed uint8 q4 [N, K / 2] with K % 128 == 0 and uint8 scale [N, K / 32] needed, "
                         f"got {q4.dtype} {tuple(q4.shape)} and {scale.dtype} {tuple(scale.shape)}")
    if out is None:
        out = torch.empty(N, K, device=q4.device, dtype=torch.bfloat16 if _gpu(q4) else torch.float32)
    if _gpu(q4):
        _ext().dequant_w8(q4, scale, out)
    else:
        out.copy_(_mx4_what(q4, scale).to(out.dtype))
    return out


# mxfp8 activation rows: e4m3 elements with one e8m0 scale per 32 k, the scales inside the row (as in the int8 KV
# cache), for the scaled-MFMA GEMM against MXFP4 weights (csrc/kernels/gemm_mx.hip).  Names of this module only
FP8 = torch.float8_e4m3fn
E4M3_MAX = 448.0


def mx8_row_bytes(K: int) -> int:
    """bytes of one MXFP8 row: K codes, K / 32 scale bytes, zero padding to a multiple of 16"""
    return (K + K // MX_GROUP + 15) // 16 * 16


def _mx8_rows(x: torch.Tensor) -> torch.Tensor:
    """the rows of :func:`quantize_mx8_rows` as uint8 [M, mx8_row_bytes(K)]: tensor code, any device"""
    M, K = x.shape
    G = K // MX_GROUP
    xf = x.detach().float().reshape(M, G, MX_GROUP)
    amax = xf.abs().amax(dim=2)
    E = (torch.frexp(amax)[1].to(torch.int32) - 9).clamp_(-127, 127)       # amax = m 2^ex, m in [0.5, 1)
    # 2^-E from its bits (E <= 120: the exponent field stays in [7, 254]), so the products are exact
    E = E + (amax * ((127 - E) << 23).view(torch.float32) > E4M3_MAX).to(torch.int32)
    live = amax > 0
    inv = torch.where(live, ((127 - E) << 23).view(torch.float32), torch.zeros_like(amax))
    code = (xf * inv[:, :, None]).to(FP8).view(torch.uint8).reshape(M, K)
    rows = torch.zeros(M, mx8_row_bytes(K), device=x.device, dtype=torch.uint8)
    rows[:, :K] = torch.where(code == 0x80, torch.zeros_like(code), code)  # -0 is stored as 0
    rows[:, K: K + G] = torch.where(live, E + 127, torch.zeros_like(E)).to(torch.uint8)
    return rows


def quantize_mx8_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MXFP8 rows of ``x [M, K]`` (bf16 or f32 rows of any stride, ``K % 128 == 0``, else ValueError) ->
    ``torch.float8_e4m3fn [M, mx8_row_bytes(K)]``, contiguous.  Bytes ``[0, K)`` of a row are OCP e4m3
    codes in k order, bytes ``[K, K + K / 32)`` the e8m0 byte of each group of 32 (``e`` stands for
    ``2^(e - 127)``), the rest zeros.  Per group, in f32: ``E = floor(log2 amax) - 8``, plus 1 if
    ``amax * 2^-E > 448``, clamped to [-127, 127]; each element is ``x * 2^-E`` (exact) rounded to nearest
    even into e4m3, subnormals kept, so no element exceeds 448 and nothing saturates.  A group of zeros
    gets byte 0 and codes 0; a value that rounds to zero gets code 0; byte 255 is never written.  On the
    GPU one kernel writes exactly these bytes: no synchronisation and, given ``out``, no allocation."""
    if x.dim() != 2 or x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("quantize_mx8_rows: x must be bf16 or f32 [M, K]")
    M, K = x.shape
    if M < 1 or K < W4_GROUP or K % W4_GROUP != 0:
        raise ValueError(f"quantize_mx8_rows: K = {K} must be a multiple of {W4_GROUP}")
    if out is None:
        out = torch.empty(M, mx8_row_bytes(K), device=x.device, dtype=FP8)
    if out.dtype != FP8 or tuple(out.shape) != (M, mx8_row_bytes(K)) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"quantize_mx8_rows: out must be contiguous float8_e4m3fn [{M}, {mx8_row_bytes(K)}] on x's device")
    if _gpu(x):
        _ext().cast_f32_bf16(x, out)
    else:
        out.view(torch.uint8).copy_(_mx8_rows(x))
    return out


def dequantize_mx8_rows(xq: torch.Tensor, K: int, dtype=torch.float32) -> torch.Tensor:
    """``[M, K]`` values of MXFP8 rows: e4m3(code) * 2^(byte - 127), exact in f32."""
    if xq.dtype != FP8 or xq.dim() != 2 or K % MX_GROUP != 0 or xq.shape[1] != mx8_row_bytes(K):
        raise ValueError(f"dequantize_mx8_rows: float8_e4m3fn [M, {mx8_row_bytes(K)}] rows needed, got {xq.dtype} "
                         f"{tuple(xq.shape)}")
    e8 = torch.tensor([2.0 ** (e - 127) for e in range(255)] + [float("nan")], device=xq.device)
    s = e8[xq.view(torch.uint8)[:, K: K + K // MX_GROUP].to(torch.int64)]
    return (xq[:, :K].float() * s.repeat_interleave(MX_GROUP, dim=1)).to(dtype)


def _mx4a8_matmul_cpu(x, q4, scale):
    xh = dequantize_mx8_rows(quantize_mx8_rows(x.detach()), x.shape[1])
    return (xh.double() @ _mx4_what(q4, scale).double().t()).float()


def linear_mx4a8(x: torch.Tensor, q4: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 xq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(Xhat @ What^T + bias) (+ residual) for any number of rows, with ``Xhat`` the MXFP8 rows of
    ``x`` (:func:`quantize_mx8_rows`) and ``What`` MXFP4 weights as :func:`quantize_mx4` stores them.  On
    the GPU two kernels: the quantiser into ``xq`` (a contiguous float8_e4m3fn buffer of at least
    ``M * mx8_row_bytes(K)`` elements; allocated here if None), then the GEMM on
    v_mfma_scale_f32_16x16x128_f8f6f4, which reads both operands as stored and accumulates in f32.  No
    scratch, no synchronisation, and with ``out`` and ``xq`` no allocation.  Row m of the result does not
    depend on M or on the other rows.  On the CPU: the product of the two dequantised operands, with the
    epilogue of the other quantised linears.  Returns y."""
    f = MX_FORMATS["mxfp4"]
    M, N, K, out = _checked("linear_mx4a8", f, x, q4, scale, bias, act, residual, out)
    if not _gpu(x):
        return _linear_cpu(f._replace(matmul_cpu=_mx4a8_matmul_cpu), x, q4, scale, bias, act, residual, out)
    need = M * mx8_row_bytes(K)
    if xq is None:
        xq = torch.empty(need, device=x.device, dtype=FP8)
    if xq.dtype != FP8 or not xq.is_contiguous() or xq.numel() < need:
        raise ValueError(f"linear_mx4a8: xq must be contiguous float8_e4m3fn with at least {need} elements")
    rows = quantize_mx8_rows(x, out=xq.view(-1)[:need].view(M, -1))
    _ext().gemv_skinny(rows, q4, scale, out, bias, residual, act != "none", 0)
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
# the formats of power-of-two block scales; ``QUANT_FORMATS`` keeps its two entries
MX_FORMATS = {
    "mxfp4": _Format(_mx4_check, _mx4_matmul_cpu, quantize_mx4, dequant_mx4, W4_GROUP, W4_GROUP,
                     "linear_skinny_mx4", "linear_mx4", "linear_mx4 takes any M"),
}


def quant_format(fmt: str) -> _Format:
    """The record of a format of either table by its name (KeyError otherwise)."""
    return QUANT_FORMATS[fmt] if fmt in QUANT_FORMATS else MX_FORMATS[fmt]


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


def _skinny(f, x, q, scale, bias, act, residual, out, force_split, checked=None, name=None, max_m=SKINNY_MAX_M):
    name = name or f.skinny
    M, N, K, out = checked or _checked(name, f, x, q, scale, bias, act, residual, out)
    if M < 1 or M > max_m:
        raise ValueError(f"{name}: M = {M} outside [1, {max_m}] ({f.any_m})")
    if K % f.k_skinny != 0:
        raise ValueError(f"{name}: K = {K} must be a multiple of {f.k_skinny}")
    if not _gpu(x):
        return _linear_cpu(f, x, q, scale, bias, act, residual, out)
    if M > SKINNY_MAX_M and not _x_aligned(x):
        raise ValueError(f"{name}: more than {SKINNY_MAX_M} rows need 16-byte aligned x rows (the data pointer and "
                         f"a row stride of a multiple of 8 elements)")
    _ext().gemv_skinny(x, q, scale, out, bias, residual, act != "none", int(force_split))
    return out


def _x_aligned(x):
    """x rows the 64-row kernel can read as 16-byte chunks"""
    return x.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0 and x.stride(1) == 1


def reads_weights_directly(x: torch.Tensor, fmt: str, rows64: bool = False) -> bool:
    """Whether :func:`linear_q` runs a GPU ``x`` [M, K] on the quantised matrix itself (the
    skinny kernel, or with ``rows64`` its 64-row sibling) and so needs no scratch.  The one
    statement of that route: ``linear_q`` and the generator both ask here."""
    M, K = x.shape
    if K % quant_format(fmt).k_skinny != 0:
        return False
    # the 64-row sibling has no MXFP4 instantiation: those layers dequantise above 16 rows
    rows64 = rows64 and fmt not in MX_FORMATS
    return M <= W8_SKINNY_MAX_M or (rows64 and M <= SKINNY64_MAX_M and _x_aligned(x))


def linear_q(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, fmt: str, bias: Optional[torch.Tensor] = None,
             act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             scratch: Optional[torch.Tensor] = None, rows64: bool = False) -> torch.Tensor:
    """:func:`linear_w8` / :func:`linear_w4` / :func:`linear_mx4` by the name of the format, a key of
    ``QUANT_FORMATS`` or ``MX_FORMATS``.
    ``rows64=True``: on the GPU, ``W8_SKINNY_MAX_M < M <= SKINNY64_MAX_M`` rows (16-byte aligned,
    ``K`` a multiple of the format's skinny step) run :func:`linear_skinny64` on the quantised
    matrix itself instead of dequantising: no scratch is touched."""
    f = quant_format(fmt)
    M, N, K, out = _checked(f.linear, f, x, q, scale, bias, act, residual, out)
    if not _gpu(x):
        return _linear_cpu(f, x, q, scale, bias, act, residual, out)
    if reads_weights_directly(x, fmt, rows64):
        return _skinny(f, x, q, scale, bias, act, residual, out, 0, checked=(M, N, K, out),
                       max_m=SKINNY64_MAX_M if rows64 and fmt not in MX_FORMATS else SKINNY_MAX_M)
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


def linear_skinny64(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None, act: str = "none", residual: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, force_split: int = 0) -> torch.Tensor:
    """:func:`linear_skinny` / :func:`linear_skinny_w4` for up to ``SKINNY64_MAX_M`` = 64 rows, by
    the dtype of ``w``: int8 [N, K] with ``scale`` [N], uint8 packed 4-bit [N, K / 2] with
    ``scale`` [K / 128, N], or bf16 [N, K] without a scale.  Above 16 rows the weights are still
    streamed and converted once (csrc/kernels/gemv_rows64.hip), and row m of the result is bit
    for bit what the 16-row call gives for that row, for every M, epilogue and ``force_split``:
    the K-chains of the plan do not change.  More than 16 rows need 16-byte aligned x rows.
    Everything else is as in :func:`linear_skinny`.  Returns y."""
    f = QUANT_FORMATS["int4g128" if w.dtype == torch.uint8 else "int8"]
    return _skinny(f, x, w, scale, bias, act, residual, out, force_split, name="linear_skinny64", max_m=SKINNY64_MAX_M)


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


def linear_skinny_mx4(x: torch.Tensor, q4: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
                      act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      force_split: int = 0) -> torch.Tensor:
    """:func:`linear_skinny` over MXFP4 weights (:func:`quantize_mx4`): ``q4`` uint8 [N, K / 2],
    ``scale`` uint8 [N, K / 32] (any alignment), at most 16 rows of x.  The kernel converts
    codes and scale to the bf16 effective weight in one instruction and accumulates
    ``x @ What^T`` in f32.  Everything else is as in :func:`linear_skinny`.  Returns y."""
    return _skinny(MX_FORMATS["mxfp4"], x, q4, scale, bias, act, residual, out, force_split)


def linear_mx4(x: torch.Tensor, q4: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
               act: str = "none", residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`linear` over MXFP4 weights, any number of rows: the skinny kernel on ``q4`` itself
    up to ``W8_SKINNY_MAX_M`` rows, :func:`dequant_mx4` into ``scratch`` and the training GEMM
    above (there is no 64-row kernel for this format).  Returns y."""
    return linear_q(x, q4, scale, "mxfp4", bias, act, residual, out, scratch)
