"""The f32-input MFMA GEMM (csrc/kernels/gemm_f32.hip, csrc/bindings/gemm_f32.cpp): the engine
call with its epilogue codes, and the autograd classes that put an f32 module's linears and
attention projections on it -- the reference-precision path (the reference's own f32 model,
helper:36-46)."""
from __future__ import annotations

from typing import Optional

import torch

from ._base import _ext

__all__ = ["F32_NONE", "F32_BIAS", "F32_BIAS_RELU", "F32_RES", "F32_BIAS_RES", "F32_DRELU", "linear_f32", "F32Linear",
           "F32MultiheadAttention", "use_f32_kernels"]

# f32 GEMM epilogues (csrc/kernels/gemm_f32.hip mp_gemm_f32_ex)
F32_NONE, F32_BIAS, F32_BIAS_RELU, F32_RES, F32_BIAS_RES, F32_DRELU = range(6)


def _gemm_f32(A, B, C, bias=None, R=None, X=None, epi=F32_NONE, alpha=1.0, accumulate=False, p_drop=0.0, seed=0):
    """C = epi(alpha * A @ B (+ C)) on the f32 MFMA engine; A [M,K], B [K,N] views with a unit
    stride in either dimension.  Raises if the layout is not supported (the f32 GPU path has
    no ATen fallback: the reference-precision numbers must come from our kernels)."""
    if not _ext().gemm_f32_ex(A, B, C, bias, R, X, int(epi), float(alpha), bool(accumulate), float(p_drop), int(seed), 0):
        raise RuntimeError(f"gemm_f32_ex: unsupported layout A{tuple(A.shape)}/{A.stride()} B{tuple(B.shape)}/{B.stride()}")
    return C


class _LinearF32(torch.autograd.Function):
    """y = x W^T + b with the forward and both backward GEMMs on gemm_f32 (exact f32
    products, f32 accumulate); any layout the kernel does not take falls back to ATen."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.reshape(-1, x.shape[-1])
        out = torch.empty(x2.shape[0], w.shape[0], device=x.device, dtype=torch.float32)
        if not _ext().gemm_f32(x2, w.t(), out, b, 1.0, False):
            out = torch.addmm(b, x2, w.t()) if b is not None else torch.mm(x2, w.t())
        ctx.save_for_backward(x2, w)
        ctx.has_b = b is not None
        ctx.in_shape = x.shape
        return out.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, w = ctx.saved_tensors
        g2 = gy.reshape(-1, gy.shape[-1])
        if g2.stride(1) != 1:
            g2 = g2.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(g2.shape[0], w.shape[1], device=gy.device, dtype=torch.float32)
            if not _ext().gemm_f32(g2, w, dx, None, 1.0, False):
                dx = torch.mm(g2, w)
            dx = dx.view(ctx.in_shape)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            if not _ext().gemm_f32(g2.t(), x2, dw, None, 1.0, False):
                dw = torch.mm(g2.t(), x2)
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = g2.sum(0)
        return dx, dw, db


def linear_f32(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear for f32 CUDA tensors on the f32 MFMA GEMM (autograd-aware)."""
    return _LinearF32.apply(x, w, b)


class F32Linear(torch.nn.Linear):
    """``nn.Linear`` whose f32 GPU forward/backward run on :func:`linear_f32` (other dtypes
    and CPU: ATen).  Installed by class swap (:func:`use_f32_kernels`): same parameters,
    same state_dict keys."""

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.float32 and self.weight.dtype == torch.float32:
            return _LinearF32.apply(x, self.weight, self.bias)
        return super().forward(x)


def _mha_projected(mod: torch.nn.MultiheadAttention, query, key, value, is_causal: bool, linear):
    """``nn.MultiheadAttention`` forward without attention weights: packed / k-v-shared /
    separate input projections through ``linear``, SDPA core, output projection."""
    same_qkv, same_kv = query is key and key is value, key is value
    if not mod.batch_first:
        query, key, value = (t.transpose(0, 1) for t in (query, key, value))
    B, L, E = query.shape
    H = mod.num_heads
    w, b = mod.in_proj_weight, mod.in_proj_bias

    def part(lo, hi):
        return w[lo:hi], (b[lo:hi] if b is not None else None)
    if same_qkv:
        q, k, v = linear(query, w, b).chunk(3, dim=-1)
    elif same_kv:
        q = linear(query, *part(0, E))
        k, v = linear(key, *part(E, 3 * E)).chunk(2, dim=-1)
    else:
        q = linear(query, *part(0, E))
        k = linear(key, *part(E, 2 * E))
        v = linear(value, *part(2 * E, 3 * E))

    def heads(t):
        return t.reshape(B, t.shape[1], H, E // H).transpose(1, 2)
    o = torch.nn.functional.scaled_dot_product_attention(
        heads(q), heads(k), heads(v), dropout_p=mod.dropout if mod.training else 0.0, is_causal=is_causal)
    o = o.transpose(1, 2).reshape(B, L, E)
    o = linear(o, mod.out_proj.weight, mod.out_proj.bias)
    return o.transpose(0, 1) if not mod.batch_first else o


class F32MultiheadAttention(torch.nn.MultiheadAttention):
    """``nn.MultiheadAttention`` whose input / output projections run on :func:`linear_f32`
    and whose core is SDPA -- the path torch's own ``multi_head_attention_forward`` takes
    with ``need_weights=False`` (what ``nn.TransformerDecoderLayer`` passes, helper:40-44).
    Anything else (weights requested, masks, separate k/v dims, bias_k, add_zero_attn, CPU,
    non-f32) runs the stock module."""

    def forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None,
                average_attn_weights=True, is_causal=False):
        stock = (need_weights or key_padding_mask is not None or attn_mask is not None or not query.is_cuda
                 or query.dtype != torch.float32 or not self._qkv_same_embed_dim or self.bias_k is not None
                 or self.add_zero_attn or query.dim() != 3)
        if stock:
            return super().forward(query, key, value, key_padding_mask=key_padding_mask, need_weights=need_weights,
                                   attn_mask=attn_mask, average_attn_weights=average_attn_weights, is_causal=is_causal)
        return _mha_projected(self, query, key, value, is_causal, _LinearF32.apply), None


_F32_SWAP = {torch.nn.Linear: F32Linear, torch.nn.modules.linear.NonDynamicallyQuantizableLinear: F32Linear,
             torch.nn.MultiheadAttention: F32MultiheadAttention}


def use_f32_kernels(module: torch.nn.Module, on: bool = True) -> int:
    """Route an f32 module's linears and attention projections to the f32 MFMA GEMM by
    swapping the class of its ``nn.Linear`` / ``nn.MultiheadAttention`` submodules (and back
    with ``on=False``).  Parameters, buffers and state_dict keys are untouched, and nothing
    outside ``module`` changes (no global patch of ``torch.nn.functional``).  Returns the
    number of submodules switched."""
    n = 0
    for mod in module.modules():
        if on:
            cls = _F32_SWAP.get(type(mod))
            if cls is not None:
                mod._mipipe_f32_orig_cls = type(mod)
                mod.__class__ = cls
                n += 1
        elif type(mod) in (F32Linear, F32MultiheadAttention):
            mod.__class__ = mod.__dict__.pop("_mipipe_f32_orig_cls")
            n += 1
    return n
