"""The memory-bound ops and the optimizer (csrc/bindings/elementwise_optim.cpp): activations,
column sums, SwiGLU, RoPE, the dropout step counter, reductions, fused AdamW, casts."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ._base import ACT, _act_cpu, _act_grad_cpu, _cpu_dropout_mask, _ext, _gpu

__all__ = ["act_fwd", "act_bwd", "colsum", "swiglu_fwd", "swiglu_bwd", "rope_tables", "rope_", "set_dropout_step",
           "zero_", "mean", "sumsq", "adamw_", "cast_f32_bf16"]


# ======================================================================================
# elementwise
# ======================================================================================
def act_fwd(a: torch.Tensor, act: str, p_drop: float = 0.0, seed: int = 0, out=None):
    if out is None:
        out = torch.empty_like(a)
    if _gpu(a):
        _ext().act_fwd(a, out, ACT[act], float(p_drop), int(seed))
        return out
    y = _act_cpu(a.float(), act)
    if p_drop > 0:
        y = y * _cpu_dropout_mask(a.shape, p_drop, seed, a.device)
    out.copy_(y.to(out.dtype))
    return out


def act_bwd(dg: torch.Tensor, a: torch.Tensor, act: str, dbias: Optional[torch.Tensor] = None,
            p_drop: float = 0.0, seed: int = 0, out=None, saved: str = "pre"):
    """dA = dG * act'(.) (dropout mask regenerated from (seed, element index)), plus the
    column sums into ``dbias``.  ``saved`` says what ``a`` holds: "pre" -- the pre-activation
    (act_fwd's input; ReLU's aux from :func:`linear`) -- or "grad" -- act' itself, which is
    what ``linear(act="gelu_tanh")`` stores in its aux (the two forms are not
    interchangeable; passing a GELU aux as "pre" would silently give wrong gradients)."""
    if saved not in ("pre", "grad"):
        raise ValueError(f"saved must be 'pre' or 'grad', not {saved!r}")
    if out is None:
        out = torch.empty_like(dg)
    if saved == "grad":
        d = dg.float() * a.float()
        if p_drop > 0:
            if _gpu(dg):
                raise ValueError("the dropout mask with a saved derivative is fused into linear_dx's epilogue")
            d = d * _cpu_dropout_mask(a.shape, p_drop, seed, a.device)
        out.copy_(d.to(out.dtype))
        if dbias is not None:
            if _gpu(dg):
                _ext().colsum(out, dbias)
            else:
                dbias += out.float().reshape(-1, out.shape[-1]).sum(0)
        return out
    if _gpu(dg):
        _ext().act_bwd(dg, a, out, dbias, ACT[act], float(p_drop), int(seed))
        return out
    d = dg.float() * _act_grad_cpu(a.float(), act)
    if p_drop > 0:
        d = d * _cpu_dropout_mask(a.shape, p_drop, seed, a.device)
    out.copy_(d.to(out.dtype))
    if dbias is not None:
        dbias += out.float().reshape(-1, out.shape[-1]).sum(0)
    return out


def colsum(x: torch.Tensor, dbias: torch.Tensor):
    if _gpu(x):
        _ext().colsum(x, dbias)
        return dbias
    dbias += x.float().reshape(-1, x.shape[-1]).sum(0)
    return dbias


def swiglu_fwd(gu: torch.Tensor, out=None):
    T, F2 = gu.shape
    F = F2 // 2
    if out is None:
        out = torch.empty(T, F, device=gu.device, dtype=gu.dtype)
    if _gpu(gu):
        _ext().swiglu_fwd(gu, out)
        return out
    g, u = gu.float()[:, :F], gu.float()[:, F:]
    out.copy_((torch.nn.functional.silu(g) * u).to(out.dtype))
    return out


def swiglu_bwd(gu: torch.Tensor, dy: torch.Tensor, out=None):
    if out is None:
        out = torch.empty_like(gu)
    if _gpu(gu):
        _ext().swiglu_bwd(gu, dy, out)
        return out
    F = dy.shape[-1]
    g, u, d = gu.float()[:, :F], gu.float()[:, F:], dy.float()
    sg = torch.sigmoid(g)
    out[:, F:] = (d * g * sg).to(out.dtype)
    out[:, :F] = (d * u * sg * (1 + g * (1 - sg))).to(out.dtype)
    return out


def rope_tables(S: int, Dh: int, theta: float, device) -> Tuple[torch.Tensor, torch.Tensor]:
    inv = 1.0 / (theta ** (torch.arange(0, Dh, 2, dtype=torch.float64) / Dh))
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.cos(ang).float().to(device), torch.sin(ang).float().to(device)


def rope_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, S: int, H: int, Hkv: int, Dh: int,
          pos_offset: int = 0, inverse: bool = False):
    """In-place rotate-half RoPE on the q and k heads of a packed [T, (H+2Hkv)*Dh] buffer."""
    if _gpu(qkv):
        _ext().rope(qkv, cos, sin, int(S), int(H), int(Hkv), int(Dh), int(pos_offset), bool(inverse))
        return qkv
    T = qkv.shape[0]
    x = qkv.float().reshape(T, H + 2 * Hkv, Dh)
    pos = torch.arange(T) % S + pos_offset
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    if inverse:
        s = -s
    half = Dh // 2
    rot = x[:, : H + Hkv]
    a, b = rot[..., :half], rot[..., half:]
    new = torch.cat([a * c - b * s, b * c + a * s], -1)
    x[:, : H + Hkv] = new
    qkv.copy_(x.reshape(T, -1).to(qkv.dtype))
    return qkv


# ======================================================================================
# optimizer
# ======================================================================================
def set_dropout_step(step: int, device: Optional[torch.device] = None) -> None:
    """Set the training-step counter every dropout kernel mixes into its seed (device
    memory, stream-ordered on the current stream).  Issued once per step outside any
    captured graph, it lets HIP-graph replays draw a fresh mask each step.  No-op on CPU."""
    if device is not None and device.type != "cuda":
        return
    _ext().set_dropout_step(int(step))


def zero_(t: torch.Tensor) -> torch.Tensor:
    """t <- 0 (GPU: hipMemsetAsync on the current stream instead of an ATen fill kernel)."""
    if _gpu(t) and t.is_contiguous():
        _ext().zero_(t)
        return t
    return t.zero_()


def mean(x: torch.Tensor) -> torch.Tensor:
    """Mean of an f32 tensor as a 0-dim f32 tensor (GPU: one deterministic workgroup,
    optim.hip scaled_sum_kernel -- e.g. the microbatch's mean token loss)."""
    if _gpu(x) and x.dtype == torch.float32 and x.is_contiguous():
        out = torch.empty((), device=x.device, dtype=torch.float32)
        _ext().scaled_sum(x, 1.0 / max(1, x.numel()), out)
        return out
    return x.mean()


def sumsq(g: torch.Tensor, out: torch.Tensor):
    if _gpu(g):
        _ext().sumsq(g, out)
        return out
    out += (g.float() ** 2).sum()
    return out


def adamw_(p, g, m, v, w16, n_decay: int, lr: float, b1: float, b2: float, eps: float, wd: float, step: int,
           sumsq_buf=None, max_norm: float = 0.0, grad_scale: float = 1.0, zero_grad: bool = True):
    """Fused AdamW over flat f32 buffers; also refreshes the bf16 copy ``w16`` and zeroes g."""
    if _gpu(p):
        _ext().adamw(p, g, m, v, w16, int(n_decay), float(lr), float(b1), float(b2), float(eps), float(wd), int(step),
                     sumsq_buf, float(max_norm), float(grad_scale), bool(zero_grad))
        return
    coef = grad_scale
    if max_norm > 0 and sumsq_buf is not None:
        nrm = math.sqrt(float(sumsq_buf.item())) * grad_scale
        coef *= min(1.0, max_norm / (nrm + 1e-6))
    gr = g * coef
    m.mul_(b1).add_(gr, alpha=1 - b1)
    v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = (m / bc1) / ((v / bc2).sqrt() + eps)
    decay = torch.zeros_like(p)
    decay[:n_decay] = wd
    p.sub_(lr * (upd + decay * p))
    if zero_grad:
        g.zero_()
    if w16 is not None:
        w16.copy_(p.to(w16.dtype))


def cast_f32_bf16(src: torch.Tensor, dst: torch.Tensor):
    if _gpu(src):
        _ext().cast_f32_bf16(src, dst)
    else:
        dst.copy_(src.to(dst.dtype))
    return dst
