"""Training attention (csrc/bindings/attention.cpp): forward, backward, the launch plan, the
document bounds of packed sequences, and the CPU masks of their reference paths."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ._base import LOG2E, _cpu_dropout_mask, _ext, _gpu

__all__ = ["attn_plan", "attn_fwd", "attn_bwd", "doc_bounds"]


def _heads(t: torch.Tensor, B: int, S: int, nh: int, D: int):
    """token-major [B*S, stride] view (first nh*D cols) -> [B, nh, S, D] f32"""
    return t[:, : nh * D].float().reshape(B, S, nh, D).permute(0, 2, 1, 3)


def _cpu_attn_mask(B, H, Sq, Sk, causal, device, doc_start=None):
    """True where the key is hidden.  With ``doc_start`` (int32 [B*S], clamped into [0, i] as
    the kernels do) the mask is per sequence, [B, 1, S, S]: key j hidden unless
    doc_start[i] <= j <= i."""
    if not causal:
        return None
    shift = Sk - Sq
    q = torch.arange(Sq)[:, None]
    k = torch.arange(Sk)[None, :]
    if doc_start is None:
        return (k > q + shift).to(device)
    ds = torch.minimum(doc_start.reshape(B, Sq).cpu().long().clamp_min(0), torch.arange(Sq)[None, :])
    return ((k > q)[None] | (k[None] < ds[:, :, None]))[:, None].to(device)


def _doc_check(name, q, B, Sq, Sk, D, causal, p_drop, dbias, arrays):
    """Argument checks of the document-masked path (ValueError, before any launch)."""
    if not causal:
        raise ValueError(f"{name}: the document mask needs causal attention")
    if Sq != Sk:
        raise ValueError(f"{name}: the document mask needs self-attention (Sq {Sq} != Sk {Sk})")
    if p_drop > 0:
        raise ValueError(f"{name}: the document mask does not support dropout (p_drop {p_drop})")
    if dbias is not None:
        raise ValueError(f"{name}: the document mask has no fused QKV-bias sums (dbias given)")
    if _gpu(q) and q.dtype != torch.bfloat16:
        raise ValueError(f"{name}: the document-masked kernels are bf16 only on the GPU (got {q.dtype})")
    if _gpu(q) and D not in (64, 128):
        raise ValueError(f"{name}: the document-masked kernels support head_dim 64 and 128 (got {D})")
    for nm, a in arrays:
        if a is None:
            raise ValueError(f"{name}: {nm} is required with a document mask")
        if a.dtype != torch.int32 or a.numel() != B * Sq or a.device != q.device or not a.is_contiguous():
            raise ValueError(f"{name}: {nm} must be a contiguous int32 tensor of B*S = {B * Sq} entries on q's "
                             f"device (got {a.dtype}, {tuple(a.shape)}, {a.device})")


def doc_bounds(tokens: torch.Tensor, eos: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(doc_start, doc_end), int32 [B*S], of ``tokens`` (int64 [B, S]): position i starts a
    document iff i == 0 or tokens[i-1] == eos, so the end-of-text token closes its own
    document; the last document of a row ends at S-1.  On the GPU one kernel, no host sync."""
    if tokens.dim() != 2 or tokens.dtype != torch.int64:
        raise ValueError(f"doc_bounds: tokens must be int64 [B, S] (got {tokens.dtype}, {tuple(tokens.shape)})")
    if _gpu(tokens):
        ds, de = _ext().doc_bounds(tokens.contiguous(), int(eos))
        return ds, de
    B, S = tokens.shape
    pos = torch.arange(S, device=tokens.device)[None, :].expand(B, S)
    is_eos = tokens == eos
    start = torch.ones_like(is_eos)
    start[:, 1:] = is_eos[:, :-1]
    ds = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 1).values
    end = is_eos.clone()
    end[:, -1] = True
    de = torch.cummin(torch.where(end, pos, torch.full_like(pos, S - 1)).flip(1), 1).values.flip(1)
    return ds.reshape(-1).to(torch.int32), de.reshape(-1).to(torch.int32)


def _cpu_attn_drop(B, H, Sq, Sk, p, seed, device):
    if p <= 0:
        return None
    return _cpu_dropout_mask((B, H, Sq, Sk), p, seed, device)


def attn_plan(B: int, Sq: int, Sk: int, H: int, Hkv: int, D: int, qs: int, ks: int, vs: int, os: int, causal: bool,
              drop: bool, env: Optional[dict] = None) -> dict:
    """What the bf16 :func:`attn_fwd` / :func:`attn_bwd` launch for a problem with row strides
    qs / ks / vs / os (elements) of q / k / v / o: ``{"fwd": launch, "bwd": [launch, ...]}``, a
    launch being ``{"kernel", "dp", "grid": (x, y), "lds"}`` (csrc/include/mp_attn_plan.h).
    ``env``: MIPIPE_ATTN_* switches over their defaults; None: the process environment.  Needs
    the built extension, not a GPU."""
    return _ext().attn_plan(int(B), int(Sq), int(Sk), int(H), int(Hkv), int(D), int(qs), int(ks), int(vs), int(os),
                            bool(causal), bool(drop), env=env)


def attn_fwd(q, k, v, o, lse, B: int, Sq: int, Sk: int, H: int, Hkv: int, D: int, causal: bool,
             scale: Optional[float] = None, p_drop: float = 0.0, seed: int = 0,
             doc_start: Optional[torch.Tensor] = None):
    """q/k/v/o: token-major 2-D views ([B*S, row_stride], head h at cols h*D).  lse: f32
    [B*H*Sq] (log2 units).  Writes o and lse.  ``doc_start`` (int32 [B*S]): the document mask
    of packed sequences, key j visible to query i iff doc_start[i] <= j <= i."""
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if doc_start is not None:
        _doc_check("attn_fwd", q, B, Sq, Sk, D, causal, p_drop, None, (("doc_start", doc_start),))
        if _gpu(q):
            _ext().attn_doc_fwd(q, k, v, o, lse, doc_start, B, Sq, H, Hkv, D, True, float(scale), 0.0)
            return o
    if _gpu(q):
        _ext().attn_fwd(q, k, v, o, lse, B, Sq, Sk, H, Hkv, D, bool(causal), float(scale), float(p_drop), int(seed))
        return o
    Q, K, V = _heads(q, B, Sq, H, D), _heads(k, B, Sk, Hkv, D), _heads(v, B, Sk, Hkv, D)
    rep = H // Hkv
    K, V = K.repeat_interleave(rep, 1), V.repeat_interleave(rep, 1)
    s = (Q @ K.transpose(-1, -2)) * scale
    mask = _cpu_attn_mask(B, H, Sq, Sk, causal, q.device, doc_start)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    l2 = torch.logsumexp(s, -1) * LOG2E
    p = torch.softmax(s, -1)
    dm = _cpu_attn_drop(B, H, Sq, Sk, p_drop, seed, q.device)
    if dm is not None:
        p = p * dm
    out = (p @ V).permute(0, 2, 1, 3).reshape(B * Sq, H * D)
    o[:, : H * D].copy_(out.to(o.dtype))
    lse.view(-1)[: B * H * Sq].copy_(l2.reshape(-1))
    return o


def attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B: int, Sq: int, Sk: int, H: int, Hkv: int, D: int, causal: bool,
             scale: Optional[float] = None, p_drop: float = 0.0, seed: int = 0, delta=None,
             dbias: Optional[torch.Tensor] = None, doc_start: Optional[torch.Tensor] = None,
             doc_end: Optional[torch.Tensor] = None):
    """Writes dq, dk, dv (token-major views like the inputs).  ``dbias`` (f32
    [(H + 2 Hkv) D]): also accumulate the QKV bias gradient (column sums of dq | dk | dv).
    ``doc_start`` / ``doc_end`` (int32 [B*S], both or neither): the document mask of
    :func:`attn_fwd`; the dK/dV kernel reads it as j <= i <= doc_end[j]."""
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if doc_start is not None or doc_end is not None:
        _doc_check("attn_bwd", q, B, Sq, Sk, D, causal, p_drop, dbias,
                   (("doc_start", doc_start), ("doc_end", doc_end)))
        if _gpu(q):
            if delta is None:
                delta = torch.empty(B * H * Sq, device=q.device, dtype=torch.float32)
            _ext().attn_doc_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, doc_start, doc_end, B, Sq, H, Hkv, D, True,
                                float(scale), 0.0)
            return dq, dk, dv
    if _gpu(q):
        if delta is None:
            delta = torch.empty(B * H * Sq, device=q.device, dtype=torch.float32)
        _ext().attn_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, B, Sq, Sk, H, Hkv, D, bool(causal),
                        float(scale), float(p_drop), int(seed), dbias)
        return dq, dk, dv
    rep = H // Hkv
    Q, K, V = _heads(q, B, Sq, H, D), _heads(k, B, Sk, Hkv, D), _heads(v, B, Sk, Hkv, D)
    dO, O = _heads(do, B, Sq, H, D), _heads(o, B, Sq, H, D)
    Kr, Vr = K.repeat_interleave(rep, 1), V.repeat_interleave(rep, 1)
    s = (Q @ Kr.transpose(-1, -2)) * scale
    mask = _cpu_attn_mask(B, H, Sq, Sk, causal, q.device, doc_start)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1)
    dm = _cpu_attn_drop(B, H, Sq, Sk, p_drop, seed, q.device)
    pd = p * dm if dm is not None else p
    dV = pd.transpose(-1, -2) @ dO
    dP = dO @ Vr.transpose(-1, -2)
    if dm is not None:
        dP = dP * dm
    delta_ = (dO * O).sum(-1, keepdim=True)
    dS = p * (dP - delta_)
    dQ = (dS @ Kr) * scale
    dK = (dS.transpose(-1, -2) @ Q) * scale
    dK = dK.reshape(B, Hkv, rep, Sk, D).sum(2)
    dV = dV.reshape(B, Hkv, rep, Sk, D).sum(2)
    dq[:, : H * D].copy_(dQ.permute(0, 2, 1, 3).reshape(B * Sq, H * D).to(dq.dtype))
    dk[:, : Hkv * D].copy_(dK.permute(0, 2, 1, 3).reshape(B * Sk, Hkv * D).to(dk.dtype))
    dv[:, : Hkv * D].copy_(dV.permute(0, 2, 1, 3).reshape(B * Sk, Hkv * D).to(dv.dtype))
    if dbias is not None:
        dbias[: H * D] += dq[:, : H * D].float().sum(0)
        dbias[H * D:(H + Hkv) * D] += dk[:, : Hkv * D].float().sum(0)
        dbias[(H + Hkv) * D:] += dv[:, : Hkv * D].float().sum(0)
    return dq, dk, dv
