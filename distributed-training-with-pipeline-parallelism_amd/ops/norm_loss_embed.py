"""Normalisation (+ fused residual add / dropout), fused softmax cross-entropy and the
embeddings: the ops of csrc/bindings/norm_loss_embed.cpp with their CPU reference paths."""
from __future__ import annotations

from typing import Optional

import torch

from ._base import _cpu_dropout_mask, _ext, _gpu

__all__ = ["norm_fwd", "norm_bwd", "xent_fwd_bwd", "embed_fwd", "embed_bwd"]


# ======================================================================================
# normalisation (+ fused residual add / dropout)
# ======================================================================================
def norm_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
             branch: Optional[torch.Tensor] = None, kind: str = "layernorm", eps: float = 1e-5,
             p_drop: float = 0.0, seed: int = 0, y=None, s=None, mean=None, rstd=None):
    """s = x + dropout(branch) (if branch given); y = norm(s) * w (+ bias).  Returns (y, s, mean, rstd)."""
    rms = kind == "rmsnorm"
    D = x.shape[-1]
    rows = x.numel() // D
    if y is None:
        y = torch.empty_like(x)
    if branch is not None and s is None:
        s = torch.empty_like(x)
    if rstd is None:
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    if mean is None and not rms:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    if _gpu(x):
        _ext().norm_fwd(rms, x, branch, w, bias, s if branch is not None else None, y, mean, rstd, float(eps),
                        float(p_drop), int(seed))
        return y, (s if branch is not None else x), mean, rstd
    xf = x.float()
    if branch is not None:
        bf = branch.float()
        if p_drop > 0:
            bf = bf * _cpu_dropout_mask(bf.shape, p_drop, seed, x.device)
        xf = (xf + bf).to(x.dtype).float()
        s.copy_(xf.to(x.dtype))
    src = xf.reshape(rows, D)
    mu = torch.zeros(rows) if rms else src.mean(-1)
    var = (src - mu[:, None]).pow(2).mean(-1)
    r = torch.rsqrt(var + eps)
    out = (src - mu[:, None]) * r[:, None] * w.float()
    if bias is not None:
        out = out + bias.float()
    y.copy_(out.reshape(x.shape).to(y.dtype))
    rstd.copy_(r)
    if not rms:
        mean.copy_(mu)
    return y, (s if branch is not None else x), mean, rstd


def norm_bwd(dy: torch.Tensor, s: torch.Tensor, w: torch.Tensor, mean, rstd, kind: str = "layernorm",
             dres: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
             dbias: Optional[torch.Tensor] = None, p_drop: float = 0.0, seed: int = 0, ds=None, dbranch=None,
             want_branch: bool = False, colsum_dres: Optional[torch.Tensor] = None,
             colsum_ds: Optional[torch.Tensor] = None, colsum_branch: Optional[torch.Tensor] = None):
    """ds = d(norm input) (+ dres); dw/dbias (f32) accumulate.  Optionally also accumulates
    the column sums of ``dres`` and of ``ds`` (f32) -- the bias grads of the projections
    around this residual point -- in the same pass; ``colsum_branch`` (needs
    ``want_branch``): the column sums of the returned branch gradient (= ds without
    dropout, ds * mask with it).  Returns (ds, dbranch)."""
    rms = kind == "rmsnorm"
    D = dy.shape[-1]
    rows = dy.numel() // D
    if ds is None:
        ds = torch.empty_like(dy)
    need_branch = want_branch and p_drop > 0
    if need_branch and dbranch is None:
        dbranch = torch.empty_like(dy)
    if colsum_branch is not None:
        if not want_branch or colsum_ds is not None:
            raise ValueError("colsum_branch needs want_branch and excludes colsum_ds")
    if _gpu(dy):
        cs_ds = colsum_branch if colsum_branch is not None else colsum_ds
        rc = _ext().norm_bwd(rms, dy, s, w, mean, rstd, dres, ds, dbranch if need_branch else None, dw, dbias,
                             float(p_drop), int(seed), colsum_dres, cs_ds)
        out_branch = dbranch if need_branch else (ds if want_branch else None)
        if rc == -3:     # no fused column sums for this shape: separate passes
            if colsum_dres is not None:
                _ext().colsum(dres, colsum_dres)
            if cs_ds is not None:
                _ext().colsum(out_branch if colsum_branch is not None else ds, cs_ds)
        return ds, out_branch
    d = dy.float().reshape(rows, D)
    x = s.float().reshape(rows, D)
    mu = torch.zeros(rows) if rms else mean.float()
    xh = (x - mu[:, None]) * rstd[:, None]
    g = d * w.float()
    s1 = torch.zeros(rows, 1) if rms else g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    v = rstd[:, None] * (g - s1 - xh * s2)
    if dres is not None:
        v = v + dres.float().reshape(rows, D)
    ds.copy_(v.reshape(dy.shape).to(ds.dtype))
    if colsum_dres is not None:
        colsum_dres += dres.float().reshape(rows, D).sum(0)
    if colsum_ds is not None:
        colsum_ds += ds.float().reshape(rows, D).sum(0)
    if dw is not None:
        dw += (d * xh).sum(0)
    if dbias is not None:
        dbias += d.sum(0)
    if need_branch:
        m = _cpu_dropout_mask(dy.shape, p_drop, seed, dy.device)
        dbranch.copy_((v.reshape(dy.shape) * m).to(dbranch.dtype))
        if colsum_branch is not None:
            colsum_branch += dbranch.float().reshape(rows, D).sum(0)
        return ds, dbranch
    if colsum_branch is not None:
        colsum_branch += ds.float().reshape(rows, D).sum(0)
    return ds, (ds if want_branch else None)


# ======================================================================================
# fused softmax cross-entropy
# ======================================================================================
def xent_fwd_bwd(logits: torch.Tensor, target: torch.Tensor, vocab: int, grad_scale: float,
                 ignore_index: int = -100, write_grad: bool = True, loss: Optional[torch.Tensor] = None):
    """Per-row CE loss (f32 [T]); if write_grad, logits are overwritten IN PLACE by
    (softmax - onehot) * grad_scale (padded vocab columns -> 0)."""
    Vp = logits.shape[-1]
    T = logits.numel() // Vp
    if loss is None:
        loss = torch.empty(T, device=logits.device, dtype=torch.float32)
    if _gpu(logits):
        _ext().xent(logits, target, loss, int(vocab), float(grad_scale), int(ignore_index), bool(write_grad))
        return loss
    lg = logits.float().reshape(T, Vp)[:, :vocab]
    tg = target.reshape(T)
    lse = torch.logsumexp(lg, -1)
    valid = tg != ignore_index
    tsafe = torch.where(valid, tg, torch.zeros_like(tg))
    l = lse - lg.gather(1, tsafe[:, None])[:, 0]
    loss.copy_(torch.where(valid, l, torch.zeros_like(l)))
    if write_grad:
        p = torch.softmax(lg, -1)
        p[torch.arange(T), tsafe] -= 1.0
        p = p * grad_scale * valid[:, None].float()
        out = torch.zeros(T, Vp)
        out[:, :vocab] = p
        logits.copy_(out.reshape(logits.shape).to(logits.dtype))
    return loss


# ======================================================================================
# embeddings
# ======================================================================================
def embed_fwd(idx: torch.Tensor, wte: torch.Tensor, wpe: Optional[torch.Tensor], S: int, pos_offset: int = 0,
              out: Optional[torch.Tensor] = None, positions: Optional[torch.Tensor] = None):
    """``positions`` (int32 [T] on wte's device): one token per sequence, row t at position
    ``positions[t]`` read on the device (clamped to the table) instead of ``t % S +
    pos_offset`` -- the decode step of a ragged batch (csrc/kernels/generate.hip)."""
    T = idx.numel()
    D = wte.shape[1]
    if out is None:
        out = torch.empty(T, D, device=wte.device, dtype=wte.dtype)
    if positions is not None:
        if positions.dtype != torch.int32 or positions.device != wte.device or positions.numel() != T:
            raise ValueError("embed_fwd: positions must be int32 [T] on wte's device")
        if _gpu(wte):
            _ext().embed_pos(idx.reshape(-1), positions.reshape(-1), wte, wpe, out)
            return out
        e = wte.float()[idx.reshape(-1).clamp(0, wte.shape[0] - 1)]
        if wpe is not None:
            e = e + wpe.float()[positions.reshape(-1).long().clamp(0, wpe.shape[0] - 1)]
        out.copy_(e.to(out.dtype))
        return out
    if _gpu(wte):
        _ext().embed_fwd(idx.reshape(-1), wte, wpe, out, int(S), int(pos_offset))
        return out
    e = wte.float()[idx.reshape(-1)]
    if wpe is not None:
        pos = torch.arange(T) % S + pos_offset
        e = e + wpe.float()[pos]
    out.copy_(e.to(out.dtype))
    return out


def embed_bwd(idx: torch.Tensor, dout: torch.Tensor, dwte: torch.Tensor, dwpe: Optional[torch.Tensor], S: int,
              pos_offset: int = 0):
    if _gpu(dout):
        _ext().embed_bwd(idx.reshape(-1), dout, dwte, dwpe, int(S), int(pos_offset))
        return
    T = idx.numel()
    d = dout.float().reshape(T, -1)
    dwte.index_add_(0, idx.reshape(-1), d)
    if dwpe is not None:
        pos = torch.arange(T) % S + pos_offset
        dwpe.index_add_(0, pos, d)
