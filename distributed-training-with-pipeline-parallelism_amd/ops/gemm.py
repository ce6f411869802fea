"""The bf16 GEMM engines (csrc/bindings/gemm.cpp) and the linear layers built on them: forward
with its fused epilogues, dX, dW; the hipBLASLt auto-picker of the plain shapes.  The switches
``GEMM_BACKEND`` and ``GEMM_V`` live here and nowhere else: another module reads them as
``gemm.GEMM_BACKEND`` when it runs, never through a copy made at import."""
from __future__ import annotations

import os
from typing import Optional

import torch

from ._base import (ACT, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RELU, EPI_BIAS_RES, EPI_DGELU, EPI_DRELU, EPI_NONE, EPI_RES,
                    _act_cpu, _act_grad_cpu, _cpu_dropout_mask, _ext, _gpu)
from .gemm_f32 import F32_BIAS, F32_BIAS_RELU, F32_BIAS_RES, F32_DRELU, F32_NONE, F32_RES, _gemm_f32

__all__ = ["GEMM_BACKEND", "GEMM_V", "plain_gemm_choices", "transpose", "linear", "linear_dx", "linear_dw"]

# GEMM backend for plain (epilogue-free) GEMMs on GPU: "hip" (default: our MFMA engines),
# "blas" (hipBLASLt through torch, also for the dW GEMMs) or "auto": each plain forward /
# dX GEMM shape is timed once on both (outside graph capture) and keeps the faster.
# hipBLASLt wins some isolated K = 768 - 3072 NT shapes by 5-12 %
# (profiles/r2_kernel_microbench.json) but not inside the GPT-2 / reference steps
# (tools/runs/archive/ab_plain_gemm.sh: 883.6K / 889.4K tok/s auto vs 889.9K / 888.1K hip), so "auto"
# stays opt-in.  Fused-epilogue GEMMs always use the HIP kernels.
GEMM_BACKEND = os.environ.get("MIPIPE_GEMM", "hip")
_PLAIN_BEST: dict = {}


def _plain_pick(key, run_hip, run_lib) -> str:
    """Backend of one plain GEMM shape: decided by timing both (3 runs each after a warm
    run, CUDA events) the first time the shape is seen outside graph capture."""
    if GEMM_BACKEND != "auto":
        return GEMM_BACKEND
    d = _PLAIN_BEST.get(key)
    if d is not None:
        return d
    if torch.cuda.is_current_stream_capturing():
        return "hip"
    t = {}
    for name, fn in (("hip", run_hip), ("blas", run_lib)):
        fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(3):
            fn()
        e.record()
        e.synchronize()
        t[name] = s.elapsed_time(e)
    d = "blas" if t["blas"] < 0.97 * t["hip"] else "hip"
    _PLAIN_BEST[key] = d
    return d


def plain_gemm_choices() -> dict:
    """{"fwd|dx MxNxK": backend} of the plain GEMM shapes decided so far (bench JSON)."""
    return {f"{k[0]} {k[1]}x{k[2]}x{k[3]}": v for k, v in sorted(_PLAIN_BEST.items())}
# GEMM engine: 2 = 8-wave glds engine (gemm2.hip) with fallback to 1 (gemm.hip) for
# combinations v2 does not instantiate; 1 = always gemm.hip.
GEMM_V = int(os.environ.get("MIPIPE_GEMM_V", "2"))


def _gemm(A, B, C, bias=None, residual=None, aux=None, transA=False, transB=False, epi=EPI_NONE, accum=False,
          alpha=1.0, cfg: int = -1, colsum=None, p_drop: float = 0.0, seed: int = 0):
    """``colsum`` (f32 [N]): also accumulate the column sums of the bf16 output (fused in
    the GEMM epilogue where the engine supports it, else one extra pass).  ``p_drop``
    (EPI_BIAS_RELU / EPI_DRELU, contiguous output): dropout after the activation / the
    dropout mask times the activation derivative, regenerated from (seed, element index)
    exactly as act_fwd / act_bwd do."""
    e = _ext()
    if GEMM_V >= 2:
        rc = e.gemm2(A, B, C, bias, residual, aux, bool(transA), bool(transB), int(epi), bool(accum), float(alpha),
                     int(cfg), colsum, float(p_drop), int(seed))
        if rc:
            if rc == 2 and colsum is not None:
                e.colsum(C, colsum)
            return C
    if p_drop > 0:
        raise RuntimeError("GEMM dropout epilogue needs the v2 engine for this shape")
    e.gemm(A, B, C, bias, residual, aux, bool(transA), bool(transB), int(epi), bool(accum), float(alpha))
    if colsum is not None:
        e.colsum(C, colsum)
    return C


def transpose(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x^T for a 2-D bf16 matrix (row-contiguous views allowed)."""
    if out is None:
        out = torch.empty(x.shape[1], x.shape[0], device=x.device, dtype=x.dtype)
    if _gpu(x):
        _ext().transpose(x, out)
    else:
        out.copy_(x.t())
    return out


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           aux: Optional[torch.Tensor] = None, p_drop: float = 0.0, seed: int = 0):
    """y = drop(act(x @ w^T + bias)) (+ residual).  x [T,K], w [N,K].  With an activation
    ``aux`` receives what the backward's dX epilogue needs (``linear_dx(act_input=aux)``):
    the pre-activation for ReLU, GELU's derivative at the pre-activation for GELU (one
    sigmoid serves both here; the backward then multiplies).  Unfused, a GELU aux goes to
    ``act_bwd(..., saved="grad")``, a ReLU aux to ``act_bwd(..., saved="pre")``.  ``p_drop``
    (ReLU only) applies the fused dropout of the reference FFN.  Returns (y, aux)."""
    if p_drop > 0 and act != "relu":
        raise ValueError("the fused GEMM dropout follows a ReLU epilogue")
    T, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(T, N, device=x.device, dtype=x.dtype)
    if act != "none" and aux is None:
        aux = torch.empty(T, N, device=x.device, dtype=x.dtype)
    if _gpu(x) and x.dtype == torch.float32:
        # the reference-precision path: f32 MFMA GEMM with the same fused epilogues
        if act not in ("none", "relu"):
            raise ValueError("f32 GEMM epilogues: ReLU only")
        if act == "relu":
            if bias is None or residual is not None:
                raise ValueError("activation epilogue needs a bias and no residual")
            _gemm_f32(x, w.t(), out, bias=bias, X=aux, epi=F32_BIAS_RELU, p_drop=p_drop, seed=seed)
        elif residual is not None:
            _gemm_f32(x, w.t(), out, bias=bias, R=residual, epi=F32_BIAS_RES if bias is not None else F32_RES)
        else:
            _gemm_f32(x, w.t(), out, bias=bias, epi=F32_BIAS if bias is not None else F32_NONE)
        return out, aux
    if _gpu(x):
        if act != "none":
            if bias is None or residual is not None:
                raise ValueError("activation epilogue needs a bias and no residual")
            _gemm(x, w, out, bias=bias, aux=aux, epi=EPI_BIAS_GELU if ACT[act] == 1 else EPI_BIAS_RELU,
                  p_drop=p_drop, seed=seed)
        elif residual is not None:
            _gemm(x, w, out, bias=bias, residual=residual, epi=EPI_BIAS_RES if bias is not None else EPI_RES)
        elif bias is not None:
            _gemm(x, w, out, bias=bias, epi=EPI_BIAS)
        else:
            run_hip = lambda: _gemm(x, w, out)
            run_lib = lambda: torch.mm(x, w.t(), out=out)
            (run_lib if _plain_pick(("fwd", T, N, K), run_hip, run_lib) == "blas" else run_hip)()
        return out, aux
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if act != "none":
        pre = y.to(x.dtype)
        aux.copy_(_act_grad_cpu(pre.float(), act) if ACT[act] == 1 else pre)
        y = _act_cpu(pre.float(), act)
        if p_drop > 0:
            y = y * _cpu_dropout_mask(y.shape, p_drop, seed, y.device)
    if residual is not None:
        y = y + residual.float()
    out.copy_(y.to(out.dtype))
    return out, aux


def _plain_dx_hip(dy, wt, out):
    T, K = out.shape
    N = dy.shape[1]
    if (T // 256) * (K // 192) < 128 and N >= 4096:
        acc = torch.zeros(T, K, device=dy.device, dtype=torch.float32)
        _gemm(dy, wt, acc, accum=True)
        out.copy_(acc)
    else:
        _gemm(dy, wt, out)
    return out


def linear_dx(dy: torch.Tensor, w: torch.Tensor, act_input: Optional[torch.Tensor] = None, act: str = "none",
              out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
              wt: Optional[torch.Tensor] = None, colsum: Optional[torch.Tensor] = None, p_drop: float = 0.0,
              seed: int = 0):
    """dx = dy @ w  (w [N,K]), optionally times act'(.) given by ``act_input`` -- what
    ``linear(act=...)`` saved in ``aux``: ReLU's pre-activation, or GELU's derivative itself
    -- and plus ``residual``.  With ``wt`` (= w^T, [K,N], kept by the param arena) the GEMM
    runs in the both-K-contiguous form on the v2 engine."""
    T, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty(T, K, device=dy.device, dtype=dy.dtype)
    if _gpu(dy) and dy.dtype == torch.float32:
        if act not in ("none", "relu"):
            raise ValueError("f32 GEMM epilogues: dReLU only")
        if act == "relu":
            if residual is not None:
                raise ValueError("dReLU epilogue takes no residual")
            _gemm_f32(dy, w, out, R=act_input, epi=F32_DRELU, p_drop=p_drop, seed=seed)
        elif residual is not None:
            _gemm_f32(dy, w, out, R=residual, epi=F32_RES)
        else:
            _gemm_f32(dy, w, out)
        if colsum is not None:
            _ext().colsum(out, colsum)
        return out
    if (_gpu(dy) and wt is not None and act == "none" and residual is None and colsum is None and
            _plain_pick(("dx", T, K, N), lambda: _plain_dx_hip(dy, wt, out), lambda: torch.mm(dy, w, out=out)) == "blas"):
        torch.mm(dy, w, out=out)
        return out
    if _gpu(dy) and wt is not None and GEMM_BACKEND != "blas":
        if act == "none" and residual is None and (T // 256) * (K // 192) < 128 and N >= 4096:
            # few output tiles, long reduction (a distributed-head chunk: [Tc, D] = dl[Tc, V] W):
            # split-K into an f32 buffer fills the chip; one cast pass at the end
            acc = torch.zeros(T, K, device=dy.device, dtype=torch.float32)
            _gemm(dy, wt, acc, accum=True)
            out.copy_(acc)
            return out
        if act != "none":
            _gemm(dy, wt, out, aux=act_input, epi=EPI_DGELU if ACT[act] == 1 else EPI_DRELU, colsum=colsum,
                  p_drop=p_drop, seed=seed)
        elif residual is not None:
            _gemm(dy, wt, out, residual=residual, epi=EPI_RES, colsum=colsum)
        else:
            _gemm(dy, wt, out, colsum=colsum)
        return out
    if _gpu(dy):
        if act != "none":
            _gemm(dy, w, out, aux=act_input, transB=True, epi=EPI_DGELU if ACT[act] == 1 else EPI_DRELU,
                  p_drop=p_drop, seed=seed)
        elif residual is not None:
            _gemm(dy, w, out, residual=residual, transB=True, epi=EPI_RES)
        elif GEMM_BACKEND == "blas":
            torch.mm(dy, w, out=out)
        else:
            _gemm(dy, w, out, transB=True)
        if colsum is not None:
            _ext().colsum(out, colsum)
        return out
    g = dy.float() @ w.float()
    if act != "none":
        g = g * (act_input.float() if ACT[act] == 1 else _act_grad_cpu(act_input.float(), act))
        if p_drop > 0:
            g = g * _cpu_dropout_mask(g.shape, p_drop, seed, g.device)
    if residual is not None:
        g = g + residual.float()
    out.copy_(g.to(out.dtype))
    if colsum is not None:
        colsum += out.float().sum(0)
    return out


def linear_dw(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, alpha: float = 1.0):
    """dw (f32 [N,K]) += alpha * dy^T @ x   (dy [T,N], x [T,K])."""
    if _gpu(dy) and dy.dtype == torch.float32:
        return _gemm_f32(dy.t(), x, dw, alpha=alpha, accumulate=True)
    if _gpu(dy):
        if GEMM_BACKEND == "blas":
            dw.add_(torch.mm(dy.t(), x, out_dtype=torch.float32), alpha=alpha)
        else:
            _gemm(dy, x, dw, transA=True, transB=True, accum=True, alpha=alpha)
        return dw
    dw += alpha * (dy.float().t() @ x.float())
    return dw
