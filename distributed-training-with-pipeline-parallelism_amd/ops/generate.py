"""The ops of KV-cache generation (csrc/bindings/generate.cpp): single-token and multi-token
attention over a cache, the fused RoPE + K/V append at a device-side position, and on-device
sampling with its CPU reference.

The int8 KV cache ("kv8", csrc/kernels/attention_kv8.hip): :func:`attn_decode`,
:func:`attn_append` and :func:`rope_kv_append` take ``torch.int8`` caches ``[B, Smax, W]`` in
the row format of :func:`kv_quantize` and pick the int8 kernels by the caches' dtype.  The
format's three functions (:func:`kv8_row_bytes`, :func:`kv_quantize`, :func:`kv_dequantize`)
are reached as ``ops.generate.<name>``: the names of ``ops`` itself are a pinned table."""
from __future__ import annotations

import math
from typing import Optional

import torch

from ._base import _ext, _gpu

__all__ = ["attn_decode_plan", "attn_decode", "attn_append_plan", "attn_append", "rope_kv_append", "sample"]


# ======================================================================================
# the int8 KV-cache row: payload | f32 scales | zero padding
# ======================================================================================
def kv8_row_bytes(Hkv: int, D: int) -> int:
    """Bytes ``W`` of one int8 cache row (one token of one sequence, K or V) of ``Hkv`` heads
    of dim ``D``: ``Hkv * D`` int8 values head-major, ``Hkv`` little-endian f32 scales, zero
    padding up to a multiple of 16."""
    return (int(Hkv) * int(D) + 4 * int(Hkv) + 15) // 16 * 16


def kv_quantize(x: torch.Tensor, Hkv: int, D: int) -> torch.Tensor:
    """x ``[..., Hkv * D]`` (the values a float cache would store) -> int8 ``[..., W]`` rows,
    ``W = kv8_row_bytes(Hkv, D)``.  Per head, all in f32: ``amax = max |x|``, ``scale = amax /
    127`` (0 for a zero head), ``inv = 127 / amax`` (0 for a zero head), ``q = clamp(
    round_half_even(x * inv), -127, 127)``; the effective value is ``q * scale``.  -128 is
    never written.  Pure tensor code, the same bits on every device and in the HIP kernel."""
    Hkv, D = int(Hkv), int(D)
    if x.shape[-1] != Hkv * D:
        raise ValueError(f"kv_quantize: the last dimension must be Hkv * D = {Hkv * D}, got {x.shape[-1]}")
    lead = x.shape[:-1]
    xf = x.detach().float().reshape(*lead, Hkv, D)
    amax = xf.abs().amax(dim=-1)
    # tensor divisors: dividing by a Python scalar is a multiplication by its reciprocal on the
    # GPU, an ulp away from the CPU's quotient in some rows (the rule of quantize_w8)
    c127 = torch.full_like(amax, 127.0)
    scale = amax / c127
    inv = torch.where(amax > 0, c127 / torch.where(amax > 0, amax, torch.ones_like(amax)), torch.zeros_like(amax))
    q = torch.round(xf * inv[..., None]).clamp_(-127, 127).to(torch.int8)
    out = torch.zeros(*lead, kv8_row_bytes(Hkv, D), dtype=torch.int8, device=x.device)
    out[..., : Hkv * D] = q.reshape(*lead, Hkv * D)
    out[..., Hkv * D: Hkv * D + 4 * Hkv] = scale.contiguous().view(torch.int8)
    return out


def kv_dequantize(rows: torch.Tensor, Hkv: int, D: int, dtype=torch.float32) -> torch.Tensor:
    """int8 rows ``[..., W]`` of :func:`kv_quantize` -> their effective values ``[..., Hkv * D]``
    (``q * scale`` in f32, then rounded to ``dtype``)."""
    Hkv, D = int(Hkv), int(D)
    if rows.dtype != torch.int8 or rows.shape[-1] != kv8_row_bytes(Hkv, D):
        raise ValueError(f"kv_dequantize: rows must be int8 [..., {kv8_row_bytes(Hkv, D)}], got {rows.dtype} "
                         f"{tuple(rows.shape)}")
    lead = rows.shape[:-1]
    q = rows[..., : Hkv * D].float().reshape(*lead, Hkv, D)
    scale = rows[..., Hkv * D: Hkv * D + 4 * Hkv].clone(memory_format=torch.contiguous_format).view(torch.float32)
    return (q * scale[..., None]).reshape(*lead, Hkv * D).to(dtype)


def _kv8(fn: str, k_cache: torch.Tensor, v_cache: torch.Tensor, Hkv: int, D: int) -> bool:
    """True for a pair of int8 caches (checked: both int8, rows of ``W`` bytes)."""
    if k_cache.dtype != torch.int8 and v_cache.dtype != torch.int8:
        return False
    W = kv8_row_bytes(Hkv, D)
    if k_cache.dtype != v_cache.dtype or k_cache.shape[-1] != W or v_cache.shape[-1] != W:
        raise ValueError(f"{fn}: int8 caches are a pair of [B, Smax, {W}] tensors (kv8_row_bytes(Hkv, D) bytes per "
                         f"row), got {k_cache.dtype} {tuple(k_cache.shape)} and {v_cache.dtype} {tuple(v_cache.shape)}")
    return True


def _cache_rows_f32(cache: torch.Tensor, b: int, n: int, Hkv: int, D: int, kv8: bool) -> torch.Tensor:
    """the first n rows of sequence b as f32 [Hkv, n, D] (the CPU reference paths)"""
    rows = kv_dequantize(cache[b, :n], Hkv, D) if kv8 else cache[b, :n, : Hkv * D].float()
    return rows.reshape(n, Hkv, D).permute(1, 0, 2)


def attn_decode_plan(B: int, Hkv: int, max_len: int) -> int:
    """Key splits :func:`attn_decode` picks (``splits=0``) for ``B`` sequences x ``Hkv`` KV
    heads over caches of up to ``max_len`` keys (csrc/kernels/attention_decode.hip)."""
    return int(_ext().attn_decode_plan(int(B), int(Hkv), int(max_len)))


def attn_decode(q, k_cache, v_cache, lens, o, H: int, Hkv: int, D: int, scale: Optional[float] = None,
                splits: int = 0, max_len: Optional[int] = None):
    """Attention of one new token per sequence over its KV cache.  q/o: [B, H*D] row views
    (q is a slice of the packed qkv row); k_cache/v_cache: [B, Smax, Hkv*D] views; lens:
    int32 [B] on q's device, the valid keys per sequence including the current token.
    Causal by construction: a decode query sees every cached key.  ``max_len`` (a host
    int >= max(lens), default Smax) sizes the GPU grid; ``splits``: 0 = the kernel's
    planner, n > 0 forces n key splits.  Rows at positions >= lens[b] never enter the
    result.  Writes o."""
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if D not in (64, 128) and _gpu(q):
        raise ValueError(f"attn_decode: head_dim {D} is not supported by the HIP kernel (64 or 128)")
    if H % Hkv or (_gpu(q) and H // Hkv > 8):
        raise ValueError(f"attn_decode: H = {H}, Hkv = {Hkv} is not supported (H % Hkv == 0, H / Hkv <= 8)")
    if lens.dtype != torch.int32 or lens.device != q.device:
        raise ValueError("attn_decode: lens must be an int32 tensor on q's device")
    B, Smax = q.shape[0], k_cache.shape[1]
    max_len = Smax if max_len is None else int(max_len)
    kv8 = _kv8("attn_decode", k_cache, v_cache, Hkv, D)
    if _gpu(q):
        _ext().attn_decode(q, k_cache, v_cache, lens, o, int(H), int(Hkv), int(D), max_len, float(scale), int(splits))
        return o
    rep = H // Hkv
    for b, n in enumerate(lens.tolist()):
        n = max(0, min(int(n), Smax))
        if n == 0:
            o[b, : H * D].zero_()
            continue
        Q = q[b, : H * D].float().reshape(H, 1, D)
        K = _cache_rows_f32(k_cache, b, n, Hkv, D, kv8).repeat_interleave(rep, 0)
        V = _cache_rows_f32(v_cache, b, n, Hkv, D, kv8).repeat_interleave(rep, 0)
        p = torch.softmax((Q @ K.transpose(-1, -2)) * scale, -1)
        o[b, : H * D].copy_((p @ V).reshape(H * D).to(o.dtype))
    return o


def attn_append_plan(B: int, T: int, Hkv: int, rep: int, max_len: int) -> int:
    """Key splits :func:`attn_append` picks (``splits=0``) for ``B`` sequences x ``T`` new
    tokens x ``Hkv`` KV heads of ``rep`` query heads each over caches of up to ``max_len``
    keys (csrc/kernels/attention_append.hip)."""
    return int(_ext().attn_append_plan(int(B), int(T), int(Hkv), int(rep), int(max_len)))


def attn_append(q, k_cache, v_cache, base, counts, o, T: int, H: int, Hkv: int, D: int,
                scale: Optional[float] = None, splits: int = 0, max_len: Optional[int] = None):
    """Attention of ``T`` new tokens per sequence over its KV cache.  q/o: [B*T, H*D] row
    views (q is a slice of the packed qkv rows; row ``b*T + t`` is new token t of sequence
    b); k_cache/v_cache: [B, Smax, Hkv*D] views that already hold the new tokens' rows at
    ``base[b] + t``; base: int32 [B] on q's device, the valid cache rows before this call
    (clamped to [0, Smax]); counts: int32 [B] on q's device or None (= T), how many of the
    row's T tokens are real (clamped to [0, min(T, Smax - base)]).  Query (b, t) with
    ``t < counts[b]`` sees the keys ``j <= base[b] + t``; a query with ``t >= counts[b]``
    gets a zero row.  Cache rows at or beyond ``base[b] + counts[b]`` never enter a result.
    ``max_len`` (a host int >= max(base + counts), default Smax) sizes the GPU grid;
    ``splits``: 0 = the kernel's planner, n > 0 forces n key splits.  Writes o."""
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if D not in (64, 128) and _gpu(q):
        raise ValueError(f"attn_append: head_dim {D} is not supported by the HIP kernel (64 or 128)")
    if H % Hkv or (_gpu(q) and H // Hkv > 8):
        raise ValueError(f"attn_append: H = {H}, Hkv = {Hkv} is not supported (H % Hkv == 0, H / Hkv <= 8)")
    B, Smax, T = k_cache.shape[0], k_cache.shape[1], int(T)
    if T < 1 or q.shape[0] != B * T or o.shape[0] != B * T:
        raise ValueError(f"attn_append: q/o must hold B * T = {B} * {T} rows")
    if base.dtype != torch.int32 or base.device != q.device or base.numel() != B:
        raise ValueError("attn_append: base must be an int32 [B] tensor on q's device")
    if counts is not None and (counts.dtype != torch.int32 or counts.device != q.device or counts.numel() != B):
        raise ValueError("attn_append: counts must be an int32 [B] tensor on q's device")
    max_len = Smax if max_len is None else int(max_len)
    kv8 = _kv8("attn_append", k_cache, v_cache, Hkv, D)
    if _gpu(q):
        _ext().attn_append(q, k_cache, v_cache, base, counts, o, T, int(H), int(Hkv), int(D), max_len, float(scale),
                           int(splits))
        return o
    rep = H // Hkv
    cl = [T] * B if counts is None else counts.tolist()
    for b, n0 in enumerate(base.tolist()):
        n0 = max(0, min(int(n0), Smax))
        c = max(0, min(int(cl[b]), T, Smax - n0))
        o[b * T + c:(b + 1) * T, : H * D].zero_()
        if c == 0:
            continue
        n = n0 + c
        Q = q[b * T:b * T + c, : H * D].float().reshape(c, H, D).permute(1, 0, 2)
        K = _cache_rows_f32(k_cache, b, n, Hkv, D, kv8).repeat_interleave(rep, 0)
        V = _cache_rows_f32(v_cache, b, n, Hkv, D, kv8).repeat_interleave(rep, 0)
        s = (Q @ K.transpose(-1, -2)) * scale
        hidden = torch.arange(n)[None, :] > (n0 + torch.arange(c))[:, None]
        p = torch.softmax(s.masked_fill(hidden, float("-inf")), -1)
        o[b * T:b * T + c, : H * D].copy_((p @ V).permute(1, 0, 2).reshape(c, H * D).to(o.dtype))
    return o


# ======================================================================================
# the ragged decode step: K/V append at a device-side position, on-device sampling
# ======================================================================================
def rope_kv_append(qkv: torch.Tensor, cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], k_cache: torch.Tensor,
                   v_cache: torch.Tensor, pos: torch.Tensor, active: Optional[torch.Tensor], H: int, Hkv: int, Dh: int,
                   rope: bool = True, T: int = 1, counts: Optional[torch.Tensor] = None):
    """``T`` new tokens per sequence (default one).  qkv: packed [B*T, (H + 2 Hkv) * Dh] rows,
    row ``b*T + t`` being token t of sequence b at position ``p = pos[b] + t``; pos: int32 [B]
    on qkv's device (positions are clamped to [0, Smax - 1]); active: uint8 [B] or None (all
    active); counts: int32 [B] or None (all T): only rows ``t < counts[b]`` are touched.  For
    such a row of an active sequence: q is rotated in place at position p (``rope``), k is
    rotated and written to ``k_cache[b, p]`` (the k columns of qkv keep their unrotated
    values), v is copied to ``v_cache[b, p]``.  The rotation is :func:`rope_`'s at
    ``pos_offset = p``, bit for bit.  Any other row is left alone: nothing is written for it."""
    T = int(T)
    if T < 1 or qkv.shape[0] % T:
        raise ValueError(f"rope_kv_append: {qkv.shape[0]} qkv rows are no multiple of T = {T}")
    B, Smax = qkv.shape[0] // T, k_cache.shape[1]
    if counts is not None and (counts.dtype != torch.int32 or counts.device != qkv.device or counts.numel() != B):
        raise ValueError("rope_kv_append: counts must be int32 [B] on qkv's device")
    if pos.dtype != torch.int32 or pos.device != qkv.device or pos.numel() != B:
        raise ValueError("rope_kv_append: pos must be int32 [B] on qkv's device")
    if active is not None and (active.dtype != torch.uint8 or active.device != qkv.device or active.numel() != B):
        raise ValueError("rope_kv_append: active must be uint8 [B] on qkv's device")
    if rope and (cos is None or sin is None or cos.shape[0] < Smax or sin.shape[0] < Smax):
        raise ValueError(f"rope_kv_append: the RoPE tables need at least Smax = {Smax} rows")
    if _gpu(qkv) and Dh not in (64, 128):
        raise ValueError(f"rope_kv_append: head_dim {Dh} is not supported by the HIP kernel (64 or 128)")
    kv8 = _kv8("rope_kv_append", k_cache, v_cache, Hkv, Dh)
    if _gpu(qkv):
        _ext().rope_kv_append(qkv, cos if rope else None, sin if rope else None, k_cache, v_cache, pos, active,
                              int(H), int(Hkv), int(Dh), bool(rope), T, counts)
        return qkv
    half = Dh // 2
    tt = torch.arange(T).repeat(B)                                   # token index of every row
    bb = torch.arange(B).repeat_interleave(T)                        # ... and its sequence
    p = (pos.long().clamp(0, Smax - 1)[bb] + tt).clamp(max=Smax - 1)
    on = torch.ones(B * T, dtype=torch.bool)
    if active is not None:
        on &= active.reshape(-1)[bb] != 0
    if counts is not None:
        on &= tt < counts.long()[bb]
    rows = torch.nonzero(on)[:, 0]
    if rows.numel() == 0:
        return qkv
    x = qkv[rows].float().reshape(-1, H + 2 * Hkv, Dh)
    if rope:
        c, s = cos[p[rows]][:, None, :].float(), sin[p[rows]][:, None, :].float()
        a, b = x[:, : H + Hkv, :half], x[:, : H + Hkv, half:]
        rot = torch.cat([a * c - b * s, b * c + a * s], -1)
    else:
        rot = x[:, : H + Hkv]
    if rope:
        qkv[rows, : H * Dh] = rot[:, :H].reshape(-1, H * Dh).to(qkv.dtype)
    if kv8:
        # the rows a cache of qkv's dtype would hold, quantised: all W bytes of a row are written
        k_cache[bb[rows], p[rows]] = kv_quantize(rot[:, H:].reshape(-1, Hkv * Dh).to(qkv.dtype), Hkv, Dh)
        v_cache[bb[rows], p[rows]] = kv_quantize(x[:, H + Hkv:].reshape(-1, Hkv * Dh).to(qkv.dtype), Hkv, Dh)
        return qkv
    k_cache[bb[rows], p[rows], : Hkv * Dh] = rot[:, H:].reshape(-1, Hkv * Dh).to(k_cache.dtype)
    v_cache[bb[rows], p[rows], : Hkv * Dh] = x[:, H + Hkv:].reshape(-1, Hkv * Dh).to(v_cache.dtype)
    return qkv


def _sample_cpu(z: torch.Tensor, u: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    """f32 reference of the sampling rule (csrc/kernels/generate.hip) on z = logits[:, :V]."""
    B, V = z.shape
    if temperature == 0:
        return z.argmax(-1)
    z = z / torch.tensor(temperature, dtype=torch.float32) + 0.0
    keep = torch.ones_like(z, dtype=torch.bool)
    if 0 < top_k < V:
        keep = z >= z.topk(int(top_k), dim=-1).values[:, -1:]
    w = torch.exp(z - z.max(-1, keepdim=True).values) * keep
    if top_p < 1.0:
        need = torch.tensor(top_p, dtype=torch.float32) * w.sum(-1)
        for b in range(B):
            vals, inv = torch.unique(z[b][keep[b]], return_inverse=True)         # ascending
            mass = torch.zeros(vals.numel()).index_add_(0, inv, w[b][keep[b]])
            above = mass.flip(0).cumsum(0).flip(0)                                 # mass of {z >= vals[i]}
            ok = torch.nonzero(above >= need[b])[:, 0]
            t = vals[int(ok.max())] if ok.numel() else vals[0]
            keep[b] &= z[b] >= t
        w = w * keep
    c = w.cumsum(-1)
    hit = keep & (c > (u.float() * c[:, -1])[:, None])
    idx = torch.arange(V).expand(B, V)
    first = torch.where(hit, idx, torch.full_like(idx, V)).min(-1).values
    last = torch.where(keep, idx, torch.full_like(idx, -1)).max(-1).values
    return torch.where(first < V, first, last).clamp(0, V - 1)


def sample(logits: torch.Tensor, vocab: int, u: torch.Tensor, temperature: float = 0.0, top_k: int = 0,
           top_p: float = 1.0, done: Optional[torch.Tensor] = None, stop_token: int = -1, pad_token: int = 0,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One token id per row of ``logits`` [B, Vp] (bf16 or f32 rows, any row stride) over the
    first ``vocab`` columns only, in f32 with z = logit / temperature:

    1. ``temperature == 0``: argmax, ties to the lowest index;
    2. ``top_k`` (0 = off): keep z >= the k-th largest z (ties at the threshold all kept);
    3. ``top_p`` (1 = off): over the kept set, keep z >= the largest z whose upper set has
       at least ``top_p`` of the mass (ties kept whole);
    4. the smallest kept j whose running sum of exp(z - max), in index order, exceeds
       ``u[b]`` times the total (``u``: f32 [B] in [0, 1)).

    ``done`` (uint8 [B], optional): a row already done gets ``pad_token``; a row that emits
    ``stop_token`` sets ``done[b]``.  Writes and returns ``out`` (int64 [B])."""
    if logits.dim() != 2:
        raise ValueError("sample: logits must be [B, Vp]")
    B, Vp = logits.shape
    vocab, top_k = int(vocab), int(top_k or 0)
    top_p = 1.0 if top_p is None else float(top_p)
    if not 1 <= vocab <= Vp:
        raise ValueError(f"sample: vocab {vocab} outside [1, Vp = {Vp}]")
    if not temperature >= 0 or top_k < 0 or not 0.0 < top_p <= 1.0:
        raise ValueError("sample: needs temperature >= 0, top_k >= 0 and 0 < top_p <= 1")
    if u.dtype != torch.float32 or u.device != logits.device or u.numel() != B:
        raise ValueError("sample: u must be f32 [B] on the logits' device")
    if done is not None and (done.dtype != torch.uint8 or done.device != logits.device or done.numel() != B):
        raise ValueError("sample: done must be uint8 [B] on the logits' device")
    if out is None:
        out = torch.empty(B, device=logits.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or out.device != logits.device or out.numel() != B:
        raise ValueError("sample: out must be int64 [B] on the logits' device")
    if _gpu(logits):
        _ext().sample(logits, vocab, u, float(temperature), top_k, top_p, done, int(stop_token), int(pad_token), out)
        return out
    tok = _sample_cpu(logits[:, :vocab].float(), u.reshape(-1), float(temperature), top_k, top_p)
    if done is not None:
        was = done.reshape(-1) != 0
        tok = torch.where(was, torch.full_like(tok, int(pad_token)), tok)
        done.reshape(-1)[(~was) & (tok == int(stop_token))] = 1
    out.copy_(tok.reshape(out.shape))
    return out
