"""Independent numpy reference of the int8 KV-cache row format and float64 attention over it.

One row (one token of one sequence, K or V) of ``Hkv`` heads of dim ``D`` is ``W =
round_up(Hkv * D + 4 * Hkv, 16)`` bytes: ``Hkv * D`` int8 values head-major, ``Hkv`` little-endian
f32 scales, zero padding.  Per head, in f32: ``amax = max |x|``, ``scale = amax / 127``, ``inv =
127 / amax`` (both 0 for a zero head), ``q = clip(rint(x * inv), -127, 127)``.  Rows are packed and
unpacked through a byte view.  Imports nothing from the package under test."""
import math

import numpy as np


def row_bytes(Hkv, D):
    return (Hkv * D + 4 * Hkv + 15) // 16 * 16


def pack(x, Hkv, D):
    """x: float array [..., Hkv * D] -> int8 [..., W]"""
    x = np.asarray(x, dtype=np.float32)
    lead = x.shape[:-1]
    xh = x.reshape(lead + (Hkv, D))
    amax = np.abs(xh).max(-1).astype(np.float32)
    scale = (amax / np.float32(127.0)).astype(np.float32)
    inv = np.zeros_like(amax)
    nz = amax > 0
    inv[nz] = (np.float32(127.0) / amax[nz]).astype(np.float32)
    q = np.clip(np.rint((xh * inv[..., None]).astype(np.float32)), -127, 127).astype(np.int8)
    out = np.zeros(lead + (row_bytes(Hkv, D),), dtype=np.uint8)
    out[..., : Hkv * D] = q.reshape(lead + (Hkv * D,)).view(np.uint8)
    out[..., Hkv * D: Hkv * D + 4 * Hkv] = np.ascontiguousarray(scale.astype("<f4")).view(np.uint8).reshape(
        lead + (4 * Hkv,))
    return out.view(np.int8)


def unpack(rows, Hkv, D):
    """int8 [..., W] -> (q int8 [..., Hkv, D], scale f32 [..., Hkv], padding uint8 [..., npad])"""
    rows = np.ascontiguousarray(np.asarray(rows)).view(np.uint8)
    lead = rows.shape[:-1]
    assert rows.shape[-1] == row_bytes(Hkv, D)
    q = np.ascontiguousarray(rows[..., : Hkv * D]).view(np.int8).reshape(lead + (Hkv, D))
    scale = np.ascontiguousarray(rows[..., Hkv * D: Hkv * D + 4 * Hkv]).view("<f4").reshape(lead + (Hkv,))
    return q, scale, rows[..., Hkv * D + 4 * Hkv:]


def values(rows, Hkv, D):
    """the effective values, float64 [..., Hkv * D]"""
    q, scale, _ = unpack(rows, Hkv, D)
    return (q.astype(np.float64) * scale.astype(np.float64)[..., None]).reshape(q.shape[:-2] + (Hkv * D,))


def _attend(qv, K, V, scale):
    s = (K @ qv) * scale
    w = np.exp(s - s.max())
    return (w / w.sum()) @ V


def attn_decode_ref(q, k_rows, v_rows, lens, H, Hkv, D, scale=None):
    """q float [B, H*D], k_rows / v_rows int8 [B, Smax, W], lens host ints -> float64 [B, H*D]
    (a zero row for an empty sequence)"""
    q = np.asarray(q, dtype=np.float64)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    rep = H // Hkv
    B, Smax = k_rows.shape[0], k_rows.shape[1]
    out = np.zeros((B, H * D))
    for b in range(B):
        n = max(0, min(int(lens[b]), Smax))
        if n == 0:
            continue
        K, V = values(k_rows[b, :n], Hkv, D), values(v_rows[b, :n], Hkv, D)
        for h in range(H):
            kv = h // rep
            out[b, h * D:(h + 1) * D] = _attend(q[b, h * D:(h + 1) * D], K[:, kv * D:(kv + 1) * D],
                                                V[:, kv * D:(kv + 1) * D], scale)
    return out


def attn_append_ref(q, k_rows, v_rows, base, counts, T, H, Hkv, D, scale=None):
    """q float [B*T, H*D]; query (b, t), t < counts[b], sees the keys j <= base[b] + t; other
    rows are zero -> float64 [B*T, H*D]"""
    q = np.asarray(q, dtype=np.float64)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    rep = H // Hkv
    B, Smax = k_rows.shape[0], k_rows.shape[1]
    out = np.zeros((B * T, H * D))
    for b in range(B):
        n0 = max(0, min(int(base[b]), Smax))
        c = T if counts is None else int(counts[b])
        c = max(0, min(c, T, Smax - n0))
        if c == 0:
            continue
        K, V = values(k_rows[b, :n0 + c], Hkv, D), values(v_rows[b, :n0 + c], Hkv, D)
        for t in range(c):
            n = n0 + t + 1
            for h in range(H):
                kv = h // rep
                out[b * T + t, h * D:(h + 1) * D] = _attend(q[b * T + t, h * D:(h + 1) * D],
                                                            K[:n, kv * D:(kv + 1) * D], V[:n, kv * D:(kv + 1) * D],
                                                            scale)
    return out


def poison(rows, Hkv, D):
    """in place: payload -128, NaN scale bits, 0xFF padding (what no valid row holds)"""
    u = rows.view(np.uint8)
    u[..., : Hkv * D] = 0x80
    u[..., Hkv * D:] = 0xFF
    return rows
