"""Float64 reference of append attention (ops.attn_append) and the shared test inputs.

The reference is one explicit masked softmax per (sequence, token, head): it shares no code
with the op's CPU path, which batches the tokens of a sequence through matrix products."""
import math

import torch

PAD = 8


def attn_append_ref(q, k_cache, v_cache, base, counts, T, H, Hkv, D, scale=None):
    """q [B*T, >= H*D], caches [B, Smax, >= Hkv*D], base / counts: host ints [B] (counts None
    = T) -> float64 [B*T, H*D].  Query (b, t), t < counts[b], sees the keys j <= base[b] + t;
    a query with t >= counts[b] gets a zero row.  base and counts are clamped as the kernel
    clamps them."""
    B, Smax = k_cache.shape[0], k_cache.shape[1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    rep = H // Hkv
    out = torch.zeros(B * T, H * D, dtype=torch.float64)
    for b in range(B):
        n0 = max(0, min(int(base[b]), Smax))
        c = T if counts is None else int(counts[b])
        c = max(0, min(c, T, Smax - n0))
        for t in range(c):
            n = n0 + t + 1                                    # the keys 0 .. base + t
            for h in range(H):
                kv = h // rep
                qv = q[b * T + t, h * D:(h + 1) * D].double()
                K = k_cache[b, :n, kv * D:(kv + 1) * D].double()
                V = v_cache[b, :n, kv * D:(kv + 1) * D].double()
                s = (K @ qv) * scale
                w = torch.exp(s - s.max())
                out[b * T + t, h * D:(h + 1) * D] = (w / w.sum()) @ V
    return out


def bases_counts(T, smax):
    """The (base, counts) cases of the GPU test for B = 2: the empty cache; one cached key
    beside a long cache; a partial row beside a chunk edge crossed inside the new tokens; a
    full cache beside a row with nothing to do."""
    return [([0, 0], None), ([1, 300], None), ([255, 5], [T, max(T - 1, 0)]), ([smax - T, 256], [T, 0])]


def make_inputs(T, H, Hkv, D, base, counts, smax, seed=0, dtype=torch.bfloat16):
    """CPU tensors in the model's layout: q = the leading columns of packed qkv rows, caches
    behind PAD leading columns; cache rows at or beyond base + counts and q rows with
    t >= counts hold NaN."""
    g = torch.Generator().manual_seed(seed)
    nb = len(base)
    qkv = torch.randn(nb * T, (H + 2 * Hkv) * D, generator=g).to(dtype)
    kbuf = torch.randn(nb, smax, PAD + Hkv * D, generator=g).to(dtype)
    vbuf = torch.randn(nb, smax, PAD + Hkv * D, generator=g).to(dtype)
    for b in range(nb):
        c = T if counts is None else counts[b]
        kbuf[b, base[b] + c:] = float("nan")
        vbuf[b, base[b] + c:] = float("nan")
        qkv[b * T + c:(b + 1) * T] = float("nan")
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32)
    return qkv, kbuf, vbuf, torch.tensor(base, dtype=torch.int32), cnt
