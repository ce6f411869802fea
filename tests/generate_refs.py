"""Float64 references of the generation kernels (csrc/kernels/generate.hip) and the shared
list of sampler cases.  Not a test file: test_generate_refs_cpu.py checks these references
against torch, test_generate_kernels_gpu.py holds the kernels to them.

``sample_ref`` also returns the case's **decision margin**: the smallest distance, as a
share of the total mass W of the set it concerns, between any quantity the rule compares
and what it compares it with -- the mass of the upper set against ``top_p`` on both sides of
the deciding threshold, and ``u * W`` against both edges of the chosen token's interval.
Counting comparisons (top-k) are exact and have no margin.  Every listed case has a margin
>= ``MARGIN`` = 1e-4 by construction (test_generate_refs_cpu.py asserts it): that is above
the worst-case f32 error of a blocked sum of 50 304 non-negative terms, (197 + 8) * 2^-24
~ 1.2e-5 plus 2^-22 per exp, so a correct f32 kernel decides every case the way float64
does and the GPU tests may ask for the reference's token exactly.

Case construction: a random permutation picks 40 "top" tokens with logits 4 + i ln 0.8
(geometric probabilities), every other token gets -30 + 0.5 randn, everything is rounded to
bf16 (so bf16 and f32 kernels read the same values).  ``top_p`` is a midpoint between two
consecutive cumulative masses of the first 20 ranks at the case's temperature and top-k;
``u`` is the midpoint of a kept token's interval of the index-ordered CDF.
"""
import functools
import math
from dataclasses import dataclass
from typing import List, Optional

import torch

MARGIN = 1e-4
SIZES = [(60, 64), (4093, 4096), (50257, 50304)]        # (V, Vp)
PAD_LOGIT = 100.0                                        # what the padded columns hold: attractive


# ------------------------------------------------------------------------------ sampler
def _kept(z: torch.Tensor, top_k: int, top_p: float):
    """z: float64 [V] -> (kept mask, margin of the top-p decision as a share of W)."""
    V = z.numel()
    keep = torch.ones(V, dtype=torch.bool)
    margin = math.inf
    if 0 < top_k < V:
        keep = z >= torch.sort(z, descending=True).values[top_k - 1]
    if top_p < 1.0:
        w = torch.where(keep, torch.exp(z - z.max()), torch.zeros_like(z))
        W = float(w.sum())
        vals, inv = torch.unique(z[keep], return_inverse=True)                  # ascending
        mass = torch.zeros(vals.numel(), dtype=torch.float64).index_add_(0, inv, w[keep])
        above = mass.flip(0).cumsum(0).flip(0)                                   # mass of {z >= vals[i]}
        ok = torch.nonzero(above >= top_p * W)[:, 0]
        i = int(ok.max())                                                        # above[0] = W >= top_p W
        margin = (float(above[i]) - top_p * W) / W
        if i + 1 < vals.numel():
            margin = min(margin, (top_p * W - float(above[i + 1])) / W)
        keep = keep & (z >= vals[i])
    return keep, margin


def sample_ref(logits: torch.Tensor, u: float, temperature: float, top_k: int = 0, top_p: float = 1.0):
    """The sampling rule of ops.sample in float64 on one row ``logits`` [V] (the real
    vocabulary only).  Returns (token, decision margin, kept mask)."""
    x = logits.double()
    V = x.numel()
    if temperature == 0:
        return int(torch.argmax(x)), math.inf, x == x.max()       # torch.argmax: the first maximum
    z = x / float(torch.tensor(temperature, dtype=torch.float32))  # the kernel divides by the f32 value
    keep, margin = _kept(z, int(top_k), float(top_p))
    w = torch.where(keep, torch.exp(z - z.max()), torch.zeros_like(z))
    c = w.cumsum(0)
    W = float(c[-1])
    hit = torch.nonzero(keep & (c > u * W))[:, 0]
    j = int(hit[0]) if hit.numel() else int(torch.nonzero(keep)[-1, 0])
    lo = float(c[j] - w[j])
    margin = min(margin, (float(c[j]) - u * W) / W, (u * W - lo) / W)
    return j, margin, keep


@dataclass
class SampleCase:
    name: str
    V: int
    Vp: int
    logits: torch.Tensor          # f32 [B, Vp], every value exact in bf16; columns >= V hold PAD_LOGIT
    u: torch.Tensor               # f32 [B]
    temperature: float
    top_k: int
    top_p: float
    _ref: Optional[list] = None

    @property
    def B(self) -> int:
        return self.logits.shape[0]

    def ref(self):
        """[(token, margin, kept mask)] per row, computed once."""
        if self._ref is None:
            self._ref = [sample_ref(self.logits[b, : self.V], float(self.u[b]), self.temperature, self.top_k,
                                    self.top_p) for b in range(self.B)]
        return self._ref

    def tokens(self) -> torch.Tensor:
        return torch.tensor([r[0] for r in self.ref()], dtype=torch.int64)

    def margin(self) -> float:
        return min(r[1] for r in self.ref())


def make_row(V: int, Vp: int, seed: int):
    """One row of logits (f32 [Vp], bf16-exact) and its 40 top tokens in rank order."""
    g = torch.Generator().manual_seed(seed)
    top = torch.randperm(V, generator=g)[:40]
    x = -30.0 + 0.5 * torch.randn(V, generator=g)
    x[top] = 4.0 + torch.arange(40, dtype=torch.float32) * math.log(0.8)
    row = torch.full((Vp,), PAD_LOGIT)
    row[:V] = x
    return row.bfloat16().float(), top


def _rank_cum(row: torch.Tensor, V: int, temperature: float, top_k: int) -> torch.Tensor:
    """Cumulative mass, as a share of the kept set's total, of the first ranks (float64)."""
    z = row[:V].double() / float(torch.tensor(temperature, dtype=torch.float32))
    zs = torch.sort(z, descending=True).values
    if 0 < top_k < V:
        zs = zs[zs >= zs[top_k - 1]]
    w = torch.exp(zs - zs[0])
    return w.cumsum(0) / w.sum()


def _mid_u(row: torch.Tensor, V: int, temperature: float, top_k: int, top_p: float, rank: int) -> float:
    """u at the midpoint of the interval of the kept token of rank ``rank`` (clipped to the
    kept set) in the index-ordered CDF."""
    z = row[:V].double() / float(torch.tensor(temperature, dtype=torch.float32))
    keep, _ = _kept(z, top_k, top_p)
    order = torch.argsort(z, descending=True)
    j = int(order[min(rank, int(keep.sum()) - 1)])
    w = torch.where(keep, torch.exp(z - z.max()), torch.zeros_like(z))
    c = w.cumsum(0)
    return float((c[j] - 0.5 * w[j]) / c[-1])


@functools.lru_cache(maxsize=None)
def sample_cases() -> List[SampleCase]:
    cases: List[SampleCase] = []
    n = 0
    for V, Vp in SIZES:
        for B in (1, 5):
            rows = [make_row(V, Vp, 1000 * V + 10 * B + b)[0] for b in range(B)]
            cases.append(SampleCase(f"greedy-V{V}-B{B}", V, Vp, torch.stack(rows), torch.full((B,), 0.5), 0.0, 0, 1.0))
        for temperature in (0.7, 1.5):
            for top_k in (0, 1, 2, 40):
                for mid in (False, True):
                    n += 1
                    B = 5 if n % 2 else 1
                    rows = [make_row(V, Vp, 7919 * n + b)[0] for b in range(B)]
                    top_p = 1.0
                    if mid:
                        cum = _rank_cum(rows[0], V, temperature, top_k)
                        if cum.numel() == 1:
                            top_p = 0.5
                        else:
                            m = 1 if top_k == 2 else 1 + (5 * n) % 19        # ranks kept: m + 1
                            top_p = float(0.5 * (cum[m - 1] + cum[m]))
                    u = [_mid_u(rows[b], V, temperature, top_k, top_p, (3 * b + n) % 20) for b in range(B)]
                    cases.append(SampleCase(f"T{temperature}-k{top_k}-p{'mid' if mid else '1'}-V{V}-B{B}", V, Vp,
                                            torch.stack(rows), torch.tensor(u, dtype=torch.float32), temperature,
                                            top_k, top_p))
    # a row with -inf entries (tail tokens that can never be drawn)
    V, Vp = 4093, 4096
    row, top = make_row(V, Vp, 31)
    tail = torch.ones(V, dtype=torch.bool)
    tail[top] = False
    row[:V][tail & (torch.arange(V) % 3 == 0)] = -math.inf
    for temperature, top_k, top_p, rank in ((0.0, 0, 1.0, 0), (0.7, 0, 1.0, 6), (1.5, 40, 1.0, 11)):
        u = 0.5 if temperature == 0 else _mid_u(row, V, temperature, top_k, top_p, rank)
        cases.append(SampleCase(f"neginf-T{temperature}-k{top_k}", V, Vp, row[None].clone(),
                                torch.tensor([u], dtype=torch.float32), temperature, top_k, top_p))
    # the two largest logits equal: greedy takes the lower index; top_k = 1 keeps both
    row, top = make_row(V, Vp, 37)
    row[top[1]] = row[top[0]]
    lo_hi = sorted((int(top[0]), int(top[1])))
    cases.append(SampleCase("tie-greedy", V, Vp, row[None].clone(), torch.tensor([0.5]), 0.0, 0, 1.0))
    cases.append(SampleCase("tie-k1-low", V, Vp, row[None].clone(), torch.tensor([0.25]), 1.0, 1, 1.0))
    cases.append(SampleCase("tie-k1-high", V, Vp, row[None].clone(), torch.tensor([0.75]), 1.0, 1, 1.0))
    for c, want in zip(cases[-3:], (lo_hi[0], lo_hi[0], lo_hi[1])):
        assert int(c.tokens()[0]) == want and (c.temperature == 0 or int(c.ref()[0][2].sum()) == 2), c.name
    return cases


# ------------------------------------------------------------------------ rope_kv_append
def rope_kv_append_ref(qkv: torch.Tensor, cos, sin, pos: torch.Tensor, Smax: int, H: int, Hkv: int, Dh: int,
                       rope: bool = True):
    """Float64 reference of one row per sequence: (q [B, H*Dh] after the rotation, the K row
    and the V row to append [B, Hkv*Dh], the clamped positions [B])."""
    B = qkv.shape[0]
    p = pos.long().clamp(0, Smax - 1)
    x = qkv.double().reshape(B, H + 2 * Hkv, Dh)
    half = Dh // 2
    rot = x[:, : H + Hkv]
    if rope:
        c, s = cos.double()[p][:, None, :], sin.double()[p][:, None, :]
        a, b = rot[..., :half], rot[..., half:]
        rot = torch.cat([a * c - b * s, b * c + a * s], -1)
    return (rot[:, :H].reshape(B, H * Dh), rot[:, H:].reshape(B, Hkv * Dh), x[:, H + Hkv:].reshape(B, Hkv * Dh), p)
