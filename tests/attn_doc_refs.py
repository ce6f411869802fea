"""float64 reference of the document-masked attention kernels (attention_doc.hip), a
pure-Python ``doc_bounds``, and the cases of the GPU tests.

Semantics: for B sequences of length S, ``doc_start[b*S + i]`` / ``doc_end[b*S + i]`` (int32)
are the positions inside sequence b of the first / last token of the document that holds
position i.  Key j is visible to query i iff doc_start[i] <= j <= i, which for well-formed
arrays equals j <= i <= doc_end[j].  Position i starts a document iff i == 0 or
tokens[i-1] == eos.

The references return the fields of ``attn_refs.attn_fwd_ref`` / ``attn_bwd_ref``, so
``attn_refs.check_outputs`` and ``Report`` apply unchanged.  ``vis`` may be given directly
([B, 1, S, S] bool): the CPU tests use that to emulate wrong kernels."""
import math
from types import SimpleNamespace as NS

import torch

from attn_refs import FLUSH, LOG2E, f64, heads, round_to, rows


# ------------------------------------------------------------------ bounds
def doc_bounds_py(tokens, eos):
    """The definition as a loop.  tokens: [B, S] integers.  Returns int32 [B*S] x 2."""
    B, S = tokens.shape
    ds, de = torch.zeros(B, S, dtype=torch.int32), torch.zeros(B, S, dtype=torch.int32)
    for b in range(B):
        row = tokens[b].tolist()
        start = 0
        for i in range(S):
            if i == 0 or row[i - 1] == eos:
                start = i
            ds[b, i] = start
        end = S - 1
        for i in range(S - 1, -1, -1):
            if i == S - 1 or row[i] == eos:
                end = i
            de[b, i] = end
    return ds.reshape(-1), de.reshape(-1)


def bounds_from_starts(S, starts_per_row):
    """(doc_start, doc_end) int32 [B*S] from the list of document start positions of each row
    (every list begins with 0)."""
    ds, de = [], []
    for starts in starts_per_row:
        assert starts[0] == 0 and list(starts) == sorted(set(starts)) and starts[-1] < S
        edges = list(starts) + [S]
        for a, b in zip(edges[:-1], edges[1:]):
            ds += [a] * (b - a)
            de += [b - 1] * (b - a)
    return torch.tensor(ds, dtype=torch.int32), torch.tensor(de, dtype=torch.int32)


def clamp_bounds(doc_start, doc_end, B, S):
    """What the kernels and the CPU path make of any array contents: doc_start[i] into [0, i],
    doc_end[j] into [j, S-1]."""
    pos = torch.arange(S)[None, :]
    ds = torch.minimum(doc_start.reshape(B, S).long().clamp_min(0), pos)
    de = None if doc_end is None else torch.maximum(doc_end.reshape(B, S).long().clamp_max(S - 1), pos)
    return ds, de


def visible_q(doc_start, B, S):
    """[B, 1, S, S] bool, the forward / dQ form: doc_start[i] <= j <= i."""
    ds, _ = clamp_bounds(doc_start, None, B, S)
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return ((j <= i)[None] & (j[None] >= ds[:, :, None]))[:, None]


def visible_k(doc_end, B, S):
    """[B, 1, S, S] bool, the dK/dV form: j <= i <= doc_end[j]."""
    _, de = clamp_bounds(torch.zeros(B * S, dtype=torch.int32), doc_end, B, S)
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return ((j <= i)[None] & (i[None] <= de[:, None, :]))[:, None]


# ------------------------------------------------------------------ float64 reference
def attn_doc_fwd_ref(q, k, v, B, S, H, Hkv, D, scale, doc_start=None, vis=None):
    """O [B*S, H*D], lse [B*H*S] (log2 units), P, A_O, S, Pa, vis: attn_refs.attn_fwd_ref's fields
    under the per-sequence visibility matrix."""
    rep = H // Hkv
    vis = visible_q(doc_start, B, S) if vis is None else vis
    Q = heads(q, B, S, H, D)
    K = heads(k, B, S, Hkv, D).repeat_interleave(rep, 1)
    V = heads(v, B, S, Hkv, D).repeat_interleave(rep, 1)
    s = (Q @ K.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m) & (m < 0)
    e = torch.exp(s - torch.where(empty, torch.zeros_like(m), m))
    l = e.sum(-1, keepdim=True)
    P = e / torch.where(empty, torch.ones_like(l), l)
    lse = torch.where(empty, torch.full_like(m, float("inf")), (m + torch.log(l)) * LOG2E)
    Pa = P + FLUSH * vis
    return NS(O=rows(P @ V), lse=lse.reshape(-1), P=P, A_O=rows(Pa @ V.abs()), S=s, Pa=Pa, vis=vis)


def attn_doc_bwd_ref(q, k, v, o, do, B, S, H, Hkv, D, scale, doc_start=None, vis=None):
    """attn_refs.attn_bwd_ref's fields (backward from the STORED ``o``) under the document mask."""
    rep = H // Hkv
    f = attn_doc_fwd_ref(q, k, v, B, S, H, Hkv, D, scale, doc_start, vis)
    Q = heads(q, B, S, H, D)
    K = heads(k, B, S, Hkv, D).repeat_interleave(rep, 1)
    V = heads(v, B, S, Hkv, D).repeat_interleave(rep, 1)
    dO, O = heads(do, B, S, H, D), heads(o, B, S, H, D)
    delta = (dO * O).sum(-1, keepdim=True)
    dP = dO @ V.transpose(-1, -2)
    # a masked pair contributes nothing whatever the other operand holds (NaN data of another
    # document included)
    dP = torch.where(f.vis.expand_as(dP), dP, torch.zeros_like(dP))
    dS = f.P * (dP - delta)
    adS = f.P * (dP.abs() + delta.abs()) + FLUSH * f.vis * (dP.abs() + delta.abs()).clamp_min(1.0)

    def group(x):
        return x.reshape(B, Hkv, rep, S, D).sum(2)

    dQ, dK, dV = rows(dS @ K * scale), rows(group(dS.transpose(-1, -2) @ Q * scale)), rows(group(f.P.transpose(-1, -2) @ dO))
    dt = q.dtype
    return NS(dQ=dQ, dK=dK, dV=dV, delta=delta.reshape(-1),
              A_dQ=rows(adS @ K.abs() * scale), A_dK=rows(group(adS.transpose(-1, -2) @ Q.abs() * scale)),
              A_dV=rows(group(f.Pa.transpose(-1, -2) @ dO.abs())),
              colsum=torch.cat([round_to(g, dt).sum(0) for g in (dQ, dK, dV)]), fwd=f)


# ------------------------------------------------------------------ cases
class DocCase:
    def __init__(self, name, B, S, H, Hkv, D, starts, seed=0):
        self.name, self.B, self.S, self.H, self.Hkv, self.D, self.starts, self.seed = name, B, S, H, Hkv, D, starts, seed
        self.scale = 1.0 / math.sqrt(D)

    @property
    def id(self):
        return f"{self.name}-B{self.B}-S{self.S}-H{self.H}-Hkv{self.Hkv}-D{self.D}"

    def bounds(self):
        return bounds_from_starts(self.S, self.starts)

    @property
    def ndocs(self):
        return max(len(s) for s in self.starts)

    def __repr__(self):
        return self.id


CASES = [
    # documents that start at, one before and one after a 64-key tile edge; row 1 is one document
    DocCase("edges", 2, 256, 4, 2, 64, [[0, 1, 63, 64, 65, 128, 200], [0]], seed=1),
    # partial last tile; queries 128..129 and 130.. meet a fully masked tile before their first
    # visible one (the -inf running-maximum path)
    DocCase("neginf", 1, 200, 2, 2, 128, [[0, 96, 130]], seed=2),
    DocCase("onetoken", 1, 129, 2, 2, 64, [[0, 128]], seed=3),
    DocCase("alone", 1, 130, 2, 2, 64, [list(range(130))], seed=4),
    DocCase("s1", 1, 1, 2, 2, 64, [[0]], seed=5),
    # GQA group of 8, block-aligned documents
    DocCase("aligned", 3, 384, 8, 1, 64, [[0, 128, 256]] * 3, seed=6),
]
ALIGNED = CASES[-1]


def make_inputs(c, dtype=torch.bfloat16):
    """(q, k, v, do): N(0, 1), [B*S, heads*D] contiguous CPU tensors of ``dtype``."""
    g = torch.Generator().manual_seed(2000 + c.seed)
    T = c.B * c.S
    q, do = torch.randn(T, c.H * c.D, generator=g), torch.randn(T, c.H * c.D, generator=g)
    k, v = torch.randn(T, c.Hkv * c.D, generator=g), torch.randn(T, c.Hkv * c.D, generator=g)
    return tuple(t.to(dtype) for t in (q, k, v, do))


# the four eos layouts of the doc_bounds tests
def eos_layouts(S, eos=3, seed=0):
    """name -> tokens [2, S] int64 over a vocabulary without ``eos`` except where placed."""
    g = torch.Generator().manual_seed(seed + S)
    base = torch.randint(4, 50, (2, S), generator=g, dtype=torch.int64)
    out = {"none": base.clone()}
    t = base.clone(); t[:, 0] = eos; out["first"] = t
    t = base.clone(); t[:, S - 1] = eos; out["last"] = t
    t = base.clone()
    for p in (S // 3, S // 3 + 1, S // 3 + 2, (2 * S) // 3):
        t[0, min(p, S - 1)] = eos
    t[1, : min(3, S)] = eos
    out["consecutive"] = t
    return out
