"""The document-masked attention kernels (attention_doc.hip) against the float64 reference of
attn_doc_refs.py (validated on the CPU in test_attn_doc_refs_cpu.py, with the teeth of the
check), at the bounds of the v1 kernels whose arithmetic they copy (attn_refs.BOUND, with the
older tests' tolerances asserted alongside by check_outputs).

Tile skipping is shown with NaN as plain data: a document filled with NaN must not reach
another document's outputs, which holds only if its tiles are never multiplied (0 * NaN
survives the matrix cores)."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import attn_refs as R
import attn_doc_refs as DR

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32), b.view(torch.int16 if a.dtype == BF16 else torch.int32))


def run_kernels(c, ins, ds, de):
    """Forward and backward on the GPU; q | k | v packed side by side in one buffer (the fused
    QKV layout), gradients likewise.  Returns CPU tensors."""
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    T, wq, wk = B * S, H * D, Hkv * D
    q, k, v, do = ins
    qkv = torch.cat([q, k, v], 1).to(DEV)
    g = torch.full_like(qkv, -77.0)
    qd, kd, vd = qkv[:, :wq], qkv[:, wq: wq + wk], qkv[:, wq + wk:]
    dq, dk, dv = g[:, :wq], g[:, wq: wq + wk], g[:, wq + wk:]
    o = torch.full((T, wq), -77.0, dtype=BF16, device=DEV)
    lse = torch.full((B * H * S,), -77.0, dtype=F32, device=DEV)
    delta = torch.full((B * H * S,), -77.0, dtype=F32, device=DEV)
    dod = do.to(DEV)
    dsd, ded = ds.to(DEV), de.to(DEV)
    ops.attn_fwd(qd, kd, vd, o, lse, B, S, S, H, Hkv, D, True, doc_start=dsd)
    ops.attn_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, B, S, S, H, Hkv, D, True, delta=delta, doc_start=dsd, doc_end=ded)
    torch.cuda.synchronize()
    return {n: t.cpu().contiguous() for n, t in dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv).items()}


_REFS = {}


def refs_of(c):
    """Float64 reference of a case from its clean inputs and the kernel's stored O (computed
    once per case and kept)."""
    if c.id not in _REFS:
        ins = DR.make_inputs(c)
        ds, de = c.bounds()
        got = run_kernels(c, ins, ds, de)
        f = DR.attn_doc_fwd_ref(*ins[:3], c.B, c.S, c.H, c.Hkv, c.D, c.scale, ds)
        b = DR.attn_doc_bwd_ref(*ins[:3], got["o"], ins[3], c.B, c.S, c.H, c.Hkv, c.D, c.scale, ds)
        _REFS[c.id] = (ins, (ds, de), got, f, b)
    return _REFS[c.id]


@pytest.mark.parametrize("c", DR.CASES, ids=lambda c: c.id)
def test_doc_kernels_match_reference(c):
    ins, _, got, f, b = refs_of(c)
    rep = R.Report(c.id)
    R.check_outputs(rep, "bf16", f, b, got, c.B, c.S, c.H, c.Hkv, c.D)
    rep.finish()


def test_every_token_its_own_document_is_exact():
    c = next(x for x in DR.CASES if x.name == "alone")
    ins, _, got, f, b = refs_of(c)
    q, k, v, do = ins
    rep = c.H // c.Hkv
    vrows = v.reshape(c.B * c.S, c.Hkv, c.D).repeat_interleave(rep, 1).reshape(c.B * c.S, c.H * c.D)
    assert bits_equal(got["o"], vrows)
    self_score = (R.heads(q, c.B, c.S, c.H, c.D) * R.heads(k, c.B, c.S, c.Hkv, c.D).repeat_interleave(rep, 1)).sum(-1)
    want = (self_score * c.scale * R.LOG2E).reshape(-1)
    err = float(((got["lse"].double() - want).abs() / (want.abs() + min(1.0, float(want.abs().max())))).max())
    print(f"MEASURE alone.lse {err:.4g} rel")
    assert err <= R.BOUND["attn.bf16.lse"]


def _doc_rows(c, docs):
    """bool [B*S]: tokens of the given document indices (same starts on every row)."""
    edges = list(c.starts[0]) + [c.S]
    pos = torch.arange(c.B * c.S) % c.S
    m = torch.zeros(c.B * c.S, dtype=torch.bool)
    for d in docs:
        m |= (pos >= edges[d]) & (pos < edges[d + 1])
    return m


def _check_rows(c, got, f, b, keep, names, what):
    """check_outputs restricted to the token rows ``keep`` (reference and outputs alike)."""
    B, S, H = c.B, c.S, c.H
    vec = keep.reshape(B, 1, S).expand(B, H, S).reshape(-1)
    zero = lambda t, m: torch.where(m.reshape(-1, *[1] * (t.dim() - 1)), t, torch.zeros_like(t))   # noqa: E731
    for n in names:
        sel = vec if n in ("lse", "delta") else keep
        assert torch.isfinite(got[n][sel]).all(), f"{what}: {n} is not finite outside the NaN documents"
    from types import SimpleNamespace as NS
    f2 = NS(O=zero(f.O, keep), A_O=zero(f.A_O, keep), lse=torch.where(vec, f.lse, torch.zeros_like(f.lse)))
    b2 = NS(dQ=zero(b.dQ, keep), A_dQ=zero(b.A_dQ, keep), dK=zero(b.dK, keep), A_dK=zero(b.A_dK, keep),
            dV=zero(b.dV, keep), A_dV=zero(b.A_dV, keep), delta=torch.where(vec, b.delta, torch.zeros_like(b.delta)))
    g2 = {n: (torch.where(vec, got[n], torch.zeros_like(got[n])) if n in ("lse", "delta") else zero(got[n], keep))
          for n in names}
    rep = R.Report(f"{c.id}-{what}")
    R.check_outputs(rep, "bf16", f2, b2, g2, B, S, H, c.Hkv, c.D)
    rep.finish()


def test_tile_skipping_nan_document_0():
    c = DR.ALIGNED
    ins, (ds, de), _, f, b = refs_of(c)
    d0 = _doc_rows(c, [0])
    nan_ins = tuple(torch.where(d0[:, None], torch.full_like(t, float("nan")), t) for t in ins)
    got = run_kernels(c, nan_ins, ds, de)
    _check_rows(c, got, f, b, ~d0, ("o", "lse", "delta", "dq", "dk", "dv"), "nan-doc0")


def test_tile_skipping_nan_queries_of_documents_1_2():
    c = DR.ALIGNED
    ins, (ds, de), _, f, b = refs_of(c)
    d12 = _doc_rows(c, [1, 2])
    q, k, v, do = ins
    nanq = torch.where(d12[:, None], torch.full_like(q, float("nan")), q)
    nando = torch.where(d12[:, None], torch.full_like(do, float("nan")), do)
    got = run_kernels(c, (nanq, k, v, nando), ds, de)
    _check_rows(c, got, f, b, ~d12, ("dk", "dv"), "nan-q-doc12")


def test_deterministic():
    c = DR.ALIGNED
    ins, (ds, de), got, _, _ = refs_of(c)
    again = run_kernels(c, ins, ds, de)
    for n in got:
        assert bits_equal(got[n], again[n]), n


def test_binding_checks_raise_before_launch():
    c = DR.CASES[2]
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    q, k, v, do = (t.to(DEV) for t in DR.make_inputs(c))
    ds, de = (t.to(DEV) for t in c.bounds())
    o, lse = torch.zeros_like(q), torch.zeros(B * H * S, device=DEV)
    ext = ops.kernels._ext()

    def fwd(q=q, k=k, v=v, o=o, ds=ds, D=D, H=H, Hkv=Hkv, causal=True, p=0.0):
        ext.attn_doc_fwd(q, k, v, o, lse, ds, B, S, H, Hkv, D, causal, c.scale, p)

    def bwd(ds=ds, de=de):
        ext.attn_doc_bwd(q, k, v, o, do, lse, torch.zeros_like(lse), torch.zeros_like(q), torch.zeros_like(k),
                         torch.zeros_like(v), ds, de, B, S, H, Hkv, D, True, c.scale, 0.0)

    wide = torch.zeros(B * S, 2, dtype=torch.int32, device=DEV)
    f32 = [t.float() for t in (q, k, v, o)]
    bad = [lambda: fwd(ds=ds.long()), lambda: fwd(ds=ds[:-1]), lambda: fwd(ds=wide[:, 0]),
           lambda: fwd(ds=ds.cpu()), lambda: fwd(p=0.1), lambda: fwd(causal=False),
           lambda: fwd(q=f32[0], k=f32[1], v=f32[2], o=f32[3]), lambda: fwd(H=3, Hkv=2),
           lambda: bwd(de=de.long()), lambda: bwd(de=de[:-1]), lambda: bwd(ds=wide[:, 0])]
    # D 96: tensors of that width, so only the head dim is wrong
    q96 = torch.zeros(B * S, H * 96, dtype=BF16, device=DEV)
    bad.append(lambda: fwd(q=q96, k=q96, v=q96, o=torch.zeros_like(q96), D=96))
    # rows that are not 16-byte aligned: a column slice at an odd offset
    buf = torch.zeros(B * S, H * D + 4, dtype=BF16, device=DEV)
    bad.append(lambda: fwd(q=buf[:, 1: 1 + H * D]))
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
        assert float(o.abs().sum()) == 0.0, f"check {i} launched"
    # the ops wrapper turns the semantic ones into ValueError
    for kw in (dict(p_drop=0.1), ):
        with pytest.raises(ValueError):
            ops.attn_fwd(q, k, v, o, lse, B, S, S, H, Hkv, D, True, doc_start=ds, **kw)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, k, v, o, lse, B, S, S, H, Hkv, D, False, doc_start=ds)
    with pytest.raises(ValueError):
        ops.attn_fwd(f32[0], f32[1], f32[2], f32[3], lse, B, S, S, H, Hkv, D, True, doc_start=ds)


@pytest.mark.parametrize("S", [1, 64, 65, 1000])
def test_doc_bounds_gpu_matches_cpu(S):
    for name, tok in DR.eos_layouts(S).items():
        want = ops.doc_bounds(tok, 3)
        got = ops.doc_bounds(tok.to(DEV), 3)
        for g, w in zip(got, want):
            assert g.dtype == torch.int32 and g.is_cuda
            assert torch.equal(g.cpu(), w), (name, S)
