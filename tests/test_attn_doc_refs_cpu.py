"""The float64 document-mask reference of attn_doc_refs.py against per-document
``scaled_dot_product_attention``, the CPU path of ``ops.attn_fwd`` / ``ops.attn_bwd`` /
``ops.doc_bounds`` against the reference, and the teeth of the check the GPU tests run: on
every case with at least two documents it must reject six wrong kernels emulated here."""
import pytest
import torch
import torch.nn.functional as F

import mipipe  # noqa: F401
from mipipe import ops

import attn_refs as R
import attn_doc_refs as DR

BF16 = torch.bfloat16
LN2 = 0.6931471805599453


def close64(a, b, atol):
    torch.testing.assert_close(a.double(), b.double(), atol=atol, rtol=0.0)


@pytest.mark.parametrize("c", DR.CASES, ids=lambda c: c.id)
def test_ref_matches_sdpa_per_document(c):
    """Every document alone through causal SDPA (float64, autograd) gives the same rows."""
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    q, k, v, do = (t.double() for t in DR.make_inputs(c, torch.float32))
    ds, de = c.bounds()
    f = DR.attn_doc_fwd_ref(q, k, v, B, S, H, Hkv, D, c.scale, ds)
    b = DR.attn_doc_bwd_ref(q, k, v, f.O, do, B, S, H, Hkv, D, c.scale, ds)
    assert torch.equal(DR.visible_q(ds, B, S), DR.visible_k(de, B, S))
    rep = H // Hkv
    for bi, starts in enumerate(c.starts):
        edges = list(starts) + [S]
        for a, e in zip(edges[:-1], edges[1:]):
            r = slice(bi * S + a, bi * S + e)
            ql, kl, vl = (t[r].clone().requires_grad_() for t in (q, k, v))
            n = e - a
            hd = lambda t, nh: t.reshape(1, n, nh, D).permute(0, 2, 1, 3)   # noqa: E731
            out = F.scaled_dot_product_attention(hd(ql, H), hd(kl, Hkv).repeat_interleave(rep, 1),
                                                 hd(vl, Hkv).repeat_interleave(rep, 1), is_causal=True, scale=c.scale)
            O = out.permute(0, 2, 1, 3).reshape(n, H * D)
            O.backward(do[r])
            close64(f.O[r], O.detach(), 1e-12)
            close64(b.dQ[r], ql.grad, 1e-12)
            close64(b.dK[r], kl.grad, 1e-12)
            close64(b.dV[r], vl.grad, 1e-12)
    close64(f.P.sum(-1), torch.ones(B, H, S, dtype=torch.float64), 1e-12)


def _run_ops_cpu(c, ds, de):
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    q, k, v, do = DR.make_inputs(c, torch.float32)
    o, lse = torch.empty_like(q), torch.empty(B * H * S)
    ops.attn_fwd(q, k, v, o, lse, B, S, S, H, Hkv, D, True, doc_start=ds)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    ops.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, S, S, H, Hkv, D, True, doc_start=ds, doc_end=de)
    return (q, k, v, do), (o, lse, dq, dk, dv)


@pytest.mark.parametrize("c", DR.CASES, ids=lambda c: c.id)
def test_ref_matches_ops_cpu_branch(c):
    ds, de = c.bounds()
    (q, k, v, do), (o, lse, dq, dk, dv) = _run_ops_cpu(c, ds, de)
    f = DR.attn_doc_fwd_ref(q, k, v, c.B, c.S, c.H, c.Hkv, c.D, c.scale, ds)
    b = DR.attn_doc_bwd_ref(q, k, v, o, do, c.B, c.S, c.H, c.Hkv, c.D, c.scale, ds)
    close64(o, f.O, 2e-5)
    close64(lse, f.lse, 2e-5)
    close64(dq, b.dQ, 1e-4)
    close64(dk, b.dK, 1e-4)
    close64(dv, b.dV, 1e-4)


def test_ops_cpu_branch_clamps_malformed_arrays():
    """doc_start outside [0, i] acts as its clamped value; nothing else about the array matters."""
    c = DR.CASES[0]
    ds, de = c.bounds()
    bad = ds.clone()
    bad[5] = -7            # below 0 -> 0 (document 1 starts at 1: query 5 now also sees key 0)
    bad[70] = 10 ** 6      # above i -> i
    bad[c.S + 9] = 300     # row 1
    good = bad.clone()
    good[5], good[70], good[c.S + 9] = 0, 70, 9
    (q, k, v, do), got = _run_ops_cpu(c, bad, de)
    _, want = _run_ops_cpu(c, good, de)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    f = DR.attn_doc_fwd_ref(q, k, v, c.B, c.S, c.H, c.Hkv, c.D, c.scale, bad)
    close64(got[0], f.O, 2e-5)
    assert not torch.equal(got[0], _run_ops_cpu(c, ds, de)[1][0])


def test_ops_doc_argument_errors_cpu():
    c = DR.CASES[2]
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    ds, de = c.bounds()
    q, k, v, do = DR.make_inputs(c, torch.float32)
    o, lse = torch.empty_like(q), torch.empty(B * H * S)
    fwd = lambda **kw: ops.attn_fwd(q, k, v, o, lse, B, S, kw.pop("Sk", S), H, Hkv, D, kw.pop("causal", True), **kw)   # noqa: E731
    with pytest.raises(ValueError):
        fwd(causal=False, doc_start=ds)
    with pytest.raises(ValueError):
        fwd(p_drop=0.1, doc_start=ds)
    with pytest.raises(ValueError):
        fwd(Sk=S + 1, doc_start=ds)
    with pytest.raises(ValueError):
        fwd(doc_start=ds.long())
    with pytest.raises(ValueError):
        fwd(doc_start=ds[:-1])
    with pytest.raises(ValueError):
        fwd(doc_start=torch.stack([ds, ds], 1)[:, 0])
    bwd = lambda **kw: ops.attn_bwd(q, k, v, o, do, lse, q.clone(), k.clone(), v.clone(), B, S, S, H, Hkv, D, True, **kw)   # noqa: E731
    with pytest.raises(ValueError):
        bwd(doc_start=ds)                     # both or neither
    with pytest.raises(ValueError):
        bwd(doc_start=ds, doc_end=de, dbias=torch.zeros((H + 2 * Hkv) * D))
    with pytest.raises(ValueError):
        bwd(doc_start=ds, doc_end=de, p_drop=0.1)


@pytest.mark.parametrize("S", [1, 2, 64, 65, 1000])
def test_doc_bounds_cpu_matches_loop(S):
    for name, tok in DR.eos_layouts(S).items():
        ds, de = ops.doc_bounds(tok, 3)
        rs, re_ = DR.doc_bounds_py(tok, 3)
        assert ds.dtype == torch.int32 and de.dtype == torch.int32 and ds.shape == (2 * S,)
        assert torch.equal(ds, rs) and torch.equal(de, re_), name
        # the two forms of the mask agree
        if S <= 65:
            assert torch.equal(DR.visible_q(ds, 2, S), DR.visible_k(de, 2, S)), name


def test_doc_bounds_semantics():
    tok = torch.tensor([[3, 5, 3, 3, 7, 8]])
    ds, de = ops.doc_bounds(tok, 3)
    assert ds.tolist() == [0, 1, 1, 3, 4, 4] and de.tolist() == [0, 2, 2, 3, 5, 5]


# ------------------------------------------------------------------ teeth
def _bwd_from_P(q, k, v, o, do, P, c):
    """Gradients a kernel computes from an arbitrary probability matrix P [B, H, S, S]."""
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    rep = H // Hkv
    Q = R.heads(q, B, S, H, D)
    K = R.heads(k, B, S, Hkv, D).repeat_interleave(rep, 1)
    V = R.heads(v, B, S, Hkv, D).repeat_interleave(rep, 1)
    dO, O = R.heads(do, B, S, H, D), R.heads(o, B, S, H, D)
    dS = P * (dO @ V.transpose(-1, -2) - (dO * O).sum(-1, keepdim=True))
    group = lambda x: x.reshape(B, Hkv, rep, S, D).sum(2)   # noqa: E731
    return (R.rows(dS @ K * c.scale), R.rows(group(dS.transpose(-1, -2) @ Q * c.scale)),
            R.rows(group(P.transpose(-1, -2) @ dO)))


def _mutants(c):
    """name -> outputs (o, lse, dq, dk, dv in float64) of a wrong kernel on case c."""
    B, S, H, Hkv, D = c.B, c.S, c.H, c.Hkv, c.D
    q, k, v, do = DR.make_inputs(c)
    ds, de = c.bounds()
    true_f = DR.attn_doc_fwd_ref(q, k, v, B, S, H, Hkv, D, c.scale, ds)
    o = true_f.O.to(BF16)
    true_b = DR.attn_doc_bwd_ref(q, k, v, o, do, B, S, H, Hkv, D, c.scale, ds)
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    causal = (j <= i)[None, None].expand(B, 1, S, S)
    dsl, del_ = ds.reshape(B, S).long(), de.reshape(B, S).long()
    out = {}

    def whole(name, vis):   # forward and backward under one wrong visibility
        f = DR.attn_doc_fwd_ref(q, k, v, B, S, H, Hkv, D, c.scale, vis=vis)
        om = f.O.to(BF16)
        b = DR.attn_doc_bwd_ref(q, k, v, om, do, B, S, H, Hkv, D, c.scale, vis=vis)
        out[name] = dict(o=f.O, lse=f.lse, dq=b.dQ, dk=b.dK, dv=b.dV)

    whole("plain-causal", causal)
    for d in (-1, 1):   # the bound used without the clamp
        whole(f"doc_start{d:+d}", causal & (j[None] >= (dsl + d)[:, :, None])[:, None])
    # unmasked scores against the true lse: what a kernel's backward recomputes
    s_all = (R.heads(q, B, S, H, D) @ R.heads(k, B, S, Hkv, D).repeat_interleave(H // Hkv, 1).transpose(-1, -2)) * c.scale
    p_all = torch.exp(s_all - true_f.lse.reshape(B, H, S, 1) * LN2)
    for d in (-1, 1):   # dK / dV under a wrong doc_end, everything else right
        vis_k = causal & (i[None] <= (del_ + d)[:, None, :])[:, None]
        _, dk, dv = _bwd_from_P(q, k, v, o, do, p_all * vis_k, c)
        out[f"doc_end{d:+d}"] = dict(o=true_f.O, lse=true_f.lse, dq=true_b.dQ, dk=dk, dv=dv)
    dq, dk, dv = _bwd_from_P(q, k, v, o, do, p_all * causal, c)
    out["fwd-only"] = dict(o=true_f.O, lse=true_f.lse, dq=dq, dk=dk, dv=dv)
    return (true_f, true_b), out


def _judge(c, refs, got):
    rep = R.Report(c.id)
    got = {n: (t.to(BF16) if n not in ("lse",) else t.float()) for n, t in got.items()}
    R.check_outputs(rep, "bf16", refs[0], refs[1], got, c.B, c.S, c.H, c.Hkv, c.D)
    return rep.fails


@pytest.mark.parametrize("c", [c for c in DR.CASES if c.ndocs >= 2], ids=lambda c: c.id)
def test_check_rejects_wrong_kernels(c):
    refs, muts = _mutants(c)
    # the emulation itself is sound: the right kernel, rounded to bf16, passes
    ok = dict(o=refs[0].O, lse=refs[0].lse, dq=refs[1].dQ, dk=refs[1].dK, dv=refs[1].dV)
    assert not _judge(c, refs, ok)
    for name, got in muts.items():
        assert _judge(c, refs, got), f"{name} passes the check on {c.id}"
