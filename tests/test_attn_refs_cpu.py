"""The float64 attention reference of attn_refs.py against float64
``scaled_dot_product_attention`` with autograd and against the CPU branch of ``ops.attn_fwd`` /
``ops.attn_bwd``; the check of the GPU edge tests against eight subtly wrong kernels, each of
which must fail it at the recorded ``BOUND``; and the inputs of the GPU cases against the
conditions their groups state.  This is what validates the oracle of test_attn_edges_gpu.py
on a machine without a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import mipipe  # noqa: F401
from mipipe import ops
from mipipe.ops import kernels as opk

import attn_refs as R

BF16 = torch.bfloat16


def close64(a, b, atol, rtol=0.0):
    torch.testing.assert_close(a.double(), b.double(), atol=atol, rtol=rtol)


def inputs64(B, Sq, Sk, H, Hkv, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda r, c: torch.randn(r, c, generator=g, dtype=torch.float64)   # noqa: E731
    return mk(B * Sq, H * D), mk(B * Sk, Hkv * D), mk(B * Sk, Hkv * D), mk(B * Sq, H * D)


SDPA = [  # B, Sq, Sk, H, Hkv, D, causal, scale
    (2, 65, 65, 3, 3, 64, False, None), (2, 65, 65, 3, 3, 64, True, None), (1, 129, 129, 2, 2, 40, True, 0.3),
    (1, 100, 300, 2, 2, 64, False, None), (1, 300, 100, 2, 2, 64, False, 0.3), (2, 65, 200, 3, 3, 128, True, None),
    (1, 129, 257, 2, 2, 64, True, 0.3), (1, 100, 100, 8, 2, 64, False, None), (1, 65, 65, 8, 1, 8, True, 0.3),
    (1, 1, 129, 4, 1, 64, True, None), (1, 1, 1, 2, 2, 64, True, None)]


@pytest.mark.parametrize("B,Sq,Sk,H,Hkv,D,causal,scale", SDPA)
def test_ref_matches_sdpa_float64(B, Sq, Sk, H, Hkv, D, causal, scale):
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    q, k, v, do = inputs64(B, Sq, Sk, H, Hkv, D)
    f = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, causal, scale)
    b = R.attn_bwd_ref(q, k, v, f.O, do, B, Sq, Sk, H, Hkv, D, causal, scale)
    ql, kl, vl = (t.clone().requires_grad_() for t in (q, k, v))
    rep = H // Hkv
    hd = lambda t, S, nh: t.reshape(B, S, nh, D).permute(0, 2, 1, 3)   # noqa: E731
    Q = hd(ql, Sq, H)
    K, V = hd(kl, Sk, Hkv).repeat_interleave(rep, 1), hd(vl, Sk, Hkv).repeat_interleave(rep, 1)
    out = F.scaled_dot_product_attention(Q, K, V, attn_mask=R.visible(Sq, Sk, causal), scale=scale)
    O = out.permute(0, 2, 1, 3).reshape(B * Sq, H * D)
    O.backward(do)
    close64(f.O, O.detach(), 1e-12)
    close64(b.dQ, ql.grad, 1e-12)
    close64(b.dK, kl.grad, 1e-12)
    close64(b.dV, vl.grad, 1e-12)
    s = (Q @ K.transpose(-1, -2)).detach() * scale
    s = s.masked_fill(~R.visible(Sq, Sk, causal), float("-inf"))
    close64(f.lse, torch.logsumexp(s, -1).reshape(-1) * R.LOG2E, 1e-12)
    close64(f.P.sum(-1), torch.ones(B, H, Sq, dtype=torch.float64), 1e-12)
    close64(b.delta, (do * f.O).reshape(B, Sq, H, D).sum(-1).permute(0, 2, 1).reshape(-1), 1e-12)
    close64(b.colsum, torch.cat([b.dQ.sum(0), b.dK.sum(0), b.dV.sum(0)]), 1e-12)
    assert (f.A_O >= f.O.abs() - 1e-12).all() and (b.A_dQ >= b.dQ.abs() - 1e-12).all()
    assert (b.A_dK >= b.dK.abs() - 1e-12).all() and (b.A_dV >= b.dV.abs() - 1e-12).all()


@pytest.mark.parametrize("Sq,Sk", [(200, 65), (257, 129), (3, 1)])
def test_ref_rows_without_keys(Sq, Sk):
    """Causal with Sk < Sq: the first Sq - Sk queries see no key.  They give O = 0, lse = +inf
    and dQ = 0, and everything else equals the square causal problem of the last Sk queries."""
    B, H, Hkv, D = 2, 4, 2, 16
    q, k, v, do = inputs64(B, Sq, Sk, H, Hkv, D)
    f = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, True, 0.25)
    b = R.attn_bwd_ref(q, k, v, f.O, do, B, Sq, Sk, H, Hkv, D, True, 0.25)
    dead = (torch.arange(B * Sq) % Sq) < Sq - Sk
    assert torch.isinf(f.lse.reshape(B, H, Sq)[:, :, : Sq - Sk]).all() and (f.lse.reshape(B, H, Sq)[:, :, : Sq - Sk] > 0).all()
    assert torch.isfinite(f.lse.reshape(B, H, Sq)[:, :, Sq - Sk:]).all()
    for t in (f.O, f.A_O, b.dQ, b.A_dQ):
        assert torch.count_nonzero(t[dead]) == 0
    live = lambda t: t[~dead]   # noqa: E731
    f2 = R.attn_fwd_ref(live(q), k, v, B, Sk, Sk, H, Hkv, D, True, 0.25)
    b2 = R.attn_bwd_ref(live(q), k, v, f2.O, live(do), B, Sk, Sk, H, Hkv, D, True, 0.25)
    close64(live(f.O), f2.O, 1e-13)
    close64(live(b.dQ), b2.dQ, 1e-13)
    close64(b.dK, b2.dK, 1e-13)
    close64(b.dV, b2.dV, 1e-13)
    close64(b.A_dK, b2.A_dK, 1e-13)
    assert torch.isfinite(b.dK).all() and torch.isfinite(b.dV).all()


OPS_CPU = [  # B, Sq, Sk, H, Hkv, D, causal, scale, p
    (2, 65, 65, 3, 3, 64, True, None, 0.0), (1, 100, 300, 2, 2, 64, False, 0.3, 0.0), (1, 129, 257, 4, 1, 40, True, None, 0.0),
    (1, 100, 100, 8, 2, 128, False, None, 0.3), (1, 200, 200, 4, 1, 64, True, None, 0.1)]


@pytest.mark.parametrize("B,Sq,Sk,H,Hkv,D,causal,scale,p", OPS_CPU)
def test_ref_matches_ops_cpu_branch(B, Sq, Sk, H, Hkv, D, causal, scale, p):
    """The f32 CPU branch of the wrappers, with its own dropout mask handed to the reference."""
    sc = 1.0 / math.sqrt(D) if scale is None else scale
    q, k, v, do = (t.float() for t in inputs64(B, Sq, Sk, H, Hkv, D, seed=1))
    keep = opk._cpu_attn_drop(B, H, Sq, Sk, p, 77, "cpu")
    if p:
        assert set(keep.unique().tolist()) == {0.0, float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))}
    o, lse = torch.empty_like(q), torch.empty(B * H * Sq)
    ops.attn_fwd(q, k, v, o, lse, B, Sq, Sk, H, Hkv, D, causal, scale=scale, p_drop=p, seed=77)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    dbias = torch.full(((H + 2 * Hkv) * D,), 0.25)
    ops.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, Sq, Sk, H, Hkv, D, causal, scale=scale, p_drop=p, seed=77, dbias=dbias)
    f = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, causal, sc, keep)
    b = R.attn_bwd_ref(q, k, v, o, do, B, Sq, Sk, H, Hkv, D, causal, sc, keep)
    close64(o, f.O, 2e-5)
    close64(lse, f.lse, 2e-5)
    close64(dq, b.dQ, 1e-4)
    close64(dk, b.dK, 1e-4)
    close64(dv, b.dV, 1e-4)
    close64(dbias - 0.25, b.colsum, 2e-3)


def test_ref_matches_ops_cpu_branch_live_rows():
    """Rows that see no key: the CPU branch yields NaN and -inf there, the rest must agree."""
    B, Sq, Sk, H, Hkv, D = 1, 200, 65, 2, 2, 64
    q, k, v, _ = (t.float() for t in inputs64(B, Sq, Sk, H, Hkv, D, seed=2))
    o, lse = torch.empty_like(q), torch.empty(B * H * Sq)
    ops.attn_fwd(q, k, v, o, lse, B, Sq, Sk, H, Hkv, D, True)
    f = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, True, 0.125)
    close64(o[Sq - Sk:], f.O[Sq - Sk:], 2e-5)
    live = torch.isfinite(f.lse)
    assert int(live.sum()) == B * H * Sk
    close64(lse[live], f.lse[live], 2e-5)


# ------------------------------------------------------------------ the metric has teeth
def kernel_model(c, q, k, v, do, keep, mut=None):
    """What a kernel stores for case ``c``, computed in float64 and rounded to bf16 -- or, with
    ``mut``, what a kernel with one specific bug stores.  Written out separately from the
    reference (head-major loops instead of its batched products) so that ``mut=None`` passing
    the check also cross-checks the reference."""
    B, Sq, Sk, H, Hkv, D = c.shape()
    rep, p_inv = H // Hkv, 1.0 / (1.0 - c.p)
    scale = c.scale * (1.02 if mut == "scale" else 1.0)
    shift = 0 if mut == "shift" else Sk - Sq
    o = torch.zeros(B * Sq, H * D, dtype=torch.float64)
    lse, delta = torch.zeros(B, H, Sq, dtype=torch.float64), torch.zeros(B, H, Sq, dtype=torch.float64)
    dq, dk, dv = torch.zeros_like(o), torch.zeros(B * Sk, Hkv * D, dtype=torch.float64), torch.zeros(B * Sk, Hkv * D, dtype=torch.float64)
    i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    vis = (j <= i + shift - (1 if mut == "diagonal" else 0)) if c.causal else torch.ones(Sq, Sk, dtype=torch.bool)
    if mut == "last_key":
        vis = vis & (j < Sk - 1)
    for b in range(B):
        for h in range(H):
            hk = h % Hkv if mut == "kv_head" else h // rep
            rq, rk = slice(b * Sq, (b + 1) * Sq), slice(b * Sk, (b + 1) * Sk)
            cq, ck = slice(h * D, (h + 1) * D), slice(hk * D, (hk + 1) * D)
            Q, K, V, dO = q[rq, cq].double(), k[rk, ck].double(), v[rk, ck].double(), do[rq, cq].double()
            s = (Q @ K.T * scale).masked_fill(~vis, float("-inf"))
            m = s.amax(-1, keepdim=True)
            dead = torch.isinf(m)
            e = torch.exp(s - torch.where(dead, torch.zeros_like(m), m))
            l = e.sum(-1, keepdim=True)
            P = e / torch.where(dead, torch.ones_like(l), l)
            lse[b, h] = torch.where(dead, torch.full_like(m, float("inf")), (m + l.log()) * R.LOG2E)[:, 0]
            kp = torch.ones_like(P) if keep is None else keep[b, h].double()
            if mut == "no_rescale":
                kp = kp / p_inv
            O = (P * kp) @ V
            o[rq, cq] = O
            Ost = O if mut == "delta" else R.round_to(O, BF16)
            dl = (dO * Ost).sum(-1, keepdim=True)
            delta[b, h] = dl[:, 0]
            dS = P * ((dO @ V.T) * kp - dl)
            dq[rq, cq] = dS @ K * scale
            contrib = dS.T[:, :, None] * Q[None, :, :] * scale            # [key, query, d]
            if mut == "dk_tile":
                contrib[:, 64:128] *= 2.0
            dk[rk, ck] += contrib.sum(1)
            dv[rk, ck] += (P * kp).T @ dO
    got = {n: t.to(BF16) for n, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv))}
    got.update(lse=lse.reshape(-1).float(), delta=delta.reshape(-1).float())
    colsum = torch.cat([got[n].double().sum(0) for n in ("dq", "dk", "dv")])
    got.update(dbias=(colsum + 0.25).float(), dbias0=0.25)
    return got


def run_model(c, mut, big=1.0):
    q, k, v, do = R.make_inputs(c)
    v, do = (v.double() * big).to(BF16), (do.double() * big).to(BF16)
    B, Sq, Sk, H, Hkv, D = c.shape()
    keep = None
    if c.p:
        g = torch.Generator().manual_seed(5)
        keep = (torch.rand(B, H, Sq, Sk, generator=g) >= c.p).double() / (1.0 - c.p)
    got = kernel_model(c, q, k, v, do, keep, mut)
    f = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, c.causal, c.scale, keep)
    o_stored = kernel_model(c, q, k, v, do, keep)["o"] if mut else got["o"]
    b = R.attn_bwd_ref(q, k, v, o_stored, do, B, Sq, Sk, H, Hkv, D, c.causal, c.scale, keep)
    rep = R.Report(f"{c.id} mut={mut}")
    R.check_outputs(rep, "bf16", f, b, got, B, Sq, H, Hkv, D)
    return rep


MUTANTS = {  # mutation -> (case, magnitude of v and dO)
    "last_key": (R.Case("", 2, 65, 65, 3, 3, 64, False), 1.0),            # the last key dropped
    "diagonal": (R.Case("", 2, 129, 129, 3, 3, 64, True), 1.0),           # the causal diagonal moved by one
    "scale": (R.Case("", 1, 257, 257, 2, 2, 64, True, kind="q6"), 1.0),   # scale x 1.02
    "no_rescale": (R.Case("", 1, 200, 200, 2, 2, 64, True, p=0.1), 1.0),  # dropout without 1 / (1 - p)
    "kv_head": (R.Case("", 1, 100, 100, 8, 2, 64, False), 1.0),           # KV head h % Hkv
    "shift": (R.Case("", 2, 129, 257, 3, 3, 64, True), 1.0),              # the Sk - Sq shift ignored
    "delta": (R.Case("", 2, 129, 129, 3, 3, 64, True), 4.0),              # delta from the unrounded O, v and dO x 4
    "dk_tile": (R.Case("", 1, 257, 257, 2, 2, 64, True), 1.0),            # query rows 64..127 counted twice in dK
}


def test_mutant_cases_are_gpu_cases():
    ids = {(c.shape(), c.causal, c.kind, c.p) for c in R.CASES if c.prec == "bf16"}
    for c, _ in MUTANTS.values():
        assert (c.shape(), c.causal, c.kind, c.p) in ids, c.id


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_check_fails_on_a_wrong_kernel(mut, capsys):
    """A correct kernel model passes the check at the recorded bounds (with no more than the
    bf16 half-ulp of its own rounding), the same model with one bug fails it."""
    c, big = MUTANTS[mut]
    good = run_model(c, None, big)
    good.finish()
    assert all(good.seen[f"attn.bf16.{n}"] <= 0.5 for n in ("o", "dq", "dk", "dv")), good.seen
    assert all(good.seen[f"attn.bf16.{n}"] <= 1e-6 for n in ("lse", "delta", "dbias")), good.seen
    bad = run_model(c, mut, big)
    with pytest.raises(AssertionError):
        bad.finish()
    over = [f for f in bad.fails if "> bound" in f or "non-zero" in f or "exactly zero" in f or "+inf" in f]
    assert over, bad.fails   # the metric itself, not only the older tolerances


# ------------------------------------------------------------------ the GPU cases' inputs
def test_case_ids_unique_and_groups_present():
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    bf = [c for c in R.CASES if c.prec == "bf16"]
    for S in (1, 7, 63, 64, 65, 127, 128, 129, 191, 257, 385):
        for D in (64, 128):
            for causal in (True, False):
                assert any(c.Sq == c.Sk == S and c.D == D and c.causal == causal and c.B * c.H == 6 for c in bf)
    assert any(c.B * c.H == 8 and c.D == 64 and c.causal for c in bf)
    for D in (8, 40, 72, 96, 192, 200, 256):
        for S in (65, 129):
            assert sum(c.Sq == c.Sk == S and c.D == D for c in bf) >= 2
    assert {c.H // c.Hkv for c in bf} >= {1, 4, 8} and any(c.Hkv == 1 for c in bf)
    assert {c.layout for c in bf} == {"packed", "q_kv", "sep", "gradstride", "bigstride"}
    branches = {x for c in bf for x in R.path(c)}
    for want in ("ks2-1iter", "ks2-loop", "fwd2x1pairodd", "fwd2x1paireven", "fwd2x2pairodd", "fwd2x2paireven",
                 "fwd1dp64", "fwd1dp128", "fwd1dp256", "short1+1", "short1+2", "short2+1", "short2+2", "short1+3"):
        assert (want in branches) == (want != "short1+3"), want
    bw = {x for b in branches for x in b.split("+")}
    assert bw >= {"dq1dp64", "dq1dp128", "dq1dp256", "dkdv1dp64", "dkdv1dp128", "dkdv1dp256", "dq3x1pairodd",
                  "dq3x2paireven", "dkdv3x2pairodd", "dq3x3", "dkdv3x3"}, bw
    # the non-default kernels
    v1 = {x for c in R.CHILD_CASES for x in "+".join(R.path(c, R.env_flags(R.CHILD_ENVS["v1"]))).split("+")}
    v2 = {x for c in R.CHILD_CASES for x in "+".join(R.path(c, R.env_flags(R.CHILD_ENVS["v2"]))).split("+")}
    assert v1 == {"fwd1dp64", "fwd1dp128", "dq1dp64", "dq1dp128", "dkdv1dp64", "dkdv1dp128"}, v1
    assert {"dq2", "dkdv2"} <= v2 and not any(x.startswith(("dq3", "dkdv3")) for x in v2), v2


def test_dp256_noncausal_backward_is_two_kernel():
    for c in R.CASES:
        if c.prec == "bf16" and c.D > 128 and not c.causal:
            assert R.path(c)[1] == "dq1dp256+dkdv1dp256"
    assert R.path(R.Case("", 1, 100, 100, 8, 2, 64, False))[1].startswith("dq3")   # short, GQA: two kernels


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_gpu_case_inputs_meet_their_conditions(c):
    B, Sq, Sk, H, Hkv, D = c.shape()
    assert B * H <= 8 and max(Sq, Sk) <= 400 and min(B, Sq, Sk, H, Hkv) > 0
    assert H % Hkv == 0 and D % 8 == 0 and D <= 256 and c.p in (0.0, 0.1, 0.3)
    if c.prec == "f32":
        assert D in R.F32_DIMS and H == Hkv and not c.causal
    if c.layout == "packed":
        assert Sq == Sk
    if c.layout == "bigstride":
        assert D == 64 and B == 1 and Sq == Sk == 128 and (Sk + 128) * R.BIG_STRIDE * 2 >= 2 ** 31
        assert (Sq + 1) * R.BIG_STRIDE * 2 < 1.15e9
    q, k, v, do = R.make_inputs(c)
    assert all(t.dtype == c.dtype and torch.isfinite(t).all() for t in (q, k, v, do))
    f = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, c.causal, c.scale)
    b = R.attn_bwd_ref(q, k, v, R.round_to(f.O, c.dtype), do, B, Sq, Sk, H, Hkv, D, c.causal, c.scale)
    for t in (f.O, b.dQ, b.dK, b.dV, b.delta, b.colsum):
        assert torch.isfinite(t).all() and float(t.abs().max()) < 1e4
    n_dead = int(torch.isinf(f.lse).sum())
    assert n_dead == (B * H * (Sq - Sk) if c.causal and Sk < Sq else 0)
    s = f.S
    if c.kind == "q6":
        assert float(f.P.amax(-1).median()) > 0.5, "q x 6: the softmax is not nearly one-hot"
    if c.kind in ("rising", "falling"):
        full = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, False, c.scale).S
        tiles = [full[..., t: t + R.TILE].amax(-1) for t in range(0, Sk, R.TILE)]
        assert len(tiles) == 5
        step = torch.stack([b_ - a_ for a_, b_ in zip(tiles, tiles[1:])])
        step = step if c.kind == "rising" else -step
        assert float(step.min()) > 20.0, float(step.min())
    if c.kind == "common":
        vis = torch.isfinite(s)
        assert 45.0 < float(s[vis].min()) and float(s[vis].max()) < 75.0
        assert abs(float(s[vis].mean()) - R.COMMON) < 1.0
