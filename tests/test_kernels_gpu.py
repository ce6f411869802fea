"""HIP kernel numerics vs. the PyTorch f32 reference of the same op (SURVEY §4 tier 3).

Every GPU op in mipipe.ops is compared with its CPU/f32 implementation (which is itself
checked against torch.nn.functional in test_ops_cpu.py).  bf16 tolerances."""
import math

import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def rnd(*shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape) * scale).to(dtype)


def gelu_grad_ref(a):
    """d/dx of tanh-GELU (f32), what the GELU GEMM epilogue saves for the backward."""
    k0, k1 = 0.7978845608028654, 0.044715
    t = torch.tanh(k0 * (a + k1 * a ** 3))
    return 0.5 * (1 + t) + 0.5 * a * (1 - t * t) * k0 * (1 + 3 * k1 * a * a)


def close(a, b, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("kind", ["layernorm", "rmsnorm"])
@pytest.mark.parametrize("D", [64, 768, 1024, 4096])
@pytest.mark.parametrize("branch", [False, True])
def test_norm_fwd_bwd(kind, D, branch):
    torch.manual_seed(0)
    T = 257
    x, w = rnd(T, D), rnd(D, scale=0.5) + 1
    bias = rnd(D, scale=0.1) if kind == "layernorm" else None
    br = rnd(T, D) if branch else None
    dy, dres = rnd(T, D), rnd(T, D)
    outs = []
    for dev in ("cpu", DEV):
        mv = lambda t: None if t is None else t.to(dev)
        y, s, mean, rstd = ops.norm_fwd(mv(x), mv(w), mv(bias), mv(br), kind=kind)
        dw = torch.zeros(D, device=dev)
        db = torch.zeros(D, device=dev) if bias is not None else None
        ds, _ = ops.norm_bwd(mv(dy), s, mv(w), mean, rstd, kind=kind, dres=mv(dres), dw=dw, dbias=db)
        outs.append((y, s, mean, rstd, ds, dw, db))
    for a, b in zip(*outs):
        if a is not None:
            close(b, a, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("V,Vp", [(50257, 50304), (10000, 10000), (1000, 1024), (128256, 128256)])
def test_xent(V, Vp):
    torch.manual_seed(0)
    T = 64
    logits = rnd(T, Vp, scale=3.0)
    tgt = torch.randint(0, V, (T,))
    tgt[5] = -100
    ref_l = logits.clone()
    ref = ops.xent_fwd_bwd(ref_l, tgt, V, 1.0 / T)
    gl = logits.to(DEV)
    got = ops.xent_fwd_bwd(gl, tgt.to(DEV), V, 1.0 / T)
    close(got, ref, atol=2e-3, rtol=1e-3)
    close(gl, ref_l, atol=1e-4, rtol=2e-2)
    # against torch.nn.functional
    t2 = torch.nn.functional.cross_entropy(logits[:, :V].float(), tgt, reduction="none")
    close(got, t2, atol=2e-3, rtol=1e-3)


def test_embedding():
    torch.manual_seed(0)
    V, D, S, B = 1000, 768, 64, 4
    wte, wpe = rnd(V, D), rnd(S, D)
    idx = torch.randint(0, V, (B * S,))
    ref = ops.embed_fwd(idx, wte, wpe, S)
    got = ops.embed_fwd(idx.to(DEV), wte.to(DEV), wpe.to(DEV), S)
    close(got, ref, atol=1e-2, rtol=1e-2)
    dout = rnd(B * S, D)
    dw1, dp1 = torch.zeros(V, D), torch.zeros(S, D)
    ops.embed_bwd(idx, dout, dw1, dp1, S)
    dw2, dp2 = torch.zeros(V, D, device=DEV), torch.zeros(S, D, device=DEV)
    ops.embed_bwd(idx.to(DEV), dout.to(DEV), dw2, dp2, S)
    close(dw2, dw1, atol=1e-3, rtol=1e-3)
    close(dp2, dp1, atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize("M,N,K", [(256, 384, 128), (8192 // 8, 768, 768), (300, 136, 192), (128, 10000, 64)])
@pytest.mark.parametrize("epi", ["none", "bias", "gelu", "relu", "bias_res"])
def test_linear_fwd(M, N, K, epi):
    torch.manual_seed(0)
    x, w, b, r = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1), rnd(M, N)
    kw = dict(bias=None, act="none", residual=None)
    if epi in ("bias", "gelu", "relu", "bias_res"):
        kw["bias"] = b
    if epi in ("gelu", "relu"):
        kw["act"] = "gelu_tanh" if epi == "gelu" else "relu"
    if epi == "bias_res":
        kw["residual"] = r
    ref, ref_aux = ops.linear(x, w, **kw)
    g = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    got, got_aux = ops.linear(x.to(DEV), w.to(DEV), **g)
    close(got, ref)
    if ref_aux is not None:
        close(got_aux, ref_aux)


@pytest.mark.parametrize("M,N,K", [(512, 768, 3072), (256, 384, 128), (200, 128, 136)])
@pytest.mark.parametrize("act", ["none", "gelu_tanh", "relu"])
def test_linear_dx(M, N, K, act):
    torch.manual_seed(0)
    dy, w, a = rnd(M, N), rnd(N, K, scale=N ** -0.5), rnd(M, K)
    ref = ops.linear_dx(dy, w, act_input=a if act != "none" else None, act=act)
    got = ops.linear_dx(dy.to(DEV), w.to(DEV), act_input=a.to(DEV) if act != "none" else None, act=act)
    close(got, ref)


@pytest.mark.parametrize("T,N,K", [(1024, 768, 768), (512, 2304, 768), (256, 136, 200), (128, 10000, 64)])
def test_linear_dw(T, N, K):
    torch.manual_seed(0)
    dy, x = rnd(T, N, scale=0.1), rnd(T, K)
    base = torch.randn(N, K)
    ref = ops.linear_dw(dy, x, base.clone())
    got = ops.linear_dw(dy.to(DEV), x.to(DEV), base.clone().to(DEV))
    close(got, ref, atol=2e-2, rtol=1e-2)


def test_grouped_wgrad_jobs_vs_f32():
    """run_wjobs issues the short-token DW jobs of a list as ONE grouped launch
    (gemms_tt_grouped_kernel): every problem (different N/K, strided row views, two
    halves of one gradient, alpha) must match the f32 reference; non-groupable jobs and
    plain callables still run."""
    torch.manual_seed(0)
    T = 1024
    shapes = [(2304, 768), (768, 768), (2048, 768), (768, 2048), (1536, 768), (768, 768), (8, 64), (136, 200)]
    jobs_cpu, jobs_gpu, outs = [], [], []
    big = rnd(T, 3 * 768, scale=0.1)            # row-strided column views (dq / dkv of one buffer)
    for i, (N, K) in enumerate(shapes):
        dy = big[:, :N] if i == 1 else rnd(T, N, scale=0.1)
        x = rnd(T, K)
        base = torch.randn(N, K)
        g_cpu, g_gpu = base.clone(), base.clone().to(DEV)
        jobs_cpu.append(ops.DW(dy, x, g_cpu, 0.5))
        jobs_gpu.append(ops.DW(dy.to(DEV) if i != 1 else big.to(DEV)[:, :N], x.to(DEV), g_gpu, 0.5))
        outs.append((g_cpu, g_gpu))
    gw = torch.zeros(1536, 768)
    dy2, x2 = rnd(T, 1536, scale=0.1), rnd(T, 768)
    gw_gpu = gw.clone().to(DEV)
    jobs_cpu += [ops.DW(dy2[:, :768], x2, gw[:768]), ops.DW(dy2[:, 768:], x2, gw[768:])]
    jobs_gpu += [ops.DW(dy2.to(DEV)[:, :768], x2.to(DEV), gw_gpu[:768]),
                 ops.DW(dy2.to(DEV)[:, 768:], x2.to(DEV), gw_gpu[768:])]
    assert sum(j.groupable() for j in jobs_gpu) == len(jobs_gpu)
    big_job = ops.DW(rnd(8192, 768, scale=0.1).to(DEV), rnd(8192, 768).to(DEV), torch.zeros(768, 768, device=DEV))
    assert not big_job.groupable()
    hit = []
    jobs_gpu.append(lambda: hit.append(1))
    ops.run_wjobs(jobs_gpu + [big_job])
    ops.run_wjobs(jobs_cpu)
    torch.cuda.synchronize()
    assert hit == [1]
    for g_cpu, g_gpu in outs + [(gw, gw_gpu)]:
        close(g_gpu, g_cpu, atol=2e-2, rtol=1e-2)


def test_gemm_asymmetric_layout_check():
    """A = I with an asymmetric B catches transposed C writes (cdna guide §3)."""
    n = 128
    eye = torch.eye(n, dtype=torch.bfloat16)
    B = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 61 - 30).to(torch.bfloat16)
    got, _ = ops.linear(eye.to(DEV), B.to(DEV))
    close(got, B.t().contiguous(), atol=0, rtol=0)


@pytest.mark.parametrize("act", ["gelu_tanh", "relu"])
def test_act_and_colsum(act):
    torch.manual_seed(0)
    a, dg = rnd(333, 3072), rnd(333, 3072)
    close(ops.act_fwd(a.to(DEV), act), ops.act_fwd(a, act))
    db1, db2 = torch.zeros(3072), torch.zeros(3072, device=DEV)
    r = ops.act_bwd(dg, a, act, dbias=db1)
    g = ops.act_bwd(dg.to(DEV), a.to(DEV), act, dbias=db2)
    close(g, r)
    close(db2, db1, atol=5e-2, rtol=2e-2)
    c1, c2 = torch.zeros(3072), torch.zeros(3072, device=DEV)
    close(ops.colsum(dg.to(DEV), c2), ops.colsum(dg, c1), atol=5e-2, rtol=2e-2)


def test_swiglu_and_rope():
    torch.manual_seed(0)
    T, F = 130, 1024
    gu, dy = rnd(T, 2 * F), rnd(T, F)
    close(ops.swiglu_fwd(gu.to(DEV)), ops.swiglu_fwd(gu))
    close(ops.swiglu_bwd(gu.to(DEV), dy.to(DEV)), ops.swiglu_bwd(gu, dy))
    S, H, Hkv, Dh = 65, 4, 2, 128
    qkv = rnd(2 * S, (H + 2 * Hkv) * Dh)
    cs, sn = ops.rope_tables(S, Dh, 500000.0, "cpu")
    r = ops.rope_(qkv.clone(), cs, sn, S, H, Hkv, Dh)
    g = ops.rope_(qkv.clone().to(DEV), cs.to(DEV), sn.to(DEV), S, H, Hkv, Dh)
    close(g, r)
    back = ops.rope_(g.clone(), cs.to(DEV), sn.to(DEV), S, H, Hkv, Dh, inverse=True)
    close(back, qkv, atol=3e-2, rtol=3e-2)


ATTN = [  # B, S, H, Hkv, D, causal
    (2, 256, 4, 4, 64, True), (2, 256, 4, 4, 64, False), (1, 200, 2, 2, 64, True),
    (2, 128, 8, 8, 96, False), (1, 256, 4, 2, 128, True), (1, 128, 4, 4, 192, False), (1, 1024, 2, 2, 64, True),
    (1, 200, 4, 2, 128, True), (2, 136, 4, 4, 64, False),
    # short non-causal (one-launch backward): partial second tile, one tile only, GQA (two-kernel path)
    (3, 100, 4, 4, 64, False), (2, 64, 4, 4, 128, False), (2, 128, 4, 2, 96, False),
    # forward v2 (d_h 64): paired causal blocks with the XCD grouping (B*H % 8 == 0), an odd
    # block count without it, a ragged last block, and a non-causal grid of >= 256 blocks
    (2, 1280, 4, 4, 64, True), (3, 640, 4, 2, 64, True), (1, 1000, 6, 3, 64, True), (8, 512, 8, 8, 64, False)]


@pytest.mark.parametrize("B,S,H,Hkv,D,causal", ATTN)
def test_attention_fwd_bwd(B, S, H, Hkv, D, causal):
    torch.manual_seed(0)
    T = B * S
    qkv = rnd(T, (H + 2 * Hkv) * D)
    q, k, v = qkv[:, : H * D], qkv[:, H * D:(H + Hkv) * D], qkv[:, (H + Hkv) * D:]
    do = rnd(T, H * D)
    res = {}
    for dev in ("cpu", DEV):
        Q = qkv.to(dev)
        qq, kk, vv = Q[:, : H * D], Q[:, H * D:(H + Hkv) * D], Q[:, (H + Hkv) * D:]
        o = torch.empty(T, H * D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B * H * S, device=dev)
        ops.attn_fwd(qq, kk, vv, o, lse, B, S, S, H, Hkv, D, causal)
        dqkv = torch.zeros_like(Q)
        dq, dk, dv = dqkv[:, : H * D], dqkv[:, H * D:(H + Hkv) * D], dqkv[:, (H + Hkv) * D:]
        dbias = torch.full(((H + 2 * Hkv) * D,), 0.25, device=dev)   # fused QKV bias grad (accumulates)
        ops.attn_bwd(qq, kk, vv, o, do.to(dev), lse, dq, dk, dv, B, S, S, H, Hkv, D, causal, dbias=dbias)
        res[dev] = (o, lse, dqkv, dbias)
    close(res[DEV][0], res["cpu"][0], atol=2e-2, rtol=2e-2)
    close(res[DEV][1], res["cpu"][1], atol=2e-2, rtol=1e-3)
    close(res[DEV][2], res["cpu"][2], atol=5e-2, rtol=5e-2)
    # the kernels' column sums agree with the sums of the gradients they wrote
    close(res[DEV][3], res[DEV][2].float().sum(0).cpu() + 0.25, atol=0.05 * T ** 0.5, rtol=2e-2)
    close(res[DEV][3], res["cpu"][3], atol=0.1 * T ** 0.5, rtol=5e-2)


@pytest.mark.parametrize("Sq,Sk", [(384, 512), (512, 384), (200, 328)])
def test_attention_cross_lengths_causal_d64(Sq, Sk):
    """Causal attention with Sq != Sk (query i sees keys <= i + Sk - Sq): with Sk < Sq the
    first queries see no key at all (zero output, LSE +inf) -- the forward v2 lazy rescale
    must keep those rows finite-free of NaN while later rows start from a fully masked
    running maximum."""
    torch.manual_seed(0)
    B, H, D = 2, 4, 64
    q, do = rnd(B * Sq, H * D), rnd(B * Sq, H * D)
    k, v = rnd(B * Sk, H * D), rnd(B * Sk, H * D)
    res = {}
    for dev in ("cpu", DEV):
        o = torch.empty(B * Sq, H * D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B * H * Sq, device=dev)
        ops.attn_fwd(q.to(dev), k.to(dev), v.to(dev), o, lse, B, Sq, Sk, H, H, D, True)
        res[dev] = (o.float().cpu().nan_to_num(0.0), lse.cpu())   # (the f32 softmax of no key is NaN)
    assert torch.isfinite(res[DEV][0]).all()
    close(res[DEV][0], res["cpu"][0], atol=2e-2, rtol=2e-2)
    fin = torch.isfinite(res["cpu"][1])
    assert torch.equal(fin, torch.isfinite(res[DEV][1]))
    close(res[DEV][1][fin], res["cpu"][1][fin], atol=2e-2, rtol=1e-3)


def test_attention_dropout_consistency():
    """fwd/bwd regenerate the same mask: gradient check by finite differences in f32 space
    is too noisy in bf16, so check the keep-rate and that dropout=0 reproduces no-dropout."""
    torch.manual_seed(0)
    B, S, H, D = 1, 128, 2, 64
    T = B * S
    qkv = rnd(T, 3 * H * D).to(DEV)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    o1 = torch.empty(T, H * D, dtype=torch.bfloat16, device=DEV)
    o2 = torch.empty_like(o1)
    lse = torch.empty(B * H * S, device=DEV)
    ops.attn_fwd(q, k, v, o1, lse, B, S, S, H, H, D, False, p_drop=0.0)
    ops.attn_fwd(q, k, v, o2, lse, B, S, S, H, H, D, False, p_drop=0.1, seed=7)
    assert not torch.equal(o1, o2)
    rel = (o2.float().mean() / o1.float().mean()).item()
    assert abs(rel - 1.0) < 0.2


def _keep_rate_ok(mask: torch.Tensor, p: float):
    """Bernoulli(1 - p) keep rate within 5 sigma."""
    n = mask.numel()
    rate = mask.float().mean().item()
    assert abs(rate - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n), (rate, n)


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_attention_dropout_mask_exact(p):
    """Recover the in-kernel attention dropout mask exactly: q = k = 0 makes P uniform
    (1/Sk) and V = I (Sk = D) turns O into the kept-mask rows, dO = I turns dV into its
    transpose.  The forward and backward kernels must regenerate the identical mask, at
    the requested keep rate, and differently per (batch, head)."""
    B, S, H, D = 4, 64, 4, 64
    T = B * S
    q = torch.zeros(T, H * D, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros_like(q)
    eye = torch.eye(S, D, dtype=torch.bfloat16, device=DEV)
    v = eye.repeat(B, H)                      # every (b, h) block is I
    o = torch.empty_like(q)
    lse = torch.empty(B * H * S, device=DEV)
    ops.attn_fwd(q, k, v, o, lse, B, S, S, H, H, D, False, p_drop=p, seed=1234)
    do = v.clone()
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    ops.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, S, S, H, H, D, False, p_drop=p, seed=1234)
    torch.cuda.synchronize()
    # [B, S(query), H, S(key)] masks
    m_f = (o.float().view(B, S, H, D) > 0)
    m_b = (dv.float().view(B, S, H, D) > 0).transpose(1, 3)   # dV[key, query] -> [B, query, H, key]
    assert torch.equal(m_f, m_b), "forward and backward dropout masks differ"
    _keep_rate_ok(m_f, p)
    # kept entries carry exactly P / (1 - p)
    kept = o.float().view(B, S, H, D)[m_f]
    torch.testing.assert_close(kept, torch.full_like(kept, 1.0 / (S * (1 - p))), rtol=1e-2, atol=0)
    # distinct masks per head and per batch element
    assert not torch.equal(m_f[:, :, 0], m_f[:, :, 1])
    assert not torch.equal(m_f[0], m_f[1])


@pytest.mark.parametrize("S,D,causal,B", [(128, 128, False, 2), (96, 96, False, 2), (64, 64, False, 2),
                                          (64, 64, True, 2), (64, 64, False, 64)])
def test_attention_dropout_bwd_matches_reference(S, D, causal, B):
    """Dropout attention forward + backward against an f32 reference that uses the kernels'
    own mask (recovered exactly as in test_attention_dropout_mask_exact: q = k = 0, V = I).
    Non-causal S <= 128 runs the one-launch short backward (dQ and dK/dV roles in one grid);
    causal, and non-causal grids of >= 256 blocks (B 64), run the d_h-64 v2 kernels, whose
    softmax normaliser must sum P before the dropout mask (with V = I the kept entries carry
    exactly dinv / (number of visible keys))."""
    torch.manual_seed(0)
    H, p, seed = 4, 0.1, 4321
    T = B * S
    z = torch.zeros(T, H * D, dtype=torch.bfloat16, device=DEV)
    eye = torch.eye(S, D, dtype=torch.bfloat16, device=DEV).repeat(B, H)
    om = torch.empty_like(z)
    lse = torch.empty(B * H * S, device=DEV)
    ops.attn_fwd(z, z, eye, om, lse, B, S, S, H, H, D, causal, p_drop=p, seed=seed)
    omf = om.float().view(B, S, H, S).permute(0, 2, 1, 3).cpu()                          # [B, H, q, k]
    keep = (omf > 0).float() / (1 - p)
    seen = torch.arange(1, S + 1).view(S, 1).float() if causal else torch.full((S, 1), float(S))
    kept = omf[omf > 0]
    torch.testing.assert_close(kept, ((keep / seen.view(1, 1, S, 1).expand_as(keep)))[omf > 0], rtol=1e-2, atol=0)
    q, k, v, do = (rnd(T, H * D).to(DEV) for _ in range(4))
    o = torch.empty_like(q)
    ops.attn_fwd(q, k, v, o, lse, B, S, S, H, H, D, causal, p_drop=p, seed=seed)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    dbias = torch.zeros(3 * H * D, device=DEV)
    ops.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, S, S, H, H, D, causal, p_drop=p, seed=seed, dbias=dbias)
    torch.cuda.synchronize()
    hd = lambda t: t.float().cpu().view(B, S, H, D).permute(0, 2, 1, 3)   # noqa: E731
    Q, K, V, dO, O = hd(q), hd(k), hd(v), hd(do), hd(o)
    sc = 1.0 / math.sqrt(D)
    sco = Q @ K.transpose(-1, -2) * sc
    if causal:
        sco = sco.masked_fill(torch.ones(S, S).triu(1).bool(), float("-inf"))
    P = torch.softmax(sco, -1)
    O_ref = (P * keep) @ V
    dV = (P * keep).transpose(-1, -2) @ dO
    dP = (dO @ V.transpose(-1, -2)) * keep
    dS = P * (dP - (dO * O).sum(-1, keepdim=True))
    dQ, dK = dS @ K * sc, dS.transpose(-1, -2) @ Q * sc
    close(O, O_ref, atol=2e-2, rtol=2e-2)
    for got, ref in ((dq, dQ), (dk, dK), (dv, dV)):
        close(hd(got), ref, atol=5e-2, rtol=5e-2)
    sums = torch.cat([dq.float().sum(0), dk.float().sum(0), dv.float().sum(0)]).cpu()
    close(dbias.cpu(), sums, atol=0.05 * T ** 0.5, rtol=2e-2)


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_norm_dropout_mask_exact(p):
    """Residual-branch dropout in the fused norm: x = 0, branch = 1 makes s the scaled
    keep mask; with dy = 0, dres = 1 the backward's branch gradient is the same mask."""
    T, D = 1024, 768
    x = torch.zeros(T, D, dtype=torch.bfloat16, device=DEV)
    br = torch.ones_like(x)
    w = torch.ones(D, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros_like(w)
    y, s, mean, rstd = ops.norm_fwd(x, w, b, br, kind="layernorm", p_drop=p, seed=99)
    ds, dbr = ops.norm_bwd(torch.zeros_like(x), s, w, mean, rstd, kind="layernorm", dres=torch.ones_like(x),
                           dw=torch.zeros(D, device=DEV), dbias=torch.zeros(D, device=DEV), p_drop=p, seed=99,
                           want_branch=True)
    torch.cuda.synchronize()
    m_f, m_b = s.float() != 0, dbr.float() != 0
    assert torch.equal(m_f, m_b), "forward and backward dropout masks differ"
    _keep_rate_ok(m_f, p)
    torch.testing.assert_close(s.float()[m_f], torch.full_like(s.float()[m_f], 1 / (1 - p)), rtol=1e-2, atol=0)
    torch.testing.assert_close(dbr.float()[m_b], torch.full_like(dbr.float()[m_b], 1 / (1 - p)), rtol=1e-2, atol=0)


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_act_dropout_mask_exact(p):
    """ReLU + dropout (the reference FFN): a = 1 makes the output the scaled keep mask, and
    act_bwd with dg = 1 must return the identical mask."""
    T, F = 1024, 3072
    a = torch.ones(T, F, dtype=torch.bfloat16, device=DEV)
    out = ops.act_fwd(a, "relu", p_drop=p, seed=5)
    da = ops.act_bwd(torch.ones_like(a), a, "relu", p_drop=p, seed=5)
    torch.cuda.synchronize()
    m_f, m_b = out.float() != 0, da.float() != 0
    assert torch.equal(m_f, m_b), "forward and backward dropout masks differ"
    _keep_rate_ok(m_f, p)


def test_adamw():
    torch.manual_seed(0)
    n = 10007
    p, g = torch.randn(n), torch.randn(n)
    m, v = torch.zeros(n), torch.zeros(n)
    ref = [t.clone() for t in (p, g, m, v)]
    w16 = torch.empty(n, dtype=torch.bfloat16)
    ops.adamw_(*ref, w16, 5000, 1e-3, 0.9, 0.95, 1e-8, 0.1, 1)
    gp = [t.clone().to(DEV) for t in (p, g, m, v)]
    gw = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    ops.adamw_(*gp, gw, 5000, 1e-3, 0.9, 0.95, 1e-8, 0.1, 1)
    for a, b in zip(gp, ref):
        close(a, b, atol=1e-5, rtol=1e-5)
    close(gw, w16, atol=1e-2, rtol=1e-2)
    ss = torch.zeros(1, device=DEV)
    ops.sumsq(g.to(DEV), ss)
    assert abs(ss.item() - (g.double() ** 2).sum().item()) / ss.item() < 1e-4


def _probe_engines():
    from mipipe.ops import kernels as _k
    return bool(_k.load_ext().gemm2_has_probe_engines())


needs_probe_engines = pytest.mark.skipif("not __import__('os').environ.get('MIPIPE_EXT_VARIANT') == 'probes'",
                                         reason="gemm4 / gemm5 live in the A/B variant build only "
                                                "(tools/build_ext.py --variant probes -D MP_PROBE_ENGINES)")


def test_default_build_has_no_probe_engines():
    """The production extension carries no null-result probe engines (gemm4 / gemm5)."""
    import os
    if os.environ.get("MIPIPE_EXT_VARIANT"):
        pytest.skip("variant build loaded")
    assert not _probe_engines()


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, pytest.param(8, marks=needs_probe_engines), 9, 10, 11, 12, 15, 16])
@pytest.mark.parametrize("M,N,K,epi", [(512, 768, 768, "bias_gelu"), (1000, 2304, 256, "bias"), (256, 384, 128, "res"),
                                       (520, 136, 64, "none"), (512, 768, 3072, "dgelu"), (1000, 1000, 640, "none"),
                                       (768, 512, 128, "bias")])
def test_gemm2_configs(cfg, M, N, K, epi):
    from mipipe.ops import kernels as _k
    torch.manual_seed(0)
    x, w, b, r = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1), rnd(M, N)
    xg, wg, bg, rg = (t.to(DEV) for t in (x, w, b, r))
    y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    aux = rnd(M, N).to(DEV)
    epi_id = dict(none=0, bias=1, bias_gelu=2, res=5, dgelu=6)[epi]
    _k._gemm(xg, wg, y, bias=bg if "bias" in epi else None, residual=rg if epi == "res" else None,
             aux=aux if "gelu" in epi else None, epi=epi_id, cfg=cfg)
    ref = x.float() @ w.float().t()
    if "bias" in epi:
        ref = ref + b.float()
    if epi == "bias_gelu":
        # aux: GELU's derivative at the (bf16-rounded) pre-activation
        close(aux, gelu_grad_ref(ref.to(torch.bfloat16).float()).to(torch.bfloat16))
        ref = torch.nn.functional.gelu(ref.to(torch.bfloat16).float(), approximate="tanh")
    if epi == "res":
        ref = ref + r.float()
    if epi == "dgelu":
        ref = ref * aux.float().cpu()          # aux holds the saved GELU derivative
    close(y, ref)


@needs_probe_engines
@pytest.mark.parametrize("M,N,K,epi", [(8192, 768, 768, "bias"), (4000, 1000, 640, "none"),
                                       (32768, 768, 2304, "bias_gelu"), (24576, 768, 3072, "res"),
                                       (8192, 768, 2304, "dgelu"), (8192, 768, 3072, "colsum")])
def test_gemm7_stream_k(M, N, K, epi):
    """gemm7 (the partial round split into K chunks over all CUs, XCD-grouped, sc1 partial
    hand-off; whole rounds first as a gemm3 launch on the leading tiles): grids of 64-384
    tiles incl. ragged M / N edges, every fused epilogue class, the fused column sums; also
    bit-for-bit stable across repeated launches (each tile's partials are summed in a fixed
    order) -- which also checks the self-clearing hand-off flags of the previous launch."""
    from mipipe.ops import kernels as _k
    e = _k.load_ext()
    assert e.gemm2_plan(M, N, K, False, False, False, 14)[0] == 14, "split-tail engine should accept this grid"
    torch.manual_seed(0)
    x, w, b, r = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1), rnd(M, N)
    xg, wg, bg, rg = (t.to(DEV) for t in (x, w, b, r))
    y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    aux = rnd(M, N).to(DEV)
    epi_id = dict(none=0, bias=1, bias_gelu=2, res=5, dgelu=6, colsum=0)[epi]
    cs = torch.zeros(N, device=DEV) if epi == "colsum" else None
    run = lambda out: _k._gemm(xg, wg, out, bias=bg if "bias" in epi else None,  # noqa: E731
                               residual=rg if epi == "res" else None, aux=aux if "gelu" in epi else None,
                               epi=epi_id, colsum=cs, cfg=14)
    run(y)
    ref = x.float() @ w.float().t()
    if "bias" in epi:
        ref = ref + b.float()
    if epi == "bias_gelu":
        # aux: GELU's derivative at the (bf16-rounded) pre-activation
        close(aux, gelu_grad_ref(ref.to(torch.bfloat16).float()).to(torch.bfloat16))
        ref = torch.nn.functional.gelu(ref.to(torch.bfloat16).float(), approximate="tanh")
    if epi == "res":
        ref = ref + r.float()
    if epi == "dgelu":
        ref = ref * aux.float().cpu()          # aux holds the saved GELU derivative
    close(y, ref)
    if cs is not None:
        torch.testing.assert_close(cs.cpu(), y.float().sum(0).cpu(), rtol=2e-2, atol=2e-1 * M ** 0.5 * 1e-1)
    if epi in ("none", "bias", "res"):
        y2 = torch.empty_like(y)
        for _ in range(3):
            run(y2)
        torch.cuda.synchronize()
        assert torch.equal(y, y2)


@needs_probe_engines
@pytest.mark.parametrize("cfg", [7, 108, 103])
@pytest.mark.parametrize("M,N,K", [(1024, 768, 768), (1000, 776, 512), (520, 264, 64), (1536, 1280, 128),
                                   (2048, 512, 1344)])
@pytest.mark.parametrize("epi", ["none", "bias"])
def test_gemm4_persistent_deferred_store(cfg, M, N, K, epi):
    """gemm4 (persistent 256x256 NT, part of each tile's C written during the next tile's
    main loop) vs f32: 7 = default grid, 100 + G = G workgroups, so small problems walk
    several tiles per workgroup (deferred stores, short-K flushes, M/N edges)."""
    from mipipe.ops import kernels as _k
    torch.manual_seed(0)
    x, w, b = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1)
    y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    alpha = 0.5 if K == 512 else 1.0
    _k._gemm(x.to(DEV), w.to(DEV), y, bias=b.to(DEV) if epi == "bias" else None, epi=1 if epi == "bias" else 0,
             cfg=cfg, alpha=alpha)
    ref = alpha * (x.float() @ w.float().t())
    if epi == "bias":
        ref = ref + b.float()
    assert not torch.isnan(y.float()).any(), "unwritten outputs"
    close(y, ref)


@pytest.mark.parametrize("cfg", [0, 2, 3, 6, 13, -1])
@pytest.mark.parametrize("M,N,K", [(768, 768, 8192), (2304, 768, 1024), (136, 200, 512), (3072, 768, 2048), (1000, 776, 1024),
                                   (768, 2048, 1024)])
def test_gemm2_dw_splitk(cfg, M, N, K):
    from mipipe.ops import kernels as _k
    torch.manual_seed(0)
    dy, x = rnd(K, M, scale=0.1), rnd(K, N)
    base = torch.randn(M, N)
    g = base.clone().to(DEV)
    _k._gemm(dy.to(DEV), x.to(DEV), g, transA=True, transB=True, accum=True, cfg=cfg)
    close(g, base + dy.float().t() @ x.float(), atol=3e-2, rtol=1e-2)


@pytest.mark.parametrize("cfg", [-1, 1, 4, 5, 9, 10])
@pytest.mark.parametrize("M,N,K", [(512, 768, 50304), (2048, 768, 8192), (300, 200, 4096)])
def test_gemm2_nt_splitk_accumulate(cfg, M, N, K):
    """Both-K-contiguous operands into an f32 accumulator with split-K (distributed-head dX)."""
    from mipipe.ops import kernels as _k
    torch.manual_seed(0)
    a, b = rnd(M, K, scale=0.1), rnd(N, K)
    base = torch.randn(M, N)
    g = base.clone().to(DEV)
    _k._gemm(a.to(DEV), b.to(DEV), g, accum=True, cfg=cfg)
    close(g, base + a.float() @ b.float().t(), atol=5e-2, rtol=1e-2)


@pytest.mark.parametrize("cfg", [10, 11, 12, 1, 9, -1])
@pytest.mark.parametrize("M,N,K", [(1024, 768, 768), (1024, 2304, 768), (1000, 2048, 768), (1024, 768, 2048)])
def test_gemm_small_engine_bias_relu_and_colsum(cfg, M, N, K):
    """Small-tile NT engine (reference-model 1024-token shapes): fused bias + ReLU with the
    pre-activation in aux, and the fused output column sums (-1: the planner's pick)."""
    from mipipe.ops import kernels as _k
    torch.manual_seed(0)
    x, w, b = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    _k._gemm(x.to(DEV), w.to(DEV), y, bias=b.to(DEV), aux=aux, epi=3, cfg=cfg)
    pre = x.float() @ w.float().t() + b.float()
    close(aux, pre.to(torch.bfloat16))
    close(y, torch.relu(pre.to(torch.bfloat16).float()))
    cs = torch.zeros(N, device=DEV)
    y2 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    _k._gemm(x.to(DEV), w.to(DEV), y2, cfg=cfg, colsum=cs)
    ref = x.float() @ w.float().t()
    close(y2, ref)
    close(cs, y2.float().sum(0), atol=5e-1, rtol=2e-2)


def test_linear_dx_with_transposed_weight():
    torch.manual_seed(0)
    dy, w, a = rnd(1024, 2304), rnd(2304, 768, scale=0.02), rnd(1024, 768)
    wt = ops.transpose(w.to(DEV))
    close(wt, w.t().contiguous(), atol=0, rtol=0)
    ref = ops.linear_dx(dy, w, act_input=a, act="gelu_tanh")
    got = ops.linear_dx(dy.to(DEV), w.to(DEV), act_input=a.to(DEV), act="gelu_tanh", wt=wt)
    close(got, ref)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("D", [768, 2048])
def test_norm_bwd_branch_colsum(p_drop, D):
    """colsum_branch: the column sums of the (dropout-masked) branch gradient accumulate
    in the norm backward pass itself (the reference block's out_proj / linear2 bias grads)."""
    torch.manual_seed(0)
    T = 1024
    x, w, b = rnd(T, D), rnd(D, scale=0.5) + 1, rnd(D, scale=0.1)
    dy = rnd(T, D)
    xg, wg, bg, dyg = (t.to(DEV) for t in (x, w, b, dy))
    y, s_, mean, rstd = ops.norm_fwd(xg, wg, bg, kind="layernorm", eps=1e-5)
    cs = torch.zeros(D, device=DEV)
    dw, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    ds, dbr = ops.norm_bwd(dyg, xg, wg, mean, rstd, dw=dw, dbias=db, p_drop=p_drop, seed=7, want_branch=True,
                           colsum_branch=cs)
    close(cs, dbr.float().sum(0), atol=5e-1, rtol=2e-2)
    ref_ds, ref_br = ops.norm_bwd(dyg, xg, wg, mean, rstd, dw=torch.zeros(D, device=DEV),
                                  dbias=torch.zeros(D, device=DEV), p_drop=p_drop, seed=7, want_branch=True)
    close(ds, ref_ds, atol=0, rtol=0)
    close(dbr, ref_br, atol=0, rtol=0)


def test_norm_bwd_fused_colsums():
    torch.manual_seed(0)
    T, D = 300, 768
    x, w, b = rnd(T, D), rnd(D, scale=0.5) + 1, rnd(D, scale=0.1)
    dy, dres = rnd(T, D), rnd(T, D)
    outs = []
    for dev in ("cpu", DEV):
        mv = lambda t: t.to(dev)
        y, s, mean, rstd = ops.norm_fwd(mv(x), mv(w), mv(b))
        dw, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        c1, c2 = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        ds, _ = ops.norm_bwd(mv(dy), s, mv(w), mean, rstd, dres=mv(dres), dw=dw, dbias=db, colsum_dres=c1,
                             colsum_ds=c2)
        outs.append((ds, dw, db, c1, c2))
    for a, g in zip(*outs):
        close(g, a, atol=5e-2, rtol=2e-2)


def test_native_rccl_engine_self_transfer():
    """csrc/comm/rccl_engine.cpp: a one-rank engine sends to itself (grouped send+recv on
    the p2p channels' comm streams, stream-ordered completion), runs its collectives on the
    collective channel, reuses the process-wide comm streams, and only one RCCL is loaded."""
    from mipipe.ops import kernels as _k
    from mipipe.parallel.comm import load_native_rccl
    ext = _k.load_ext()
    load_native_rccl(ext)
    dev = torch.cuda.current_device()
    uid = lambda k: b"".join(ext.RcclEngine.unique_id() for _ in range(k))
    eng = ext.RcclEngine(uid(3), 1, 0, dev, [0, 1, 2])
    assert eng.channels == 3 and len({eng.stream_handle(c) for c in range(3)}) == 3
    assert [eng.stream_handle(c) for c in range(3)] == [ext.comm_stream(dev, c) for c in range(3)]
    src = torch.randn(1 << 20, device=DEV).to(torch.bfloat16)
    dst = torch.empty_like(src)
    src2 = torch.arange(1000, device=DEV, dtype=torch.int64)
    dst2 = torch.zeros_like(src2)
    h = eng.post(0, [(src, 0)], [(dst, 0)])          # channel 0 (activations)
    h2 = eng.post(1, [(src2, 0)], [(dst2, 0)])       # channel 1 (gradients)
    g = torch.randn(4096, device=DEV)
    ref = g.clone()
    h3 = eng.coll(2, 0, g, g)                        # all-reduce (1 rank: identity), in place
    out = torch.empty(4096, device=DEV)
    h4 = eng.coll(2, 2, g, out)                      # all-gather into another buffer
    mx = torch.tensor([3.0], device=DEV)
    h5 = eng.coll(2, 3, mx, mx)                      # all-reduce max
    # reduce-scatter (the ZeRO-1 head / DP gradient path): 1 rank -> send numel == recv
    # numel, in place (recv = send[0:n]) and into another buffer, f32 and bf16
    rs = torch.randn(8192, device=DEV)
    rs_ref = rs.clone()
    h6 = eng.coll(2, 1, rs, rs[:8192])
    rs16 = torch.randn(8192, device=DEV).to(torch.bfloat16)
    rs16_out = torch.empty_like(rs16)
    h7 = eng.coll(2, 1, rs16, rs16_out)
    for x in (h, h2, h3, h4, h5, h6, h7):
        eng.wait(x)
    torch.cuda.synchronize()
    assert torch.equal(dst, src) and torch.equal(dst2, src2)
    assert torch.equal(g, ref) and torch.equal(out, ref) and float(mx) == 3.0
    assert torch.equal(rs, rs_ref) and torch.equal(rs16_out, rs16)
    assert eng.query(h) and eng.query(h2)
    # non-consuming waits (microbatch lanes): two streams wait on one group, then release
    src3 = torch.randn(1 << 16, device=DEV)
    dst3 = torch.empty_like(src3)
    h8 = eng.post(0, [(src3, 0)], [(dst3, 0)])
    side = torch.cuda.Stream()
    eng.wait_keep(h8)
    with torch.cuda.stream(side):
        eng.wait_keep(h8)
        out_side = dst3 * 2.0
    torch.cuda.current_stream().wait_stream(side)
    out_main = dst3 * 3.0
    eng.release(h8)
    eng.release(h8)     # idempotent
    torch.cuda.synchronize()
    assert torch.equal(out_side, src3 * 2.0) and torch.equal(out_main, src3 * 3.0)
    assert eng.async_error() == ""
    eng.close()
    # a second engine (e.g. the DP group's, one channel on the collective slot) reuses the
    # process-wide streams: no stream per engine, no drift of the hardware-queue mapping
    eng2 = ext.RcclEngine(uid(1), 1, 0, dev, [2])
    assert eng2.stream_handle(0) == ext.comm_stream(dev, 2)
    eng2.close()
    with open("/proc/self/maps") as f:
        libs = {line.split()[-1] for line in f if "librccl" in line}
    assert len(libs) == 1, libs


def test_native_rccl_engine_reports_incomplete_groups():
    """a stalled step's watchdog report names the transfer it waits on. A
    group held behind a spinning compute kernel shows in progress() (channel, kind, peers,
    bytes, age) and in comm_progress_report; once it completes the list is empty."""
    from mipipe.ops import kernels as _k
    from mipipe.parallel.comm import comm_progress_report, load_native_rccl
    ext = _k.load_ext()
    load_native_rccl(ext)
    dev = torch.cuda.current_device()
    eng = ext.RcclEngine(b"".join(ext.RcclEngine.unique_id() for _ in range(3)), 1, 0, dev, [0, 1, 2])
    src = torch.randn(1 << 18, device=DEV)
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    n0 = eng.issued()
    torch.cuda._sleep(200_000_000)                  # ~0.1 s spin on the compute stream
    h = eng.post(1, [(src, 0)], [(dst, 0)])          # ordered after the spin
    g = torch.ones(1024, device=DEV)
    h2 = eng.coll(2, 0, g, g)
    pend = eng.progress()
    assert eng.issued() == n0 + 2
    assert [d["kind"] for d in pend] == ["p2p", "all_reduce"], pend
    assert pend[0]["channel"] == 1 and pend[0]["sends"] == [0] and pend[0]["recvs"] == [0]
    assert pend[0]["bytes"] == 2 * src.numel() * 4 and pend[1]["bytes"] == 4096
    rep = comm_progress_report({"p2p": eng, "dp": None})
    assert "2 incomplete" in rep and "channel 1 p2p send->[0] recv<-[0]" in rep, rep
    for x in (h, h2):
        eng.wait(x)
    torch.cuda.synchronize()
    assert eng.progress() == [] and torch.equal(dst, src)
    assert "0 incomplete" in comm_progress_report({"p2p": eng})
    eng.close()


def test_native_rccl_engines_interleaved_from_two_threads():
    """VERDICT r4 #6b: the concurrency shape of the first multi-GPU run inside one process --
    two engines of three 1-rank communicators each (the second maps its channels onto the
    three comm stream slots in the reverse order), driven from two host threads on their own
    compute streams, each interleaving grouped posts and collectives over all channels in a
    different order every iteration.  Every transfer must land and no thread may stall
    (1-rank transfers cannot deadlock on peers, so this checks communicator / stream
    co-residency and the process-wide stream slots under concurrent issue)."""
    import threading
    from mipipe.ops import kernels as _k
    from mipipe.parallel.comm import load_native_rccl
    ext = _k.load_ext()
    load_native_rccl(ext)
    dev = torch.cuda.current_device()
    uid = lambda k: b"".join(ext.RcclEngine.unique_id() for _ in range(k))
    engines = [ext.RcclEngine(uid(3), 1, 0, dev, [0, 1, 2]), ext.RcclEngine(uid(3), 1, 0, dev, [2, 1, 0])]
    assert engines[1].stream_handle(0) == engines[0].stream_handle(2)
    errors = []

    def work(i):
        try:
            torch.cuda.set_device(dev)
            eng = engines[i]
            with torch.cuda.stream(torch.cuda.Stream()):
                for it in range(40):
                    order = [0, 1, 2] if (it + i) % 2 == 0 else [2, 0, 1]
                    want, got, hs = [], [], []
                    for c in order:
                        src = torch.full((1 << 15,), float(100 * it + 10 * i + c), device=DEV)
                        if c == 1:     # a collective (1 rank: all-reduce = identity, in place)
                            hs.append(eng.coll(c, 0, src, src))
                            want.append(src.clone())
                            got.append(src)
                        else:
                            dst = torch.empty_like(src)
                            hs.append(eng.post(c, [(src, 0)], [(dst, 0)]))
                            want.append(src)
                            got.append(dst)
                    for h in hs:
                        eng.wait(h)
                    torch.cuda.current_stream().synchronize()
                    for w_, g_ in zip(want, got):
                        if not torch.equal(w_, g_):
                            errors.append((i, it))
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in ts), "an issuing thread stalled"
    assert not errors, errors[:5]
    for eng in engines:
        assert eng.async_error() == ""
        eng.close()


def test_queue_probe_detects_shared_and_separate_queues():
    """csrc/kernels/probe.hip: the bounded spinner sees the flag store of another stream
    when the two streams run on separate hardware queues, and times out (never hangs) when
    the store is queued behind it on the SAME stream (a queue shared by construction)."""
    from mipipe.parallel.queues import check_comm_queues, shares_queue
    dev = torch.device(DEV)
    s1 = torch.cuda.Stream(priority=-1)
    shared, us = shares_queue(s1.cuda_stream, s1.cuda_stream, dev, timeout_us=5000)
    assert shared and us >= 4000, (shared, us)
    rep = check_comm_queues(dev, timeout_us=20000)
    assert set(rep["pairs"]) >= {"comm:fwd|comm:bwd", "comm:fwd|compute", "comm:coll|dw_side"}
    print(rep)


@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 5, 15])
@pytest.mark.parametrize("epi", ["dgelu", "none", "res"])
def test_gemm_fused_colsum(cfg, epi):
    """Output column sums accumulated in the GEMM epilogue (the next layer's bias grad);
    configs without the fused path (256x192) fall back to a separate pass."""
    from mipipe.ops import kernels as _k
    torch.manual_seed(1)
    M, N, K = 1024, 768, 512
    x, w, r, aux = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(M, N), rnd(M, N)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    cs = torch.full((N,), 0.5, device=DEV)
    epi_id = dict(none=0, res=5, dgelu=6)[epi]
    _k._gemm(x.to(DEV), w.to(DEV), y, residual=r.to(DEV) if epi == "res" else None,
             aux=aux.to(DEV) if epi == "dgelu" else None, epi=epi_id, cfg=cfg, colsum=cs)
    ref = y.float().cpu().sum(0) + 0.5
    close(cs, ref, atol=0.05 * (M ** 0.5), rtol=2e-2)


@pytest.mark.parametrize("cfg", [-1, 10, 11, 5, 15])
def test_gemm_dropout_epilogues_match_act_kernels(cfg):
    """Reference FFN fusions: linear1 + bias + ReLU + dropout in the GEMM epilogue equals
    linear1 -> act_fwd(relu, p); the linear2 dX GEMM with dReLU x mask (+ the linear1 bias
    grad column sums) equals dX -> act_bwd(relu, p, dbias) -- same masks (seed, element
    index, device step counter)."""
    from mipipe.ops import kernels as _k
    torch.manual_seed(0)
    T, D, F, p = 1024, 768, 2048, 0.1
    ops.set_dropout_step(3, torch.device(DEV))
    x, w1, b1 = rnd(T, D).to(DEV), rnd(F, D, scale=D ** -0.5).to(DEV), rnd(F, scale=0.1).to(DEV)
    out = torch.empty(T, F, dtype=torch.bfloat16, device=DEV)
    aux = torch.empty(T, F, dtype=torch.bfloat16, device=DEV)
    _k._gemm(x, w1, out, bias=b1, aux=aux, epi=3, cfg=cfg, p_drop=p, seed=1234)
    a, _ = ops.linear(x, w1, b1)
    ref = ops.act_fwd(a, "relu", p_drop=p, seed=1234)
    close(aux, a, atol=2e-2, rtol=2e-2)     # another engine may have computed `a`
    close(out, ref, atol=2e-2, rtol=2e-2)
    keep = (out != 0) | (ref == 0)
    assert keep.float().mean() > 0.999
    df, w2 = rnd(T, D).to(DEV), rnd(D, F, scale=F ** -0.5).to(DEV)
    w2t = ops.transpose(w2)
    cs = torch.zeros(F, device=DEV)
    da = ops.linear_dx(df, w2, act_input=aux, act="relu", wt=w2t, colsum=cs, p_drop=p, seed=99)
    dg = ops.linear_dx(df, w2, wt=w2t)
    cs_ref = torch.zeros(F, device=DEV)
    da_ref = ops.act_bwd(dg, aux, "relu", dbias=cs_ref, p_drop=p, seed=99)
    close(da, da_ref, atol=2e-2, rtol=2e-2)
    close(cs, cs_ref, atol=0.5, rtol=2e-2)


@pytest.mark.parametrize("M,N,K", [(1024, 2304, 768), (256, 128, 32), (1000, 776, 516), (132, 260, 100)])
@pytest.mark.parametrize("a_t,b_t", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_f32_mfma(M, N, K, a_t, b_t):
    """gemm_f32 (v_mfma_f32_32x32x2_f32) vs an f64 reference, every operand layout
    (K- or M-contiguous A, N- or K-contiguous B), tile edges, bias, accumulate."""
    torch.manual_seed(0)
    A = torch.randn(M, K, dtype=torch.float64)
    B = torch.randn(K, N, dtype=torch.float64)
    bias = torch.randn(N, dtype=torch.float64)
    Ag = (A.t().contiguous().to(DEV).float().t() if a_t else A.to(DEV).float())
    Bg = (B.t().contiguous().to(DEV).float().t() if b_t else B.to(DEV).float())
    C = torch.full((M, N), 0.5, device=DEV)
    assert _ext_call(Ag, Bg, C, bias.float().to(DEV), 0.75, True) == 1
    ref = 0.5 + 0.75 * (A @ B) + bias
    err = (C.double().cpu() - ref).abs().max().item()
    scale = (A.abs() @ B.abs()).max().item()
    assert err < 2e-6 * scale, (err, scale)


def _ext_call(A, B, C, bias, alpha, acc):
    return ops.load_ext().gemm_f32(A, B, C, bias, alpha, acc)


def test_linear_f32_autograd_matches_aten():
    torch.manual_seed(0)
    torch.backends.cuda.matmul.allow_tf32 = False
    x = torch.randn(8, 128, 768, device=DEV, requires_grad=True)
    w = torch.randn(2048, 768, device=DEV, requires_grad=True)
    b = torch.randn(2048, device=DEV, requires_grad=True)
    gy = torch.randn(8, 128, 2048, device=DEV)
    y = ops.linear_f32(x, w, b)
    y.backward(gy)
    g1 = [t.grad.clone() for t in (x, w, b)]
    for t in (x, w, b):
        t.grad = None
    y2 = torch.nn.functional.linear(x, w, b)
    y2.backward(gy)
    torch.testing.assert_close(y, y2, rtol=1e-5, atol=1e-4)
    for a_, b_ in zip(g1, (x.grad, w.grad, b.grad)):
        torch.testing.assert_close(a_, b_, rtol=1e-5, atol=2e-3)
