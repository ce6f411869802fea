"""The float64 references of membound_refs.py against torch.nn.functional and against the
CPU branch of the matching ``ops`` wrapper, at a few of the shapes the GPU edge tests use.
This is what validates the oracle of test_membound_edges_gpu.py on a machine without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import mipipe  # noqa: F401
from mipipe import ops

import membound_refs as R


def close64(a, b, atol, rtol=0.0):
    torch.testing.assert_close(a.double(), b.double(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("V,Vp", [(5, 8), (1000, 1024), (4093, 4096)])
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_xent_ref(V, Vp, ignore_index):
    torch.manual_seed(0)
    T = 8
    logits = torch.randn(T, Vp) * 5
    tgt = torch.randint(0, V, (T,))
    tgt[1], tgt[2], tgt[6] = V - 1, 0, ignore_index
    loss, grad = R.xent(logits, tgt, V, 0.125, ignore_index)
    lg = logits[:, :V].double().requires_grad_()
    ref = F.cross_entropy(lg, tgt, reduction="none", ignore_index=ignore_index)
    (ref.sum() * 0.125).backward()
    close64(loss, ref.detach(), 1e-12)
    close64(grad[:, :V], lg.grad, 1e-14)
    assert torch.count_nonzero(grad[:, V:]) == 0
    ign = tgt == ignore_index
    assert ign.any() and torch.count_nonzero(grad[ign]) == 0 and torch.count_nonzero(loss[ign]) == 0
    # the wrapper's CPU branch (f32 math)
    buf = logits.clone()
    l32 = ops.xent_fwd_bwd(buf, tgt, V, 0.125, ignore_index=ignore_index)
    close64(l32, loss, 2e-5)
    close64(buf, grad, 1e-6)


@pytest.mark.parametrize("kind", ["layernorm", "rmsnorm"])
@pytest.mark.parametrize("rows,D,eps", [(3, 8, 1e-5), (257, 520, 1e-6), (5, 1544, 1e-5)])
def test_norm_ref(kind, rows, D, eps):
    torch.manual_seed(0)
    x, br = torch.randn(rows, D), torch.randn(rows, D)
    w, b = torch.randn(D) * 0.5 + 1, (torch.randn(D) * 0.1 if kind == "layernorm" else None)
    dy, dres = torch.randn(rows, D), torch.randn(rows, D)
    y, mean, rstd, s = R.norm_fwd(x, w, b, br, kind, eps)
    close64(s, (x + br), 0.0)
    # autograd through torch's own norm, in float64
    s64 = s.clone().requires_grad_()
    w64 = w.double().requires_grad_()
    b64 = b.double().requires_grad_() if b is not None else None
    if kind == "layernorm":
        yt = F.layer_norm(s64, (D,), w64, b64, eps)
        close64(mean, s.mean(-1), 1e-14)
        close64(rstd, (s.var(-1, unbiased=False) + eps).rsqrt(), 1e-12)
    else:
        yt = s64 * torch.rsqrt(s64.pow(2).mean(-1, keepdim=True) + eps) * w64
        assert mean is None
    close64(y, yt.detach(), 1e-12)
    (yt * dy.double()).sum().backward()
    ds, dw, db, cs_res, cs_ds = R.norm_bwd(dy, s.float(), w, None if mean is None else mean.float(), rstd.float(),
                                           kind, dres)
    # the reference backward reads f32 mean / rstd like the kernel: f32 rounding of those only
    close64(ds, s64.grad + dres.double(), 1e-5)
    close64(dw, w64.grad, 1e-4)
    if b64 is not None:
        close64(db, b64.grad, 1e-12)
    close64(cs_res, dres.double().sum(0), 1e-12)
    close64(cs_ds, ds.float().double().sum(0), 1e-12)
    # the wrapper's CPU branch
    y32, s32, m32, r32 = ops.norm_fwd(x, w, b, br, kind=kind, eps=eps)
    close64(y32, y, 2e-5)
    close64(s32, s, 0.0)
    close64(r32, rstd, 1e-5, 1e-5)
    if mean is not None:
        close64(m32, mean, 1e-6)
    dw32, db32 = torch.zeros(D), (torch.zeros(D) if b is not None else None)
    c1, c2 = torch.ones(D), torch.ones(D)
    ds32, _ = ops.norm_bwd(dy, s32, w, m32, r32, kind=kind, dres=dres, dw=dw32, dbias=db32, colsum_dres=c1,
                           colsum_ds=c2)
    ds_r, dw_r, db_r, cr_r, cd_r = R.norm_bwd(dy, s32, w, m32, r32, kind, dres)
    close64(ds32, ds_r, 2e-5)
    close64(dw32, dw_r, 1e-3 * rows ** 0.5)
    if b is not None:
        close64(db32, db_r, 1e-4)
    close64(c1, cr_r + 1, 1e-4)
    close64(c2, cd_r + 1, 1e-4)


@pytest.mark.parametrize("D,T,S,pos,with_pe", [(8, 1, 1, 17, True), (520, 257, 16, 48, True), (768, 257, 64, 0, False)])
def test_embedding_ref(D, T, S, pos, with_pe):
    torch.manual_seed(0)
    V = 50
    wte = torch.randn(V, D)
    wpe = torch.randn(min(T, S) + pos, D) if with_pe else None
    idx = torch.randint(0, V, (T,))
    idx[::2] = V - 1
    e = R.embed_fwd(idx, wte, wpe, S, pos)
    pid = torch.arange(T) % S + pos
    want = F.embedding(idx, wte).double()
    if with_pe:
        want = want + F.embedding(pid, wpe).double()
    close64(e, want, 0.0)
    close64(ops.embed_fwd(idx, wte, wpe, S, pos), e, 1e-6)
    dout = torch.randn(T, D)
    a0, b0 = torch.randn(V, D), (torch.randn_like(wpe) if with_pe else None)
    dwte, dwpe = R.embed_bwd(idx, dout, a0, b0, S, pos)
    wl, pl = wte.double().requires_grad_(), (wpe.double().requires_grad_() if with_pe else None)
    out = F.embedding(idx, wl) + (F.embedding(pid, pl) if with_pe else 0)
    (out * dout.double()).sum().backward()
    close64(dwte, a0.double() + wl.grad, 1e-12)
    a1, b1 = a0.clone(), (b0.clone() if with_pe else None)
    ops.embed_bwd(idx, dout, a1, b1, S, pos)
    close64(a1, dwte, 1e-4)
    if with_pe:
        close64(dwpe, b0.double() + pl.grad, 1e-12)
        close64(b1, dwpe, 1e-4)


def test_activation_refs():
    x = torch.cat([torch.linspace(-12, 12, 1537), torch.tensor([30.0, -30.0, 0.0, -0.0])])
    xl = x.double().requires_grad_()
    g = F.gelu(xl, approximate="tanh")
    g.sum().backward()
    close64(R.act(x, "gelu_tanh"), g.detach(), 1e-14)
    close64(R.act_grad(x, "gelu_tanh"), xl.grad, 1e-13)
    close64(R.act(x, "relu"), F.relu(x.double()), 0.0)
    close64(R.act_grad(x, "relu"), (x > 0).double(), 0.0)
    for kind in ("gelu_tanh", "relu"):
        close64(ops.act_fwd(x, kind), R.act(x, kind), 1e-5)
        dg = torch.randn_like(x)
        db = torch.ones(x.numel())
        da = ops.act_bwd(dg[None], x[None], kind, dbias=db)
        da_r, db_r = R.act_bwd(dg[None], x[None], kind)
        close64(da, da_r, 1e-5)
        close64(db, db_r + 1, 1e-5)
    # largest finite bf16: tanh saturates in float64, the derivative is exactly 1 / 0
    big = torch.tensor([3.3895e38, -3.3895e38])
    assert R.act_grad(big, "gelu_tanh").tolist() == [1.0, 0.0]
    assert R.act(big, "gelu_tanh")[0] == big[0].double()


@pytest.mark.parametrize("T,Fd", [(1, 8), (130, 136)])
def test_swiglu_ref(T, Fd):
    torch.manual_seed(0)
    gu = torch.randn(T, 2 * Fd) * 3
    gu[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    dy = torch.randn(T, Fd)
    gl = gu.double().requires_grad_()
    y = F.silu(gl[:, :Fd]) * gl[:, Fd:]
    (y * dy.double()).sum().backward()
    close64(R.swiglu_fwd(gu), y.detach(), 1e-14, 1e-14)
    close64(R.swiglu_bwd(gu, dy), gl.grad, 1e-13, 1e-13)
    close64(ops.swiglu_fwd(gu), R.swiglu_fwd(gu), 1e-5)
    close64(ops.swiglu_bwd(gu, dy), R.swiglu_bwd(gu, dy), 1e-4)
    assert torch.isfinite(R.swiglu_bwd(gu, dy)).all()


@pytest.mark.parametrize("Dh", [8, 64])
@pytest.mark.parametrize("T,S,pos", [(130, 65, 0), (3, 1, 17), (8, 4, 60)])
def test_rope_ref(Dh, T, S, pos):
    torch.manual_seed(0)
    H, Hkv = 4, 2
    qkv = torch.randn(T, (H + 2 * Hkv) * Dh)
    cs, sn = ops.rope_tables(min(T, S) + pos, Dh, 10000.0, "cpu")
    r = R.rope(qkv, cs, sn, S, H, Hkv, Dh, pos)
    # complex-number form: (a + i b) * exp(i theta) per (a, b) = (x[j], x[j + Dh/2])
    x = qkv.double().reshape(T, H + 2 * Hkv, Dh)
    p = torch.arange(T) % S + pos
    rot = torch.polar(torch.ones(T, Dh // 2, dtype=torch.float64), torch.atan2(sn.double(), cs.double())[p])
    z = torch.complex(x[..., : Dh // 2], x[..., Dh // 2:]) * rot[:, None, :]
    want = torch.cat([z.real, z.imag], -1)
    got = r.reshape(T, H + 2 * Hkv, Dh)
    close64(got[:, : H + Hkv], want[:, : H + Hkv], 1e-6)
    assert torch.equal(got[:, H + Hkv:], x[:, H + Hkv:])
    close64(R.rope(r, cs, sn, S, H, Hkv, Dh, pos, inverse=True), qkv, 1e-6)
    close64(ops.rope_(qkv.clone(), cs, sn, S, H, Hkv, Dh, pos_offset=pos), r, 1e-5)


@pytest.mark.parametrize("n,n_decay", [(1, 1), (3, 2), (10007, 5003)])
@pytest.mark.parametrize("max_norm,grad_scale", [(0.0, 1.0), (0.5, 0.125), (1e6, 1.0)])
def test_adamw_ref(n, n_decay, max_norm, grad_scale):
    """The project's AdamW formula (ops.adamw_, CPU branch, f32) agrees with torch.optim.AdamW
    in float64 (two groups, clip_grad_norm_ on grad * grad_scale) over three steps."""
    torch.manual_seed(0)
    hp = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)
    p = torch.randn(n)
    ref = R.AdamW(p, n_decay, **hp)
    p32, m, v = p.clone(), torch.zeros(n), torch.zeros(n)
    for step in (1, 2, 3):
        g = torch.randn(n)
        g[n // 2: n // 2 + n // 8] *= 1e-8
        g[n // 4: n // 4 + n // 8] = 0
        ss = torch.zeros(1)
        ops.sumsq(g, ss)
        assert abs(ss.item() - R.sumsq(g)) <= 1e-5 * R.sumsq(g)
        ref.step(g, max_norm, grad_scale)
        gg = g.clone()
        ops.adamw_(p32, gg, m, v, None, n_decay, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step,
                   sumsq_buf=ss, max_norm=max_norm, grad_scale=grad_scale)
        assert torch.count_nonzero(gg) == 0
        close64(p32, ref.p, 3e-6)
        close64(m, ref.m, 1e-6)
        close64(v, ref.v, 1e-6)


def test_adamw_ref_resume():
    """first_step / m0 / v0: one step number 1000 from given moments."""
    torch.manual_seed(0)
    n = 64
    p, g, m0, v0 = torch.randn(n), torch.randn(n), torch.randn(n) * 0.1, torch.rand(n) * 0.1
    ref = R.AdamW(p, 13, 1e-3, 0.9, 0.95, 1e-8, 0.1, first_step=1000, m0=m0, v0=v0)
    ref.step(g)
    p32, m, v = p.clone(), m0.clone(), v0.clone()
    ops.adamw_(p32, g.clone(), m, v, None, 13, 1e-3, 0.9, 0.95, 1e-8, 0.1, 1000)
    close64(p32, ref.p, 1e-6)
    close64(m, ref.m, 1e-6)
    close64(v, ref.v, 1e-6)
