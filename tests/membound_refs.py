"""float64 references of the memory-bound, loss and optimizer kernels.

Plain functions: no ``ops`` import, each takes the tensors the kernel sees (bf16 or f32, any
device) and computes on the CPU in float64.  They are validated against
``torch.nn.functional`` and the CPU branch of the ``ops`` wrappers in
test_membound_refs_cpu.py and used as the oracle in test_membound_edges_gpu.py."""
import torch

K0, K1 = 0.7978845608028654, 0.044715


def f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def round_to(t64, dtype):
    """float64 -> storage dtype -> float64: what a kernel that stores ``dtype`` keeps."""
    return t64.to(dtype).double()


# ------------------------------------------------------------------ cross-entropy
def xent(logits, target, vocab, grad_scale, ignore_index=-100):
    """(loss [T], grad [T, Vp]) of the fused cross-entropy: loss = lse - x[target] over the
    first ``vocab`` columns, grad = (softmax - onehot) * grad_scale there and 0 in the padding
    columns; rows whose target is ``ignore_index`` give zero loss and a zero gradient row."""
    Vp = logits.shape[-1]
    lg = f64(logits).reshape(-1, Vp)[:, :vocab]
    T = lg.shape[0]
    tg = target.detach().cpu().reshape(T)
    valid = tg != ignore_index
    ts = torch.where(valid, tg, torch.zeros_like(tg))
    lse = torch.logsumexp(lg, -1)
    loss = torch.where(valid, lse - lg.gather(1, ts[:, None])[:, 0], torch.zeros_like(lse))
    p = torch.exp(lg - lse[:, None])
    p[torch.arange(T), ts] -= 1.0
    p *= grad_scale * valid[:, None].double()
    grad = torch.zeros(T, Vp, dtype=torch.float64)
    grad[:, :vocab] = p
    return loss, grad


# ------------------------------------------------------------------ LayerNorm / RMSNorm
def norm_fwd(x, w, bias=None, branch=None, kind="layernorm", eps=1e-5):
    """Returns (y, mean, rstd, s): s = round_T(x + branch) is the stored residual (None
    without a branch: the input itself is normalised), mean is None for RMSNorm."""
    D = x.shape[-1]
    xs = f64(x).reshape(-1, D)
    s = None
    if branch is not None:
        s = round_to(xs + f64(branch).reshape(-1, D), x.dtype)
        xs = s
    rms = kind == "rmsnorm"
    mean = torch.zeros(xs.shape[0], dtype=torch.float64) if rms else xs.mean(-1)
    var = (xs - mean[:, None]).pow(2).mean(-1)
    rstd = (var + eps).pow(-0.5)
    y = (xs - mean[:, None]) * rstd[:, None] * f64(w)
    if bias is not None:
        y = y + f64(bias)
    return y, (None if rms else mean), rstd, s


def norm_bwd(dy, s, w, mean, rstd, kind="layernorm", dres=None):
    """Backward from the saved (s, mean, rstd) the kernel reads.  Returns (ds, dw, dbias,
    colsum_dres, colsum_ds); colsum_ds sums ds as stored (rounded to dy's dtype), colsum_dres
    is None without dres."""
    D = dy.shape[-1]
    d = f64(dy).reshape(-1, D)
    x = f64(s).reshape(-1, D)
    rms = kind == "rmsnorm"
    mu = torch.zeros(d.shape[0], dtype=torch.float64) if rms else f64(mean)
    r = f64(rstd)[:, None]
    xh = (x - mu[:, None]) * r
    g = d * f64(w)
    s1 = torch.zeros(d.shape[0], 1, dtype=torch.float64) if rms else g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    ds = r * (g - s1 - xh * s2)
    cs_res = None
    if dres is not None:
        dr = f64(dres).reshape(-1, D)
        ds = ds + dr
        cs_res = dr.sum(0)
    return ds, (d * xh).sum(0), d.sum(0), cs_res, round_to(ds, dy.dtype).sum(0)


# ------------------------------------------------------------------ embedding
def positions(T, S, pos_offset=0):
    return torch.arange(T) % S + pos_offset


def embed_fwd(idx, wte, wpe, S, pos_offset=0):
    i = idx.detach().cpu().reshape(-1)
    e = f64(wte)[i]
    if wpe is not None:
        e = e + f64(wpe)[positions(i.numel(), S, pos_offset)]
    return e


def embed_bwd(idx, dout, dwte0, dwpe0, S, pos_offset=0):
    """Scatter-add of dout onto the starting gradients; returns (dwte, dwpe)."""
    i = idx.detach().cpu().reshape(-1)
    d = f64(dout).reshape(i.numel(), -1)
    dwte = f64(dwte0).clone().index_add_(0, i, d)
    dwpe = None
    if dwpe0 is not None:
        dwpe = f64(dwpe0).clone().index_add_(0, positions(i.numel(), S, pos_offset), d)
    return dwte, dwpe


# ------------------------------------------------------------------ activations
def act(x, kind):
    x = f64(x)
    if kind in ("gelu", "gelu_tanh"):
        return 0.5 * x * (1.0 + torch.tanh(K0 * (x + K1 * x ** 3)))
    if kind == "relu":
        return torch.clamp_min(x, 0.0)
    raise ValueError(kind)


def act_grad(x, kind):
    x = f64(x)
    if kind in ("gelu", "gelu_tanh"):
        t = torch.tanh(K0 * (x + K1 * x ** 3))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * K0 * (1.0 + 3.0 * K1 * x * x)
    if kind == "relu":
        return (x > 0).double()
    raise ValueError(kind)


def act_bwd(dg, a, kind):
    """(da, dbias): da = dg * act'(a); dbias sums da as stored (rounded to dg's dtype)."""
    da = f64(dg) * act_grad(a, kind)
    return da, round_to(da, dg.dtype).reshape(-1, da.shape[-1]).sum(0)


def colsum(x):
    return f64(x).reshape(-1, x.shape[-1]).sum(0)


def swiglu_fwd(gu):
    F = gu.shape[-1] // 2
    g, u = f64(gu)[:, :F], f64(gu)[:, F:]
    return g * torch.sigmoid(g) * u


def swiglu_bwd(gu, dy):
    """[T, 2F]: d gate | d up."""
    F = gu.shape[-1] // 2
    g, u, d = f64(gu)[:, :F], f64(gu)[:, F:], f64(dy)
    sg = torch.sigmoid(g)
    return torch.cat([d * u * sg * (1.0 + g * (1.0 - sg)), d * g * sg], -1)


# ------------------------------------------------------------------ RoPE
def rope(qkv, cos, sin, S, H, Hkv, Dh, pos_offset=0, inverse=False):
    """Rotate-half RoPE of the q and k heads of a packed [T, (H + 2 Hkv) Dh] buffer; v heads
    pass through."""
    T = qkv.shape[0]
    x = f64(qkv).reshape(T, H + 2 * Hkv, Dh).clone()
    pos = positions(T, S, pos_offset)
    c, s = f64(cos)[pos][:, None, :], f64(sin)[pos][:, None, :]
    if inverse:
        s = -s
    half = Dh // 2
    a, b = x[:, : H + Hkv, :half].clone(), x[:, : H + Hkv, half:].clone()
    x[:, : H + Hkv, :half] = a * c - b * s
    x[:, : H + Hkv, half:] = b * c + a * s
    return x.reshape(T, -1)


# ------------------------------------------------------------------ optimizer
class AdamW:
    """``torch.optim.AdamW`` in float64 over two parameter groups: elements [0, n_decay) with
    weight decay, the rest without.  ``step(g, max_norm, grad_scale)`` clips with
    ``torch.nn.utils.clip_grad_norm_`` on g * grad_scale.  ``first_step`` > 1 with (m0, v0)
    resumes a run: the next step is number ``first_step``."""

    def __init__(self, p, n_decay, lr, b1, b2, eps, wd, first_step=1, m0=None, v0=None):
        p = f64(p)
        self.nd = int(n_decay)
        self.params = [torch.nn.Parameter(p[: self.nd].clone()), torch.nn.Parameter(p[self.nd:].clone())]
        self.opt = torch.optim.AdamW([{"params": [self.params[0]], "weight_decay": wd},
                                      {"params": [self.params[1]], "weight_decay": 0.0}],
                                     lr=lr, betas=(b1, b2), eps=eps, foreach=False)
        m0 = torch.zeros_like(p) if m0 is None else f64(m0)
        v0 = torch.zeros_like(p) if v0 is None else f64(v0)
        for q, sl in zip(self.params, (slice(0, self.nd), slice(self.nd, None))):
            self.opt.state[q] = {"step": torch.tensor(float(first_step - 1)), "exp_avg": m0[sl].clone(),
                                 "exp_avg_sq": v0[sl].clone()}

    def step(self, g, max_norm=0.0, grad_scale=1.0):
        g = f64(g) * grad_scale
        self.params[0].grad = g[: self.nd].clone()
        self.params[1].grad = g[self.nd:].clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.params, max_norm)
        self.opt.step()

    def _cat(self, key):
        return torch.cat([self.opt.state[q][key] for q in self.params]).detach()

    @property
    def p(self):
        return torch.cat([q.detach() for q in self.params])

    @property
    def m(self):
        return self._cat("exp_avg")

    @property
    def v(self):
        return self._cat("exp_avg_sq")


def sumsq(g):
    return float((f64(g) ** 2).sum())


def bf16_bits(t):
    """bf16 tensor -> int16 bit patterns (for bit-exact comparisons that must tell -0 from 0
    and compare NaNs)."""
    return t.detach().cpu().contiguous().view(torch.int16)


def f32_bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)

