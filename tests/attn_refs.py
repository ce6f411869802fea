"""float64 reference of the training attention kernels (attention.hip, attention_f32.hip),
the componentwise error scales of its outputs, the check the GPU edge tests run, and the
inputs they use.

Plain functions: no ``ops`` import.  The references take the tensors the kernel sees (token-major
row views ``[B*S, >= heads*D]``, head ``h`` at columns ``h*D``; bf16 or f32, any device) and
compute on the CPU in float64.  They are validated against
``torch.nn.functional.scaled_dot_product_attention`` and the CPU branch of the ``ops``
wrappers in test_attn_refs_cpu.py, which also shows that the check fails on eight subtly
wrong kernels, and are the oracle of test_attn_edges_gpu.py.

Conventions (the kernels' own): causal means key j is visible to query i iff
j <= i + Sk - Sq; the KV head of query head h is h // (H // Hkv); the LSE is kept in log2
units; a query row that sees no key has O = 0, LSE = +inf and contributes nothing to any
gradient.

Error metric.  A bf16 output element is a sum of products of rounded factors, rounded once
more when stored, so its error is measured against what was summed for it:

    err = max |got - ref| / (2^-8 (|ref| + A))

with A the same sum over absolute values (``A_O = (P o keep) |V|`` and so on below).  A small
element next to large terms is not forgiven more than those terms explain.  One absolute term
joins A: f32 arithmetic cannot hold a probability (or a dS) below its smallest normal number,
2^-126, so every summand may be off by 2^-126 times its other factor.  In the metric's
relative unit that is FLUSH = 2^-126 / 2^-8 added to P (and to |dS|) inside the A sums.  It
matters only for keys whose weight underflows (scores 87 below the row maximum).  f32 outputs
and reductions use the project's f32 metric, max |got - ref| / (|ref| + min(1, max |ref|)).
"""
import math
import re
from types import SimpleNamespace as NS

import torch

LOG2E = 1.4426950408889634
EPS_BF16 = 2.0 ** -8
FLUSH = 2.0 ** -126 / EPS_BF16

# bound = 2 x the largest error measured on an MI355X over two runs of test_attn_edges_gpu.py
# (the measured value in the comment).  Only dbias ends in f32 atomics and varies from run to run.
BOUND = {
    "attn.bf16.o": 1.74,        # 0.8691 (d_h 200, forward v1 DP 256)
    "attn.bf16.dq": 1.66,       # 0.8255 (causal 200 x 65, d_h 128)
    "attn.bf16.dk": 2.02,       # 1.005 (q x 6, d_h 64, dK dV v3)
    "attn.bf16.dv": 2.0,        # 0.9972 (q x 6, d_h 64, dK dV v3)
    "attn.bf16.lse": 7.1e-7,    # 3.533e-07
    "attn.bf16.lse_v2": 3.0e-3,  # 1.491e-03: forward v2 sums the bf16-rounded P (see check_outputs)
    "attn.bf16.delta": 3.2e-6,  # 1.558e-06
    "attn.bf16.dbias": 0.48,    # 0.2368 (q x 6, d_h 128: the kernels sum the gradients before rounding them)
    "attn.f32.o": 9.8e-7,       # 4.899e-07
    "attn.f32.lse": 4.9e-7,     # 2.419e-07
    "attn.f32.delta": 1.0e-6,   # 4.990e-07
    "attn.f32.dq": 1.6e-6,      # 7.869e-07
    "attn.f32.dk": 1.6e-6,      # 7.928e-07
    "attn.f32.dv": 1.5e-6,      # 7.067e-07
}

# what the older tests of the same kernels allow (atol, rtol): asserted alongside, so the
# new check is never looser (test_kernels_gpu.py::test_attention_fwd_bwd,
# test_f32_gpu.py::test_attention_f32_fwd_bwd)
OLD_TOL = {
    "attn.bf16.o": (2e-2, 2e-2), "attn.bf16.lse": (2e-2, 1e-3), "attn.bf16.lse_v2": (2e-2, 1e-3),
    "attn.bf16.dq": (5e-2, 5e-2), "attn.bf16.dk": (5e-2, 5e-2), "attn.bf16.dv": (5e-2, 5e-2),
    "attn.f32.o": (1e-5, 1e-4), "attn.f32.lse": (1e-5, 1e-5),
    "attn.f32.dq": (2e-5, 1e-4), "attn.f32.dk": (2e-5, 1e-4), "attn.f32.dv": (2e-5, 1e-4),
}


def f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def round_to(t64, dtype):
    return t64.to(dtype).double()


def heads(t, B, S, nh, D):
    """token-major view (first B*S rows, first nh*D columns) -> float64 [B, nh, S, D]"""
    return f64(t[: B * S, : nh * D]).reshape(B, S, nh, D).permute(0, 2, 1, 3)


def rows(x):
    """[B, nh, S, D] -> token-major [B*S, nh*D]"""
    B, nh, S, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, nh * D)


def visible(Sq, Sk, causal):
    """bool [Sq, Sk]: key j is visible to query i"""
    if not causal:
        return torch.ones(Sq, Sk, dtype=torch.bool)
    return torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None] + (Sk - Sq)


def attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, causal, scale, keep=None):
    """O [B*Sq, H*D], lse [B*H*Sq] (log2 units, +inf on rows that see no key), P [B, H, Sq, Sk]
    (the softmax before dropout), A_O = (P o keep) |V| shaped like O, and S, the scaled scores
    with -inf on masked keys.  ``keep``: [B, H, Sq, Sk] of 0 or 1 / (1 - p)."""
    rep = H // Hkv
    Q = heads(q, B, Sq, H, D)
    K = heads(k, B, Sk, Hkv, D).repeat_interleave(rep, 1)
    V = heads(v, B, Sk, Hkv, D).repeat_interleave(rep, 1)
    s = (Q @ K.transpose(-1, -2)) * scale
    vis = visible(Sq, Sk, causal)
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m) & (m < 0)
    e = torch.exp(s - torch.where(empty, torch.zeros_like(m), m))
    l = e.sum(-1, keepdim=True)
    P = e / torch.where(empty, torch.ones_like(l), l)
    lse = torch.where(empty, torch.full_like(m, float("inf")), (m + torch.log(l)) * LOG2E)
    kp = torch.ones_like(P) if keep is None else f64(keep)
    Pa = (P + FLUSH * vis) * kp
    return NS(O=rows((P * kp) @ V), lse=lse.reshape(-1), P=P, A_O=rows(Pa @ V.abs()), S=s, Pa=Pa, vis=vis)


def attn_bwd_ref(q, k, v, o, do, B, Sq, Sk, H, Hkv, D, causal, scale, keep=None):
    """Backward from the STORED ``o`` (as the kernels' delta = rowsum(dO o O) is).  Returns
    dQ / dK / dV (token-major, unrounded float64), delta [B*H*Sq], the error scales
    A_dV = (P o keep)^T |dO|, A_dQ = scale |dS| |K|, A_dK = scale |dS|^T |Q| with
    |dS| = P o (|dP| + |delta|) (summed over the query heads of a KV head), and
    ``colsum``: the float64 column sums of the gradients rounded to the storage dtype, q | k | v,
    which is what ``dbias`` accumulates."""
    rep = H // Hkv
    f = attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, causal, scale, keep)
    Q = heads(q, B, Sq, H, D)
    K = heads(k, B, Sk, Hkv, D).repeat_interleave(rep, 1)
    V = heads(v, B, Sk, Hkv, D).repeat_interleave(rep, 1)
    dO, O = heads(do, B, Sq, H, D), heads(o, B, Sq, H, D)
    kp = torch.ones_like(f.P) if keep is None else f64(keep)
    Pk = f.P * kp
    delta = (dO * O).sum(-1, keepdim=True)
    dP = (dO @ V.transpose(-1, -2)) * kp
    dS = f.P * (dP - delta)
    adS = f.P * (dP.abs() + delta.abs()) + FLUSH * f.vis * (dP.abs() + delta.abs()).clamp_min(1.0)

    def group(x):   # sum over the query heads of each KV head
        return x.reshape(B, Hkv, rep, Sk, D).sum(2)

    dQ, dK, dV = rows(dS @ K * scale), rows(group(dS.transpose(-1, -2) @ Q * scale)), rows(group(Pk.transpose(-1, -2) @ dO))
    dt = q.dtype
    return NS(dQ=dQ, dK=dK, dV=dV, delta=delta.reshape(-1),
              A_dQ=rows(adS @ K.abs() * scale), A_dK=rows(group(adS.transpose(-1, -2) @ Q.abs() * scale)),
              A_dV=rows(group(f.Pa.transpose(-1, -2) @ dO.abs())),
              colsum=torch.cat([round_to(g, dt).sum(0) for g in (dQ, dK, dV)]), fwd=f)


# ------------------------------------------------------------------ the check
class Report:
    """Collects the figures of one case: every check prints its MEASURE line and records a
    failure; ``finish`` raises once, after all figures are out."""

    def __init__(self, what, bound=None):
        self.what, self.fails, self.seen = what, [], {}
        self.bound = BOUND if bound is None else bound

    def fail(self, msg):
        self.fails.append(f"{self.what}: {msg}")

    def expect(self, cond, msg):
        if not cond:
            self.fail(msg)

    def _common(self, key, got, ref):
        got, ref = f64(got).reshape(-1), f64(ref).reshape(-1)
        if got.shape != ref.shape:
            self.fail(f"{key}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
            return None, None
        if not torch.isfinite(got).all():
            self.fail(f"{key}: non-finite output")
            return None, None
        if key in OLD_TOL and got.numel():
            atol, rtol = OLD_TOL[key]
            over = float(((got - ref).abs() - (atol + rtol * ref.abs())).max())
            self.expect(over <= 0, f"{key}: outside the older test's atol {atol} / rtol {rtol} by {over:.3e}")
        return got, ref

    def _record(self, key, err, unit):
        self.seen[key] = max(self.seen.get(key, 0.0), err)
        print(f"MEASURE {key} {err:.4g} {unit} {self.what}")
        self.expect(err <= self.bound[key], f"{key}: error {err:.4g} > bound {self.bound[key]:.4g}")

    def bf16(self, key, got, ref, A):
        """err = max |got - ref| / (2^-8 (|ref| + A)); elements with nothing summed are exact."""
        got, ref = self._common(key, got, ref)
        if got is None or not got.numel():
            return
        den = EPS_BF16 * (ref.abs() + f64(A).reshape(-1))
        zero = den == 0
        self.expect(bool((got[zero] == 0).all()), f"{key}: non-zero where nothing is summed")
        err = float(((got - ref).abs()[~zero] / den[~zero]).max()) if (~zero).any() else 0.0
        self._record(key, err, "x 2^-8 (|ref| + A)")

    def f32(self, key, got, ref, A=None):
        """max |got - ref| / (|ref| + min(1, max |ref|)).  With ``A`` (the sums of absolute terms
        behind ``ref``) the floor is min(1, max(max |ref|, max A)): a gradient that cancels to
        zero everywhere (one key: dS = 0) is not the size of what was computed for it."""
        got, ref = self._common(key, got, ref)
        if got is None or not got.numel():
            return
        mag = float(ref.abs().max()) if A is None else max(float(ref.abs().max()), float(f64(A).abs().max()))
        floor = max(min(1.0, mag), 1e-30)
        self._record(key, float(((got - ref).abs() / (ref.abs() + floor)).max()), "rel")

    def finish(self):
        assert not self.fails, "\n".join(self.fails)


def check_outputs(rep, prec, fwd, bwd, got, B, Sq, H, Hkv, D, lse_key="lse"):
    """``got``: dict of the kernel's outputs as CPU tensors: token-major o / dq / dk / dv cut
    to their [B*S, heads*D] region, flat lse / delta, and optionally dbias (with ``dbias0``,
    the value it started from).  ``prec``: 'bf16' or 'f32'.  Missing keys are not checked.
    ``lse_key``: 'lse_v2' for the forward v2 kernel without dropout, whose row sum is taken on
    the matrix cores over the bf16-rounded probabilities (a 2^-9 relative error per term in
    l, against 2^-24 of the f32 sums of every other kernel), so it has a bound of its own."""
    key = lambda n: f"attn.{prec}.{n}"   # noqa: E731
    val = rep.bf16 if prec == "bf16" else rep.f32
    if "o" in got:
        val(key("o"), got["o"], fwd.O, fwd.A_O)
    if "lse" in got:
        lse, inf = f64(got["lse"]), torch.isinf(fwd.lse)
        rep.expect(bool((lse[inf] == float("inf")).all()), "lse: not +inf on a row that sees no key")
        rep.f32(key(lse_key), lse[~inf], fwd.lse[~inf])
    if bwd is None:
        return
    for n, ref, A in (("dq", bwd.dQ, bwd.A_dQ), ("dk", bwd.dK, bwd.A_dK), ("dv", bwd.dV, bwd.A_dV)):
        if n in got:
            val(key(n), got[n], ref, A)
    if "dq" in got:
        dead = torch.isinf(fwd.lse).reshape(B, H, Sq).permute(0, 2, 1).reshape(B * Sq, H)
        dqh = f64(got["dq"]).reshape(B * Sq, H, D)
        rep.expect(bool((dqh[dead] == 0).all()), "dq: not exactly zero on a row that sees no key")
    if "delta" in got:
        rep.f32(key("delta"), got["delta"], bwd.delta)
    if "dbias" in got:
        rep.f32(key("dbias"), f64(got["dbias"]) - got["dbias0"], bwd.colsum)


# ------------------------------------------------------------------ cases and their inputs
class Case:
    """One attention problem of the GPU edge tests.  ``kind`` selects the inputs (make_inputs),
    ``layout`` how the runner places them in memory, ``branch`` names the launcher branches
    it reaches (it is part of the test id)."""

    def __init__(self, branch, B, Sq, Sk, H, Hkv, D, causal, scale=None, p=0.0, layout=None, kind="randn",
                 prec="bf16", seed=0):
        self.branch, self.B, self.Sq, self.Sk, self.H, self.Hkv, self.D = branch, B, Sq, Sk, H, Hkv, D
        self.causal, self.p, self.kind, self.prec, self.seed = causal, p, kind, prec, seed
        self.scale = 1.0 / math.sqrt(D) if scale is None else scale
        self.layout = layout or ("packed" if Sq == Sk else "q_kv")

    @property
    def dtype(self):
        return torch.bfloat16 if self.prec == "bf16" else torch.float32

    @property
    def id(self):
        s = f"{self.prec}-{'c' if self.causal else 'nc'}-B{self.B}-Sq{self.Sq}-Sk{self.Sk}-H{self.H}-Hkv{self.Hkv}-D{self.D}"
        if self.kind != "randn":
            s += f"-{self.kind}"
        if self.scale != 1.0 / math.sqrt(self.D):
            s += f"-scale{self.scale:g}"
        if self.p:
            s += f"-p{self.p:g}"
        return f"{s}-{self.layout}-{self.branch}"

    def shape(self):
        return self.B, self.Sq, self.Sk, self.H, self.Hkv, self.D

    def __repr__(self):
        return self.id


TILE = 64
RISE = 30.0      # step of the row maximum from one 64-key tile to the next ('rising' / 'falling')
COMMON = 60.0    # the score every key shares ('common')


def make_inputs(c):
    """(q, k, v, do) as CPU tensors of the case's dtype, [B*S, heads*D] contiguous.

    randn    N(0, 1) everywhere, as the older tests.
    q6       q x 6: scores ~ N(0, 36 D scale^2), the softmax is nearly one-hot.
    rising   column 0 of every head carries q = 32 and k = t * RISE / (32 scale) for the key's
             64-key tile t, so the row maximum rises by about RISE (> 20) at every tile: each
             tile rescales everything accumulated before it.  falling: the reverse order.
    common   column 0 carries q = 32 and k = COMMON / (32 scale): every score is near +60.
    In the last three dO is N(0, 1/16): dQ's column 0 is a sum of dS times the shared key
    component that cancels (rows of dS sum to zero), so the bf16 rounding of dS shows there in
    full; the metric accounts for that, the older test's absolute 0.05 would not at dO ~ 1."""
    B, Sq, Sk, H, Hkv, D = c.shape()
    g = torch.Generator().manual_seed(1000 + c.seed)
    q, do = torch.randn(B * Sq, H * D, generator=g), torch.randn(B * Sq, H * D, generator=g)
    k, v = torch.randn(B * Sk, Hkv * D, generator=g), torch.randn(B * Sk, Hkv * D, generator=g)
    if c.kind == "q6":
        q *= 6.0
    elif c.kind in ("rising", "falling", "common"):
        q[:, ::D] = 32.0
        do *= 0.25
        t = (torch.arange(B * Sk) % Sk) // TILE
        if c.kind == "falling":
            t = (Sk - 1) // TILE - t
        col = t.double() * RISE / (32.0 * c.scale) if c.kind != "common" else torch.full((B * Sk,), COMMON / (32.0 * c.scale))
        k[:, ::D] = col.float()[:, None]
    elif c.kind != "randn":
        raise ValueError(c.kind)
    return tuple(t.to(c.dtype) for t in (q, k, v, do))


def identity_window(S, D, w, nh, B, dtype):
    """[B*S, nh*D]: in every head, row j holds e_(j - w D) if w D <= j < (w + 1) D, else 0.
    With q = k = 0 (uniform P) and this as V, O's head columns are P o keep over keys
    w D .. (w + 1) D - 1: ceil(Sk / D) passes recover the kernel's dropout mask for any Sk."""
    x = torch.zeros(S, D)
    n = min(D, S - w * D)
    x[w * D: w * D + n, :n] = torch.eye(n)
    return x.repeat(B, nh).to(dtype)


# ------------------------------------------------------------------ which kernels a case reaches
F32_DIMS = (64, 96, 128, 192)
BIG_STRIDE = (1 << 22) + 8   # 'bigstride' layout: (S + 128) * stride * 2 >= 2^31 at S = 128

DEFAULT_ENV = {"FWD": "", "BWD_DQ": "", "BWD_DKDV": "", "KS2": "", "BWD_SHORT": ""}


def env_flags(environ):
    return {k: environ.get("MIPIPE_ATTN_" + k, "") for k in DEFAULT_ENV}


def path(c, env=DEFAULT_ENV):
    """(forward, backward) kernels the launch plan (csrc/include/mp_attn_plan.h) picks for this
    case, as text: the same conditions, re-stated by hand and independently of it
    (test_attn_plan_cpu.py holds the two against each other).  ``env``: the MIPIPE_ATTN_* switches."""
    B, Sq, Sk, H, Hkv, D = c.shape()
    if c.prec == "f32":
        return "f32", "f32"
    DP = 64 if D <= 64 else (128 if D <= 128 else 256)
    narrow = c.layout != "bigstride"          # 32-bit buffer offsets reach every row
    nqb, nkb = (Sq + 127) // 128, (Sk + 127) // 128
    pair = lambda n: f"x{(n + 1) // 2}pair{'odd' if n % 2 else 'even'}" if c.causal else f"x{n}"   # noqa: E731
    if not c.causal and DP <= 128 and env["KS2"] != "0" and nqb * B * H < 256:
        fwd = "ks2-" + ("1iter" if ((Sk + 63) // 64 + 1) // 2 == 1 else "loop")
    elif DP == 64 and env["FWD"] != "1" and narrow:
        fwd = "fwd2" + pair(nqb)
    else:
        fwd = f"fwd1dp{DP}"
    if not c.causal and DP <= 128 and env["BWD_SHORT"] != "0" and Sq <= 128 and Sk <= 128 and H == Hkv:
        return fwd, f"short{(Sq + 63) // 64}+{(Sk + 63) // 64}"
    if DP == 64 and env["BWD_DQ"] != "1" and narrow:
        dq = "dq2" if env["BWD_DQ"] == "2" else "dq3" + pair(nqb)
    else:
        dq = f"dq1dp{DP}"
    if DP == 64 and env["BWD_DKDV"] != "1" and narrow:
        dkdv = "dkdv2" if env["BWD_DKDV"] == "2" else "dkdv3" + pair(nkb)
    else:
        dkdv = f"dkdv1dp{DP}"
    return fwd, dq + "+" + dkdv


def path_kernels(p):
    """the kernel names (mp_attn_plan.h) in a path() answer, forward first"""
    labels = [p[0]] + (["short"] if p[1].startswith("short") else p[1].split("+"))
    return [re.match(r"ks2|fwd[12]|short|dq[123]|dkdv[123]", x).group(0) for x in labels]


def planned_kernels(plan):
    """the same list from an ``ops.attn_plan`` answer"""
    return [plan["fwd"]["kernel"]] + [l["kernel"] for l in plan["bwd"]]


def plan_env(flags):
    """env_flags form -> the ``env`` argument of ``ops.attn_plan``"""
    return {"MIPIPE_ATTN_" + k: v for k, v in flags.items()}


def case_strides(c):
    """(qs, ks, vs, os): row strides of q / k / v / o as the case's layout places them, without
    the GPU runner's few sentinel columns (the plan only asks whether (S + 128) * stride * 2
    reaches 2^31): 'packed' has q | k | v side by side in one row, 'q_kv' k | v."""
    wq, wk = c.H * c.D, c.Hkv * c.D
    if c.layout == "bigstride":
        return (BIG_STRIDE,) * 4
    if c.layout == "packed":
        return (wq + 2 * wk,) * 3 + (wq,)
    return (wq, 2 * wk, 2 * wk, wq) if c.layout == "q_kv" else (wq, wk, wk, wq)


def _cases():
    cs = []
    add = lambda *a, **k: cs.append(Case("", *a, **k))   # noqa: E731
    # self-attention, B*H = 6; d_h 64: forward v2 / dQ v3 / dK/dV v3 (causal, paired 128-row
    # blocks: 1, 2, 3 and 4 blocks), key-split forward + short or v3 backward (non-causal);
    # d_h 128: the v1 kernels
    for S in (1, 7, 63, 64, 65, 127, 128, 129, 191, 257, 385):
        for causal in (True, False):
            for D in (64, 128):
                add(2, S, S, 3, 3, D, causal, seed=S)
    add(2, 257, 257, 4, 4, 64, True, seed=1)          # B*H = 8: the XCD grouping of the paired kernels
    add(1, 385, 385, 8, 8, 64, True, seed=2)
    # head dims: padded to DP 64 / 128 / 256
    for D in (8, 40, 72, 96, 192, 200, 256):
        for S in (65, 129):
            for causal in (True, False):
                add(1, S, S, 2, 2, D, causal, seed=D + S)
    # GQA 4:1 and 8:1, MQA.  S 100 non-causal is short but must take the two-kernel backward.
    for H, Hkv in ((8, 2), (8, 1), (4, 1)):
        for D in (64, 128):
            add(1, 100, 100, H, Hkv, D, False, seed=H + Hkv)
            add(1, 257, 257, H, Hkv, D, True, seed=H + Hkv)
    # cross lengths, forward and backward
    for D in (64, 128):
        for Sq, Sk in ((1, 129), (129, 1), (65, 128), (128, 65), (100, 300), (300, 100)):
            add(2, Sq, Sk, 3, 3, D, False, seed=Sq)
        for Sq, Sk in ((64, 128), (100, 40)):      # the short backward with 1 + 2 and 2 + 1 role blocks
            add(2, Sq, Sk, 3, 3, D, False, seed=Sq)
        for Sq, Sk in ((65, 200), (200, 65), (257, 129), (129, 257)):
            add(2, Sq, Sk, 3, 3, D, True, seed=Sq)
    # layouts (packed is the default of every self-attention case above, q_kv of every cross one)
    for layout in ("q_kv", "sep", "gradstride"):
        add(2, 129, 129, 4, 2, 64, True, layout=layout, seed=3)
        add(1, 100, 100, 2, 2, 128, False, layout=layout, seed=4)
    add(1, 129, 129, 4, 2, 64, True, layout="packed", seed=3)
    # 64-bit offsets: the v1 kernels at d_h 64
    add(1, 128, 128, 2, 2, 64, True, layout="bigstride", seed=5)
    # score ranges
    for D in (64, 128):
        for causal in (True, False):
            add(1, 257, 257, 2, 2, D, causal, scale=0.3, seed=6)
            for kind in ("q6", "rising", "falling", "common"):
                add(1, 257, 257, 2, 2, D, causal, kind=kind, seed=7)
    # dropout against the reference with the kernel's own mask
    for p in (0.1, 0.3):
        add(1, 200, 200, 2, 2, 64, True, p=p, seed=8)
        add(1, 385, 385, 2, 2, 64, True, p=p, seed=8)
        add(1, 257, 257, 2, 2, 128, True, p=p, seed=8)
        add(1, 200, 200, 4, 1, 64, True, p=p, seed=8)
        add(1, 100, 300, 2, 2, 64, False, p=p, seed=8)
        add(1, 100, 100, 2, 2, 64, False, p=p, seed=8)
    # f32 kernels: non-causal, H == Hkv
    for D in F32_DIMS:
        for Sq, Sk in ((1, 1), (65, 65), (257, 257), (100, 300), (300, 100)):
            for layout in ("packed" if Sq == Sk else "q_kv", "sep"):
                add(2, Sq, Sk, 3, 3, D, False, prec="f32", layout=layout, seed=D)
    add(1, 100, 300, 2, 2, 64, False, prec="f32", p=0.1, layout="gradstride", seed=9)
    for c in cs:
        c.branch = "+".join(path(c))
    return cs


CASES = _cases()


def _child_cases():
    """The reduced list the non-default kernels run (MIPIPE_ATTN_*): one case per group above
    at d_h 64, plus the short GQA case at d_h 128."""
    want = [(2, 257, 257, 3, 3, 64, True, "randn", 0.0), (2, 129, 129, 3, 3, 64, False, "randn", 0.0),
            (2, 64, 64, 3, 3, 64, False, "randn", 0.0), (2, 257, 257, 4, 4, 64, True, "randn", 0.0),
            (1, 129, 129, 2, 2, 40, True, "randn", 0.0), (1, 100, 100, 8, 2, 64, False, "randn", 0.0),
            (1, 257, 257, 8, 1, 64, True, "randn", 0.0), (2, 100, 300, 3, 3, 64, False, "randn", 0.0),
            (2, 300, 100, 3, 3, 64, False, "randn", 0.0), (2, 200, 65, 3, 3, 64, True, "randn", 0.0),
            (2, 129, 257, 3, 3, 64, True, "randn", 0.0), (1, 257, 257, 2, 2, 64, True, "rising", 0.0),
            (1, 257, 257, 2, 2, 64, False, "common", 0.0), (1, 385, 385, 2, 2, 64, True, "randn", 0.1),
            (1, 100, 100, 2, 2, 64, False, "randn", 0.3), (1, 100, 100, 8, 2, 128, False, "randn", 0.0)]
    out = []
    for w in want:
        hit = [c for c in CASES if c.prec == "bf16" and (*c.shape()[:1], c.Sq, c.Sk, c.H, c.Hkv, c.D, c.causal, c.kind, c.p) == w
               and c.scale == 1.0 / math.sqrt(c.D)]
        assert hit, w
        out.append(hit[0])
    out += [c for c in CASES if c.prec == "bf16" and c.layout in ("sep", "gradstride") and c.D == 64]
    return out


CHILD_CASES = _child_cases()
CHILD_ENVS = {
    "v1": {"MIPIPE_ATTN_FWD": "1", "MIPIPE_ATTN_BWD_DQ": "1", "MIPIPE_ATTN_BWD_DKDV": "1", "MIPIPE_ATTN_KS2": "0",
           "MIPIPE_ATTN_BWD_SHORT": "0"},
    "v2": {"MIPIPE_ATTN_BWD_DQ": "2", "MIPIPE_ATTN_BWD_DKDV": "2"},
}
