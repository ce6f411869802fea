"""float64 reference of the GEMM engines (gemm.hip, gemm2.hip + mp_gemm_*.h, gemm_f32.hip), the componentwise
error scale of every output, the check the GPU edge tests run, and the cases they use.

Plain functions: no ``ops`` import.  ``gemm_ref`` takes the tensors the kernel sees (views with
any row stride, bf16 or f32, any device; ``transA`` / ``transB`` as the bindings define them:
A is [M, K], or [K, M] with transA; B is [N, K], or [K, N] with transB) and computes on the CPU
in float64.  It is validated against ``torch.matmul`` / ``torch.nn.functional.gelu`` and the
CPU branches of the ``ops`` wrappers in test_gemm_refs_cpu.py, which also shows that the check
fails on twelve subtly wrong results, and is the oracle of test_gemm_edges_gpu.py.

Error metric.  An output element is a sum of products (plus bias, residual, incoming C),
rounded once when stored, so its error is measured against what was summed for it:

    bf16 outputs:                             err = max |got - ref| / (2^-8  (|ref| + A))
    f32 outputs, accumulators, column sums:   err = max |got - ref| / (2^-23 (|ref| + A))

with A the same expression over absolute values, |alpha| |A| |B| + |bias| + |R| + |C0|, carried
through an activation with the magnitude of its derivative.  A small element next to large
products is forgiven only as much as those products explain; where nothing at all is summed
(A = 0 and ref = 0) the output must be exactly 0.

The bf16 kernels round the pre-activation to bf16 before GELU / ReLU.  The reference never
picks one rounding of it: it returns the unrounded pre-activation, and the derivative that
scales A is the largest over the half-ulp interval [pre - h, pre + h], h = 2^-8 |pre| + the
f32 summation allowance 2^-18 A_pre, so a half-ulp step of the pre-activation, propagated through
the activation, costs at most 1.0 in the metric.  ReLU's output and saved pre-activation are
continuous in the pre-activation, so only the choice "derivative 0 or 1" depends on its sign:
elements with |pre| <= h are ``unsure`` (derivative 1, either branch passes), they are counted,
and a case may hold at most UNSURE_CAP of them.  dGELU / dReLU read a saved bf16 tensor that is
an input here, so ``aux > 0`` is exact and nothing is excluded.

Column sums.  The fused epilogue sums the f32 values before they are rounded, so '.colsum' is
compared with colsum0 + the sums of the unrounded reference (A: the sums of A_out): a few f32
units.  Behind GELU / ReLU the summed values come from the bf16-rounded pre-activation, a
half-ulp step per element that no sum can tell from a wrong one: those are '.colsum_act',
compared with the sums of the STORED output (``stored``), about 2^14 / sqrt(M) units.  A
separate column-sum pass over C ('.colsum_sep': split-K, accumulate, v1) is compared with the
stored sums and is exact to f32 summation.

One mutation of the issue's list cannot be seen by construction: "pre-activation rounded after
instead of before the activation, in aux only".  For GELU it moves the saved derivative by at
most |gelu''| times the half-ulp step of the pre-activation, which the check must allow.  The
CPU test therefore uses its ReLU form (aux = relu(pre), which loses every negative value)."""
import math
from types import SimpleNamespace as NS

import torch

EPS_BF16 = 2.0 ** -8
EPS_F32 = 2.0 ** -23
SUM_SLACK = 2.0 ** -18          # f32 summation error allowed inside h, relative to A_pre
UNSURE_CAP = 1e-3
BK = 64                         # K-tile of the bf16 engines
BK_F32 = 32                     # K-tile of the f32 engines (a pair is 64)
BF16, F32 = torch.bfloat16, torch.float32

EPI = dict(none=0, bias=1, bias_gelu=2, bias_relu=3, bias_res=4, res=5, dgelu=6, drelu=7)
F32_EPI = dict(none=0, bias=1, bias_relu=2, res=3, bias_res=4, drelu=5)
DROP_EPIS = ("bias_gelu", "bias_relu", "dgelu", "drelu")
ONE_ROUNDING = ("none", "bias", "res", "bias_res")   # one f32 sum rounded once

# bound = 2 x the largest error measured on an MI355X over two runs of test_gemm_edges_gpu.py
# (the measured value in the comment).  '<class>.out' is the bf16 output of the one-rounding
# epilogues and may never exceed 1.0; '.act' the output behind GELU / ReLU / dGELU / dReLU,
# '.aux' what the forward saves, '.acc' an f32 accumulator, '.colsum' the fused column sums.
BOUND = {
    "g2.acc": 1.27,                    # 0.6352 (shape tn 264 x 264 x 320 none-acc-a-2-force2-cfg2.s1)
    "g2.act": 0.988,                   # 0.4942 (range nt 264 x 136 x 192 bias_gelu-gelumax-force2-cfg2.s1)
    "g2.aux": 1.81,                    # 0.9061 (epi nt 256 x 256 x 192 bias_gelu-force0-cfg0.s1)
    "g2.colsum": 1.12,                 # 0.5623 (epi nt 264 x 200 x 320 bias_res-cs-force1-cfg1.s1)
    "g2.colsum_act": 8010,             # 4006 (epi nt 136 x 136 x 320 bias_gelu-cs-force3-cfg3.s1)
    "g2.colsum_sep": 0.291,            # 0.1455 (epi nt 264 x 136 x 320 none-acc-a0.5-cs-force2-cfg2.s1)
    "g2.out": 0.818,                   # 0.409 (shape nt 128 x 264 x 64 none-force3-cfg3.s1)
    "g3nt.act": 0.988,                 # 0.4942 (range nt 264 x 264 x 192 bias_gelu-gelumax-force5-cfg5.s1)
    "g3nt.aux": 1.81,                  # 0.9071 (epi nt 256 x 256 x 192 bias_gelu-force4-cfg4.s1)
    "g3nt.colsum": 1.46,               # 0.7277 (epi nt 264 x 264 x 320 bias-cs-force5-cfg5.s1)
    "g3nt.colsum_act": 5060,           # 2532 (epi nt 264 x 264 x 320 bias_gelu-cs-force5-cfg5.s1)
    "g3nt.out": 0.766,                 # 0.383 (shape nt 256 x 264 x 64 none-force4-cfg4.s1)
    "g3tt.acc": 1.37,                  # 0.6855 (range tn 264 x 264 x 192 none-acc-big-force6-cfg6.s1)
    "g6.act": 0.988,                   # 0.4942 (range nt 264 x 200 x 192 bias_gelu-gelumax-force9-cfg9.s1)
    "g6.aux": 1.78,                    # 0.8883 (stride nt 264 x 264 x 192 bias_gelu-bigldx-force9-cfg9.s1)
    "g6.colsum": 1.05,                 # 0.5273 (epi nt 264 x 200 x 320 bias-cs-force9-cfg9.s1)
    "g6.colsum_act": 5200,             # 2598 (epi nt 264 x 200 x 320 bias_gelu-cs-force9-cfg9.s1)
    "g6.out": 0.666,                   # 0.3332 (shape nt 264 x 392 x 64 none-force9-cfg9.s1)
    "g8.act": 0.988,                   # 0.4942 (range nt 264 x 200 x 192 bias_gelu-gelumax-force15-cfg15.s1)
    "g8.aux": 1.81,                    # 0.9046 (drop nt 264 x 200 x 192 bias_gelu-p0.25-force15-cfg15.s1)
    "g8.colsum": 0.77,                 # 0.385 (epi nt 264 x 200 x 320 bias-cs-force15-cfg15.s1)
    "g8.colsum_act": 5690,             # 2844 (epi nt 264 x 200 x 320 bias_gelu-cs-force16-cfg16.s1)
    "g8.out": 0.736,                   # 0.3682 (shape nt 520 x 392 x 64 none-force15-cfg15.s1)
    "snt.act": 0.917,                  # 0.4583 (wrappers)
    "snt.aux": 1.85,                   # 0.9246 (stride nt 264 x 264 x 192 bias_gelu-bigldx-force12-cfg12.s1)
    "snt.colsum": 1.26,                # 0.6302 (epi nt 72 x 72 x 320 drelu-cs-force10-cfg10.s1)
    "snt.colsum_act": 9390,            # 4695 (epi nt 72 x 72 x 320 bias_gelu-cs-force10-cfg10.s1)
    "snt.out": 0.653,                  # 0.3263 (shape nt 72 x 72 x 64 none-force10-cfg10.s1)
    "stt.acc": 1.33,                   # 0.6665 (stride tn 264 x 264 x 320 none-acc-a0.5-bigldc-force13-cfg13.s1)
    "grouped.acc": 1.11,               # 0.5539 (grouped-two-ragged)
    "v1.act": 1.03,                    # 0.5156 (v1 nt 129 x 8 x 64 bias_gelu-v1)
    "v1.aux": 1.84,                    # 0.9205 (v1 nt 7 x 136 x 128 bias_gelu-v1)
    "v1.out": 0.655,                   # 0.3274 (v1 nt 129 x 8 x 64 bias_res-v1)
    "skepi.act": 0.988,                # 0.4942 (range nt 264 x 136 x 704 bias_gelu-gelumax-force3-cfg3.s3)
    "skepi.aux": 1.68,                 # 0.8388 (splitk nt 264 x 136 x 704 bias_gelu-force3-cfg3.s3)
    "skepi.colsum_sep": 0.222,         # 0.1109 (splitk nt 264 x 136 x 704 bias-cs-force3-cfg3.s3)
    "skepi.out": 0.386,                # 0.1929 (splitk nt 264 x 136 x 704 none-force5-cfg5.s3)
    "skred.acc": 0.703,                # 0.3514 (splitk nt 264 x 136 x 704 none-acc-a0.5-force0-cfg0.s2)
    "f32.64.acc": 1.99,                # 0.9962 (shape tn 68 x 132 x 32 none-f32.64)
    "f32.64.aux": 1.49,                # 0.7455 (stride nt 264 x 264 x 100 bias_relu-bigldx-f32.64)
    "f32.128.acc": 4.72,               # 2.358 (big tn 2044 x 3580 x 100 bias_res-f32.128)
    "f32.128.aux": 3.37,               # 1.686 (stride nt 264 x 264 x 100 bias_relu-bigldx-f32.64)
    "f32.split.acc": 0.836,            # 0.4179 (stride nt 264 x 264 x 420 none-bigldb-f32.64.s3)
    "f32.split.aux": 0.702,            # 0.3511 (stride nt 264 x 264 x 420 bias_relu-bigldx-f32.64.s3)
    "f32.sk.acc": 1.87,                # 0.9333 (epi nt 1156 x 1156 x 164 none-f32.sk)
    "f32.sk.aux": 1.72,                # 0.8593 (epi nt 1156 x 1156 x 164 bias_relu-f32.sk)
}

# what the older tests of the same paths allow (atol, rtol), asserted alongside so the new
# check is never looser: test_kernels_gpu.py (test_gemm2_configs, test_gemm_asymmetric_*,
# split-K accumulate), test_gemm_epilogue_inflight_gpu.py, test_f32_gpu.py (2e-4 sqrt(K) at
# the largest K used here, 448 / 196)
OLD_TOL = {}
for _c in ("g2", "g3nt", "g6", "g8", "snt", "v1", "skepi"):
    OLD_TOL.update({f"{_c}.out": (2e-2, 2e-2), f"{_c}.act": (2e-2, 2e-2), f"{_c}.aux": (2e-2, 2e-2),
                    f"{_c}.colsum": (0.3, 2e-2), f"{_c}.colsum_act": (0.3, 2e-2),
                    f"{_c}.colsum_sep": (0.3, 2e-2)})   # column sums: 0.05 sqrt(M) at the smallest M here, 40
for _c in ("g2", "g3tt", "stt", "grouped", "skred"):
    OLD_TOL[f"{_c}.acc"] = (3e-2, 1e-2)
for _c in ("f32.64", "f32.128", "f32.split", "f32.sk"):
    OLD_TOL.update({f"{_c}.acc": (4e-4, 1e-5), f"{_c}.aux": (4e-4, 1e-5)})   # 2e-4 sqrt(K) at K = 4

K0, K1 = 0.7978845608028654, 0.044715


def f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def gelu_parts(x):
    """tanh-GELU, its first and its second derivative, float64"""
    u = K0 * (x + K1 * x ** 3)
    t = torch.tanh(u)
    s = 1 - t * t
    du = K0 * (1 + 3 * K1 * x * x)
    g = 0.5 * x * (1 + t)
    d1 = 0.5 * (1 + t) + 0.5 * x * s * du
    d2 = s * du + 0.5 * x * (-2 * t * s * du * du + s * 6 * K0 * K1 * x)
    return g, d1, d2


def _max3(fn, x, h):
    return torch.maximum(torch.maximum(fn(x - h).abs(), fn(x).abs()), fn(x + h).abs())


def gemm_ref(A, B, transA=False, transB=False, alpha=1.0, epi="none", bias=None, R=None, aux=None, C0=None,
             keep=None, colsum0=None, stored=None, f32=False):
    """Everything one GEMM call writes, unrounded, with its error scales.

    bf16 engines (``f32`` False): ``epi`` is a key of EPI; ``aux`` is the saved tensor dGELU /
    dReLU read; C0 the incoming f32 C of an accumulating call.  f32 engines: ``epi`` is a key
    of F32_EPI, ``R`` is the residual or, for drelu, the saved pre-activation; C0 may join any
    epilogue (v = alpha acc + C0 + bias, as epi_store has it).  ``keep``: [M, N] of 0 or
    1 / (1 - p), the dropout mask of the four epilogues that take one.

    Returns out / A_out, pre / A_pre (before the activation), aux / A_aux (what bias_gelu and
    bias_relu save: GELU's derivative, ReLU's pre-activation), unsure (bool [M, N], see the
    module docstring), colsum / A_colsum if ``colsum0`` is given."""
    a, b = f64(A), f64(B)
    a = a.t() if transA else a
    b = b if transB else b.t()
    acc, aacc = a @ b, a.abs() @ b.abs()
    pre, A_pre = alpha * acc, abs(alpha) * aacc
    if C0 is not None:
        pre, A_pre = pre + f64(C0), A_pre + f64(C0).abs()
    if "bias" in epi:
        pre, A_pre = pre + f64(bias)[None, :], A_pre + f64(bias).abs()[None, :]
    kp = torch.ones_like(pre) if keep is None else f64(keep)
    assert keep is None or epi in DROP_EPIS or (f32 and epi in ("bias_relu", "drelu"))
    r = NS(pre=pre, A_pre=A_pre, aux=None, A_aux=None, unsure=torch.zeros_like(pre, dtype=torch.bool))
    h = (0.0 if f32 else EPS_BF16) * pre.abs() + SUM_SLACK * A_pre
    if epi in ("none", "bias"):
        out, A_out = pre, A_pre
    elif epi in ("res", "bias_res"):
        out, A_out = pre + f64(R), A_pre + f64(R).abs()
    elif epi == "bias_gelu":
        g, d1, _ = gelu_parts(pre)
        out, A_out = g * kp, _max3(lambda x: gelu_parts(x)[1], pre, h) * A_pre * kp
        r.aux, r.A_aux = d1, _max3(lambda x: gelu_parts(x)[2], pre, h) * A_pre
    elif epi == "bias_relu":
        r.unsure = pre.abs() <= h
        live = (pre > -h).double()
        out, A_out = torch.relu(pre) * kp, live * A_pre * kp
        r.aux, r.A_aux = pre, A_pre
    elif epi == "dgelu":
        out, A_out = pre * f64(aux) * kp, A_pre * f64(aux).abs() * kp
    elif epi == "drelu":
        gate = ((f64(R) if f32 else f64(aux)) > 0).double()
        out, A_out = pre * gate * kp, A_pre * gate * kp
    else:
        raise ValueError(epi)
    r.out, r.A_out = out, A_out
    if colsum0 is not None:
        s = out if stored is None else f64(stored)
        r.colsum, r.A_colsum = f64(colsum0) + s.sum(0), f64(colsum0).abs() + s.abs().sum(0)
    return r


# ------------------------------------------------------------------ the check
def metric(got, ref, A, eps):
    """(err, bad): err = max |got - ref| / (eps (|ref| + A)) over the elements with a non-zero
    denominator; bad = elements that are non-finite, or non-zero where nothing was summed."""
    got, ref, A = f64(got).reshape(-1), f64(ref).reshape(-1), f64(A).reshape(-1)
    den = eps * (ref.abs() + A)
    zero = den == 0
    bad = int((~torch.isfinite(got)).sum()) + int((got[zero] != 0).sum())
    ok = ~zero & torch.isfinite(got)
    err = float(((got - ref).abs()[ok] / den[ok]).max()) if ok.any() else 0.0
    return err, bad


class Report:
    """Collects the figures of one case: every check prints its MEASURE line and records a
    failure; ``finish`` raises once, after all figures are out."""

    def __init__(self, what, bound=None, old_tol=None):
        self.what, self.fails, self.seen = what, [], {}
        self.bound = BOUND if bound is None else bound
        self.old_tol = OLD_TOL if old_tol is None else old_tol

    def fail(self, msg):
        self.fails.append(f"{self.what}: {msg}")

    def expect(self, cond, msg):
        if not cond:
            self.fail(msg)

    def value(self, key, got, ref, A, eps=None, old=True):
        """one output against the metric, BOUND[key] and (``old``) OLD_TOL[key]"""
        eps = (EPS_BF16 if got.dtype == BF16 else EPS_F32) if eps is None else eps
        if tuple(got.shape) != tuple(ref.shape):
            self.fail(f"{key}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
            return
        err, bad = metric(got, ref, A, eps)
        self.expect(bad == 0, f"{key}: {bad} elements non-finite, or non-zero where nothing is summed")
        if old and key in self.old_tol and bad == 0:
            atol, rtol = self.old_tol[key]
            over = float(((f64(got) - f64(ref)).abs() - (atol + rtol * f64(ref).abs())).max())
            self.expect(over <= 0, f"{key}: outside the older test's atol {atol} / rtol {rtol} by {over:.3e}")
        self.seen[key] = max(self.seen.get(key, 0.0), err)
        print(f"MEASURE {key} {err:.4g} {self.what}")
        if key not in self.bound:
            self.fail(f"{key}: no bound recorded (measured {err:.4g})")
        else:
            self.expect(err <= self.bound[key], f"{key}: error {err:.4g} > bound {self.bound[key]:.4g}")

    def exact(self, name, got, want):
        """every element equal (exact-input cases: nothing is rounded; +0 and -0 are one value)"""
        if got.dtype != want.dtype or got.shape != want.shape or not torch.isfinite(f64(got)).all():
            self.fail(f"{name}: dtype, shape or a non-finite value")
        elif not torch.equal(f64(got), f64(want)):
            self.fail(f"{name}: {int((f64(got) != f64(want)).sum())} elements differ from the exact result")

    def finish(self):
        assert not self.fails, "\n".join(self.fails)


def check_outputs(rep, cls, ref, got, epi="none", old=True):
    """``got``: the kernel's outputs as CPU tensors cut to [M, N]: out (bf16 or f32), and where
    the call wrote them aux and colsum.  ``cls``: the engine class, first part of the BOUND key.
    ``old``: also assert OLD_TOL (not for inputs scaled to the ends of the number range: the
    older tests' absolute tolerances are those of O(1) values)."""
    out = got["out"]
    if out.dtype == F32:
        key = "acc"
    else:
        key = "out" if epi in ONE_ROUNDING else "act"
    rep.value(f"{cls}.{key}", out, ref.out, ref.A_out, old=old)
    n_unsure = int(ref.unsure.sum())
    rep.expect(n_unsure <= UNSURE_CAP * ref.unsure.numel(),
               f"{n_unsure} pre-activations within half an ulp of 0: more than {UNSURE_CAP:.1%} of the case")
    if got.get("aux") is not None and ref.aux is not None:
        rep.value(f"{cls}.aux", got["aux"], ref.aux, ref.A_aux, old=old)
    if got.get("colsum") is not None:
        rep.value(f"{cls}.{got.get('colsum_key', 'colsum')}", got["colsum"], ref.colsum, ref.A_colsum, old=old)


# ------------------------------------------------------------------ inputs
def pi(m, K):
    return (37 * m + 5) % K


def pi2(m, K, nsplit=1):
    """the second hot column of row m: another K-tile than pi(m) and, with split-K, another
    split (splits own the K-tiles [y kt / S, (y + 1) kt / S))"""
    kt = K // BK
    t1 = pi(m, K) // BK
    if nsplit > 1:
        own = lambda t: max(y for y in range(nsplit) if y * kt // nsplit <= t)   # noqa: E731
        t2 = next(t for t in ((t1 + d) % kt for d in range(1, kt)) if own(t) != own(t1))
    else:
        t2 = (t1 + 1 + m % (kt - 1)) % kt if kt > 1 else t1
    return t2 * BK + (11 * m + 3) % BK


def exact_inputs(kind, M, N, K, nsplit=1, dtype=BF16):
    """(a [M, K], b [N, K], want [M, N] float64 at alpha = 1) of the exact-input cases.
    select: a[m, pi(m)] = 1, b[n, k] = ((131 n + 17 k) mod 251) - 125, so C[m, n] = b[n, pi(m)].
    twohot: a second 1 at pi2(m) (only where K holds two K-tiles), b in [-60, 60]: every sum
    is an integer of magnitude <= 120, exact in bf16."""
    m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
    a = torch.zeros(M, K, dtype=torch.float64)
    a[m, pi(m, K)] = 1.0
    b = ((131 * n[:, None] + 17 * k[None, :]) % 251 - 125).double()
    if kind == "twohot":
        b = ((131 * n[:, None] + 17 * k[None, :]) % 121 - 60).double()
        if K >= 2 * BK:
            a[m, torch.tensor([pi2(int(i), K, nsplit) for i in m])] = 1.0
    elif kind != "select":
        raise ValueError(kind)
    want = a @ b.t()
    assert torch.equal(want.to(dtype).double(), want)
    return a.to(dtype), b.to(dtype), want


def randn_inputs(M, N, K, seed, dtype=BF16, scale=1.0):
    """a [M, K], b [N, K] / sqrt(K), bias [N] (offset 0.25: keeps ReLU's pre-activation off 0
    for all but a few elements), r [M, N], aux [M, N], c0 [M, N] f32 small integers"""
    g = torch.Generator().manual_seed(7000 + seed)
    mk = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    a, b = mk(M, K) * scale, mk(N, K) * (K ** -0.5)
    bias, r, aux = mk(N) * 0.1 + 0.25, mk(M, N), mk(M, N)
    c0 = torch.randint(-8, 9, (M, N), generator=g).float()
    return NS(a=a.to(dtype), b=b.to(dtype), bias=bias.to(dtype), r=r.to(dtype), aux=aux.to(dtype), c0=c0)


BF16_MAX = (1.0 - 2.0 ** -8) * 2.0 ** 128


def make_inputs(c):
    """The inputs of a case, CPU tensors of its dtype: a [M, K], b [N, K], bias, r, aux, c0 and
    (exact kinds) ``want``, the float64 result at alpha = 1 before C0.

    randn    N(0, 1) x N(0, 1 / K), bias 0.25 + N(0, 0.01)
    select / twohot   exact_inputs; c0 holds small integers
    big      products near 2^122 (outputs near the top of the bf16 range)
    tiny     products near 2^-100 (the bottom of the f32 normal range, clear of flushed terms)
    zerorow  randn with rows 3 and M - 1 of A all zero: those outputs are exactly 0
    gelumax  bias+GELU of +-BF16_MAX (row 0), +-2^100 (row 1), +-2^30 (row 2): pre-activations
             whose square overflows f32, the regime that broke gelu_tanh_grad before
    mant24   f32 factors +-(1 + odd 2^-23): every product needs all 24 mantissa bits"""
    dt = BF16 if c.prec == "bf16" else F32
    M, N, K = c.M, c.N, c.K
    if c.kind in ("select", "twohot"):
        if c.prec == "f32":
            a, b, want = exact_inputs(c.kind, M, N, max(K, BK) if c.kind == "select" else K, 1, dt)
            a, b, want = a[:, :K], b[:, :K], None
            want = a.double() @ b.double().t()
        else:
            a, b, want = exact_inputs(c.kind, M, N, K, c.split, dt)
        x = randn_inputs(M, N, K, c.seed, dt)
        x.a, x.b, x.want = a, b, want
        return x
    x = randn_inputs(M, N, K, c.seed, dt)
    x.want = None
    if c.kind == "big":
        x.a, x.b = (x.a.double() * 2.0 ** 60).to(dt), (x.b.double() * 2.0 ** 62).to(dt)
    elif c.kind == "tiny":
        x.a, x.b = (x.a.double() * 2.0 ** -50).to(dt), (x.b.double() * 2.0 ** -50).to(dt)
    elif c.kind == "zerorow":
        x.a[min(3, M - 1)] = 0
        x.a[M - 1] = 0
    elif c.kind == "gelumax":
        sign = (1.0 - 2.0 * (torch.arange(N) % 2)).double()
        x.a[:3] = 0
        x.a[0, 0], x.a[1, 0], x.a[2, 0] = 2.0 ** 64, 2.0 ** 36, 2.0 ** -34
        x.b[:, 0] = (sign * (1.0 - 2.0 ** -8) * 2.0 ** 64).to(dt)
        x.bias = torch.zeros(N, dtype=dt)
    elif c.kind == "mant24":
        g = torch.Generator().manual_seed(c.seed)
        mk = lambda *s: ((1.0 + (2 * torch.randint(0, 2 ** 22, s, generator=g) + 1).double() * 2.0 ** -23) *   # noqa: E731
                         (1.0 - 2.0 * torch.randint(0, 2, s, generator=g))).float()
        x.a, x.b = mk(M, K), mk(N, K)
    elif c.kind != "randn":
        raise ValueError(c.kind)
    return x


# ------------------------------------------------------------------ which engine a case reaches
TILE = {0: (256, 256), 1: (256, 192), 2: (256, 128), 3: (128, 128), 4: (256, 256), 5: (256, 256), 6: (256, 256),
        9: (256, 192), 10: (64, 64), 11: (64, 32), 12: (32, 32), 13: (64, 64), 15: (256, 192), 16: (256, 192)}
CLASS = {0: "g2", 1: "g2", 2: "g2", 3: "g2", 4: "g3nt", 5: "g3nt", 6: "g3tt", 9: "g6", 10: "snt", 11: "snt", 12: "snt",
         13: "stt", 15: "g8", 16: "g8"}

# ------------------------------------------------------------------ cases
class Case:
    """One GEMM call of the GPU edge tests.  ``group`` names what the case is there for,
    ``kind`` its inputs (randn / select / twohot / big / tiny / zerorow / gelumax), ``stride``
    the one operand (lda / ldb / ldc / ldr / ldx) that lives in a buffer whose row stride is
    BIG_LD elements, ``path`` the launcher branch it reaches (the end of the id), stated
    literally: cfg<k>.s<split> as the binding gemm2_plan must report it (forced cfg k: split 1
    unless ``split`` says otherwise), v1, f32.64 / f32.128 (+ .s<split>), f32.sk."""

    def __init__(self, group, M, N, K, tA=False, tB=False, acc=False, cfg=-1, epi="none", alpha=1.0, p=0.0,
                 kind="randn", colsum=False, v1=False, prec="bf16", layout="nt", ks=0, path=None, seed=0, split=1,
                 stride=None):
        self.group, self.M, self.N, self.K, self.tA, self.tB, self.acc, self.cfg = group, M, N, K, tA, tB, acc, cfg
        self.epi, self.alpha, self.p, self.kind, self.colsum, self.v1 = epi, alpha, p, kind, colsum, v1
        self.prec, self.layout, self.ks, self.seed, self.stride = prec, layout, ks, seed, stride
        if prec == "f32":
            self.path, self.split = path, (ks if ks > 0 else 1)
            self.cls = "f32.sk" if ks == -2 else ("f32.split" if ks > 1 else path)
        elif v1:
            self.path, self.split, self.cls = "v1", 1, "v1"
        else:
            self.path = path or f"cfg{cfg}.s{split}"
            k, s = (int(x) for x in self.path[3:].split(".s"))
            assert cfg < 0 or k == cfg
            self.split, self.engine = s, k
            self.cls = CLASS[k] if s == 1 else ("skred" if acc else "skepi")

    @property
    def id(self):
        lay = self.layout if self.prec == "f32" else ("n", "t")[self.tA] + ("t", "n")[self.tB]
        s = f"{self.group}-{self.prec}-{lay}-M{self.M}-N{self.N}-K{self.K}-{self.epi}"
        s += "-acc" if self.acc else ""
        s += f"-a{self.alpha:g}" if self.alpha != 1.0 else ""
        s += f"-p{self.p:g}" if self.p else ""
        s += "-cs" if self.colsum else ""
        s += f"-{self.kind}" if self.kind != "randn" else ""
        s += f"-big{self.stride}" if self.stride else ""
        s += f"-force{self.cfg}" if self.cfg >= 0 and self.prec == "bf16" else ""
        return f"{s}-{self.path}"

    def __repr__(self):
        return self.id


KS = (64, 128, 192, 320, 448)            # kt = 1, 2, 3, 5, 7
NT_ENGINES = (0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 15, 16)
TT_ENGINES = (0, 2, 3, 6, 13)
ALPHAS = (1.0, 0.5, -2.0)


def _sizes(b):
    """one 8-wide sliver, a whole tile, a tile + 8, two tiles + a ragged third"""
    return (8, b, b + 8, 2 * b + 8)


def _bf16_cases():
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, seed=len(cs), **k))   # noqa: E731
    # shapes: every (M, N) edge combination per engine with K cycling through kt = 1, 2, 3, 5, 7,
    # and every K at the tile + 8 shape; TT engines accumulate into f32 with alpha
    for tt, engines in ((False, NT_ENGINES), (True, TT_ENGINES)):
        for e in engines:
            bm, bn = TILE[e]
            i = 0
            for M in _sizes(bm):
                for N in _sizes(bn):
                    add("shape", M, N, KS[(i + e) % 5], tt, tt, tt, e, alpha=ALPHAS[i % 3] if tt else 1.0)
                    i += 1
            for K in KS:
                add("shape", bm + 8, bn + 8, K, tt, tt, tt, e, alpha=ALPHAS[i % 3] if tt else 1.0, kind="select")
                i += 1
    # the 256x192 engines' store loop (504 of 512 threads): N = 192, 200, 392 are in _sizes(192)
    # epilogues: whole tile (in-flight store loop) and ragged (rolled), odd kt, fused column
    # sums on the ragged shape; accumulate shapes answer 2 and the wrapper sums separately
    for e in NT_ENGINES:
        bm, bn = TILE[e]
        for epi in EPI:
            add("epi", bm, bn, 192, cfg=e, epi=epi)
            add("epi", bm + 8, bn + 8, 320, cfg=e, epi=epi, colsum=True)
    # split-K, uneven (kt % split != 0): bf16 output through splitk_epi_kernel, f32
    # accumulate through splitk_reduce_kernel (row-strided C, alpha != 1), NT and TT
    for e in (0, 2, 3, 4, 5):
        for epi in (EPI if e in (3, 5) else ("none", "bias_res")):
            add("splitk", 264, 136, 704, cfg=e, epi=epi, colsum=(epi == "bias"), split=3)
    for epi in DROP_EPIS:
        add("splitk", 264, 136, 704, cfg=3, epi=epi, p=0.25, split=3)
    for e in (0, 2, 3):
        for K in (704, 832):
            add("splitk", 264, 136, K, acc=True, cfg=e, alpha=0.5, split=(2 if K == 704 else 3))
            add("splitk", 264, 136, K, True, True, True, cfg=e, alpha=-2.0, kind="twohot", split=(2 if K == 704 else 3))
    for K in (704, 832):
        add("splitk", 264, 136, K, True, True, True, cfg=6, alpha=0.5, split=(2 if K == 704 else 3))
    # the planner's own choice: long K short M NT; a dW shape on each side of K <= 4096
    add("splitk", 8, 264, 4160, kind="twohot", path="cfg2.s8")
    add("splitk", 128, 128, 4096, True, True, True, alpha=0.5, path="cfg13.s1")
    add("splitk", 128, 128, 4288, True, True, True, alpha=0.5, path="cfg2.s14")
    # an accumulate shape with column sums: gemm2 answers 2 and the caller sums C separately
    add("epi", 264, 136, 320, acc=True, cfg=2, alpha=0.5, colsum=True)
    # v1 fallback: M % 8 != 0
    for M in (1, 7, 129):
        for j, K in enumerate(KS):
            N = (8, 136, 264)[j % 3]
            for epi in ("none", "bias", "bias_gelu", "bias_relu", "bias_res", "res"):
                add("v1", M, N, K, epi=epi, v1=True)
            for epi in ("none", "dgelu", "drelu", "res"):
                add("v1", M, N, K, tB=True, epi=epi, v1=True)
    # dropout on the engines the older test leaves out, with the kernel's mask against act_fwd's
    for e in (10, 11, 12, 9, 15):
        bm, bn = TILE[e]
        for epi in DROP_EPIS:
            add("drop", bm + 8, bn + 8, 192, cfg=e, epi=epi, p=0.25)
    # exact inputs on every engine: bit for bit
    for tt, engines in ((False, NT_ENGINES), (True, TT_ENGINES)):
        for e in engines:
            bm, bn = TILE[e]
            for j, (M, N) in enumerate(((bm, bn), (bm + 8, 2 * bn + 8))):
                for kind in ("select", "twohot"):
                    add("exact", M, N, 320, tt, tt, tt, e, alpha=ALPHAS[(j + e) % 3], kind=kind)
    # value ranges, once per engine class
    for e in (2, 5, 9, 12, 15):
        bm, bn = TILE[e]
        for kind in ("big", "tiny", "zerorow"):
            add("range", bm + 8, bn + 8, 192, cfg=e, kind=kind)
        add("range", bm + 8, bn + 8, 192, cfg=e, epi="bias_gelu", kind="gelumax")
    for e in (2, 6, 13):
        bm, bn = TILE[e]
        add("range", bm + 8, bn + 8, 192, True, True, True, e, kind="zerorow")
    add("range", 7, 136, 192, epi="bias_gelu", kind="gelumax", v1=True)
    for kind in ("big", "tiny", "zerorow"):
        add("range", 129, 136, 192, kind=kind, v1=True)
        add("range", 264, 136, 704, cfg=3, kind=kind, split=3)                       # bf16 split-K epilogue pass
        add("range", 264, 136, 704, acc=True, cfg=0, kind=kind, split=2)             # f32 split-K reduce
    add("range", 264, 136, 704, cfg=3, epi="bias_gelu", kind="gelumax", split=3)
    for e in (2, 6, 13):
        bm, bn = TILE[e]
        for kind in ("big", "tiny"):
            add("range", bm + 8, bn + 8, 192, True, True, True, e, kind=kind)
    # large row strides, one operand at a time: the operand's rows are BIG_LD elements apart, so
    # from row 256 on row x stride leaves 32 bits (M or N = 264; the k-major operands of the TT
    # engines have K = 320 rows).  Every engine forms these products in 64 bits except gemm8's
    # operand loads (32-bit buffer offsets), whose launcher hands such A / B back: v1 then
    # takes the call, which the two cfg 15 cases with v1=True run.
    for e, ops_ in ((2, "abcrx"), (5, "abcrx"), (9, "abcrx"), (12, "abcrx"), (15, "crx")):
        for o in ops_:
            add("stride", 264, 264, 192, cfg=e, epi={"r": "res", "x": "bias_gelu"}.get(o, "none"), stride="ld" + o)
    for o in "abcrx":
        add("stride", 264, 264, 704, cfg=3, epi={"r": "res", "x": "bias_gelu"}.get(o, "none"), stride="ld" + o, split=3)
        add("stride", 263, 264, 192, epi={"r": "res", "x": "bias_gelu"}.get(o, "none"), stride="ld" + o, v1=True)
    for o in "ab":
        add("stride", 264, 264, 192, cfg=15, stride="ld" + o, v1=True)
    for e in (2, 6, 13):
        for o in "abc":
            add("stride", 264, 264, 320, True, True, True, e, alpha=0.5, stride="ld" + o)
    for o in "abc":
        add("stride", 264, 264, 704, True, True, True, 0, alpha=0.5, stride="ld" + o, split=2)
    return cs


BIG_LD = (1 << 23) + 8


F32_MN = (4, 60, 64, 68, 132)
F32_KS = (4, 28, 32, 36, 64, 68, 100, 196)


def _f32_cases():
    """gemm_f32_ex: ``ks`` is its force_ks (1: no split, s > 1: split s, -2: stream-K, 0: the
    planner's choice, used for the 128x128 engine, which it picks from 448 tiles on)"""
    cs, seen = [], set()

    def add(*a, **k):
        c = Case(*a, prec="f32", seed=1000 + len(cs), **k)
        if c.id not in seen:
            seen.add(c.id)
            cs.append(c)
    i = 0
    for lay in ("nt", "nn", "tn", "tt"):
        for M in F32_MN:
            for N in F32_MN:
                add("shape", M, N, F32_KS[i % 8], layout=lay, ks=1, path="f32.64", kind="select" if i % 4 == 3 else "randn")
                i += 1
        for K in F32_KS:
            add("shape", 68, 132, K, layout=lay, ks=1, path="f32.64")
    # forced split 2..8 at the smallest K the planner's own rule allows (npairs >= 2 s), + a K tail
    for s in range(2, 9):
        K = 2 * s * 64 - 28
        add("split", 68, 132, K, layout=("nt", "nn", "tn", "tt")[s % 4], ks=s, path=f"f32.64.s{s}", alpha=0.5,
            acc=(s % 2 == 0))
        add("split", 68, 132, K, layout="nt", ks=s, path=f"f32.64.s{s}", kind="twohot")
    # epilogues, alpha, accumulate, dropout on the tiled, split and stream-K paths.  Stream-K:
    # (200, 136, 4132) has 12 tiles x 65 pairs in chunks of 4 (a chunk ends inside a tile),
    # (1156, 1156, 164) 361 tiles x 3 pairs in chunks of 5 (a chunk spans three tiles); K tails
    for ks, path, shapes in ((1, "f32.64", ((68, 132, 100),)), (3, "f32.64.s3", ((68, 132, 420),)),
                             (-2, "f32.sk", ((200, 136, 4132), (1156, 1156, 164)))):
        for M, N, K in shapes:
            for epi in F32_EPI:
                add("epi", M, N, K, layout="nt", epi=epi, ks=ks, path=path, alpha=(0.5 if epi == "bias" else 1.0),
                    acc=(epi in ("res", "bias")))
            for epi in ("bias_relu", "drelu"):
                add("epi", M, N, K, layout="nt", epi=epi, ks=ks, path=path, p=0.25)
            for lay in ("nn", "tn", "tt"):
                add("epi", M, N, K, layout=lay, ks=ks, path=path, kind="select")
            add("epi", M, N, K, layout="nt", ks=ks, path=path, kind="twohot", acc=True)
    # the 128x128 engine at the smallest grid its planner accepts (448 tiles), K tails
    for j, K in enumerate((36, 100)):
        add("big", 2044, 3580, K, layout=("nt", "tn")[j], ks=0, path="f32.128", epi=("none", "bias_res")[j])
    # value ranges and large row strides on the tiled, split and stream-K paths (the 128x128
    # engine runs the same cases in its child process; in process its smallest grid is 2044 rows)
    for ks, path, (M, N, K) in ((1, "f32.64", (68, 132, 100)), (3, "f32.64.s3", (68, 132, 420)),
                                (-2, "f32.sk", (264, 136, 4132))):
        for kind in ("big", "tiny", "zerorow"):
            add("range", M, N, K, layout="nt", ks=ks, path=path, kind=kind)
        for o, epi, lay in (("a", "none", "nt"), ("a", "none", "tn"), ("b", "none", "nt"), ("b", "none", "nn"),
                            ("c", "none", "nt"), ("r", "res", "nt"), ("x", "bias_relu", "nt")):
            add("stride", 264, 264, K, layout=lay, ks=ks, path=path, epi=epi, stride="ld" + o)
    # all 24 mantissa bits: the bound must exclude a reduced-precision MFMA
    for lay in ("nt", "tt"):
        add("mant24", 68, 132, 100, layout=lay, ks=1, path="f32.64", kind="mant24")
    return cs


CASES = _bf16_cases()
F32_CASES = _f32_cases()
