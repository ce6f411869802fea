"""float64 reference of the int8 weight-only linear layers (ops.quantize_w8, ops.linear_skinny,
ops.linear_w8, ops.dequant_w8; csrc/kernels/gemv_skinny.hip), the check the GPU tests run and
the cases they use.  Plain functions: no ``ops`` import.

The effective weight is ``What = q * scale`` and the reference is ``gemm_refs.gemm_ref`` on it:
``epi(x @ What^T)`` in float64 with the error scale ``A = |x| |q| scale + |bias| + |R|`` carried
through GELU by the largest derivative over the half-ulp interval of the pre-activation, and
the metric ``err = |got - ref| / (2^-8 (|ref| + A))`` of gemm_refs.py.

Two kinds of inputs:

* ``randn_case``: random values, measured with the metric.  One-rounding epilogues (an f32 sum
  rounded once to bf16) may not exceed 1.0; GELU has the bound ``BOUND["skinny.act"]``.
* ``exact_case``: small integers in x, powers of two as scales, multiples of 1/8 and 1/4 as bias
  and residual.  Every f32 partial sum is then exact in any order, so the value before the
  final rounding is known exactly (``v``): a one-rounding output must equal ``bf16(v)`` bit for
  bit, and a GELU output must equal ``bf16(gelu(bf16(v)))`` wherever that value is clear of a
  bf16 rounding boundary.  This is what sees a second rounding (the metric forgives half an
  ulp twice): the scale applied after a bf16 rounding of the sum, GELU of the unrounded
  pre-activation.
"""
from types import SimpleNamespace as NS

import torch

import gemm_refs as GR

BF16 = torch.bfloat16
EPIS = ("none", "bias", "bias_gelu", "res", "bias_res")
MS = (1, 2, 5, 8, 16)
SPLITS = (1, 3, 0)
# an exact tile; N below one tile; a ragged N tail with an odd K-step count; 65 K-steps of 32
# (17 of 128) that no split divides evenly; large enough for the multi-workgroup plan
SHAPES = ((16, 32), (8, 32), (40, 96), (264, 2080), (2304, 768))
DEQUANT_SHAPE = (264, 320)          # linear_w8 above W8_SKINNY_MAX_M rows
DEQUANT_MS = (17, 40)

# the layer and head shapes (N, K) of the models tools/w8_time.py measures
MODEL_SHAPES = {
    "gpt2-small": ((2304, 768), (768, 768), (3072, 768), (768, 3072), (50304, 768)),
    "llama3-1b": ((3072, 2048), (2048, 2048), (16384, 2048), (2048, 8192), (128256, 2048)),
    "llama3-8b": ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128256, 4096)),
}

# GELU and the dequantising route: 2 x the largest error measured on an MI355X over two runs of
# test_gemv_skinny_gpu.py (the measured value in the comment); the one-rounding epilogues of
# the skinny kernel are held to 1.0 whatever is measured
BOUND = {
    "skinny.out": 1.0,                 # hard: an f32 sum rounded once.  Measured 0.4399 (int8 bias_res M16 N264 K2080 xmax128)
    "skinny.act": 1.23,                # 0.6163 (int8 bias_gelu M8 N16 K32 split1)
    "w8_dequant.out": 0.996,           # 0.4981 (linear_w8 bias_res M40 N264 K320)
    "w8_dequant.act": 0.84,            # 0.4201 (linear_w8 bias_gelu M40 N264 K320)
}


def quantize_ref(w):
    """the format of ops.quantize_w8, written independently (f32 arithmetic as specified)"""
    w = w.detach().float().cpu()
    scale = w.abs().max(dim=1).values / 127.0
    q = torch.zeros_like(w)
    nz = scale > 0
    q[nz] = torch.round(w[nz] / scale[nz, None]).clamp(-127, 127)
    return q.to(torch.int8), scale


def what(q, scale):
    return q.double().cpu() * scale.double().cpu()[:, None]


def w8_ref(x, q, scale, epi="none", bias=None, R=None):
    """gemm_refs.gemm_ref of epi(x @ (q * scale)^T): .out, .A_out, .pre, .A_pre"""
    return GR.gemm_ref(x, what(q, scale), epi=epi, bias=bias if "bias" in epi else None,
                       R=R if "res" in epi else None)


def bf16_ref(x, w, epi="none", bias=None, R=None):
    """the same for a bf16 weight matrix"""
    return GR.gemm_ref(x, w, epi=epi, bias=bias if "bias" in epi else None, R=R if "res" in epi else None)


def randn_case(M, N, K, seed=0, xmax=None):
    """x [M, K] bf16, q [N, K] int8 (+-127 in every non-zero row's maximum, and both signs in
    row 0), scale [N] f32 with row 1 (or 0) all zero, bias [N], r [M, N] bf16.  ``xmax``: x
    is scaled to reach +-xmax."""
    g = torch.Generator().manual_seed(9100 + seed)
    w = torch.randn(N, K, generator=g) * (K ** -0.5) * (0.5 + torch.rand(N, 1, generator=g))
    w[0, 0], w[0, 1] = w[0].abs().max() * 1.5, -w[0].abs().max() * 1.5
    w[min(1, N - 1)] = 0
    q, scale = quantize_ref(w)
    x = torch.randn(M, K, generator=g)
    if xmax is not None:
        x = x * (xmax / 4.0)
        x = x.clamp(-xmax, xmax)
        x[0, 0], x[M - 1, K - 1] = xmax, -xmax
    bias = torch.randn(N, generator=g) * 0.1 + 0.25
    r = torch.randn(M, N, generator=g)
    return NS(x=x.to(BF16), q=q, scale=scale, bias=bias.to(BF16), r=r.to(BF16), w=what(q, scale).to(BF16))


def exact_case(M, N, K, seed=0):
    """Inputs whose f32 sums are exact in any order (see the module docstring), scaled so the
    values before the final rounding are O(1..8) and need more than 8 bits.  ``v`` [M, N]
    float64: epi -> the exact value before the activation / final rounding."""
    g = torch.Generator().manual_seed(9200 + seed)
    x = torch.randint(-2, 3, (M, K), generator=g).double()
    q = torch.randint(-127, 128, (N, K), generator=g).double()
    q[:, 0] = 127.0 * (1.0 - 2.0 * (torch.arange(N) % 2))
    e = max(0, round(torch.log2(torch.tensor(100.0 * K ** 0.5)).item()) - 1)
    scale = 2.0 ** -(e + (torch.arange(N) % 3).double())
    scale[min(1, N - 1)] = 0
    q[min(1, N - 1)] = 0
    bias = torch.randint(-16, 17, (N,), generator=g).double() / 8
    r = torch.randint(-16, 17, (M, N), generator=g).double() / 4
    acc = x @ q.t()
    assert float(acc.abs().max()) < 2 ** 24
    v = {"none": acc * scale, "bias": acc * scale + bias, "bias_gelu": acc * scale + bias,
         "res": acc * scale + r, "bias_res": acc * scale + bias + r}
    for t in v.values():      # representable in f32: the kernel's own f32 epilogue is exact
        assert torch.equal(t.float().double(), t)
    return NS(x=x.to(BF16), q=q.to(torch.int8), scale=scale.float(), bias=bias.to(BF16), r=r.to(BF16), v=v,
              w=(q * scale[:, None]).to(BF16), w_exact=bool(torch.equal((q * scale[:, None]).to(BF16).double(),
                                                                      q * scale[:, None])))


def exact_expected(v, epi):
    """(want bf16 [M, N], safe bool [M, N]): the output an exact case must give, and where it
    is determined (always, except a GELU value within 2^-6 ulp of a bf16 rounding boundary)"""
    if epi != "bias_gelu":
        return v.to(BF16), torch.ones_like(v, dtype=torch.bool)
    # x sigmoid(2u), not 0.5 x (1 + tanh u): the latter cancels in the negative tail even in f64
    x = v.to(BF16).double()
    g = x * torch.sigmoid(2.0 * GR.K0 * (x + GR.K1 * x ** 3))
    want = g.to(BF16)
    # the 16 bits of f32(g) that the bf16 rounding drops, as a fraction of a bf16 ulp: the
    # rounding boundary is at 0.5.  The kernel's f32 GELU (v_exp_f32, v_rcp_f32: an ulp each, and
    # an exponent argument of magnitude up to 2.3 |u| rounded to f32) is within 2^-17 of the
    # true value for |x| <= 5, a 2^-9 fraction of a bf16 ulp; beyond 5 the negative tail's
    # exponent argument grows with |x|^3 and so does its error, so those are left out
    frac = (g.float().view(torch.int32) & 0xFFFF).double() / 65536.0
    return want, ((frac - 0.5).abs() > 2.0 ** -6) & (x.abs() <= 5.0)


def check(got, ref, epi, cls="skinny", bound=None):
    """(err, bad, ok): the metric of one bf16 output against a ``*_ref`` result and its bound"""
    b = (BOUND if bound is None else bound)[f"{cls}.{'out' if epi in GR.ONE_ROUNDING else 'act'}"]
    if epi == "bias_gelu":
        # float64 tanh is exactly -1 below u = -19 or so, where the reference and its error scale
        # become exactly 0 while the true GELU is a non-zero value below 2^-50 -- which the
        # kernel's x sigmoid(2u) form returns.  Such an output counts as the 0 it stands for.
        got = got.detach().cpu().double()
        got = torch.where((got.abs() < 2.0 ** -50) & (ref.out == 0) & (ref.A_out == 0), torch.zeros_like(got), got)
    err, bad = GR.metric(got, ref.out, ref.A_out, GR.EPS_BF16)
    return err, bad, bad == 0 and err <= b


def check_exact(got, v, epi):
    """number of elements of an exact case that differ from what they must be"""
    want, safe = exact_expected(v, epi)
    g = got.detach().cpu()
    assert g.dtype == BF16 and g.shape == want.shape
    return int(((g.double() != want.double()) & safe).sum()), int(safe.sum())
