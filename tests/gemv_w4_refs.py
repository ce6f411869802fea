"""float64 reference of the int4g128 weight-only linear layers (ops.quantize_w4,
ops.linear_skinny_w4, ops.linear_w4, ops.dequant_w4; csrc/kernels/gemv_skinny.hip), the check
the GPU tests run and the cases they use.  Plain functions: no ``ops`` import.

Format: ``q4`` uint8 [N, K / 2], byte b of a row = (q[n, 2 b] + 8) | (q[n, 2 b + 1] + 8) << 4,
``scale`` f32 [K / 128, N], effective weight ``What[n, k] = q[n, k] * scale[k // 128, n]``.  The
reference is ``gemm_refs.gemm_ref`` on What: ``epi(x @ What^T)`` in float64 with the error scale
``A = sum_g |x| |q| scale_g + |bias| + |R|`` and the metric of gemm_refs.py, exactly as
gemv_w8_refs.py does it for per-row scales.

Two kinds of inputs, as there:

* ``randn_case``: random values, measured with the metric.  One-rounding epilogues may not
  exceed 1.0 (an f32 sum rounded once); GELU and the dequantising route have ``BOUND``.
* ``exact_case``: quarters in [-2, 2] as x, q in [-7, 7], powers of two that differ per group and
  row as scales, bias in eighths, residual in quarters: every f32 partial sum is exact in any
  order, so a one-rounding output must equal ``bf16(v)`` bit for bit and a GELU output
  ``bf16(gelu(bf16(v)))`` wherever ``exact_expected`` marks it safe.
"""
from types import SimpleNamespace as NS

import torch

import gemm_refs as GR
from gemv_w8_refs import EPIS, MS, SPLITS, exact_expected  # noqa: F401  (the same epilogues, rows and splits)

BF16 = torch.bfloat16
GROUP = 128
# one tile, one group; N below a tile; ragged N with three groups that no even split divides;
# 17 groups; the multi-workgroup plan
SHAPES = ((16, 128), (8, 128), (40, 384), (264, 2176), (2304, 768))
DEQUANT_SHAPE = (264, 384)          # linear_w4 above W8_SKINNY_MAX_M rows
DEQUANT_MS = (17, 40)

# GELU and the dequantising route: 2 x the largest error measured on an MI355X over
# test_gemv_w4_gpu.py against the float64 reference (the measured value in the comment); the
# one-rounding epilogues of the skinny kernel are held to 1.0 whatever is measured
BOUND = {
    "skinny.out": 1.0,                 # hard: an f32 sum rounded once.  Measured 0.4794 (bias_res M16 N16 K128 split0)
    "skinny.act": 0.843,               # 0.4214 (bias_gelu M16 N16 K128 split0)
    "w4_dequant.out": 0.586,           # 0.2925 (linear_w4 res M40 N264 K384)
    "w4_dequant.act": 0.821,           # 0.41 (linear_w4 bias_gelu M17 N264 K384)
}


def pack(q):
    """q [N, K] integers in [-8, 7] -> uint8 [N, K / 2]"""
    u = (q.to(torch.int64) + 8)
    assert int(u.min()) >= 0 and int(u.max()) <= 15
    return (u[:, 0::2] + 16 * u[:, 1::2]).to(torch.uint8)


def unpack(q4):
    """uint8 [N, K / 2] -> float64 [N, K]: every nibble decodes as nibble - 8"""
    b = q4.cpu().to(torch.int64)
    out = torch.empty(b.shape[0], 2 * b.shape[1], dtype=torch.float64)
    out[:, 0::2] = (b % 16 - 8).double()
    out[:, 1::2] = (b // 16 - 8).double()
    return out


def quantize_ref(w):
    """the format of ops.quantize_w4, written independently (f32 arithmetic as specified, one
    group at a time)"""
    w = w.detach().float().cpu()
    N, K = w.shape
    assert K % GROUP == 0
    G = K // GROUP
    scale = torch.zeros(G, N, dtype=torch.float32)
    q = torch.zeros(N, K, dtype=torch.float32)
    for g in range(G):
        blk = w[:, GROUP * g: GROUP * (g + 1)]
        s = blk.abs().max(dim=1).values / 7.0
        scale[g] = s
        nz = s > 0
        q[nz, GROUP * g: GROUP * (g + 1)] = torch.round(blk[nz] / s[nz, None]).clamp(-7, 7)
    return pack(q), scale


def what(q4, scale):
    """float64 [N, K] effective weight"""
    return unpack(q4) * scale.double().cpu().t().repeat_interleave(GROUP, dim=1)


def w4_ref(x, q4, scale, epi="none", bias=None, R=None):
    """gemm_refs.gemm_ref of epi(x @ What^T): .out, .A_out, .pre, .A_pre"""
    return GR.gemm_ref(x, what(q4, scale), epi=epi, bias=bias if "bias" in epi else None,
                       R=R if "res" in epi else None)


def zero_group(N, K):
    """(row, group) of the all-zero group of both cases"""
    return min(1, N - 1), min(1, K // GROUP - 1)


def randn_case(M, N, K, seed=0, xmax=None):
    """x [M, K] bf16, q4 [N, K / 2] (+-7 reached in every non-zero group, both signs in row 0),
    scale [K / 128, N] f32 with one group all zero (``zero_group``), bias [N], r [M, N] bf16.
    The rows have their own magnitudes and so do the groups of a row."""
    g = torch.Generator().manual_seed(9300 + seed)
    G = K // GROUP
    w = torch.randn(N, K, generator=g) * (K ** -0.5) * (0.5 + torch.rand(N, 1, generator=g))
    w = (w.view(N, G, GROUP) * (0.25 + torch.rand(N, G, 1, generator=g))).reshape(N, K)
    w[0, 0], w[0, 1] = w[0].abs().max() * 1.5, -w[0].abs().max() * 1.5
    zr, zg = zero_group(N, K)
    w[zr, GROUP * zg: GROUP * (zg + 1)] = 0
    q4, scale = quantize_ref(w)
    x = torch.randn(M, K, generator=g)
    if xmax is not None:
        x = (x * (xmax / 4.0)).clamp(-xmax, xmax)
        x[0, 0], x[M - 1, K - 1] = xmax, -xmax
    bias = torch.randn(N, generator=g) * 0.1 + 0.25
    r = torch.randn(M, N, generator=g)
    return NS(x=x.to(BF16), q4=q4, scale=scale, bias=bias.to(BF16), r=r.to(BF16))


def exact_case(M, N, K, seed=0):
    """Inputs whose f32 sums are exact in any order (see the module docstring), scaled so the
    values before the final rounding are O(1..8) and need more than 8 bits.  ``v`` [M, N]
    float64: epi -> the exact value before the activation / final rounding."""
    g = torch.Generator().manual_seed(9400 + seed)
    G = K // GROUP
    # quarters in [-2, 2]: with |q| <= 7 a group's sum of integers would fit 8 bits
    x = torch.randint(-8, 9, (M, K), generator=g).double() / 4
    q = torch.randint(-7, 8, (N, K), generator=g).double()
    q[:, 0::GROUP] = (7.0 * (1.0 - 2.0 * (torch.arange(N) % 2)))[:, None]      # +-7 at the head of every group
    e = max(0, round(torch.log2(torch.tensor(6.0 * K ** 0.5)).item()) - 1)
    # a power of two for every (group, row), three different ones along either index
    scale = 2.0 ** -(e + ((torch.arange(G)[:, None] + 2 * torch.arange(N)[None, :]) % 3).double())
    zr, zg = zero_group(N, K)
    scale[zg, zr] = 0
    q[zr, GROUP * zg: GROUP * (zg + 1)] = 0
    bias = torch.randint(-16, 17, (N,), generator=g).double() / 8
    r = torch.randint(-16, 17, (M, N), generator=g).double() / 4
    xg, qg = x.view(M, G, GROUP), q.view(N, G, GROUP)
    part = torch.einsum("mgk,ngk->gmn", xg, qg) * scale[:, None, :]                 # [G, M, N]
    acc = part.sum(0)
    # every value any summation order can meet is a multiple of 2^-(e + 4) (x in quarters,
    # scales down to 2^-(e + 2), bias in eighths) below the sum of all magnitudes: exact in f32
    # if that sum has fewer than 2^24 such units
    mag = torch.einsum("mgk,ngk->gmn", xg.abs(), qg.abs()) * scale[:, None, :]
    assert float((mag.sum(0) + bias.abs()[None] + r.abs()).max()) * 2.0 ** (e + 4) < 2 ** 24
    v = {"none": acc, "bias": acc + bias, "bias_gelu": acc + bias, "res": acc + r, "bias_res": acc + bias + r}
    for t in v.values():
        assert torch.equal(t.float().double(), t)
    w = q * scale.t().repeat_interleave(GROUP, dim=1)
    return NS(x=x.to(BF16), q4=pack(q), scale=scale.float(), bias=bias.to(BF16), r=r.to(BF16), v=v,
              w_exact=bool(torch.equal(w.to(BF16).double(), w)))


def check(got, ref, epi, cls="skinny", bound=None):
    """(err, bad, ok): the metric of one bf16 output against a ``w4_ref`` result and its bound"""
    b = (BOUND if bound is None else bound)[f"{cls}.{'out' if epi in GR.ONE_ROUNDING else 'act'}"]
    if epi == "bias_gelu":
        # as in gemv_w8_refs.check: an output below 2^-50 where the float64 reference and its
        # error scale are exactly 0 counts as the 0 it stands for
        got = got.detach().cpu().double()
        got = torch.where((got.abs() < 2.0 ** -50) & (ref.out == 0) & (ref.A_out == 0), torch.zeros_like(got), got)
    err, bad = GR.metric(got, ref.out, ref.A_out, GR.EPS_BF16)
    return err, bad, bad == 0 and err <= b


def check_exact(got, v, epi):
    """(wrong, safe): elements of an exact case that differ from what they must be, and how
    many are determined"""
    want, safe = exact_expected(v, epi)
    g = got.detach().cpu()
    assert g.dtype == BF16 and g.shape == want.shape
    return int(((g.double() != want.double()) & safe).sum()), int(safe.sum())
