"""float64 reference of the MXFP4 weight-only linear layers (ops.quant.quantize_mx4, linear_skinny_mx4,
linear_mx4, dequant_mx4; gemv_mx4_kernel of csrc/kernels/gemv_skinny.hip) and the cases the tests use.
Plain functions: no ``ops`` import.

Format: ``q4`` uint8 [N, K / 2], byte b of a row = code[n, 2 b] | code[n, 2 b + 1] << 4, a code being
sign << 3 | index into (0, .5, 1, 1.5, 2, 3, 4, 6) and code 8 read as 0; ``scale`` uint8 [N, K / 32],
byte e = 2^(e - 127); ``What[n, k] = e2m1(code[n, k]) * 2^(scale[n, k // 32] - 127)``.  The reference is
``gemm_refs.gemm_ref`` on What with the error scale ``A = sum |x| |What| + |bias| + |R|``, checked by
``gemv_w4_refs.check`` (the same metric) against ``BOUND``."""
from types import SimpleNamespace as NS

import torch

import gemm_refs as GR
from gemv_w8_refs import EPIS, MS, SPLITS  # noqa: F401  (the same epilogues, rows and splits)

BF16 = torch.bfloat16
GROUP = 32
SHAPES = ((16, 128), (8, 128), (40, 384), (264, 2176), (2304, 768))
DEQUANT_SHAPE = (264, 384)
DEQUANT_MS = (17, 40)
MAGS = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, 0, -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)
E8M0 = torch.tensor([2.0 ** (e - 127) for e in range(255)] + [float("nan")], dtype=torch.float64)

# GELU and the dequantising route: 2 x the largest error measured on an MI355X over test_gemv_mx4_gpu.py
# against the float64 reference (the measured value in the comment); the one-rounding epilogues of the
# skinny kernel are held to 1.0 whatever is measured
BOUND = {
    "skinny.out": 1.0,                 # hard: an f32 sum rounded once.  Measured 0.3573 (bias_res M16 N16 K128 split1)
    "skinny.act": 0.6762,              # 0.3381 (bias_gelu M5 N2304 K768 split1)
    "mx4_dequant.out": 0.5144,         # 0.2572 (linear_mx4 res M40 N264 K384)
    "mx4_dequant.act": 0.8992,         # 0.4496 (linear_mx4 bias_gelu M40 N264 K384)
}


def pack(code):
    """codes [N, K] in 0..15 -> uint8 [N, K / 2]"""
    return (code[:, 0::2] + 16 * code[:, 1::2]).to(torch.uint8)


def unpack(q4):
    """uint8 [N, K / 2] -> float64 [N, K] of e2m1 values"""
    b = q4.cpu().to(torch.int64)
    return MAGS[torch.stack((b % 16, b // 16), dim=2).reshape(b.shape[0], -1)]


def what(q4, scale):
    """float64 [N, K] effective weight"""
    return unpack(q4) * E8M0[scale.cpu().to(torch.int64)].repeat_interleave(GROUP, dim=1)


def quantize_ref(w):
    """the format of ops.quant.quantize_mx4, written independently: floor(log2 amax) by counting the powers
    of two not above amax, the nearest magnitude by distance in float64 with the even codes listed first
    (argmin returns the first of two equal distances)"""
    w = w.detach().float().cpu().double()
    N, K = w.shape
    g = w.view(N, K // GROUP, GROUP)
    amax = g.abs().amax(dim=2)
    pow2 = torch.tensor([2.0 ** e for e in range(-149, 128)], dtype=torch.float64)
    E = (torch.bucketize(amax, pow2, right=True) - 1 - 149 - 2).clamp(-127, 127)
    E = torch.where(amax > 0, E, torch.full_like(E, -127))
    a = g.abs() / E8M0[E + 127][:, :, None]
    order = torch.tensor([0, 2, 4, 6, 1, 3, 5, 7])
    code = order[(a[..., None] - MAGS[order]).abs().argmin(dim=-1)]
    code = code + 8 * ((g < 0) & (code > 0))
    return pack(code.view(N, K)), (E + 127).to(torch.uint8)


def mx4_ref(x, q4, scale, epi="none", bias=None, R=None):
    return GR.gemm_ref(x, what(q4, scale), epi=epi, bias=bias if "bias" in epi else None,
                       R=R if "res" in epi else None)


def randn_case(M, N, K, seed=0):
    """x [M, K] bf16, (q4, scale) of a random w whose rows and groups have their own magnitudes (one group
    all zero), bias [N], r [M, N] bf16"""
    g = torch.Generator().manual_seed(9500 + seed)
    G = K // GROUP
    w = torch.randn(N, K, generator=g) * (K ** -0.5) * (0.5 + torch.rand(N, 1, generator=g))
    w = (w.view(N, G, GROUP) * (0.25 + torch.rand(N, G, 1, generator=g))).reshape(N, K)
    w[min(1, N - 1), GROUP: 2 * GROUP] = 0
    q4, scale = quantize_ref(w)
    assert int(scale[scale > 0].min()) >= 2 and int(scale.max()) <= 250
    x = torch.randn(M, K, generator=g)
    bias = torch.randn(N, generator=g) * 0.1 + 0.25
    r = torch.randn(M, N, generator=g)
    return NS(x=x.to(BF16), q4=q4, scale=scale, bias=bias.to(BF16), r=r.to(BF16))


def exact_case(M, N, K, seed=0):
    """x in quarters within [-2, 2], any codes, scale bytes 126..128 by group and row, bias in eighths,
    residual in quarters: every value any summation order meets is a multiple of 2^-4 (x 2^-2, e2m1 2^-1,
    scale 2^-1) below 2^24 such units, so exact in f32.  ``v``: epi -> the exact value before the
    activation / final rounding."""
    g = torch.Generator().manual_seed(9600 + seed)
    x = torch.randint(-8, 9, (M, K), generator=g).double() / 4
    q4 = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    scale = (126 + (torch.arange(K // GROUP)[None, :] + 2 * torch.arange(N)[:, None]) % 3).to(torch.uint8)
    bias = torch.randint(-16, 17, (N,), generator=g).double() / 8
    r = torch.randint(-16, 17, (M, N), generator=g).double() / 4
    W = what(q4, scale)
    acc = x @ W.t()
    assert float((x.abs() @ W.abs().t() + bias.abs() + r.abs()).max()) * 16 < 2 ** 24
    v = {"none": acc, "bias": acc + bias, "bias_gelu": acc + bias, "res": acc + r, "bias_res": acc + bias + r}
    return NS(x=x.to(BF16), q4=q4, scale=scale, bias=bias.to(BF16), r=r.to(BF16), v=v)
