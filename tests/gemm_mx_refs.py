"""Cases and bounds of the MXFP8 x MXFP4 GEMM tests (csrc/kernels/gemm_mx.hip; ops.quant.quantize_mx8_rows,
linear_mx4a8).  Weights and the float64 reference are gemv_mx4_refs.py's; the reference activation is the float64
value of the MXFP8 rows."""
from types import SimpleNamespace as NS

import torch

import gemv_mx4_refs as MX

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
# the tile edges of both plan shapes: NARROW 64 x 32 (16-row wave tiles), SQUARE 128 x 128 from 65 rows on
MS = (1, 16, 17, 33, 64, 65, 129, 200)
SHAPES = ((40, 128), (264, 384), (136, 2176))
# 'out': one-rounding epilogues, hard.  'act' (GELU): 2 x the largest error measured on an MI355X
BOUND = {
    "mx.out": 1.0,                     # measured 0.3098 (bias_res M65 N40 K128)
    "mx.act": 0.9336,                  # 0.4668 (bias_gelu M200 N40 K128)
}


def hand_groups():
    """x f32 [2, 128] of hand-built groups, their e8m0 bytes [2, 4], and (row, k) -> e4m3 byte"""
    x = torch.zeros(2, 128)
    x[0, 3] = -0.0                                               # a zero group: byte 0, codes 0
    x[0, 32], x[0, 33] = 3584.0, -8.0                            # amax = 448 * 2^3: E = 3, no bump
    x[0, 64], x[0, 65] = 3584.0 + 2.0 ** -12, 16.0               # one f32 step above: E = 4, 224.00002 -> 224
    x[0, 96:100] = torch.tensor([256.0, 17.0, 19.0, -18.0])      # E = 0; ties to even: 17 -> 16, 19 -> 20
    # e4m3 subnormals (steps of 2^-9) under amax 256: 2^-10 -> 0, 1.5 -> 2, 2.5 -> 2 steps; -2^-11 -> code 0, not -0
    x[1, 0:8] = torch.tensor([256.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.0 ** -9, 3 * 2.0 ** -9, 2.5 * 2.0 ** -9,
                              -(2.0 ** -11), -7 * 2.0 ** -9])
    x[1, 32] = 2.0 ** -130                                       # E clamps to -127: the element is 2^-3
    x[1, 64] = -1.75 * 2.0 ** 100                                # E = 92, -448
    x[1, 96], x[1, 97] = 511.0, 2.0                              # 511 > 448 bumps E to 1; 255.5 -> 256
    codes = {(0, 32): 0x7E, (0, 33): 0xB8, (0, 64): 0x76, (0, 65): 0x38, (0, 96): 0x78, (0, 97): 0x58, (0, 98): 0x5A,
             (0, 99): 0xD9, (1, 0): 0x78, (1, 1): 0, (1, 2): 2, (1, 3): 1, (1, 4): 3, (1, 5): 2, (1, 6): 0, (1, 7): 0x87,
             (1, 32): 0x20, (1, 64): 0xFE, (1, 96): 0x78, (1, 97): 0x38}
    return x, torch.tensor([[0, 130, 131, 127], [127, 0, 219, 128]], dtype=torch.uint8), codes


def randn_x(M, K, seed):
    """randn rows whose groups of 32 carry their own power of two, 2^-12 .. 2^12"""
    g = torch.Generator().manual_seed(9700 + seed)
    e = torch.randint(-12, 13, (M, K // 32, 1), generator=g).float()
    return (torch.randn(M, K // 32, 32, generator=g) * torch.exp2(e)).reshape(M, K)


def xhat(Q, x):
    """float64 [M, K] value of the MXFP8 rows of x, by ops.quant's tensor code on the CPU"""
    return Q.dequantize_mx8_rows(Q.quantize_mx8_rows(x.cpu()), x.shape[1]).double()


# the 254 finite e4m3 bytes in ascending order of value: -448 .. -2^-9, -0, 0, 2^-9 .. 448
E4M3_ORDER = list(range(0xFE, 0x7F, -1)) + list(range(0x00, 0x7F))


def all_codes_case(M=24, N=48, K=384):
    """Hand-built bytes with an exact product.  x: slot s = (row, group) holds at position p the byte
    E4M3_ORDER[s + p - 31] (0 outside), so every finite byte stands at every position of a group and a slot's bytes
    are neighbours in value; its scale byte brings them to [2^3, 2^5).  w: every e2m1 code in both nibbles of every
    byte position, scale bytes 126 .. 128.  Products are multiples of 2^-10 whose magnitudes sum below 2^24 units."""
    G = K // 32
    s = torch.arange(M * G).view(M, G, 1)
    idx = s + torch.arange(32).view(1, 1, 32) - 31
    order = torch.tensor(E4M3_ORDER, dtype=torch.uint8)
    code = torch.where((idx >= 0) & (idx < 254), order[idx.clamp(0, 253)], torch.zeros((), dtype=torch.uint8))
    val = code.view(FP8).double()
    sbyte = (127 + 3 - (torch.frexp(val.abs().amax(dim=2))[1] - 1) + s[:, :, 0] % 2).to(torch.uint8)
    rows = torch.zeros(M, (K + G + 15) // 16 * 16, dtype=torch.uint8)
    rows[:, :K], rows[:, K: K + G] = code.view(M, K), sbyte
    X = (val * MX.E8M0[sbyte.long()][:, :, None]).view(M, K)
    i = torch.arange(N * K // 2).view(N, K // 2)
    q4 = (((i + i // 64) % 16) | (((3 * i + 5 + i // 64) % 16) << 4)).to(torch.uint8)
    scale = (126 + (torch.arange(G)[None, :] * 2 + torch.arange(N)[:, None]) % 3).to(torch.uint8)
    W = MX.what(q4, scale)
    assert all((code == b).any(dim=0).any(dim=0).all() for b in E4M3_ORDER)
    assert torch.equal((X * 2 ** 8).round(), X * 2 ** 8) and float((X.abs() @ W.abs().t()).max()) * 2 ** 10 < 2 ** 24
    return NS(xq=rows.view(FP8), q4=q4, scale=scale, want=(X @ W.t()).to(BF16))
