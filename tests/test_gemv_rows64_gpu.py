"""The 64-row weight-streaming kernel (csrc/kernels/gemv_rows64.hip) through
ops.quant.linear_skinny64 and ``Generator(skinny64=True)``.

* Against the float64 references of gemv_w8_refs.py / gemv_w4_refs.py in the guarded layout of
  test_gemv_skinny_gpu.py (strided slices, NaN guard rows behind row M - 1, a sentinel around
  y), with those modules' bounds for this arithmetic: 1.0 for an f32 sum rounded once, and
  ``BOUND["skinny.act"]`` behind GELU.
* Exactly: rows [16 t, 16 t + 16) of an M-row result are bit for bit the 16-row kernel's on
  those rows -- the K-chains of the plan are the same -- and two calls are bitwise equal.
* A quantised generator with ``skinny64=True``: a 48-row prefill keeps the ``e_q <= 2 e_b``
  margin of test_generate_w8_gpu.py and allocates no dequantisation scratch, a graph-replayed
  batch of 24 gives the eager tokens, 20 rows of a linear layer equal their one-row calls."""
import math

import pytest
import torch

import mipipe
from mipipe import ops

import gemm_refs as GR
import gemv_w4_refs as W4
import gemv_w8_refs as WR
from test_gemv_skinny_gpu import DEV, PAD, _slice, _vec
from test_generate_w8_cpu import _cfg, dense_oracle
from test_generate_w8_gpu import _incremental

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
# (40, *): a ragged N and an odd step count.  (264, *): a ragged last K-step (2080 = 16 x 128 + 32)
# and 17 steps that no split divides.  (16402, 384): 32 weight rows per workgroup (G = 2: two
# M-tiles per pass, a partial last pass at M = 33, the register x path of int4g128), a ragged
# last workgroup and, with N % 4 != 0, the scalar group-scale loads.  (32770, 128): the skinny
# plan groups 64 weight rows there and this kernel 32 -- the bits must not depend on that
SHAPES = {"int8": ((40, 96), (264, 2080), (16402, 384), (32770, 128)), "bf16": ((40, 96), (264, 2080), (16402, 384)),
          "int4g128": ((40, 384), (264, 2176), (16402, 384), (32770, 128))}
CASES = [(wt, N, K) for wt, shapes in SHAPES.items() for N, K in shapes]
MS = (17, 32, 33, 64)
EPIS = ("none", "bias_gelu", "bias_res")


def _splits(N):
    """force_split: none, one that does not divide, the plan's; and the most waves of the
    grouping, whose LDS (69632 bytes) is above the default limit of a launch"""
    return (1, 3, 0) + ((16,) if N == 264 else (8,) if N > 16384 else ())


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"
    assert [ops.gemv_plan(N, 128, 1)[0] for N in (264, 16402, 32770)] == [16, 32, 64]


_CASES = {}


def _case(wt, N, K):
    """64-row inputs, their operands on the device and the float64 reference per epilogue
    (row m of it does not depend on M): made once, shared by every M"""
    if (wt, N, K) not in _CASES:
        c = (W4 if wt == "int4g128" else WR).randn_case(64, N, K)
        c.w_dev = (c.q4 if wt == "int4g128" else c.q if wt == "int8" else c.w).to(DEV)
        c.s_dev = None if wt == "bf16" else c.scale.to(DEV) if wt == "int4g128" else _vec(c.scale, torch.float32)
        c.refs = {epi: W4.w4_ref(c.x, c.q4, c.scale, epi, c.bias, c.r) if wt == "int4g128" else
                  WR.w8_ref(c.x, c.q, c.scale, epi, c.bias, c.r) if wt == "int8" else
                  WR.bf16_ref(c.x, c.w, epi, c.bias, c.r) for epi in EPIS}
        _CASES[(wt, N, K)] = c
    return _CASES[(wt, N, K)]


def _call(fn, c, epi, fs, lo, hi):
    """fn on x rows [lo, hi) in the guarded layout -> y on the CPU"""
    M, N = hi - lo, c.w_dev.shape[0]
    x, _ = _slice(c.x[lo:hi], float("nan"))
    r, _ = _slice(c.r[lo:hi], float("nan"))
    y, ybuf = _slice(torch.full((M, N), 7.0), 7.0)
    fn(x, c.w_dev, c.s_dev, bias=_vec(c.bias, BF16) if "bias" in epi else None,
       act="gelu_tanh" if epi == "bias_gelu" else "none", residual=r if "res" in epi else None, out=y, force_split=fs)
    torch.cuda.synchronize()
    sent = ybuf.clone()
    sent[:M, PAD: PAD + N] = 7.0
    assert bool((sent == 7.0).all()), "a write outside y[:M, :N]"
    return y.cpu()


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("wt,N,K", CASES)
def test_rows64(wt, N, K, M, epi):
    """One call per split (they differ in the reduction only, so they share a test id): within
    the bound of the float64 reference, repeatable, and rows [16 t, 16 t + 16) bit for bit
    what the 16-row kernel gives for those rows."""
    c = _case(wt, N, K)
    sub = GR.NS(out=c.refs[epi].out[:M], A_out=c.refs[epi].A_out[:M])
    skinny = ops.linear_skinny_w4 if wt == "int4g128" else ops.linear_skinny
    for fs in _splits(N):
        got = _call(ops.quant.linear_skinny64, c, epi, fs, 0, M)
        err, bad, ok = (W4 if wt == "int4g128" else WR).check(got, sub, epi, "skinny")
        print(f"MEASURE rows64 {wt} {epi} M{M} N{N} K{K} split{fs} err {err:.4g}")
        assert bool(torch.isfinite(got.float()).all()), f"split{fs}: a guard row or a padded entry reached y"
        assert bad == 0 and ok, f"split{fs}: err {err:.4g}, {bad} bad elements"
        again = _call(ops.quant.linear_skinny64, c, epi, fs, 0, M)
        assert torch.equal(got.view(torch.int16), again.view(torch.int16)), f"split{fs}: two calls differ"
        for lo in range(0, M, 16):
            want = _call(skinny, c, epi, fs, lo, min(lo + 16, M))
            assert torch.equal(got[lo: lo + 16].view(torch.int16), want.view(torch.int16)), f"split{fs}: rows from {lo}"


@pytest.mark.parametrize("fmt", ["int8", "int4g128"])
@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generator_skinny64(family, fmt):
    cfg, dev = _cfg(family), torch.device("cuda", 0)
    q = mipipe.Generator(cfg, dev, dtype=BF16, seed=4, weights=fmt, skinny64=True)
    oracle, base = dense_oracle(q), dense_oracle(q, dev, BF16)
    tokens = torch.randint(0, cfg.vocab_size, (2, 24 + 8), generator=torch.Generator().manual_seed(5))
    want = _incremental(oracle, tokens, 24)                  # a 48-row prefill, then 2-row steps
    e_b = float((_incremental(base, tokens, 24) - want).abs().max())
    e_q = float((_incremental(q, tokens, 24) - want).abs().max())
    print(f"\n[{family} {fmt}] e_bf16 = {e_b:.6f}  e_skinny64 = {e_q:.6f}  bound = {2 * e_b:.6f}")
    assert math.isfinite(e_q) and e_b > 0 and e_q <= 2 * e_b, (e_q, e_b)
    assert q._scratch is None, "a layer of at most 64 rows took the dequantising route"
    x = torch.randn(20, cfg.d_model, device=dev, dtype=BF16)
    many = q._linear(x, "layers.0.attn.wqkv.weight")
    assert torch.equal(torch.cat([q._linear(x[m: m + 1], "layers.0.attn.wqkv.weight") for m in range(20)]), many)
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, cfg.vocab_size, (1 + i % 2,), generator=g) for i in range(24)]
    eager, le = q.generate_batch(prompts, 8, graphs=False)
    replay, lr = q.generate_batch(prompts, 8, graphs=True)
    assert torch.equal(eager, replay) and torch.equal(le, lr)
    assert q._scratch is None        # the ragged prefill is 48 rows and every step 24
