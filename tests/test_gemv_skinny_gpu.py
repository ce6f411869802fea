"""The skinny-M kernel (csrc/kernels/gemv_skinny.hip) through ops.linear_skinny / linear_w8 /
dequant_w8 against the float64 reference of gemv_w8_refs.py.

Layout of every call: x, y and the residual are column slices of wider buffers (row stride !=
width), NaN guard rows follow row M - 1 of x and of the residual, bias and scale are cut from
longer NaN-filled vectors, and a sentinel surrounds y (columns on both sides, rows below) and
must survive.  ``q`` holds +-127 and a zero-scale row (gemv_w8_refs.randn_case).

Bounds.  One-rounding epilogues: err <= 1.0 in the metric of gemm_refs.py, hard (an f32 sum
rounded once to bf16 cannot exceed it; the largest measured is 0.44).  GELU and the
dequantising route of linear_w8: gemv_w8_refs.BOUND, 2 x the largest error measured on an
MI355X over two runs of this file (both runs gave the same figures: the kernel is
deterministic and so are the inputs).  GELU measures 0.6163, at the smallest shape (N = 16,
K = 32), against 0.46-0.52 of the existing engines on their shapes: the reference allows the
half-ulp step of the rounded pre-activation through the largest derivative, and with K = 32
the summed magnitude A is small next to |ref|, so the two roundings (pre-activation, output)
weigh more.  The dequantising route measures 0.4981 (one rounding) and 0.4201 (GELU): the
bf16 rounding of q * scale is part of it.  Every case prints its MEASURE line.

Besides the metric: the exact-input case must be right bit for bit (see gemv_w8_refs.py),
two calls are bitwise equal, and row m of an M = 16 call equals the M = 1 call on that row."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_refs as GR
import gemv_w8_refs as WR

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
PAD = 8            # columns (16 bytes) on each side of a slice
GUARD = 3          # guard rows


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _slice(t, fill, pad=PAD):
    """t [R, C] -> the same values as a column slice of a wider buffer with GUARD rows of
    ``fill`` below and ``pad`` columns of it on both sides; returns (view, buffer)"""
    R, C = t.shape
    buf = torch.full((R + GUARD, C + 2 * pad), fill, device=DEV, dtype=BF16)
    buf[:R, pad: pad + C] = t.to(DEV)
    return buf[:R, pad: pad + C], buf


def _vec(t, dtype):
    """a vector cut from a longer NaN-filled one"""
    buf = torch.full((t.numel() + 16,), float("nan"), device=DEV, dtype=dtype)
    buf[8: 8 + t.numel()] = t.to(DEV)
    return buf[8: 8 + t.numel()]


def _call(c, wt, epi, force_split=0, fn="skinny", M=None, xpad=PAD):
    """one kernel call in the guarded layout -> y [M, N] on the CPU"""
    M = c.x.shape[0] if M is None else M
    N = c.q.shape[0]
    x, _ = _slice(c.x[:M], float("nan"), xpad)
    r, _ = _slice(c.r[:M], float("nan"))
    y, ybuf = _slice(torch.full((M, N), 7.0), 7.0)
    kw = dict(bias=_vec(c.bias, BF16) if "bias" in epi else None, act="gelu_tanh" if epi == "bias_gelu" else "none",
              residual=r if "res" in epi else None, out=y)
    if fn == "w8":
        ops.linear_w8(x, c.q.to(DEV), _vec(c.scale, torch.float32), **kw)
    elif wt == "int8":
        ops.linear_skinny(x, c.q.to(DEV), _vec(c.scale, torch.float32), force_split=force_split, **kw)
    else:
        ops.linear_skinny(x, c.w.to(DEV), None, force_split=force_split, **kw)
    torch.cuda.synchronize()
    sent = ybuf.clone()
    sent[:M, PAD: PAD + N] = 7.0
    assert bool((sent == 7.0).all()), "a write outside y[:M, :N]"
    return y.cpu()


_CASES = {}


def _case(kind, N, K, seed=0):
    """16-row inputs and, per (epi, weight type), their reference: made once and shared by
    every M, split and test (row m of the reference does not depend on M either)"""
    key = (kind, N, K, seed)
    if key not in _CASES:
        c = WR.exact_case(16, N, K, seed) if kind == "exact" else \
            WR.randn_case(16, N, K, seed, xmax=128.0 if kind == "big" else None)
        c.refs = {}
        _CASES[key] = c
    return _CASES[key]


def _ref(c, wt, epi):
    if (wt, epi) not in c.refs:
        c.refs[(wt, epi)] = WR.w8_ref(c.x, c.q, c.scale, epi, c.bias, c.r) if wt == "int8" else \
            WR.bf16_ref(c.x, c.w, epi, c.bias, c.r)
    return c.refs[(wt, epi)]


def _measure(got, ref, M, epi, cls, what):
    sub = GR.NS(out=ref.out[:M], A_out=ref.A_out[:M])
    err, bad, ok = WR.check(got, sub, epi, cls)
    print(f"MEASURE {cls}.{'out' if epi in GR.ONE_ROUNDING else 'act'} {err:.4g} {what}")
    assert bool(torch.isfinite(got.float()).all()), "a guard row or a padded entry reached the output"
    assert bad == 0 and ok, f"{what}: err {err:.4g}, {bad} bad elements"
    return err


@pytest.mark.parametrize("N,K", WR.SHAPES)
@pytest.mark.parametrize("force_split", WR.SPLITS)
@pytest.mark.parametrize("M", WR.MS)
@pytest.mark.parametrize("epi", WR.EPIS)
@pytest.mark.parametrize("wt", ["int8", "bf16"])
def test_skinny_matches_reference(wt, epi, M, force_split, N, K):
    what = f"{wt} {epi} M{M} N{N} K{K} split{force_split}"
    c = _case("randn", N, K)
    got = _call(c, wt, epi, force_split, M=M)
    _measure(got, _ref(c, wt, epi), M, epi, "skinny", what)
    if epi != "bias_gelu":
        # the zero-scale row: exactly bias + residual (bf16 weights: a zero row)
        z = min(1, N - 1)
        want = torch.zeros(M, dtype=torch.float64)
        if "bias" in epi:
            want = want + c.bias[z].double()
        if "res" in epi:
            want = want + c.r[:M, z].double()
        assert torch.equal(got[:, z].double(), want.to(BF16).double()), "zero-scale row"
    # exact inputs: bit for bit
    e = _case("exact", N, K)
    gote = _call(e, wt, epi, force_split, M=M)
    wrong, safe = WR.check_exact(gote, e.v[epi][:M], epi)
    assert wrong == 0, f"{what}: {wrong} of {safe} exact-input elements differ"


@pytest.mark.parametrize("epi", ["none", "bias_gelu", "bias_res"])
@pytest.mark.parametrize("wt", ["int8", "bf16"])
def test_skinny_large_x(wt, epi):
    """|x| up to 2^7"""
    N, K = 264, 2080
    c = _case("big", N, K, seed=1)
    assert float(c.x.float().abs().max()) == 128.0
    for M in (1, 16):
        _measure(_call(c, wt, epi, M=M), _ref(c, wt, epi), M, epi, "skinny", f"{wt} {epi} M{M} N{N} K{K} xmax128")


@pytest.mark.parametrize("xpad", [3, 4])
@pytest.mark.parametrize("wt", ["int8", "bf16"])
def test_skinny_unaligned_x(wt, xpad):
    """x rows that are not 16-byte aligned (an odd column offset, a row stride of K + 6) take
    the kernel's scalar x loads: the same bits as the aligned call"""
    for N, K in ((40, 96), (264, 2080)):
        c = _case("randn", N, K)
        for M in (1, 5, 16):
            a, b = _call(c, wt, "bias_res", M=M, xpad=xpad), _call(c, wt, "bias_res", M=M)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("N,K", WR.SHAPES)
@pytest.mark.parametrize("wt", ["int8", "bf16"])
def test_skinny_repeatable_and_row_independent(wt, N, K):
    c = _case("randn", N, K)
    for epi in ("bias_gelu", "bias_res"):
        for fs in WR.SPLITS:
            full = _call(c, wt, epi, fs)
            assert torch.equal(full.view(torch.int16), _call(c, wt, epi, fs).view(torch.int16)), "two calls differ"
            for m in (0, 7, 15):
                one = GR.NS(x=c.x[m: m + 1], r=c.r[m: m + 1], q=c.q, scale=c.scale, bias=c.bias, w=c.w)
                row = _call(one, wt, epi, fs)
                assert torch.equal(row.view(torch.int16), full[m: m + 1].view(torch.int16)), \
                    f"row {m} of the M = 16 call differs from the M = 1 call ({wt} {epi} split{fs})"
            # ... and of the rows that share the call
            five = _call(c, wt, epi, fs, M=5)
            assert torch.equal(five.view(torch.int16), full[:5].view(torch.int16))


@pytest.mark.parametrize("epi", WR.EPIS)
@pytest.mark.parametrize("M", WR.DEQUANT_MS)
def test_linear_w8_dequantising_route(M, epi):
    N, K = WR.DEQUANT_SHAPE
    assert M > ops.W8_SKINNY_MAX_M or M > 16
    g = WR.randn_case(16, N, K, seed=M)
    big = WR.randn_case(M, N, K, seed=M)
    ref = WR.w8_ref(big.x, big.q, big.scale, epi, big.bias, big.r)
    got = _call(big, "int8", epi, fn="w8")
    _measure(got, ref, M, epi, "w8_dequant", f"linear_w8 {epi} M{M} N{N} K{K}")
    # at 16 rows and fewer linear_w8 is the skinny kernel itself
    a, b = _call(g, "int8", epi, fn="w8"), _call(g, "int8", epi)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("N,K", [(40, 96), (264, 2080), (5, 16)])
def test_dequant_w8_exact(N, K):
    c = WR.randn_case(1, N, K, seed=3)
    out = torch.full((N + 1, K), 7.0, device=DEV, dtype=BF16)
    ops.dequant_w8(c.q.to(DEV), c.scale.to(DEV), out[:N])
    want = (c.q.float() * c.scale[:, None]).to(BF16)
    assert torch.equal(out[:N].cpu().view(torch.int16), want.view(torch.int16))
    assert bool((out[N] == 7.0).all())


def test_skinny_rejects_unsupported_calls():
    c = _case("randn", 40, 96)
    x, q, s = c.x.to(DEV), c.q.to(DEV), c.scale.to(DEV)
    with pytest.raises(ValueError):
        ops.linear_skinny(torch.cat([x, x[:1]]), q, s)
    with pytest.raises(ValueError):
        ops.linear_skinny(x[:, :80].contiguous(), q[:, :80].contiguous(), s)
    with pytest.raises(RuntimeError):
        ops.linear_skinny(x, q, s, force_split=17)
