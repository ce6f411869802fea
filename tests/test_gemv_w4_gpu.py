"""The 4-bit instantiation of the skinny-M kernel (csrc/kernels/gemv_skinny.hip) through
ops.linear_skinny_w4 / linear_w4 / dequant_w4 against the float64 reference of gemv_w4_refs.py.

Layout of every call, as in test_gemv_skinny_gpu.py: x, y and the residual are column slices of
wider buffers (row stride != width), NaN guard rows follow row M - 1 of x and of the residual,
the bias is cut from a longer NaN-filled vector, the [K / 128, N] scales and the [N, K / 2]
weights from longer NaN / 0xFF-filled buffers, and a sentinel surrounds y and must survive.

Bounds.  One-rounding epilogues: err <= 1.0 in the metric of gemm_refs.py, hard (an f32 sum
rounded once to bf16).  GELU and the dequantising route of linear_w4: gemv_w4_refs.BOUND, 2 x
the largest error measured on an MI355X over this file.  Every case prints its MEASURE line.

Besides the metric: the exact-input case must be right bit for bit (gemv_w4_refs.py), two
calls are bitwise equal, row m of an M = 16 call equals the M = 1 call on that row, and a
captured call replays to the same bits."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_refs as GR
import gemv_w4_refs as W4

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
    R, C = t.shape
    buf = torch.full((R + GUARD, C + 2 * pad), fill, device=DEV, dtype=BF16)
    buf[:R, pad: pad + C] = t.to(DEV)
    return buf[:R, pad: pad + C], buf


def _cut(t, fill):
    """a contiguous tensor cut from a longer flat buffer of ``fill`` (64 bytes on either side)"""
    n = 64 // t.element_size()
    buf = torch.full((t.numel() + 2 * n,), fill, device=DEV, dtype=t.dtype)
    buf[n: n + t.numel()] = t.reshape(-1).to(DEV)
    return buf[n: n + t.numel()].view(t.shape)


def _call(c, epi, force_split=0, fn="skinny", M=None, xpad=PAD):
    """one kernel call in the guarded layout -> y [M, N] on the CPU"""
    M = c.x.shape[0] if M is None else M
    N = c.q4.shape[0]
    x, _ = _slice(c.x[:M], float("nan"), xpad)
    r, _ = _slice(c.r[:M], float("nan"))
    y, ybuf = _slice(torch.full((M, N), 7.0), 7.0)
    kw = dict(bias=_cut(c.bias, float("nan")) if "bias" in epi else None,
              act="gelu_tanh" if epi == "bias_gelu" else "none", residual=r if "res" in epi else None, out=y)
    q4, scale = _cut(c.q4, 0xFF), _cut(c.scale, float("nan"))
    if fn == "w4":
        ops.linear_w4(x, q4, scale, **kw)
    else:
        ops.linear_skinny_w4(x, q4, scale, force_split=force_split, **kw)
    torch.cuda.synchronize()
    sent = ybuf.clone()
    sent[:M, PAD: PAD + N] = 7.0
    assert bool((sent == 7.0).all()), "a write outside y[:M, :N]"
    return y.cpu()


_CASES = {}


def _case(kind, N, K, seed=0):
    """16-row inputs and, per epilogue, their reference: made once and shared by every M,
    split and test (row m of the reference does not depend on M either)"""
    key = (kind, N, K, seed)
    if key not in _CASES:
        c = W4.exact_case(16, N, K, seed) if kind == "exact" else \
            W4.randn_case(16, N, K, seed, xmax=128.0 if kind == "big" else None)
        c.refs = {}
        _CASES[key] = c
    return _CASES[key]


def _ref(c, epi):
    if epi not in c.refs:
        c.refs[epi] = W4.w4_ref(c.x, c.q4, c.scale, epi, c.bias, c.r)
    return c.refs[epi]


def _measure(got, ref, M, epi, cls, what):
    sub = GR.NS(out=ref.out[:M], A_out=ref.A_out[:M])
    err, bad, ok = W4.check(got, sub, epi, cls)
    print(f"MEASURE {cls}.{'out' if epi in GR.ONE_ROUNDING else 'act'} {err:.4g} {what}")
    assert bool(torch.isfinite(got.float()).all()), "a guard row or a padded entry reached the output"
    assert bad == 0 and ok, f"{what}: err {err:.4g}, {bad} bad elements"
    return err


@pytest.mark.parametrize("N,K", W4.SHAPES)
@pytest.mark.parametrize("force_split", W4.SPLITS)
@pytest.mark.parametrize("M", W4.MS)
@pytest.mark.parametrize("epi", W4.EPIS)
def test_w4_matches_reference(epi, M, force_split, N, K):
    what = f"int4g128 {epi} M{M} N{N} K{K} split{force_split}"
    c = _case("randn", N, K)
    _measure(_call(c, epi, force_split, M=M), _ref(c, epi), M, epi, "skinny", what)
    # exact inputs: bit for bit
    e = _case("exact", N, K)
    gote = _call(e, epi, force_split, M=M)
    wrong, safe = W4.check_exact(gote, e.v[epi][:M], epi)
    assert wrong == 0, f"{what}: {wrong} of {safe} exact-input elements differ"


@pytest.mark.parametrize("epi", ["none", "bias_gelu", "bias_res"])
def test_w4_large_x(epi):
    """|x| up to 2^7"""
    N, K = 264, 2176
    c = _case("big", N, K, seed=1)
    assert float(c.x.float().abs().max()) == 128.0
    for M in (1, 16):
        _measure(_call(c, epi, M=M), _ref(c, epi), M, epi, "skinny", f"int4g128 {epi} M{M} N{N} K{K} xmax128")


@pytest.mark.parametrize("xpad", [3, 4])
def test_w4_unaligned_x(xpad):
    """x rows that are not 16-byte aligned (an odd column offset, a row stride of K + 6) take
    the kernel's scalar x loads: the same bits as the aligned call"""
    for N, K in ((40, 384), (264, 2176)):
        c = _case("randn", N, K)
        for M in (1, 5, 16):
            a, b = _call(c, "bias_res", M=M, xpad=xpad), _call(c, "bias_res", M=M)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("N", [6, 37])
def test_w4_n_not_a_multiple_of_4(N):
    """the scales of a lane's four rows are then loaded one by one"""
    K = 384
    c = W4.randn_case(16, N, K, seed=N)
    ref = W4.w4_ref(c.x, c.q4, c.scale, "bias_res", c.bias, c.r)
    for fs in W4.SPLITS:
        _measure(_call(c, "bias_res", fs), ref, 16, "bias_res", "skinny", f"int4g128 bias_res M16 N{N} K{K} split{fs}")


@pytest.mark.parametrize("N,K", W4.SHAPES)
def test_w4_repeatable_and_row_independent(N, K):
    c = _case("randn", N, K)
    for epi in ("bias_gelu", "bias_res"):
        for fs in W4.SPLITS:
            full = _call(c, epi, fs)
            assert torch.equal(full.view(torch.int16), _call(c, epi, fs).view(torch.int16)), "two calls differ"
            for m in (0, 7, 15):
                one = GR.NS(x=c.x[m: m + 1], r=c.r[m: m + 1], q4=c.q4, scale=c.scale, bias=c.bias)
                row = _call(one, epi, fs)
                assert torch.equal(row.view(torch.int16), full[m: m + 1].view(torch.int16)), \
                    f"row {m} of the M = 16 call differs from the M = 1 call ({epi} split{fs})"
            five = _call(c, epi, fs, M=5)
            assert torch.equal(five.view(torch.int16), full[:5].view(torch.int16))


@pytest.mark.parametrize("epi", W4.EPIS)
@pytest.mark.parametrize("M", W4.DEQUANT_MS)
def test_linear_w4_dequantising_route(M, epi):
    N, K = W4.DEQUANT_SHAPE
    assert M > ops.W8_SKINNY_MAX_M
    g = W4.randn_case(16, N, K, seed=M)
    big = W4.randn_case(M, N, K, seed=M)
    ref = W4.w4_ref(big.x, big.q4, big.scale, epi, big.bias, big.r)
    _measure(_call(big, epi, fn="w4"), ref, M, epi, "w4_dequant", f"linear_w4 {epi} M{M} N{N} K{K}")
    # at 16 rows and fewer linear_w4 is the skinny kernel itself
    a, b = _call(g, epi, fn="w4"), _call(g, epi)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("N,K", [(40, 384), (264, 2176), (5, 128)])
def test_dequant_w4_exact(N, K):
    c = W4.randn_case(1, N, K, seed=3)
    c.q4[0, 0] = 0x0F                           # nibble 0 = -8, which the quantiser never writes
    out = torch.full((N + 1, K), 7.0, device=DEV, dtype=BF16)
    ops.dequant_w4(_cut(c.q4, 0xFF), _cut(c.scale, float("nan")), out[:N])
    want = W4.what(c.q4, c.scale).float().to(BF16)       # q * scale is exact in f64 and rounds once
    assert float(W4.what(c.q4, c.scale)[0, 1]) == -8.0 * float(c.scale[0, 0])
    assert torch.equal(out[:N].cpu().view(torch.int16), want.view(torch.int16))
    assert bool((out[N] == 7.0).all())


def test_w4_nibble_0_is_minus_8():
    """hand-built bytes through the kernel: all 16 nibble values, decoded as nibble - 8"""
    N, K = 16, 128
    q4 = ((torch.arange(N * K // 2) * 7 + 3) % 256).to(torch.uint8).view(N, K // 2)
    q4[0, :8] = torch.tensor([0x00, 0x0F, 0xF0, 0x10, 0x01, 0x80, 0x08, 0xFF], dtype=torch.uint8)
    scale = (2.0 ** -(torch.arange(N) % 3).float())[None, :].contiguous()
    x = torch.randint(-2, 3, (4, K), generator=torch.Generator().manual_seed(5)).to(BF16)
    want = (x.double() @ W4.what(q4, scale).t()).to(BF16)             # exact in f32: small integers, power-of-two scales
    got = ops.linear_skinny_w4(x.to(DEV), q4.to(DEV), scale.to(DEV)).cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_w4_graph_capture():
    N, K = 264, 2176
    c = _case("randn", N, K)
    x, q4, scale = c.x[:8].to(DEV), c.q4.to(DEV), c.scale.to(DEV)
    bias, r = c.bias.to(DEV), c.r[:8].to(DEV)
    y = torch.empty(8, N, device=DEV, dtype=BF16)
    want = ops.linear_skinny_w4(x, q4, scale, bias, residual=r).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.linear_skinny_w4(x, q4, scale, bias, residual=r, out=y)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.linear_skinny_w4(x, q4, scale, bias, residual=r, out=y)
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))
    x.copy_(c.x[8:16].to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), ops.linear_skinny_w4(x, q4, scale, bias, residual=r).view(torch.int16))


def test_w4_rejects_unsupported_calls():
    c = _case("randn", 40, 384)
    x, q4, s = c.x.to(DEV), c.q4.to(DEV), c.scale.to(DEV)
    with pytest.raises(ValueError):
        ops.linear_skinny_w4(torch.cat([x, x[:1]]), q4, s)
    with pytest.raises(ValueError):
        ops.linear_skinny_w4(x[:, :320].contiguous(), q4[:, :160].contiguous(), s)
    with pytest.raises(RuntimeError):
        ops.linear_skinny_w4(x, q4, s, force_split=17)
