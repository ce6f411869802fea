"""gemv_mx4_kernel / dequant_mx4_kernel (csrc/kernels/gemv_skinny.hip) through ops.quant.linear_skinny_mx4 /
linear_mx4 / dequant_mx4 against the float64 reference of gemv_mx4_refs.py.

Layout of every call, as in test_gemv_w4_gpu.py: x, y and the residual are column slices of wider
buffers with NaN guard rows, the bias is cut from a NaN-filled vector, q4 and the scale bytes from
0xFF-filled buffers (a scale byte read out of bounds is a NaN scale), and a sentinel surrounds y.

Bounds.  One-rounding epilogues: err <= 1.0 in the metric of gemm_refs.py, hard.  GELU and the
dequantising route of linear_mx4: gemv_mx4_refs.BOUND, 2 x the largest error measured on an MI355X over
this file.  Every case prints its MEASURE line.  Exact inputs must be right bit for bit."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_refs as GR
import gemv_mx4_refs as MX
from gemv_w4_refs import check, check_exact
from test_gemv_w4_gpu import BF16, DEV, PAD, _slice, setup_module  # noqa: F401  (the guarded slices of that file)

pytestmark = pytest.mark.gpu

Q = ops.quant


def _cut(t, fill, off=64):
    """a contiguous tensor cut from a longer flat buffer of ``fill``, ``off`` bytes into it"""
    n = off // t.element_size()
    buf = torch.full((t.numel() + 2 * 64,), fill, device=DEV, dtype=t.dtype)
    buf[n: n + t.numel()] = t.reshape(-1).to(DEV)
    return buf[n: n + t.numel()].view(t.shape)


def _call(c, epi, force_split=0, fn="skinny", M=None, xpad=PAD, soff=64):
    """one kernel call in the guarded layout -> y [M, N] on the CPU"""
    M = c.x.shape[0] if M is None else M
    N = c.q4.shape[0]
    x, _ = _slice(c.x[:M], float("nan"), xpad)
    r, _ = _slice(c.r[:M], float("nan"))
    y, ybuf = _slice(torch.full((M, N), 7.0), 7.0)
    kw = dict(bias=_cut(c.bias, float("nan")) if "bias" in epi else None,
              act="gelu_tanh" if epi == "bias_gelu" else "none", residual=r if "res" in epi else None, out=y)
    q4, scale = _cut(c.q4, 0xFF), _cut(c.scale, 0xFF, soff)
    if fn == "any_m":
        Q.linear_mx4(x, q4, scale, **kw)
    else:
        Q.linear_skinny_mx4(x, q4, scale, force_split=force_split, **kw)
    torch.cuda.synchronize()
    sent = ybuf.clone()
    sent[:M, PAD: PAD + N] = 7.0
    assert bool((sent == 7.0).all()), "a write outside y[:M, :N]"
    return y.cpu()


_CASES = {}


def _case(kind, N, K, M=16, seed=0):
    """inputs and, per epilogue, their reference: made once and shared by every M, split and test"""
    key = (kind, N, K, M, seed)
    if key not in _CASES:
        _CASES[key] = (MX.exact_case if kind == "exact" else MX.randn_case)(M, N, K, seed)
        _CASES[key].refs = {}
    return _CASES[key]


def _measure(c, got, M, epi, cls, what):
    if epi not in c.refs:
        c.refs[epi] = MX.mx4_ref(c.x, c.q4, c.scale, epi, c.bias, c.r)
    ref = GR.NS(out=c.refs[epi].out[:M], A_out=c.refs[epi].A_out[:M])
    err, bad, ok = check(got, ref, epi, cls, bound=MX.BOUND)
    print(f"MEASURE {cls}.{'out' if epi in GR.ONE_ROUNDING else 'act'} {err:.4g} {what}")
    assert bool(torch.isfinite(got.float()).all()), "a guard row, a padded entry or a scale byte out of bounds reached y"
    assert bad == 0 and ok, f"{what}: err {err:.4g}, {bad} bad elements"


@pytest.mark.parametrize("N,K", MX.SHAPES)
def test_mx4_matches_reference(N, K):
    """every epilogue, M and force_split of gemv_w8_refs on one shape: the metric on random inputs, the
    bits on exact ones"""
    c, e = _case("randn", N, K), _case("exact", N, K)
    for epi in MX.EPIS:
        for M in MX.MS:
            for fs in MX.SPLITS:
                what = f"mxfp4 {epi} M{M} N{N} K{K} split{fs}"
                _measure(c, _call(c, epi, fs, M=M), M, epi, "skinny", what)
                wrong, safe = check_exact(_call(e, epi, fs, M=M), e.v[epi][:M], epi)
                assert wrong == 0, f"{what}: {wrong} of {safe} exact-input elements differ"


@pytest.mark.parametrize("M", MX.DEQUANT_MS)
def test_linear_mx4_dequantising_route(M):
    N, K = MX.DEQUANT_SHAPE
    assert M > ops.W8_SKINNY_MAX_M
    big = _case("randn", N, K, M=M, seed=M)
    for epi in MX.EPIS:
        _measure(big, _call(big, epi, fn="any_m"), M, epi, "mx4_dequant", f"linear_mx4 {epi} M{M} N{N} K{K}")
        # at 16 rows and fewer linear_mx4 is the skinny kernel itself
        assert torch.equal(_call(big, epi, fn="any_m", M=16).view(torch.int16), _call(big, epi, M=16).view(torch.int16))


def test_mx4_all_codes_and_scales():
    """hand-built bytes: every code in both nibbles of every byte position, scale bytes that differ per
    group and row, small-integer x.  Exact in f32, so equal to the float64 product bit for bit: decides
    which nibble `sel` picks and how the instruction reads its scale operand."""
    N, K = 16, 256
    i = torch.arange(N * K // 2).view(N, K // 2)
    q4 = (((i + i // 64) % 16) | (((3 * i + 5 + i // 64) % 16) << 4)).to(torch.uint8)
    q4[0, :8] = torch.tensor([0x08, 0x80, 0x88, 0x0F, 0xF0, 0x7F, 0xF7, 0x18], dtype=torch.uint8)
    scale = (122 + (torch.arange(K // 32)[None, :] * 3 + torch.arange(N)[:, None]) % 11).to(torch.uint8)
    x = torch.randint(-2, 3, (5, K), generator=torch.Generator().manual_seed(5)).to(BF16)
    W = MX.what(q4, scale)
    assert float(W[0, 0]) == 0.0 and float(W[0, 3]) == 0.0 and sorted(set(MX.unpack(q4).flatten().tolist())) == \
        sorted(set(MX.MAGS.tolist()))
    want = (x.double() @ W.t()).to(BF16)
    for fs in MX.SPLITS:
        got = Q.linear_skinny_mx4(x.to(DEV), q4.to(DEV), scale.to(DEV), force_split=fs).cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("N,K", MX.SHAPES[2:])
def test_mx4_repeatable_row_independent_and_alignment_free(N, K):
    c = _case("randn", N, K)
    for epi in ("bias_gelu", "bias_res"):
        for fs in MX.SPLITS:
            full = _call(c, epi, fs)
            same = lambda got, want: torch.equal(got.view(torch.int16), want.view(torch.int16))  # noqa: E731
            assert same(_call(c, epi, fs), full), "two calls differ"
            for m in (0, 7, 15):
                one = GR.NS(x=c.x[m: m + 1], r=c.r[m: m + 1], q4=c.q4, scale=c.scale, bias=c.bias)
                assert same(_call(one, epi, fs), full[m: m + 1]), f"row {m} of the M = 16 call differs from the M = 1 call"
            assert same(_call(c, epi, fs, M=5), full[:5])
            # x rows at an odd column offset (scalar x loads) and a scale table at odd addresses (byte loads)
            for M in (1, 5, 16):
                assert same(_call(c, epi, fs, M=M, xpad=3), full[:M]), "unaligned x rows change the bits"
            for soff in (61, 62):
                assert same(_call(c, epi, fs, soff=soff), full), "an unaligned scale pointer changes the bits"


@pytest.mark.parametrize("N,K", [(40, 384), (264, 2176), (5, 128)])
def test_dequant_mx4_exact(N, K):
    c = MX.randn_case(1, N, K, seed=3)
    c.q4[0, 0] = 0x98                           # code 8 = -0, which the quantiser never writes, reads as 0
    out = torch.full((N + 1, K), 7.0, device=DEV, dtype=BF16)
    Q.dequant_mx4(_cut(c.q4, 0xFF), _cut(c.scale, 0xFF, 61), out[:N])
    W = MX.what(c.q4, c.scale)
    assert float(W[0, 0]) == 0.0 and torch.equal(W.to(BF16).double(), W)      # What is a bf16 value: nothing rounds
    assert torch.equal(out[:N].cpu().double(), W)
    assert bool((out[N] == 7.0).all())


def test_mx4_graph_capture():
    N, K = 264, 2176
    c = _case("randn", N, K)
    x, q4, scale = c.x[:8].to(DEV), c.q4.to(DEV), c.scale.to(DEV)
    bias, r = c.bias.to(DEV), c.r[:8].to(DEV)
    y = torch.empty(8, N, device=DEV, dtype=BF16)
    want = Q.linear_skinny_mx4(x, q4, scale, bias, residual=r).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Q.linear_skinny_mx4(x, q4, scale, bias, residual=r, out=y)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Q.linear_skinny_mx4(x, q4, scale, bias, residual=r, out=y)
    for rows in (c.x[:8], c.x[8:16], c.x[:8]):
        x.copy_(rows.to(DEV))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), Q.linear_skinny_mx4(x, q4, scale, bias, residual=r).view(torch.int16))
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


def test_mx4_rejects_unsupported_calls():
    c = _case("randn", 40, 384)
    x, q4, s = c.x.to(DEV), c.q4.to(DEV), c.scale.to(DEV)
    with pytest.raises(ValueError):
        Q.linear_skinny_mx4(torch.cat([x, x[:1]]), q4, s)
    with pytest.raises(ValueError):
        Q.linear_skinny_mx4(x[:, :320].contiguous(), q4[:, :160].contiguous(), s[:, :10].contiguous())
    with pytest.raises(RuntimeError):
        Q.linear_skinny_mx4(x, q4, s, force_split=17)
    with pytest.raises(RuntimeError):           # the binding itself: no 64-row kernel for this format
        ops.load_ext().gemv_skinny(torch.cat([x, x[:1]]), q4, s, torch.empty(17, 40, device=DEV, dtype=BF16), None, None)
