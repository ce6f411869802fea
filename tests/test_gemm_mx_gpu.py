"""mx8_quantize_rows_kernel and gemm_mx_kernel (csrc/kernels/gemm_mx.hip) through ops.quant against the tensor code
and the float64 reference, in the guarded layout of test_gemv_mx4_gpu.py (column slices, NaN guard rows, 0xFF-filled
weight buffers, a sentinel round y).  One-rounding epilogues: err <= 1.0 in the metric of gemm_refs.py, hard; GELU:
gemm_mx_refs.BOUND.  Exact inputs must be right bit for bit."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_mx_refs as R
import gemm_refs as GR
import gemv_mx4_refs as MX
from gemv_w4_refs import check
from test_gemv_mx4_gpu import _cut
from test_gemv_w4_gpu import BF16, DEV, PAD, _slice, setup_module  # noqa: F401  (the guarded slices of that file)

pytestmark = pytest.mark.gpu

Q = ops.quant
_CASES = {}


def _case(N, K):
    """gemv_mx4_refs.randn_case at the largest M, the value of its rows in MXFP8, and per epilogue the reference"""
    if (N, K) not in _CASES:
        c = _CASES[(N, K)] = MX.randn_case(max(R.MS), N, K)
        c.xhat, c.refs = R.xhat(Q, c.x), {}
    return _CASES[(N, K)]


def _ref(c, epi):
    if epi not in c.refs:
        c.refs[epi] = MX.mx4_ref(c.xhat, c.q4, c.scale, epi, c.bias, c.r)
    return c.refs[epi]


def _bits(t):
    return t.view(torch.int16)


def _call(c, epi, M, soff=64, rows=None):
    """one linear_mx4a8 call on rows [:M] (or ``rows``) of a case in the guarded layout -> y on the CPU"""
    rows = slice(0, M) if rows is None else rows
    N = c.q4.shape[0]
    x, _ = _slice(c.x[rows], float("nan"))
    r, _ = _slice(c.r[rows], float("nan"))
    M = x.shape[0]
    y, ybuf = _slice(torch.full((M, N), 7.0), 7.0)
    Q.linear_mx4a8(x, _cut(c.q4, 0xFF), _cut(c.scale, 0xFF, soff), bias=_cut(c.bias, float("nan")) if "bias" in epi else None,
                   act="gelu_tanh" if epi == "bias_gelu" else "none", residual=r if "res" in epi else None, out=y)
    torch.cuda.synchronize()
    sent = ybuf.clone()
    sent[:M, PAD: PAD + N] = 7.0
    assert bool((sent == 7.0).all()), "a write outside y[:M, :N]"
    return y.cpu()


@pytest.mark.parametrize("M", (1, 17, 33))
@pytest.mark.parametrize("K,dt,col", ((128, torch.float32, 8), (384, torch.bfloat16, 8), (128, torch.bfloat16, 3)))
def test_quantiser_kernel_matches_the_tensor_code(M, K, dt, col):
    """col 8: 16-byte aligned rows (vector loads); col 3: an odd element offset (scalar loads)"""
    x = R.randn_x(M, K, seed=M + K)
    x[0, :128] = R.hand_groups()[0][M % 2]
    x = x.to(dt)
    buf = torch.full((M + 3, K + 16), float("nan"), device=DEV, dtype=dt)      # a column slice, NaN guard rows
    buf[:M, col: col + K] = x.to(DEV)
    rb = Q.mx8_row_bytes(K)
    sent = torch.full((64 + M * rb + 64,), 0x5A, device=DEV, dtype=torch.uint8)
    out = sent[64: 64 + M * rb].view(M, rb).view(R.FP8)
    assert Q.quantize_mx8_rows(buf[:M, col: col + K], out=out) is out
    got = sent.cpu()
    assert torch.equal(got[64: 64 + M * rb].view(M, rb), Q.quantize_mx8_rows(x).view(torch.uint8)), "bytes differ"
    assert bool((got[:64] == 0x5A).all()) and bool((got[64 + M * rb:] == 0x5A).all()), "a write outside the rows"


@pytest.mark.parametrize("reps", (1, 6))
def test_all_codes_are_exact(reps):
    """24 rows (the narrow tile) and 144 rows (the square one) of hand-built bytes: decides the lane layout, the
    nibble order and the scale bytes the instruction reads"""
    c = R.all_codes_case()
    xq = c.xq.repeat(reps, 1).to(DEV)
    y = torch.empty(xq.shape[0], c.q4.shape[0], device=DEV, dtype=BF16)
    ops.load_ext().gemv_skinny(xq, c.q4.to(DEV), c.scale.to(DEV), y, None, None)
    assert torch.equal(_bits(y.cpu()), _bits(c.want.repeat(reps, 1)))


@pytest.mark.parametrize("N,K", R.SHAPES)
def test_matches_the_float64_reference(N, K):
    c = _case(N, K)
    for epi in MX.EPIS:
        ref = _ref(c, epi)
        for M in R.MS:
            got = _call(c, epi, M, soff=61 if M in (33, 129) else 64)
            err, bad, ok = check(got, GR.NS(out=ref.out[:M], A_out=ref.A_out[:M]), epi, "mx", bound=R.BOUND)
            print(f"MEASURE mx.{'out' if epi in GR.ONE_ROUNDING else 'act'} {err:.4g} mx4a8 {epi} M{M} N{N} K{K}")
            assert bool(torch.isfinite(got.float()).all()), "a guard row, a padded entry or a scale byte out of bounds reached y"
            assert bad == 0 and ok, f"mx4a8 {epi} M{M} N{N} K{K}: err {err:.4g}, {bad} bad elements"


@pytest.mark.parametrize("N,K", R.SHAPES[1:])
def test_repeatable_and_row_independent(N, K):
    c = _case(N, K)
    for epi in ("bias_gelu", "bias_res"):
        full = _call(c, epi, 200)
        assert torch.equal(_bits(_call(c, epi, 200)), _bits(full)), "two calls differ"
        for m in (0, 16, 199):
            assert torch.equal(_bits(_call(c, epi, 1, rows=slice(m, m + 1))), _bits(full[m: m + 1])), f"row {m} depends on M"
        assert torch.equal(_bits(_call(c, epi, 33)), _bits(full[:33])), "the narrow and the square tile differ"
        assert torch.equal(_bits(_call(c, epi, 129, soff=62)), _bits(full[:129])), "an unaligned scale table changes the bits"


def test_graph_capture():
    N, K, M = 264, 384, 40
    c = _case(N, K)
    x, q4, scale = c.x[:M].to(DEV), c.q4.to(DEV), c.scale.to(DEV)
    bias, r = c.bias.to(DEV), c.r[:M].to(DEV)
    y = torch.empty(M, N, device=DEV, dtype=BF16)
    xq = torch.empty(M * Q.mx8_row_bytes(K) + 32, device=DEV, dtype=R.FP8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Q.linear_mx4a8(x, q4, scale, bias, residual=r, out=y, xq=xq)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Q.linear_mx4a8(x, q4, scale, bias, residual=r, out=y, xq=xq)
    for rows in (c.x[:M], c.x[M: 2 * M], c.x[:M]):
        x.copy_(rows.to(DEV))
        y.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(Q.linear_mx4a8(x, q4, scale, bias, residual=r)))
