"""ops.quant.linear_skinny64 and linear_q(rows64=True) on CPU tensors: the f32 path of the other
quantised linears (``_linear_cpu``), the row bound of the 64-row kernel, and no change of route
where there is no GPU."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

Q = ops.quant


def _operands(fmt, N=24, K=256):
    g = torch.Generator().manual_seed(11)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    x, bias, res = torch.randn(65, K, generator=g), torch.randn(N, generator=g), torch.randn(65, N, generator=g)
    q, scale = (w, None) if fmt == "bf16" else ops.QUANT_FORMATS[fmt].quantize(w)
    return x, q, scale, bias, res


@pytest.mark.parametrize("M", [17, 64])
@pytest.mark.parametrize("fmt", ["int8", "int4g128", "bf16"])
def test_skinny64_cpu_is_the_f32_path(fmt, M):
    x, q, scale, bias, res = _operands(fmt)
    for kw in (dict(), dict(bias=bias, act="gelu_tanh"), dict(bias=bias, residual=res[:M])):
        got = Q.linear_skinny64(x[:M], q, scale, **kw)
        if fmt == "bf16":
            want = Q._linear_cpu(ops.QUANT_FORMATS["int8"], x[:M], q, None, kw.get("bias"), kw.get("act", "none"),
                                 kw.get("residual"), torch.empty(M, q.shape[0]))
        else:
            want = ops.linear_q(x[:M], q, scale, fmt, **kw)
            assert torch.equal(want, ops.linear_q(x[:M], q, scale, fmt, rows64=True, **kw))
        assert got.shape == (M, q.shape[0]) and torch.equal(got, want)


@pytest.mark.parametrize("fmt", ["int8", "int4g128", "bf16"])
def test_skinny64_row_bound(fmt):
    x, q, scale, _, _ = _operands(fmt)
    assert Q.SKINNY64_MAX_M == 64 and "SKINNY64_MAX_M" not in Q.__all__ and "linear_skinny64" not in Q.__all__
    for M in (0, 65):
        with pytest.raises(ValueError, match=rf"linear_skinny64: M = {M} outside \[1, 64\]"):
            Q.linear_skinny64(x[:M], q, scale)
