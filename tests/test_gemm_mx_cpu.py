"""The MXFP8 activation format and the CPU path of ops.quant.linear_mx4a8 (tensor code; the kernels of
csrc/kernels/gemm_mx.hip are held to the same bytes by test_gemm_mx_gpu.py)."""
import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.models.config import NativeConfig

import gemm_mx_refs as R
import gemv_mx4_refs as MX

Q = ops.quant


def test_rule_on_hand_built_groups():
    x, byte, codes = R.hand_groups()
    for dt in (torch.float32, torch.bfloat16):
        if dt == torch.bfloat16:                    # the f32 step above 448 * 2^3 is not a bf16 value
            x = x.clone()
            x[0, 64] = 3600.0
        xq = Q.quantize_mx8_rows(x.to(dt))
        assert xq.dtype == R.FP8 and tuple(xq.shape) == (2, Q.mx8_row_bytes(128)) == (2, 144) and xq.is_contiguous()
        b = xq.view(torch.uint8)
        assert torch.equal(b[:, 128:132], byte) and not bool(b[:, 132:].any()) and not bool(b[0, :32].any())
        assert {k: int(b[k]) for k in codes} == codes


@pytest.mark.parametrize("M,K", [(1, 128), (33, 384)])
def test_round_trip_within_half_an_ulp(M, K):
    x = R.randn_x(M, K, seed=M)
    x[0, 32:64] = 0
    xq = Q.quantize_mx8_rows(x)
    b = xq.view(torch.uint8)
    assert not bool((b[:, K: K + K // 32] == 255).any()) and not bool((b[:, :K] & 0x7F == 0x7F).any())
    s = MX.E8M0[b[:, K: K + K // 32].long()].repeat_interleave(32, dim=1)
    v, vh = x.double() / s, Q.dequantize_mx8_rows(xq, K).double() / s         # at the group's scale
    top = v.abs().view(M, -1, 32).amax(dim=2)                                # the scaled maximum: in (224, 448]
    assert float(top.max()) <= 448 and float(top[top > 0].min()) > 224 and int((top == 0).sum()) == 1
    # e4m3: three mantissa bits above 2^-6, steps of 2^-9 below
    ulp = torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -6))) - 3)
    assert bool(((v - vh).abs() <= ulp / 2).all())
    assert torch.equal(Q.dequantize_mx8_rows(xq, K, torch.float64), vh * s)


def test_rejects_k_not_a_multiple_of_128():
    for K in (64, 160, 32):
        with pytest.raises(ValueError):
            Q.quantize_mx8_rows(torch.zeros(2, K))
    with pytest.raises(ValueError):
        Q.linear_mx4a8(torch.zeros(2, 160), torch.zeros(8, 80, dtype=torch.uint8), torch.zeros(8, 5, dtype=torch.uint8))


@pytest.mark.parametrize("M", [5, 20])
def test_linear_mx4a8_cpu_is_the_product_of_the_dequantised_operands(M):
    c = MX.randn_case(M, 40, 256, seed=M)
    W, xh = MX.what(c.q4, c.scale), R.xhat(Q, c.x)
    want = (xh @ W.t() + c.bias.double() + c.r.double()).to(torch.bfloat16)
    got = Q.linear_mx4a8(c.x, c.q4, c.scale, c.bias, residual=c.r)
    assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_generator_takes_mxfp8_activations_with_mxfp4_weights_only():
    cfg = NativeConfig.gpt2("tiny", vocab_size=512, d_model=256, n_layers=1, n_heads=4, d_ff=1024, max_seq_len=64)
    for w in ("int8", "int4g128", "bf16"):
        with pytest.raises(ValueError):
            mipipe.Generator(cfg, "cpu", dtype=torch.float32, weights=w, activations="mxfp8")
    with pytest.raises(ValueError):
        mipipe.Generator(cfg, "cpu", dtype=torch.float32, weights="mxfp4", activations="fp8")
    gen = mipipe.Generator(cfg, "cpu", dtype=torch.float32, weights="mxfp4", activations="mxfp8")
    gen.prefill(torch.arange(20)[None], gen.new_cache(1))
    assert gen.activations == "mxfp8" and gen._scratch is None
