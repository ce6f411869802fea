"""MXFP4 weights on the CPU: the quantiser against the independent one of gemv_mx4_refs.py bit for
bit, dequant_mx4 and linear_q against the float64 reference, and ``weights="mxfp4"`` generators
against a dense generator loaded with their effective weights."""
import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.models.generate import QuantWeights

import gemv_mx4_refs as MX
from test_generate_w4_cpu import _cfg, _tokens, dense_oracle

Q = ops.quant
F32 = torch.float32


def _edge_matrix(N, K, seed):
    """random rows of mixed magnitudes plus the groups the rounding rules are about"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-20, 20, (N, 1), generator=g).float())
    w[0, :32] = 0                                                            # a zero group
    w[1, :32] = torch.randn(32, generator=g).clamp(-1, 1) * 0.5
    w[1, 3] = -0.5                                                           # amax an exact power of two
    # amax 6 * 2^-3 (E = -3, no rounding of its own), every tie point in both signs, and 7 > 6
    ties = torch.tensor([.25, .75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0])
    w[2, :32] = torch.cat([ties, -ties, torch.zeros(16)]) / 8
    w[3, :32] = torch.cat([ties, -ties, torch.zeros(16)]) / 8
    w[3, 7] = 7.0 / 8                                                        # the same E, 7 saturates to 6
    return w


@pytest.mark.parametrize("N,K,seed", [(8, 128, 0), (40, 384, 1)])
def test_quantize_mx4_matches_the_independent_quantiser(N, K, seed):
    w = _edge_matrix(N, K, seed)
    q4, scale = Q.quantize_mx4(w)
    rq, rs = MX.quantize_ref(w)
    assert q4.dtype == torch.uint8 and q4.shape == (N, K // 2) and scale.dtype == torch.uint8 and scale.shape == (N, K // 32)
    assert torch.equal(scale, rs) and torch.equal(q4, rq)
    assert int(scale[0, 0]) == 0 and not bool(q4[0, :16].any())
    assert int(scale[1, 0]) == 127 - 1 - 2 and int(scale[2, 0]) == 127 - 1 - 2
    # ties to the even code (.25 -> 0, .75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), 6 stays
    assert MX.unpack(q4)[2, :16].tolist() == [0, 1, 1, 2, 2, 4, 4, 6, 0, -1, -1, -2, -2, -4, -4, -6]
    assert int(q4[2, 4]) & 0x0F == 0                                         # -0.25 -> code 0, never 8
    assert MX.unpack(q4)[3, 7] == 6.0
    assert not bool(((q4 & 0x0F) == 8).any()) and not bool(((q4 >> 4) == 8).any()) and int(scale.max()) < 255
    # dequant_mx4: What rounded once to bf16 (exact in f32)
    W = MX.what(q4, scale)
    assert torch.equal(Q.dequant_mx4(q4, scale).double(), W)
    assert torch.equal(Q.dequant_mx4(q4, scale, torch.empty(N, K, dtype=torch.bfloat16)), W.to(torch.bfloat16))


def test_k_not_a_multiple_of_128_raises():
    with pytest.raises(ValueError, match="128"):
        Q.quantize_mx4(torch.randn(4, 96))
    cfg = mipipe.models.config.NativeConfig.gpt2("tiny", vocab_size=512, d_model=64, n_layers=2, n_heads=4, d_ff=256,
                                                 max_seq_len=32)
    with pytest.raises(ValueError, match="128"):
        mipipe.Generator(cfg, "cpu", dtype=F32, weights="mxfp4")
    for bad in (lambda: mipipe.Generator(_cfg("gpt2"), "cpu", dtype=F32, weights="int4"),
                lambda: QuantWeights(_cfg("gpt2"), "cpu", F32, "int4")):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("epi", MX.EPIS)
def test_linear_q_cpu_matches_reference(epi):
    c = MX.randn_case(5, 40, 384)
    ref = MX.mx4_ref(c.x, c.q4, c.scale, epi, c.bias, c.r)
    got = ops.linear_q(c.x.float(), c.q4, c.scale, "mxfp4", bias=c.bias.float() if "bias" in epi else None,
                       act="gelu_tanh" if epi == "bias_gelu" else "none", residual=c.r.float() if "res" in epi else None)
    torch.testing.assert_close(got.double(), ref.out, rtol=1e-4, atol=1e-5)      # f32 sums against float64
    assert Q.reads_weights_directly(c.x, "mxfp4") and not Q.reads_weights_directly(torch.empty(17, 384), "mxfp4", rows64=True)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generator_matches_dense_oracle(family):
    q = mipipe.Generator(_cfg(family), "cpu", dtype=F32, seed=4, weights="mxfp4")
    ref = dense_oracle(q)
    A = q.arena
    assert A.fmt == q.weights == "mxfp4" and A.head_name in A.q
    assert all(A.scale[n].dtype == torch.uint8 and A.scale[n].shape == (A.q[n].shape[0], A.q[n].shape[1] // 16) for n in A.q)
    tok = _tokens(2, 20)
    cq, cr = q.new_cache(2, 64), ref.new_cache(2, 64)
    torch.testing.assert_close(q.prefill(tok[:, :16], cq), ref.prefill(tok[:, :16], cr))
    for t in range(16, 20):
        torch.testing.assert_close(q.decode(tok[:, t], cq), ref.decode(tok[:, t], cr))
