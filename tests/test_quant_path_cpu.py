"""The quantised linear layers on the CPU, both formats, against results recorded from the commit
before ``ops/kernels.py`` was split and ``linear_w8`` / ``linear_w4`` became one code path over
``ops.QUANT_FORMATS``: every output bit for bit, every ValueError message in full.

``tests/golden/quant_parent.pt`` holds, by case name, the outputs of ``linear_w8`` / ``linear_w4``
(the skinny wrappers gave the same bits wherever they accept the shape; the recording asserted
it) and sha256 digests of the larger tensors (quantised weights, dequantised weights, the
effective state dict of a tiny generator).  It was written by running this file as a script on
that commit and is never regenerated from the code under test.

Inputs are multiples of 1/8 and the quantised weights are small integers, so every dot product
is exact in f32 whatever order a BLAS adds it in; what follows it (one multiply by the scale,
bias, GELU, residual) is elementwise.  M = 1, 16, 17 puts the skinny bound on both sides; int8
K = 48 is the shape the GPU sends to the dequantising route."""
import hashlib
import itertools
import os

import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops
from mipipe.models.config import NativeConfig
from mipipe.models.generate import Generator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant_parent.pt")
N, MS = 20, (1, 16, 17)
KS = {"int8": (48, 128, 256), "int4g128": (128, 256)}
FNS = {"int8": (ops.quantize_w8, ops.dequant_w8, ops.linear_w8, ops.linear_skinny),
       "int4g128": (ops.quantize_w4, ops.dequant_w4, ops.linear_w4, ops.linear_skinny_w4)}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
VARIANTS = {"plain": (False, "none", False), "bias": (True, "none", False), "bias_gelu": (True, "gelu_tanh", False),
            "bias_res": (True, "none", True), "res": (False, "none", True)}
CASES = [(f, d, k) for f in KS for d in DTYPES for k in KS[f]]


def _digest(t: torch.Tensor) -> str:
    t = t.detach().contiguous()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return f"{t.dtype} {tuple(t.shape)} " + hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def _inputs(fmt, dname, K):
    g = torch.Generator().manual_seed(1000 * K + 10 * len(fmt) + len(dname))
    dt = DTYPES[dname]
    q, scale = FNS[fmt][0](torch.randn(N, K, generator=g))
    x = (torch.randint(-8, 9, (max(MS), K), generator=g).float() / 8).to(dt)
    bias = (torch.randint(-16, 17, (N,), generator=g).float() / 4).to(dt)
    res = (torch.randint(-8, 9, (max(MS), N), generator=g).float() / 2).to(dt)
    return q, scale, x, bias, res


def _tiny_cfg():
    return NativeConfig.gpt2("tiny", vocab_size=96, d_model=128, n_layers=1, n_heads=2, d_ff=256, max_seq_len=16,
                             dropout=0.0)


def _record() -> dict:
    """Everything the tests compare, computed with the public per-format functions only."""
    out = {}
    for fmt, dname, K in CASES:
        quantize, dequant, linear, skinny = FNS[fmt]
        q, scale, x, bias, res = _inputs(fmt, dname, K)
        key = f"{fmt}/{dname}/K{K}"
        out[key + "/q"], out[key + "/scale"] = _digest(q), _digest(scale)
        out[key + "/dequant"] = _digest(dequant(q, scale))
        out[key + "/dequant_into"] = _digest(dequant(q, scale, torch.empty(N, K, dtype=DTYPES[dname])))
        for M, (vname, (b, act, r)) in itertools.product(MS, VARIANTS.items()):
            y = linear(x[:M], q, scale, bias if b else None, act, res[:M] if r else None)
            assert y.dtype == x.dtype and tuple(y.shape) == (M, N)
            if M <= ops.SKINNY_MAX_M and K % 32 == 0:
                assert torch.equal(y, skinny(x[:M], q, scale, bias if b else None, act, res[:M] if r else None))
            out[f"{key}/M{M}/{vname}"] = y
    for fmt in KS:
        sd = Generator(_tiny_cfg(), "cpu", dtype=torch.float32, seed=3, weights=fmt).arena.effective_state_dict()
        out[f"{fmt}/state_dict"] = {n: _digest(t) for n, t in sd.items()}
    return out


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=True)


@pytest.mark.parametrize("fmt,dname,K", CASES)
def test_outputs_are_the_parents_bit_for_bit(golden, fmt, dname, K):
    quantize, dequant, linear, skinny = FNS[fmt]
    q, scale, x, bias, res = _inputs(fmt, dname, K)
    key = f"{fmt}/{dname}/K{K}"
    assert (_digest(q), _digest(scale)) == (golden[key + "/q"], golden[key + "/scale"])
    q2, s2 = ops.QUANT_FORMATS[fmt].quantize(torch.randn(N, K, generator=torch.Generator().manual_seed(0)))
    q3, s3 = quantize(torch.randn(N, K, generator=torch.Generator().manual_seed(0)))
    assert torch.equal(q2, q3) and torch.equal(s2, s3)
    into = torch.empty(N, K, dtype=DTYPES[dname])
    for dq in (dequant, ops.QUANT_FORMATS[fmt].dequant):
        assert _digest(dq(q, scale)) == golden[key + "/dequant"]
        assert dq(q, scale, into) is into and _digest(into) == golden[key + "/dequant_into"]
    for M, (vname, (b, act, r)) in itertools.product(MS, VARIANTS.items()):
        args = (bias if b else None, act, res[:M] if r else None)
        want = golden[f"{key}/M{M}/{vname}"]
        runs = {"linear": linear(x[:M], q, scale, *args), "linear_q": ops.linear_q(x[:M], q, scale, fmt, *args)}
        buf = torch.full((M, N), 7.0, dtype=x.dtype)
        assert linear(x[:M], q, scale, *args, out=buf) is buf
        runs["linear(out=)"] = buf
        if M <= ops.SKINNY_MAX_M and K % 32 == 0:
            runs["skinny"] = skinny(x[:M], q, scale, *args)
        for what, y in runs.items():
            assert y.dtype == want.dtype and torch.equal(y, want), f"{key}/M{M}/{vname}: {what}"


def test_bf16_weights_on_linear_skinny(golden):
    """bf16 weights without a scale stay linear_skinny's case: x @ w^T with no scaling."""
    q, scale, x, bias, res = _inputs("int8", "bf16", 128)
    w = q.to(torch.bfloat16)
    y = ops.linear_skinny(x[:16], w, None, bias, "gelu_tanh")
    ref = torch.nn.functional.gelu((x[:16].float() @ w.float().t() + bias.float()).to(torch.bfloat16).float(),
                                   approximate="tanh").to(torch.bfloat16)
    assert torch.equal(y, ref)


@pytest.mark.parametrize("fmt", list(KS))
def test_effective_state_dict_is_the_parents(golden, fmt):
    sd = Generator(_tiny_cfg(), "cpu", dtype=torch.float32, seed=3, weights=fmt).arena.effective_state_dict()
    assert {n: _digest(t) for n, t in sd.items()} == golden[f"{fmt}/state_dict"]


def _messages():
    """(call, the parent's message) for every ValueError of the quantised functions."""
    q8, s8, x, bias, res = _inputs("int8", "bf16", 128)
    q4, s4, _, _, _ = _inputs("int4g128", "bf16", 128)
    x1, x17 = x[:1], x[:17]
    out = [
        (lambda: ops.quantize_w8(x[0]), "quantize_w8: w must be [N, K]"),
        (lambda: ops.quantize_w4(x[0]), "quantize_w4: w must be [N, K]"),
        (lambda: ops.quantize_w4(x[:, :64]), "quantize_w4: K = 64 must be a multiple of 128"),
        (lambda: ops.quantize_w4(x[:, :0]), "quantize_w4: K = 0 must be a multiple of 128"),
        (lambda: ops.dequant_w4(q4[:, :32], s4), "dequant_w4: packed uint8 q4 [N, K / 2] with K % 128 == 0 and scale "
         "[K / 128, N] needed, got torch.uint8 (20, 32) and (1, 20)"),
        (lambda: ops.dequant_w4(q8, s4), "dequant_w4: packed uint8 q4 [N, K / 2] with K % 128 == 0 and scale "
         "[K / 128, N] needed, got torch.int8 (20, 128) and (1, 20)"),
        (lambda: ops.dequant_w4(q4, s4.t()), "dequant_w4: packed uint8 q4 [N, K / 2] with K % 128 == 0 and scale "
         "[K / 128, N] needed, got torch.uint8 (20, 64) and (20, 1)"),
        (lambda: ops.linear_skinny(x17, q8, s8), "linear_skinny: M = 17 outside [1, 16] (linear_w8 / linear take any M)"),
        (lambda: ops.linear_skinny(x[:0], q8, s8), "linear_skinny: M = 0 outside [1, 16] (linear_w8 / linear take any M)"),
        (lambda: ops.linear_skinny(x1[:, :48], q8[:, :48], s8), "linear_skinny: K = 48 must be a multiple of 32"),
        (lambda: ops.linear_skinny_w4(x17, q4, s4), "linear_skinny_w4: M = 17 outside [1, 16] (linear_w4 takes any M)"),
        (lambda: ops.linear_skinny_w4(x[:0], q4, s4), "linear_skinny_w4: M = 0 outside [1, 16] (linear_w4 takes any M)"),
    ]
    for name, fn in (("linear_skinny", ops.linear_skinny), ("linear_w8", ops.linear_w8),
                     ("linear_w8", lambda *a: ops.linear_q(a[0], a[1], a[2], "int8", *a[3:]))):
        out += [
            (lambda fn=fn: fn(x[0], q8, s8), f"{name}: x [M, K] and w [N, K] needed, got (128,) and (20, 128)"),
            (lambda fn=fn: fn(x1, q8[0], s8), f"{name}: x [M, K] and w [N, K] needed, got (1, 128) and (128,)"),
            (lambda fn=fn: fn(x1, q8[:, :96], s8), f"{name}: x [M, K] and w [N, K] needed, got (1, 128) and (20, 96)"),
            (lambda fn=fn: fn(x1, q8, None), f"{name}: int8 weights take a scale, other weights none"),
            (lambda fn=fn: fn(x1, q8.to(torch.bfloat16), s8), f"{name}: int8 weights take a scale, other weights none"),
            (lambda fn=fn: fn(x1, q8, s8, bias, "relu"), f"{name}: activation 'relu' is not supported (none, gelu_tanh)"),
            (lambda fn=fn: fn(x1, q8, s8, None, "gelu"), f"{name}: activation epilogue needs a bias and no residual"),
            (lambda fn=fn: fn(x1, q8, s8, bias, "gelu_tanh", res[:1]),
             f"{name}: activation epilogue needs a bias and no residual"),
        ]
    for name, fn in (("linear_skinny_w4", ops.linear_skinny_w4), ("linear_w4", ops.linear_w4),
                     ("linear_w4", lambda *a: ops.linear_q(a[0], a[1], a[2], "int4g128", *a[3:]))):
        out += [
            (lambda fn=fn: fn(x1, q8[:, :64], s4), f"{name}: x [M, K] and packed uint8 q4 [N, K / 2] needed, got (1, 128) "
             "and torch.int8 (20, 64)"),
            (lambda fn=fn: fn(x[0], q4, s4), f"{name}: x [M, K] and packed uint8 q4 [N, K / 2] needed, got (128,) and "
             "torch.uint8 (20, 64)"),
            (lambda fn=fn: fn(x1, q4[:, :48], s4), f"{name}: x [M, K] and packed uint8 q4 [N, K / 2] needed, got (1, 128) "
             "and torch.uint8 (20, 48)"),
            (lambda fn=fn: fn(x1[:, :64], q4[:, :32], s4), f"{name}: K = 64 must be a multiple of 128"),
            (lambda fn=fn: fn(x1, q4, None), f"{name}: scale must be [K / 128, N] = [1, 20]"),
            (lambda fn=fn: fn(x1, q4, s8), f"{name}: scale must be [K / 128, N] = [1, 20]"),
            (lambda fn=fn: fn(x1, q4, s4.t()), f"{name}: scale must be [K / 128, N] = [1, 20]"),
            (lambda fn=fn: fn(x1, q4, s4, bias, "relu"), f"{name}: activation 'relu' is not supported (none, gelu_tanh)"),
            (lambda fn=fn: fn(x1, q4, s4, None, "gelu"), f"{name}: activation epilogue needs a bias and no residual"),
            (lambda fn=fn: fn(x1, q4, s4, bias, "gelu_tanh", res[:1]),
             f"{name}: activation epilogue needs a bias and no residual"),
        ]
    return out


def test_error_messages_are_the_parents():
    for call, msg in _messages():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == msg


def test_gpu_side_checks_without_a_gpu(monkeypatch):
    """What only a GPU tensor reaches -- the scratch check of the dequantising route and the skinny
    bound seen through the any-M functions -- with ``_gpu`` answering yes: each of these raises
    before anything is launched."""
    monkeypatch.setattr(ops.quant, "_gpu", lambda t: True)
    q8, s8, x, _, _ = _inputs("int8", "bf16", 256)
    q4, s4, _, _, _ = _inputs("int4g128", "bf16", 256)
    small = torch.empty(N * 256 - 1, dtype=torch.bfloat16)
    wrong = torch.empty(N * 256, dtype=torch.float32)
    strided = torch.empty(2 * N * 256, dtype=torch.bfloat16)[::2]
    for name, fn, q, s in (("linear_w8", ops.linear_w8, q8, s8), ("linear_w4", ops.linear_w4, q4, s4),
                           ("linear_w8", lambda *a, **k: ops.linear_q(*a, "int8", **k), q8, s8),
                           ("linear_w4", lambda *a, **k: ops.linear_q(*a, "int4g128", **k), q4, s4)):
        for scratch in (small, wrong, strided):
            with pytest.raises(ValueError) as e:
                fn(x[:17], q, s, scratch=scratch)
            assert str(e.value) == f"{name}: scratch must be contiguous bf16 with at least {N * 256} elements"
    # int8 with K % 32 != 0 takes the dequantising route at any M and does not raise the skinny kernel's K error
    with pytest.raises(ValueError) as e:
        ops.linear_w8(x[:1, :48], q8[:, :48], s8, scratch=small[:10])
    assert str(e.value) == f"linear_w8: scratch must be contiguous bf16 with at least {N * 48} elements"
    for fn, q, s, msg in ((ops.linear_w8, q8, s8, "linear_skinny: M = 0 outside [1, 16] (linear_w8 / linear take any M)"),
                          (ops.linear_w4, q4, s4, "linear_skinny_w4: M = 0 outside [1, 16] (linear_w4 takes any M)")):
        with pytest.raises(ValueError) as e:
            fn(x[:0], q, s)
        assert str(e.value) == msg


def test_format_table():
    from mipipe.models import generate as G
    assert G.QUANT_FORMATS == tuple(ops.QUANT_FORMATS) == ("int8", "int4g128")
    assert [(f.k_format, f.k_skinny) for f in ops.QUANT_FORMATS.values()] == [(1, 32), (128, 128)]
    with pytest.raises(ValueError) as e:
        G.QuantWeights(NativeConfig.gpt2("tiny", vocab_size=96, d_model=64, n_layers=1, n_heads=2, d_ff=128,
                                         max_seq_len=16), "cpu", torch.float32, "int4g128")
    assert str(e.value) == ("QuantWeights: int4g128 needs K % 128 == 0 in every quantised matrix; "
                            "tok_embeddings.weight is (128, 64)")


if __name__ == "__main__":      # run on the commit the golden file describes
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    torch.save(_record(), GOLDEN)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
