"""Decode and append attention over int8 KV caches (csrc/kernels/attention_kv8.hip) against the
op's CPU f32 path on the same int8 rows, at the tolerance of test_attn_decode_gpu.py /
test_attn_append_gpu.py (atol = rtol = 2e-2): both sides see the same effective values
``q * scale``, so the quantisation error does not enter.

Layout as in the model and the bf16 tests: B = 2, Smax = 384, q and o strided slices of wider
buffers, the caches views behind 16 leading pad bytes.  Rows at and beyond the valid length are
poisoned with payload -128, NaN scale bits and 0xFF padding: every output must be finite."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import attn_append_refs as AR
import kv8_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, SMAX, PAD, PADB = 2, 384, 8, 16
G = ops.generate


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def close(a, b, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol, rtol=rtol)


def _caches(nb, smax, Hkv, D, valid, g):
    """CPU int8 buffers [nb, smax, PADB + W + PADB]; rows >= valid[b] poisoned"""
    W = G.kv8_row_bytes(Hkv, D)
    bufs = []
    for _ in range(2):
        buf = torch.full((nb, smax, W + 2 * PADB), 0x5A, dtype=torch.int8)
        buf[:, :, PADB:PADB + W] = G.kv_quantize(torch.randn(nb, smax, Hkv * D, generator=g).to(torch.bfloat16), Hkv, D)
        for b, n in enumerate(valid):
            R.poison(buf[b, n:, PADB:PADB + W].numpy(), Hkv, D)
        bufs.append(buf)
    return bufs[0], bufs[1], W


# ------------------------------------------------------------------------------ decode
def _dec_inputs(H, Hkv, D, lens, smax=SMAX, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(len(lens), (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    kbuf, vbuf, W = _caches(len(lens), smax, Hkv, D, lens, g)
    return qkv, kbuf, vbuf, torch.tensor(lens, dtype=torch.int32), W


def _dec_run(H, Hkv, D, tensors, splits, dev):
    qkv, kbuf, vbuf, lens = (t.to(dev) for t in tensors[:4])
    W = tensors[4]
    obuf = torch.zeros(qkv.shape[0], H * D + 2 * PAD, device=dev, dtype=torch.bfloat16 if dev != "cpu" else torch.float32)
    o = obuf[:, PAD: PAD + H * D]
    ops.attn_decode(qkv[:, : H * D], kbuf[:, :, PADB:PADB + W], vbuf[:, :, PADB:PADB + W], lens, o, H, Hkv, D,
                    splits=splits)
    assert float(obuf[:, :PAD].abs().sum()) == 0 and float(obuf[:, PAD + H * D:].abs().sum()) == 0
    return o


_REF = {}


def _dec_ref(H, Hkv, D, lens):
    key = ("d", H, Hkv, D, tuple(lens))
    if key not in _REF:
        _REF[key] = _dec_run(H, Hkv, D, _dec_inputs(H, Hkv, D, lens), 0, "cpu")
    return _REF[key]


@pytest.mark.parametrize("lens", [[1, 1], [7, 300], [129, 5], [384, 257]])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1), (6, 3)])
def test_attn_decode_int8_matches_reference(H, Hkv, D, splits, lens):
    t = _dec_inputs(H, Hkv, D, lens)
    got = _dec_run(H, Hkv, D, t, splits, DEV)
    assert bool(torch.isfinite(got.float()).all()), "a poisoned cache row reached the output"
    close(got, _dec_ref(H, Hkv, D, lens))
    if lens == [1, 1]:
        # one key: the output is exactly bf16(q * scale) of the single V row
        v0 = G.kv_dequantize(t[2][:, 0, PADB:PADB + t[4]], Hkv, D).reshape(B, Hkv, D).repeat_interleave(H // Hkv, 1)
        assert torch.equal(got.cpu(), v0.reshape(B, H * D).to(torch.bfloat16))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1), (6, 3)])
def test_attn_decode_int8_deterministic_and_split_invariant(H, Hkv, D):
    t = _dec_inputs(H, Hkv, D, [129, 300], seed=1)
    for splits in (0, 1, 3):
        a, b = _dec_run(H, Hkv, D, t, splits, DEV), _dec_run(H, Hkv, D, t, splits, DEV)
        assert torch.equal(a, b), f"splits={splits}: two calls differ"
    close(_dec_run(H, Hkv, D, t, 1, DEV), _dec_run(H, Hkv, D, t, 3, DEV))


def test_attn_decode_int8_planner_case():
    H, Hkv, D, smax = 8, 2, 128, 1024
    assert ops.attn_decode_plan(1, Hkv, smax) == 4
    t = _dec_inputs(H, Hkv, D, [1000], smax=smax, seed=2)
    got = _dec_run(H, Hkv, D, t, 0, DEV)
    assert bool(torch.isfinite(got.float()).all())
    close(got, _dec_run(H, Hkv, D, t, 0, "cpu"))


# ------------------------------------------------------------------------------ append
def _app_inputs(T, H, Hkv, D, base, counts, smax=SMAX, seed=0):
    g = torch.Generator().manual_seed(seed)
    nb = len(base)
    qkv = torch.randn(nb * T, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    cl = [T if counts is None else counts[b] for b in range(nb)]
    kbuf, vbuf, W = _caches(nb, smax, Hkv, D, [base[b] + cl[b] for b in range(nb)], g)
    for b in range(nb):
        qkv[b * T + cl[b]:(b + 1) * T] = float("nan")
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32)
    return qkv, kbuf, vbuf, torch.tensor(base, dtype=torch.int32), cnt, W


def _app_run(T, H, Hkv, D, tensors, splits, dev):
    qkv, kbuf, vbuf, base, counts = (t if t is None else t.to(dev) for t in tensors[:5])
    W = tensors[5]
    obuf = torch.full((qkv.shape[0], H * D + 2 * PAD), 3.0, device=dev,
                      dtype=torch.bfloat16 if dev != "cpu" else torch.float32)
    o = obuf[:, PAD: PAD + H * D]
    ops.attn_append(qkv[:, : H * D], kbuf[:, :, PADB:PADB + W], vbuf[:, :, PADB:PADB + W], base, counts, o, T, H, Hkv,
                    D, splits=splits)
    assert bool((obuf[:, :PAD] == 3.0).all()) and bool((obuf[:, PAD + H * D:] == 3.0).all())
    return o


def _app_ref(T, H, Hkv, D, case):
    key = ("a", T, H, Hkv, D, case)
    if key not in _REF:
        base, counts = AR.bases_counts(T, SMAX)[case]
        _REF[key] = _app_run(T, H, Hkv, D, _app_inputs(T, H, Hkv, D, base, counts), 0, "cpu")
    return _REF[key]


# T = 1, 2, 5: the smallest of the bf16 test; with rep = 8, T = 5 is 40 rows: a 32-row query tile
# that spans tokens 0 .. 3 and a ragged second one.  The cases hold the empty cache and counts = 0.
@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1), (6, 3)])
def test_attn_append_int8_matches_reference(H, Hkv, D, splits, T, case):
    base, counts = AR.bases_counts(T, SMAX)[case]
    got = _app_run(T, H, Hkv, D, _app_inputs(T, H, Hkv, D, base, counts), splits, DEV)
    assert bool(torch.isfinite(got.float()).all()), "a poisoned cache or query row reached the output"
    close(got, _app_ref(T, H, Hkv, D, case))
    for b in range(B):
        c = T if counts is None else counts[b]
        assert float(got[b * T + c:(b + 1) * T].float().abs().sum()) == 0, "a row t >= counts[b] is not zero"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 1), (6, 3)])
def test_attn_append_int8_deterministic_and_split_invariant(H, Hkv, D):
    T = 5
    t = _app_inputs(T, H, Hkv, D, [129, 300], [5, 3], seed=1)
    for splits in (0, 1, 3):
        a, b = _app_run(T, H, Hkv, D, t, splits, DEV), _app_run(T, H, Hkv, D, t, splits, DEV)
        assert torch.equal(a, b), f"splits={splits}: two calls differ"
    close(_app_run(T, H, Hkv, D, t, 1, DEV), _app_run(T, H, Hkv, D, t, 3, DEV))


def test_attn_append_int8_planner_case():
    T, H, Hkv, D, smax = 5, 8, 2, 128, 1024
    assert ops.attn_append_plan(1, T, Hkv, H // Hkv, smax) == 4
    t = _app_inputs(T, H, Hkv, D, [1000], [4], smax=smax, seed=2)
    got = _app_run(T, H, Hkv, D, t, 0, DEV)
    assert bool(torch.isfinite(got.float()).all())
    close(got, _app_run(T, H, Hkv, D, t, 0, "cpu"))


# ------------------------------------------------------------------------------ argument checks
def test_int8_unsupported_shapes_raise():
    with pytest.raises(ValueError, match="head_dim"):
        _dec_run(4, 4, 96, _dec_inputs(4, 4, 96, [5, 9]), 0, DEV)
    with pytest.raises(ValueError, match="Hkv"):                     # rep = 16 > 8
        _dec_run(16, 1, 64, _dec_inputs(16, 1, 64, [5, 9]), 0, DEV)
    with pytest.raises(ValueError, match="head_dim"):
        _app_run(2, 4, 4, 96, _app_inputs(2, 4, 4, 96, [5, 9], None), 0, DEV)
    with pytest.raises(ValueError, match="Hkv"):
        _app_run(2, 16, 1, 64, _app_inputs(2, 16, 1, 64, [5, 9], None), 0, DEV)
    H, Hkv, D = 4, 4, 64
    qkv, kbuf, vbuf, lens, W = _dec_inputs(H, Hkv, D, [5, 9])
    qkv, kbuf, vbuf, lens = (x.to(DEV) for x in (qkv, kbuf, vbuf, lens))
    o = torch.zeros(B, H * D, device=DEV, dtype=torch.bfloat16)
    q, good = qkv[:, : H * D], vbuf[:, :, PADB:PADB + W]
    for call in (lambda k, v: ops.attn_decode(q, k, v, lens, o, H, Hkv, D),
                 lambda k, v: ops.attn_append(q, k, v, lens, None, o, 1, H, Hkv, D)):
        with pytest.raises(ValueError, match="int8"):                # a last dimension that is not W
            call(kbuf[:, :, PADB:PADB + Hkv * D], vbuf[:, :, PADB:PADB + Hkv * D])
        with pytest.raises(RuntimeError, match="16-byte"):           # a cache view that starts mid-vector
            call(kbuf[:, :, 8:8 + W], good)
        with pytest.raises(ValueError, match="int8"):                # one cache int8, the other bf16
            call(kbuf[:, :, PADB:PADB + W], torch.zeros(B, SMAX, Hkv * D, device=DEV, dtype=torch.bfloat16))
    assert float(o.float().abs().sum()) == 0                         # nothing was launched
