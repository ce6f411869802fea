"""The int8 KV-cache row format (ops/generate.py: kv8_row_bytes, kv_quantize, kv_dequantize) and
the CPU paths of the ops over int8 caches, against the independent numpy reference of
kv8_refs.py.

The quantiser is defined in f32 with two divisions per head and a multiplication per element, so
the tensor code and numpy agree bit for bit: payload, scale bits and padding are compared as
bytes.  The attention ops run f32 matrix products over the dequantised rows; against the float64
reference over the same rows the bound is f32 rounding of sums of at most D + n <= 168 terms of
magnitude <= 4: 168 * 2^-24 * 4 < 5e-5 absolute (taken as atol, with rtol 1e-5)."""
import numpy as np
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import kv8_refs as R

G = ops.generate


def _x(shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


@pytest.mark.parametrize("Hkv", [1, 3, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_quantize_equals_numpy_reference_bit_for_bit(D, Hkv):
    W = G.kv8_row_bytes(Hkv, D)
    assert W == R.row_bytes(Hkv, D) and W % 16 == 0 and 0 <= W - (Hkv * D + 4 * Hkv) < 16
    x = _x((2, 5, Hkv * D), 3, torch.bfloat16)
    x[0, 1] = 0                                         # a zero row
    x[1, 2, :D] = 0                                     # a zero head beside live ones
    x[1, 3] *= 1e-3
    x[0, 4] *= 300.0
    rows = G.kv_quantize(x, Hkv, D)
    assert rows.dtype == torch.int8 and rows.shape == (2, 5, W)
    want = R.pack(x.float().numpy(), Hkv, D)
    assert np.array_equal(rows.numpy().view(np.uint8), want.view(np.uint8))
    q, scale, pad = R.unpack(rows.numpy(), Hkv, D)
    assert int(q.min()) >= -127, "the quantiser wrote -128"
    assert not pad.any(), "padding bytes are not zero"
    assert scale[0, 1].max() == 0 and not q[0, 1].any() and scale[1, 2, 0] == 0 and not q[1, 2, 0].any()
    live = scale > 0
    assert (np.abs(q.astype(np.int32)).max(-1)[live] == 127).all(), "the largest element of a head is not +-127"
    # the largest element by sign
    xh = x.float().numpy().reshape(2, 5, Hkv, D)
    idx = np.abs(xh).argmax(-1)
    top = np.take_along_axis(q, idx[..., None], -1)[..., 0].astype(np.int32)
    assert (top[live] == 127 * np.sign(np.take_along_axis(xh, idx[..., None], -1)[..., 0])[live]).all()
    # dequantise: q * scale in f32, bit for bit, and in another dtype
    back = G.kv_dequantize(rows, Hkv, D)
    assert back.dtype == torch.float32
    assert np.array_equal(back.numpy(), (q.astype(np.float32) * scale[..., None]).reshape(2, 5, Hkv * D))
    assert torch.equal(G.kv_dequantize(rows, Hkv, D, torch.bfloat16), back.to(torch.bfloat16))
    assert np.abs(R.values(rows.numpy(), Hkv, D) - x.double().numpy()).max() <= 0.5 * float(scale.max()) * 1.0001


def test_format_argument_checks():
    with pytest.raises(ValueError):
        G.kv_quantize(torch.zeros(2, 100), 2, 64)
    with pytest.raises(ValueError):
        G.kv_dequantize(torch.zeros(2, 128, dtype=torch.int8), 2, 64)
    with pytest.raises(ValueError):
        G.kv_dequantize(torch.zeros(2, 144), 2, 64)


def _append_case(T, rope, D, H, Hkv, dtype):
    B, Smax = 2, 16
    W = G.kv8_row_bytes(Hkv, D)
    qkv = _x((B * T, (H + 2 * Hkv) * D), 7, dtype)
    cos, sin = ops.rope_tables(Smax, D, 10000.0, "cpu")
    pos = torch.tensor([2, Smax + 5], dtype=torch.int32)          # the second clamps to Smax - 1
    counts = None if T == 1 else torch.tensor([3, 1], dtype=torch.int32)
    return B, Smax, W, qkv, cos, sin, pos, counts


@pytest.mark.parametrize("active", [None, [1, 0]])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_append_is_kv_quantize_of_the_float_append(dtype, rope, T, active):
    D, H, Hkv = 64, 6, 3
    B, Smax, W, qkv, cos, sin, pos, counts = _append_case(T, rope, D, H, Hkv, dtype)
    act = None if active is None else torch.tensor(active, dtype=torch.uint8)
    kf, vf = torch.full((B, Smax, Hkv * D), 9.0, dtype=dtype), torch.full((B, Smax, Hkv * D), 9.0, dtype=dtype)
    q_float = qkv.clone()
    ops.rope_kv_append(q_float, cos, sin, kf, vf, pos, act, H, Hkv, D, rope=rope, T=T, counts=counts)
    # int8 caches as views behind 16 pad bytes of a wider buffer full of a canary byte
    kbuf = torch.full((B, Smax, W + 32), 0x5A, dtype=torch.int8)
    vbuf = torch.full((B, Smax, W + 32), 0x5A, dtype=torch.int8)
    k8, v8 = kbuf[:, :, 16:16 + W], vbuf[:, :, 16:16 + W]
    q_int = qkv.clone()
    ops.rope_kv_append(q_int, cos, sin, k8, v8, pos, act, H, Hkv, D, rope=rope, T=T, counts=counts)
    assert torch.equal(q_int.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       q_float.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    written = (kf != 9.0).any(-1)
    assert int(written.sum()) == sum(T if counts is None else int(counts[b])
                                     for b in range(B) if active is None or active[b])
    for got, flt, buf in ((k8, kf, kbuf), (v8, vf, vbuf)):
        assert torch.equal(got[written], G.kv_quantize(flt[written], Hkv, D))
        assert bool((got[~written] == 0x5A).all()), "a skipped row was touched"
        assert bool((buf[:, :, :16] == 0x5A).all()) and bool((buf[:, :, 16 + W:] == 0x5A).all())


def _cache(B, Smax, Hkv, D, lens, seed):
    k = G.kv_quantize(_x((B, Smax, Hkv * D), seed), Hkv, D)
    v = G.kv_quantize(_x((B, Smax, Hkv * D), seed + 1), Hkv, D)
    for b, n in enumerate(lens):
        R.poison(k[b, n:].numpy(), Hkv, D)
        R.poison(v[b, n:].numpy(), Hkv, D)
    return k, v


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 3), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_cpu_attn_decode_on_int8_cache(D, H, Hkv):
    B, Smax, lens = 3, 40, [1, 40, 0]
    k, v = _cache(B, Smax, Hkv, D, lens, 11)
    q = _x((B, H * D), 13)
    o = torch.full((B, H * D), 3.0)
    ops.attn_decode(q, k, v, torch.tensor(lens, dtype=torch.int32), o, H, Hkv, D)
    want = R.attn_decode_ref(q.numpy(), k.numpy(), v.numpy(), lens, H, Hkv, D)
    torch.testing.assert_close(o.double(), torch.from_numpy(want), atol=5e-5, rtol=1e-5)
    # one key: the output is that V row's effective values
    torch.testing.assert_close(o[0].reshape(H, D), G.kv_dequantize(v[0, 0], Hkv, D).reshape(Hkv, D)
                               .repeat_interleave(H // Hkv, 0), atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 3)])
@pytest.mark.parametrize("D", [64, 128])
def test_cpu_attn_append_on_int8_cache(D, H, Hkv):
    B, Smax, T = 3, 40, 3
    base, counts = [0, 30, 37], [3, 2, 0]
    k, v = _cache(B, Smax, Hkv, D, [b + c for b, c in zip(base, counts)], 17)
    q = _x((B * T, H * D), 19)
    o = torch.full((B * T, H * D), 3.0)
    ops.attn_append(q, k, v, torch.tensor(base, dtype=torch.int32), torch.tensor(counts, dtype=torch.int32), o, T, H,
                    Hkv, D)
    want = R.attn_append_ref(q.numpy(), k.numpy(), v.numpy(), base, counts, T, H, Hkv, D)
    torch.testing.assert_close(o.double(), torch.from_numpy(want), atol=5e-5, rtol=1e-5)


def test_int8_caches_of_another_width_raise():
    H, Hkv, D = 4, 4, 64
    q = torch.zeros(1, H * D)
    good = torch.zeros(1, 8, G.kv8_row_bytes(Hkv, D), dtype=torch.int8)
    bad = torch.zeros(1, 8, Hkv * D, dtype=torch.int8)
    lens = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="int8"):
        ops.attn_decode(q, bad, bad, lens, torch.zeros_like(q), H, Hkv, D)
    with pytest.raises(ValueError, match="int8"):
        ops.attn_decode(q, good, good.float(), lens, torch.zeros_like(q), H, Hkv, D)
    with pytest.raises(ValueError, match="int8"):
        ops.attn_append(q, bad, bad, lens, None, torch.zeros_like(q), 1, H, Hkv, D)
    with pytest.raises(ValueError, match="int8"):
        ops.rope_kv_append(torch.zeros(1, 3 * H * D), None, None, bad, bad, lens, None, H, Hkv, D, rope=False)
