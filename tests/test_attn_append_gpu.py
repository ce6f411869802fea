"""Append attention (csrc/kernels/attention_append.hip) against the op's CPU f32 path on the
same bf16 inputs, at the tolerance of test_attn_decode_gpu.py and in its layout: B = 2,
Smax = 384, q and o strided slices of wider buffers, caches behind 8 leading columns.

Cache rows at or beyond base + counts and q rows with t >= counts hold NaN: every output
must be finite and the rows t >= counts[b] exactly zero.  Shapes are the smallest that reach
every path: rep = H / Hkv of 1, 4 and 8, both head dims, one / three forced splits and the
planner's choice, T of 1, 2, 5 and 33 new tokens (1 to 264 (token, head) rows per KV head: a
padded 32-row tile, an exact one, several with a ragged last one), and per-sequence
(base, counts) that give the empty cache, a single cached key beside a long cache, a partial
row beside a chunk edge crossed inside the new tokens, and a full cache beside a row with
nothing to do."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import attn_append_refs as AR

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, SMAX, PAD = 2, 384, AR.PAD


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def close(a, b, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol, rtol=rtol)


def _run(T, H, Hkv, D, tensors, splits, dev):
    qkv, kbuf, vbuf, base, counts = (t if t is None else t.to(dev) for t in tensors)
    rows = qkv.shape[0]
    # the GPU output is a bf16 slice of a wider buffer; the CPU reference keeps f32
    obuf = torch.full((rows, H * D + 2 * PAD), 3.0, device=dev, dtype=torch.bfloat16 if dev != "cpu" else torch.float32)
    o = obuf[:, PAD: PAD + H * D]
    ops.attn_append(qkv[:, : H * D], kbuf[:, :, PAD:], vbuf[:, :, PAD:], base, counts, o, T, H, Hkv, D, splits=splits)
    assert bool((obuf[:, :PAD] == 3.0).all()) and bool((obuf[:, PAD + H * D:] == 3.0).all())
    return o


_REF = {}


def _ref(T, H, Hkv, D, case):
    """CPU f32 reference, computed once per case and shared by the split variants."""
    key = (T, H, Hkv, D, case)
    if key not in _REF:
        base, counts = AR.bases_counts(T, SMAX)[case]
        _REF[key] = _run(T, H, Hkv, D, AR.make_inputs(T, H, Hkv, D, base, counts, SMAX), 0, "cpu")
    return _REF[key]


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("T", [1, 2, 5, 33])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1)])
def test_attn_append_matches_reference(H, Hkv, D, splits, T, case):
    base, counts = AR.bases_counts(T, SMAX)[case]
    got = _run(T, H, Hkv, D, AR.make_inputs(T, H, Hkv, D, base, counts, SMAX), splits, DEV)
    assert bool(torch.isfinite(got.float()).all()), "a poisoned cache or query row reached the output"
    close(got, _ref(T, H, Hkv, D, case))
    for b in range(B):
        c = T if counts is None else counts[b]
        assert float(got[b * T + c:(b + 1) * T].float().abs().sum()) == 0, "a row t >= counts[b] is not zero"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1)])
def test_attn_append_one_token_is_attn_decode(H, Hkv, D):
    base = [128, 299]
    t = AR.make_inputs(1, H, Hkv, D, base, None, SMAX, seed=1)
    qkv, kbuf, vbuf, bs, _ = (x if x is None else x.to(DEV) for x in t)
    o = torch.zeros(B, H * D, device=DEV, dtype=torch.bfloat16)
    ops.attn_decode(qkv[:, : H * D], kbuf[:, :, PAD:], vbuf[:, :, PAD:], bs + 1, o, H, Hkv, D)
    close(_run(1, H, Hkv, D, t, 0, DEV), o)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1)])
def test_attn_append_deterministic_and_split_invariant(H, Hkv, D):
    T = 5
    t = AR.make_inputs(T, H, Hkv, D, [129, 300], [5, 3], SMAX, seed=1)
    for splits in (0, 1, 3):
        a, b = _run(T, H, Hkv, D, t, splits, DEV), _run(T, H, Hkv, D, t, splits, DEV)
        assert torch.equal(a, b), f"splits={splits}: two calls differ"
    close(_run(T, H, Hkv, D, t, 1, DEV), _run(T, H, Hkv, D, t, 3, DEV))


def test_attn_append_planner():
    plan = ops.attn_append_plan
    assert plan(2, 5, 4, 1, SMAX) == 1                  # a short cache is not split
    assert plan(64, 1, 8, 4, 1024) == 1                 # 512 (sequence, KV head) pairs fill the chip alone
    assert plan(1, 64, 8, 4, 8192) == 8                 # 8 query tiles per KV head: 64 groups, 512 workgroups
    for Bq, T, Hkv, rep in ((1, 8, 8, 4), (1, 1, 12, 1), (8, 4, 8, 4)):
        s = plan(Bq, T, Hkv, rep, 8192)
        assert Bq * Hkv * ((T * rep + 31) // 32) * s >= 256 and 8192 // s >= 256, (Bq, T, Hkv, rep, s)
    # the planner's own multi-split choice on a cache long enough to be split
    T, H, Hkv, D, smax = 5, 8, 2, 128, 1024
    assert plan(1, T, Hkv, H // Hkv, smax) == 4
    t = AR.make_inputs(T, H, Hkv, D, [1000], [4], smax, seed=2)
    got = _run(T, H, Hkv, D, t, 0, DEV)
    assert bool(torch.isfinite(got.float()).all())
    close(got, _run(T, H, Hkv, D, t, 0, "cpu"))


def test_attn_append_unsupported_shapes_raise():
    T = 2
    t = AR.make_inputs(T, 4, 4, 96, [5, 9], None, SMAX)
    with pytest.raises(ValueError, match="head_dim"):
        _run(T, 4, 4, 96, t, 0, DEV)
    t = AR.make_inputs(T, 16, 1, 64, [5, 9], None, SMAX)            # rep = 16 > 8
    with pytest.raises(ValueError, match="Hkv"):
        _run(T, 16, 1, 64, t, 0, DEV)
    qkv, kbuf, vbuf, base, _ = (x if x is None else x.to(DEV) for x in AR.make_inputs(T, 4, 4, 64, [5, 9], None, SMAX))
    o = torch.zeros(B * T, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="int32"):
        ops.attn_append(qkv[:, :256], kbuf[:, :, PAD:], vbuf[:, :, PAD:], base.long(), None, o, T, 4, 4, 64)
    with pytest.raises(RuntimeError, match="16-byte"):  # a cache view that starts mid-vector
        ops.attn_append(qkv[:, :256], kbuf[:, :, 4:4 + 256], vbuf[:, :, PAD:], base, None, o, T, 4, 4, 64)
    assert float(o.float().abs().sum()) == 0            # nothing was launched
