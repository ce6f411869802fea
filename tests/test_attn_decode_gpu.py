"""Split-KV decode attention (csrc/kernels/attention_decode.hip) against the op's CPU f32
path on the same bf16 inputs, at the forward tolerance of test_attention_fwd_bwd.

Shapes are the smallest that reach every path: rep = H / Hkv of 1, 4 and 8, both head dims,
one / three forced splits and the planner's choice, and per-sequence lengths that give a
single key, fewer keys than one wave's group beside a partial last chunk, one key past a
chunk edge (whole splits empty for the other sequence) and a full cache.  q and o are
strided slices of wider buffers and the caches carry leading columns, as in the model;
cache rows at positions >= lens[b] hold NaN and must never reach a result."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, SMAX, PAD = 2, 384, 8


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def close(a, b, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol, rtol=rtol)


def _inputs(H, Hkv, D, lens, smax=SMAX, seed=0):
    """CPU bf16 tensors in the model's layout: q = the leading columns of a packed qkv row,
    caches behind PAD leading columns, rows >= lens[b] poisoned."""
    g = torch.Generator().manual_seed(seed)
    nb = len(lens)
    qkv = torch.randn(nb, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    kbuf = torch.randn(nb, smax, PAD + Hkv * D, generator=g).to(torch.bfloat16)
    vbuf = torch.randn(nb, smax, PAD + Hkv * D, generator=g).to(torch.bfloat16)
    for b, n in enumerate(lens):
        kbuf[b, n:] = float("nan")
        vbuf[b, n:] = float("nan")
    return qkv, kbuf, vbuf, torch.tensor(lens, dtype=torch.int32)


def _run(H, Hkv, D, tensors, splits, dev):
    qkv, kbuf, vbuf, lens = (t.to(dev) for t in tensors)
    nb = qkv.shape[0]
    # the GPU output is a bf16 slice of a wider buffer; the CPU reference keeps f32
    obuf = torch.zeros(nb, H * D + 2 * PAD, device=dev, dtype=torch.bfloat16 if dev != "cpu" else torch.float32)
    o = obuf[:, PAD: PAD + H * D]
    ops.attn_decode(qkv[:, : H * D], kbuf[:, :, PAD:], vbuf[:, :, PAD:], lens, o, H, Hkv, D, splits=splits)
    assert float(obuf[:, :PAD].abs().sum()) == 0 and float(obuf[:, PAD + H * D:].abs().sum()) == 0
    return o


_REF = {}


def _ref(H, Hkv, D, lens):
    """CPU f32 reference, computed once per case and shared by the split variants."""
    key = (H, Hkv, D, tuple(lens))
    if key not in _REF:
        _REF[key] = _run(H, Hkv, D, _inputs(H, Hkv, D, lens), 0, "cpu")
    return _REF[key]


@pytest.mark.parametrize("lens", [[1, 1], [7, 300], [129, 5], [384, 257]])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1)])
def test_attn_decode_matches_reference(H, Hkv, D, splits, lens):
    got = _run(H, Hkv, D, _inputs(H, Hkv, D, lens), splits, DEV)
    assert bool(torch.isfinite(got.float()).all()), "a poisoned cache row reached the output"
    close(got, _ref(H, Hkv, D, lens))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1)])
def test_attn_decode_deterministic_and_split_invariant(H, Hkv, D):
    t = _inputs(H, Hkv, D, [129, 300], seed=1)
    for splits in (0, 1, 3):
        a, b = _run(H, Hkv, D, t, splits, DEV), _run(H, Hkv, D, t, splits, DEV)
        assert torch.equal(a, b), f"splits={splits}: two calls differ"
    close(_run(H, Hkv, D, t, 1, DEV), _run(H, Hkv, D, t, 3, DEV))


def test_attn_decode_planner():
    plan = ops.attn_decode_plan
    assert plan(2, 4, SMAX) == 1                     # a short cache is not split
    assert plan(64, 8, 1024) == 1                    # 512 (sequence, KV head) pairs fill the chip alone
    for Bq, Hkv in ((1, 12), (1, 8), (8, 8)):        # long caches, few pairs: cover the 256 CUs
        s = plan(Bq, Hkv, 8192)
        assert Bq * Hkv * s >= 256 and 8192 // s >= 256, (Bq, Hkv, s)
    # the planner's own multi-split choice on a cache long enough to be split
    H, Hkv, D, smax = 8, 2, 128, 1024
    assert plan(1, Hkv, smax) == 4
    t = _inputs(H, Hkv, D, [1000], smax=smax, seed=2)
    got = _run(H, Hkv, D, t, 0, DEV)
    assert bool(torch.isfinite(got.float()).all())
    close(got, _run(H, Hkv, D, t, 0, "cpu"))


def test_attn_decode_unsupported_shapes_raise():
    H, Hkv, D = 4, 4, 96
    t = _inputs(H, Hkv, D, [5, 9])
    with pytest.raises(ValueError, match="head_dim"):
        _run(H, Hkv, D, t, 0, DEV)
    t = _inputs(16, 1, 64, [5, 9])                   # rep = 16 > 8
    with pytest.raises(ValueError, match="Hkv"):
        _run(16, 1, 64, t, 0, DEV)
    qkv, kbuf, vbuf, lens = (x.to(DEV) for x in _inputs(4, 4, 64, [5, 9]))
    o = torch.zeros(2, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="int32"):
        ops.attn_decode(qkv[:, :256], kbuf[:, :, PAD:], vbuf[:, :, PAD:], lens.long(), o, 4, 4, 64)
    with pytest.raises(RuntimeError, match="16-byte"):  # a cache view that starts mid-vector
        ops.attn_decode(qkv[:, :256], kbuf[:, :, 4:4 + 256], vbuf[:, :, PAD:], lens, o, 4, 4, 64)
