"""The quantising K/V append (csrc/kernels/attention_kv8.hip: rope_kv_append into int8 caches)
against the bf16 append of generate.hip: the int8 rows it writes are ``kv_quantize`` of the rows
the bf16 kernel writes, bit for bit, all W bytes of a row (payload, scales, zero padding); the q
columns are the bf16 path's bits; nothing else is touched.

B = 2, Smax = 16, caches as views behind 16 leading pad bytes of a wider buffer filled with a
canary byte.  Rope on / off, both head dims, rep of 1, 4 and 2 with Hkv = 3 (12 scale bytes and
real padding), T = 1 and T = 3 with counts = [3, 1], an active mask, and a position past the end
that clamps to Smax - 1."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, SMAX, PADB = 2, 16, 16
G = ops.generate


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


@pytest.mark.parametrize("active", [None, [1, 0]])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (6, 3)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rope", [True, False])
def test_int8_append_is_kv_quantize_of_the_bf16_append(rope, D, H, Hkv, T, active):
    W = G.kv8_row_bytes(Hkv, D)
    g = torch.Generator().manual_seed(T * 100 + D + H)
    qkv = torch.randn(B * T, (H + 2 * Hkv) * D, generator=g).to(torch.bfloat16).to(DEV)
    qkv[0, (H + 1) * D:(H + 2) * D] = 0                                   # a zero K head
    cos, sin = ops.rope_tables(SMAX, D, 10000.0, DEV)
    pos = torch.tensor([2, SMAX + 5], dtype=torch.int32, device=DEV)      # the second clamps to Smax - 1
    counts = None if T == 1 else torch.tensor([3, 1], dtype=torch.int32, device=DEV)
    act = None if active is None else torch.tensor(active, dtype=torch.uint8, device=DEV)

    canary = 9.0
    kf = torch.full((B, SMAX, Hkv * D), canary, dtype=torch.bfloat16, device=DEV)
    vf = torch.full((B, SMAX, Hkv * D), canary, dtype=torch.bfloat16, device=DEV)
    q_bf = qkv.clone()
    ops.rope_kv_append(q_bf, cos, sin, kf, vf, pos, act, H, Hkv, D, rope=rope, T=T, counts=counts)

    kbuf = torch.full((B, SMAX, W + 2 * PADB), 0x5A, dtype=torch.int8, device=DEV)
    vbuf = torch.full((B, SMAX, W + 2 * PADB), 0x5A, dtype=torch.int8, device=DEV)
    k8, v8 = kbuf[:, :, PADB:PADB + W], vbuf[:, :, PADB:PADB + W]
    q_i8 = qkv.clone()
    ops.rope_kv_append(q_i8, cos, sin, k8, v8, pos, act, H, Hkv, D, rope=rope, T=T, counts=counts)
    torch.cuda.synchronize()

    assert torch.equal(q_i8.view(torch.int16), q_bf.view(torch.int16)), "q columns differ from the bf16 path"
    written = (vf != canary).any(-1)
    want_rows = sum(T if counts is None else int(counts[b]) for b in range(B) if active is None or active[b])
    assert int(written.sum()) == want_rows
    assert bool(written[0, 2]) and (active is not None or bool(written[1, SMAX - 1]))
    for got, flt, buf in ((k8, kf, kbuf), (v8, vf, vbuf)):
        want = G.kv_quantize(flt[written], Hkv, D)
        assert torch.equal(got[written], want), "int8 rows are not kv_quantize of the bf16 rows"
        assert int(got[written][:, : Hkv * D].min()) >= -127
        assert bool((got[~written] == 0x5A).all()), "a skipped row was touched"
        assert bool((buf[:, :, :PADB] == 0x5A).all()) and bool((buf[:, :, PADB + W:] == 0x5A).all())


def test_int8_append_argument_checks():
    H, Hkv, D = 4, 4, 64
    W = G.kv8_row_bytes(Hkv, D)
    qkv = torch.zeros(B, (H + 2 * Hkv) * D, dtype=torch.bfloat16, device=DEV)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    buf = torch.zeros(B, SMAX, W + 32, dtype=torch.int8, device=DEV)
    good = buf[:, :, 16:16 + W]
    with pytest.raises(ValueError, match="int8"):                 # a last dimension that is not W
        ops.rope_kv_append(qkv, None, None, buf[:, :, : Hkv * D], buf[:, :, : Hkv * D], pos, None, H, Hkv, D, rope=False)
    with pytest.raises(RuntimeError, match="16-byte"):            # a view that starts mid-vector
        ops.rope_kv_append(qkv, None, None, buf[:, :, 8:8 + W], good, pos, None, H, Hkv, D, rope=False)
    with pytest.raises(ValueError, match="int8"):                 # one int8 cache, one bf16
        ops.rope_kv_append(qkv, None, None, good, torch.zeros(B, SMAX, Hkv * D, dtype=torch.bfloat16, device=DEV), pos,
                           None, H, Hkv, D, rope=False)
    with pytest.raises(ValueError, match="head_dim"):
        ops.rope_kv_append(torch.zeros(B, 3 * 4 * 96, dtype=torch.bfloat16, device=DEV), None, None, good, good, pos,
                           None, 4, 4, 96, rope=False)
    assert int(buf.abs().sum()) == 0                              # nothing was launched
