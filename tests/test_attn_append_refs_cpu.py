"""The CPU (f32) paths of ops.attn_append and of the T-token ops.rope_kv_append against
float64 references: attn_append_refs.attn_append_ref (one explicit masked softmax per
(sequence, token, head)) on the cases of test_attn_append_gpu.py, and
generate_refs.rope_kv_append_ref applied token by token."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import attn_append_refs as AR
import generate_refs as R

SMAX = 384


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("T", [1, 2, 5, 33])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (8, 1)])
def test_attn_append_cpu_matches_reference(H, Hkv, D, T, case):
    base, counts = AR.bases_counts(T, SMAX)[case]
    qkv, kbuf, vbuf, bs, cnt = AR.make_inputs(T, H, Hkv, D, base, counts, SMAX)
    qkv, kbuf, vbuf = qkv.float(), kbuf.float(), vbuf.float()
    obuf = torch.full((2 * T, H * D + 2 * AR.PAD), 7.0)
    o = obuf[:, AR.PAD: AR.PAD + H * D]
    ops.attn_append(qkv[:, : H * D], kbuf[:, :, AR.PAD:], vbuf[:, :, AR.PAD:], bs, cnt, o, T, H, Hkv, D)
    ref = AR.attn_append_ref(qkv, kbuf[:, :, AR.PAD:], vbuf[:, :, AR.PAD:], base, counts, T, H, Hkv, D)
    assert bool(torch.isfinite(o).all())
    torch.testing.assert_close(o.double(), ref, atol=1e-5, rtol=1e-5)
    assert bool((obuf[:, : AR.PAD] == 7.0).all() and (obuf[:, AR.PAD + H * D:] == 7.0).all())
    for b in range(2):
        c = T if counts is None else counts[b]
        assert float(o[b * T + c:(b + 1) * T].abs().sum()) == 0


def test_attn_append_cpu_clamps_and_rejects():
    H, Hkv, D, T, smax = 4, 2, 16, 3, 10
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2 * T, H * D, generator=g)
    kc, vc = torch.randn(2, smax, Hkv * D, generator=g), torch.randn(2, smax, Hkv * D, generator=g)
    o = torch.zeros(2 * T, H * D)
    base, counts = [9, -4], [3, 7]                     # clamped: one token fits; base 0, all T
    ops.attn_append(q, kc, vc, torch.tensor(base, dtype=torch.int32), torch.tensor(counts, dtype=torch.int32), o, T,
                    H, Hkv, D)
    ref = AR.attn_append_ref(q, kc, vc, base, counts, T, H, Hkv, D)
    torch.testing.assert_close(o.double(), ref, atol=1e-5, rtol=1e-5)
    assert float(ref[1:T].abs().sum()) == 0 and float(ref[T:].abs().sum()) > 0
    with pytest.raises(ValueError, match="int32"):
        ops.attn_append(q, kc, vc, torch.tensor(base), None, o, T, H, Hkv, D)
    with pytest.raises(ValueError, match="int32"):
        ops.attn_append(q, kc, vc, torch.tensor(base, dtype=torch.int32), torch.tensor(counts), o, T, H, Hkv, D)
    with pytest.raises(ValueError, match="rows"):
        ops.attn_append(q[:-1], kc, vc, torch.tensor(base, dtype=torch.int32), None, o, T, H, Hkv, D)
    with pytest.raises(ValueError, match="Hkv"):
        ops.attn_append(q, kc, vc, torch.tensor(base, dtype=torch.int32), None, o, T, 3, 2, D)


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("H,Hkv,Dh", [(4, 4, 16), (8, 2, 64)])
def test_rope_kv_append_T_tokens_cpu_matches_reference(rope, H, Hkv, Dh):
    Smax, T = 24, 5
    cos, sin = ops.rope_tables(Smax, Dh, 10000.0, "cpu")
    g = torch.Generator().manual_seed(Dh + H)
    for base, counts, act in (([0, 7, 19], None, None), ([3, 19, 0], [5, 2, 0], None), ([19, 4, 9], [5, 5, 1], [1, 0, 1])):
        B = len(base)
        qkv0 = torch.randn(B * T, (H + 2 * Hkv) * Dh, generator=g)
        qkv = qkv0.clone()
        kc = torch.full((B, Smax, Hkv * Dh), -7.0)
        vc = torch.full((B, Smax, Hkv * Dh), 9.0)
        ops.rope_kv_append(qkv, cos, sin, kc, vc, torch.tensor(base, dtype=torch.int32),
                           None if act is None else torch.tensor(act, dtype=torch.uint8), H, Hkv, Dh, rope=rope, T=T,
                           counts=None if counts is None else torch.tensor(counts, dtype=torch.int32))
        written = torch.zeros(B, Smax, dtype=torch.bool)
        for b in range(B):
            c = T if counts is None else counts[b]
            if act is not None and not act[b]:
                c = 0
            for t in range(T):
                n = b * T + t
                if t >= c:
                    assert torch.equal(qkv[n], qkv0[n])
                    continue
                # the one-token reference at this token's position
                q_ref, k_ref, v_ref, p = R.rope_kv_append_ref(qkv0[n:n + 1], cos, sin, torch.tensor([base[b] + t]),
                                                              Smax, H, Hkv, Dh, rope)
                pb = int(p[0])
                assert pb == min(base[b] + t, Smax - 1)
                written[b, pb] = True
                torch.testing.assert_close(qkv[n, : H * Dh].double(), q_ref[0], atol=1e-5, rtol=1e-5)
                assert torch.equal(qkv[n, H * Dh:], qkv0[n, H * Dh:])
                torch.testing.assert_close(kc[b, pb].double(), k_ref[0], atol=1e-5, rtol=1e-5)
                torch.testing.assert_close(vc[b, pb].double(), v_ref[0], atol=0, rtol=0)
        assert bool((kc[~written] == -7.0).all() and (vc[~written] == 9.0).all())
    # T = 1 is the existing op
    qkv = torch.randn(3, (H + 2 * Hkv) * Dh, generator=g)
    a, b = qkv.clone(), qkv.clone()
    ka, va, kb, vb = (torch.zeros(3, Smax, Hkv * Dh) for _ in range(4))
    pos = torch.tensor([0, 23, 7], dtype=torch.int32)
    ops.rope_kv_append(a, cos, sin, ka, va, pos, None, H, Hkv, Dh, rope=rope)
    ops.rope_kv_append(b, cos, sin, kb, vb, pos, None, H, Hkv, Dh, rope=rope, T=1,
                       counts=torch.ones(3, dtype=torch.int32))
    assert torch.equal(a, b) and torch.equal(ka, kb) and torch.equal(va, vb)
    with pytest.raises(ValueError):
        ops.rope_kv_append(qkv, cos, sin, ka, va, pos, None, H, Hkv, Dh, rope=rope, T=2)
    with pytest.raises(ValueError):
        ops.rope_kv_append(qkv, cos, sin, ka, va, pos, None, H, Hkv, Dh, rope=rope, counts=torch.ones(3))
