"""The float64 references of tests/generate_refs.py against torch, the decision margin of
every listed sampler case, and the CPU (f32) paths of ops.sample / ops.rope_kv_append /
ops.embed_fwd(positions=) against those references."""
import math

import pytest
import torch

from mipipe import ops

import generate_refs as R


def _z(case, b):
    t = float(torch.tensor(case.temperature, dtype=torch.float32))
    return case.logits[b, : case.V].double() / t


def _untied(case):
    return not case.name.startswith("tie")


def test_every_case_has_the_margin():
    cases = R.sample_cases()
    assert len(cases) >= 50
    worst = min(cases, key=lambda c: c.margin())
    print(f"\n{len(cases)} cases, smallest margin {worst.margin():.3e} ({worst.name})")
    for c in cases:
        assert c.margin() >= R.MARGIN, (c.name, c.margin())
        assert int(c.tokens().max()) < c.V


def test_cases_cover_the_grid():
    cases = R.sample_cases()
    assert {(c.V, c.Vp) for c in cases} == set(R.SIZES)
    assert {c.top_k for c in cases} == {0, 1, 2, 40}
    assert {c.temperature for c in cases} >= {0.0, 0.7, 1.5}
    assert {c.B for c in cases} == {1, 5}
    assert any(c.top_p < 1 for c in cases) and any(c.top_p == 1 for c in cases)
    assert all(bool((c.logits[:, c.V:] == R.PAD_LOGIT).all()) for c in cases)
    assert all(torch.equal(c.logits, c.logits.bfloat16().float()) for c in cases)
    assert all(0.0 <= float(x) < 1.0 for c in cases for x in c.u)


def test_sample_ref_matches_torch():
    for c in R.sample_cases():
        for b in range(c.B):
            tok, _, keep = c.ref()[b]
            if c.temperature == 0:
                assert tok == int(c.logits[b, : c.V].argmax()), c.name
                continue
            z = _z(c, b)
            p = torch.softmax(z, -1)
            # the top-k set: softmax + topk, ties at the threshold kept whole
            kset = torch.ones(c.V, dtype=torch.bool)
            if 0 < c.top_k < c.V:
                kset = p >= torch.topk(p, c.top_k).values[-1]
                if _untied(c):
                    assert int(kset.sum()) == c.top_k, c.name
            if c.top_p == 1.0:
                assert torch.equal(keep, kset), c.name
            pk = torch.where(kset, p, torch.zeros_like(p))
            pk = pk / pk.sum()
            if c.top_p < 1.0 and _untied(c):
                # sort-based nucleus: the smallest prefix of the sorted tokens with mass >= top_p
                sp, si = torch.sort(pk, descending=True)
                before = sp.cumsum(0) - sp
                nuc = torch.zeros(c.V, dtype=torch.bool)
                nuc[si[before < c.top_p]] = True
                assert torch.equal(keep, nuc & kset), c.name
            # the draw: inverse CDF over the kept set in index order
            pf = torch.where(keep, p, torch.zeros_like(p))
            cdf = (pf / pf.sum()).cumsum(0)
            want = int(torch.searchsorted(cdf, torch.tensor(float(c.u[b]), dtype=torch.float64), right=True))
            assert tok == want and bool(keep[tok]), (c.name, b, tok, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_sample_cpu_matches_reference(dtype):
    for c in R.sample_cases():
        got = ops.sample(c.logits.to(dtype), c.V, c.u, c.temperature, c.top_k, c.top_p)
        assert got.dtype == torch.int64 and torch.equal(got, c.tokens()), (c.name, got, c.tokens())


def test_ops_sample_cpu_done_and_stop():
    c = next(x for x in R.sample_cases() if x.B == 5 and x.temperature > 0 and x.V == 60)
    want = c.tokens()
    stop = int(want[1])
    done = torch.tensor([0, 0, 1, 0, 0], dtype=torch.uint8)
    out = torch.full((5,), -7, dtype=torch.int64)
    ops.sample(c.logits, c.V, c.u, c.temperature, c.top_k, c.top_p, done=done, stop_token=stop, pad_token=9, out=out)
    exp = want.clone()
    exp[2] = 9
    assert torch.equal(out, exp)
    assert done.tolist() == [int(t == stop) for t in want[:2].tolist()] + [1] + [int(t == stop) for t in want[3:].tolist()]
    with pytest.raises(ValueError):
        ops.sample(c.logits, c.V, c.u, 1.0, 0, 0.0)
    with pytest.raises(ValueError):
        ops.sample(c.logits, c.Vp + 1, c.u, 1.0)
    with pytest.raises(ValueError):
        ops.sample(c.logits, c.V, c.u[:3], 1.0)
    with pytest.raises(ValueError):
        ops.sample(c.logits, c.V, c.u, -1.0)


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("H,Hkv,Dh", [(4, 4, 16), (8, 2, 64)])
def test_ops_rope_kv_append_cpu_matches_reference(rope, H, Hkv, Dh):
    B, Smax = 4, 24
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, (H + 2 * Hkv) * Dh, generator=g)
    cos, sin = ops.rope_tables(Smax, Dh, 10000.0, "cpu")
    pos = torch.tensor([0, Smax - 1, 7, Smax + 5], dtype=torch.int32)       # the last one is clamped
    active = torch.tensor([1, 1, 0, 1], dtype=torch.uint8)
    kc = torch.full((B, Smax, Hkv * Dh), 5.0)
    vc = torch.full((B, Smax, Hkv * Dh), 6.0)
    q_ref, k_ref, v_ref, p = R.rope_kv_append_ref(qkv, cos, sin, pos, Smax, H, Hkv, Dh, rope)
    before = qkv.clone()
    ops.rope_kv_append(qkv, cos, sin, kc, vc, pos, active, H, Hkv, Dh, rope=rope)
    assert p.tolist() == [0, Smax - 1, 7, Smax - 1]
    for b in range(B):
        if not active[b]:
            assert torch.equal(qkv[b], before[b])
            assert bool((kc[b] == 5.0).all()) and bool((vc[b] == 6.0).all())
            continue
        torch.testing.assert_close(qkv[b, : H * Dh].double(), q_ref[b], atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(kc[b, p[b]].double(), k_ref[b], atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(vc[b, p[b]].double(), v_ref[b], atol=0, rtol=0)
        assert torch.equal(qkv[b, H * Dh:], before[b, H * Dh:])              # k / v columns stay
        rest = torch.ones(Smax, dtype=torch.bool)
        rest[p[b]] = False
        assert bool((kc[b][rest] == 5.0).all()) and bool((vc[b][rest] == 6.0).all())
    if rope:                                          # the rotation is rope_'s at pos_offset = pos[b]
        for b in (0, 1):
            one = before[b:b + 1].clone()
            ops.rope_(one, cos, sin, 1, H, Hkv, Dh, pos_offset=int(p[b]))
            assert torch.equal(one[0, : H * Dh], qkv[b, : H * Dh])
            assert torch.equal(one[0, H * Dh:(H + Hkv) * Dh], kc[b, p[b]])
    with pytest.raises(ValueError):
        ops.rope_kv_append(qkv, cos, sin, kc, vc, pos.long(), active, H, Hkv, Dh, rope=rope)
    with pytest.raises(ValueError):
        ops.rope_kv_append(qkv, cos, sin, kc, vc, pos, active[:2], H, Hkv, Dh, rope=rope)
    if rope:
        with pytest.raises(ValueError):
            ops.rope_kv_append(qkv, cos[:5], sin[:5], kc, vc, pos, active, H, Hkv, Dh)


@pytest.mark.parametrize("with_wpe", [True, False])
def test_ops_embed_positions_cpu(with_wpe):
    g = torch.Generator().manual_seed(4)
    wte, wpe = torch.randn(20, 16, generator=g), torch.randn(12, 16, generator=g)
    idx = torch.tensor([3, 19, 0, 7])
    pos = torch.tensor([0, 11, 5, 5], dtype=torch.int32)
    got = ops.embed_fwd(idx, wte, wpe if with_wpe else None, 1, positions=pos)
    for b in range(4):
        one = ops.embed_fwd(idx[b:b + 1], wte, wpe if with_wpe else None, 1, pos_offset=int(pos[b]))
        assert torch.equal(got[b:b + 1], one)
    with pytest.raises(ValueError):
        ops.embed_fwd(idx, wte, wpe, 1, positions=pos.long())
    assert math.isfinite(float(got.sum()))
