"""The kernels of the ragged decode step (csrc/kernels/generate.hip) on the GPU.

* ``sample``: every case of tests/generate_refs.py must give the float64 reference's token
  exactly (each case's decision margin is >= 1e-4, above anything f32 summation can move:
  see that module), for bf16 and f32 logits and for a strided view, with the padded columns
  at +100; rows with -inf entries and a tied maximum are among the cases.  ``done`` /
  ``stop_token`` behaviour, a 5-sigma binomial test of the drawn distribution, and bitwise
  repeatability.
* ``rope_kv_append``: bit-identical to ``ops.rope_`` at ``S = 1, pos_offset = pos[b]``, within
  the bf16 bound of test_membound_edges_gpu.py of the float64 reference, writes exactly one
  row per active sequence (sentinel-filled caches, guard sequences before and after in the
  same allocation for out-of-range positions, which the kernel clamps), with and without RoPE.
* ``embed_fwd(positions=)``: bit-identical to ``embed_fwd`` at ``S = 1, pos_offset = p``.
* the bindings reject bad arguments before any launch.
"""
import pytest
import torch

from mipipe import ops

import generate_refs as R

pytestmark = pytest.mark.gpu


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


DEV = "cuda"


def _device_logits(case, variant):
    x = case.logits
    if variant == "bf16":
        return x.to(DEV, torch.bfloat16)
    if variant == "f32":
        return x.to(DEV)
    buf = torch.full((case.B, case.Vp + 64), R.PAD_LOGIT, device=DEV, dtype=torch.bfloat16)    # row stride > Vp
    buf[:, : case.Vp] = x.to(DEV, torch.bfloat16)
    return buf[:, : case.Vp]


@pytest.mark.parametrize("variant", ["bf16", "f32", "strided"])
def test_sample_matches_reference_exactly(variant):
    bad = []
    for c in R.sample_cases():
        lg = _device_logits(c, variant)
        assert variant != "strided" or lg.stride(0) > c.Vp
        got = ops.sample(lg, c.V, c.u.to(DEV), c.temperature, c.top_k, c.top_p).cpu()
        if not torch.equal(got, c.tokens()):
            bad.append((c.name, got.tolist(), c.tokens().tolist()))
    assert not bad, bad


def test_sample_tied_maximum():
    by = {c.name: c for c in R.sample_cases()}
    g, lo, hi = by["tie-greedy"], by["tie-k1-low"], by["tie-k1-high"]
    row = g.logits[0, : g.V]
    first, second = torch.nonzero(row == row.max())[:, 0].tolist()
    for dt in (torch.bfloat16, torch.float32):
        assert int(ops.sample(g.logits.to(DEV, dt), g.V, g.u.to(DEV))) == first
        # top_k = 1 keeps the whole tie: u picks between the two, in index order
        assert int(ops.sample(lo.logits.to(DEV, dt), lo.V, lo.u.to(DEV), 1.0, 1)) == first
        assert int(ops.sample(hi.logits.to(DEV, dt), hi.V, hi.u.to(DEV), 1.0, 1)) == second


def test_sample_done_and_stop_token():
    c = next(x for x in R.sample_cases() if x.B == 5 and x.temperature > 0 and x.V == 50257)
    want = c.tokens()
    lg, u = c.logits.to(DEV, torch.bfloat16), c.u.to(DEV)
    stop = int(want[1])
    done = torch.tensor([0, 0, 1, 0, 0], dtype=torch.uint8, device=DEV)
    out = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    ops.sample(lg, c.V, u, c.temperature, c.top_k, c.top_p, done=done, stop_token=stop, pad_token=9, out=out)
    exp = want.clone()
    exp[2] = 9                                       # a finished row writes pad_token and stays finished
    assert torch.equal(out.cpu(), exp)
    assert done.cpu().tolist() == [int(i == 2 or int(want[i]) == stop) for i in range(5)]
    # without a stop token nothing is marked
    done.zero_()
    ops.sample(lg, c.V, u, c.temperature, c.top_k, c.top_p, done=done, out=out)
    assert torch.equal(out.cpu(), want) and int(done.sum()) == 0


def test_sample_distribution_and_repeatability():
    V, Vp, n = 60, 64, 8192
    g = torch.Generator().manual_seed(12)
    row = torch.full((Vp,), R.PAD_LOGIT)
    row[:V] = 2.0 * torch.randn(V, generator=g)
    lg = row[None].expand(n, Vp).contiguous().to(DEV)
    u = torch.rand(n, generator=g).to(DEV)
    got = ops.sample(lg, V, u, 1.0)
    again = ops.sample(lg, V, u, 1.0)
    assert torch.equal(got, again)
    p = torch.softmax(row[:V].double(), -1)
    counts = torch.bincount(got.cpu(), minlength=V).double()
    assert counts.numel() == V and int(counts.sum()) == n
    sigma = torch.sqrt(n * p * (1 - p))
    worst = float(((counts - n * p).abs() / sigma).max())
    print(f"\nlargest deviation {worst:.2f} sigma over {V} tokens, {n} draws")
    assert bool(((counts - n * p).abs() <= 5 * sigma).all()), worst
    # the filtered path too, on a full-size row
    c = next(x for x in R.sample_cases() if x.V == 50257 and x.top_k == 40 and x.top_p < 1)
    big, ub = c.logits.to(DEV, torch.bfloat16), c.u.to(DEV)
    assert torch.equal(ops.sample(big, c.V, ub, c.temperature, c.top_k, c.top_p),
                       ops.sample(big, c.V, ub, c.temperature, c.top_k, c.top_p))


# ------------------------------------------------------------------------ rope_kv_append
SENT_K, SENT_V = -7.0, 9.0


def _bf16_close(got, ref, amax):
    return bool(((got.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6 * amax).all())


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("Dh", [64, 128])
def test_rope_kv_append(Dh, H, Hkv, rope):
    Smax = 24
    cos, sin = ops.rope_tables(Smax, Dh, 10000.0, DEV)
    g = torch.Generator().manual_seed(Dh + H)
    runs = [([0], None), ([Smax - 1], None), ([0, Smax - 1, 7], None), ([5, 11, 23], [1, 0, 1]),
            ([-3, Smax + 5, 11], None)]             # out of range: clamped to the sequence's own rows
    for pos_l, act_l in runs:
        B = len(pos_l)
        qkv0 = torch.randn(B, (H + 2 * Hkv) * Dh, generator=g).bfloat16()
        qkv = qkv0.to(DEV)
        # one guard sequence before and one after the cache, in the same allocation
        kbuf = torch.full((B + 2, Smax, Hkv * Dh), SENT_K, device=DEV, dtype=torch.bfloat16)
        vbuf = torch.full((B + 2, Smax, Hkv * Dh), SENT_V, device=DEV, dtype=torch.bfloat16)
        kc, vc = kbuf[1:B + 1], vbuf[1:B + 1]
        pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
        active = None if act_l is None else torch.tensor(act_l, dtype=torch.uint8, device=DEV)
        ops.rope_kv_append(qkv, cos, sin, kc, vc, pos, active, H, Hkv, Dh, rope=rope)
        q_ref, k_ref, v_ref, p = R.rope_kv_append_ref(qkv0, cos.cpu(), sin.cpu(), pos.cpu(), Smax, H, Hkv, Dh, rope)
        amax = float(qkv0.abs().max())
        kb, vb, out = kbuf.cpu(), vbuf.cpu(), qkv.cpu()
        assert bool((kb[0] == SENT_K).all() and (kb[-1] == SENT_K).all())          # the guards
        assert bool((vb[0] == SENT_V).all() and (vb[-1] == SENT_V).all())
        for b in range(B):
            krows, vrows = kb[1 + b], vb[1 + b]
            if act_l is not None and not act_l[b]:
                assert torch.equal(out[b], qkv0[b])
                assert bool((krows == SENT_K).all() and (vrows == SENT_V).all())
                continue
            pb = int(p[b])
            assert pb == min(max(pos_l[b], 0), Smax - 1)
            rest = torch.ones(Smax, dtype=torch.bool)
            rest[pb] = False
            assert bool((krows[rest] == SENT_K).all() and (vrows[rest] == SENT_V).all()), (pos_l, b)
            assert torch.equal(vrows[pb], qkv0[b, (H + Hkv) * Dh:])
            assert torch.equal(out[b, H * Dh:], qkv0[b, H * Dh:])                  # k / v columns stay
            assert _bf16_close(out[b, : H * Dh], q_ref[b], amax)
            assert _bf16_close(krows[pb], k_ref[b], amax)
            if rope:
                one = qkv0[b:b + 1].to(DEV)
                ops.rope_(one, cos, sin, 1, H, Hkv, Dh, pos_offset=pb)
                one = one.cpu()
                assert torch.equal(out[b, : H * Dh], one[0, : H * Dh]), (pos_l, b)
                assert torch.equal(krows[pb], one[0, H * Dh:(H + Hkv) * Dh]), (pos_l, b)
            else:
                assert torch.equal(out[b], qkv0[b])
                assert torch.equal(krows[pb], qkv0[b, H * Dh:(H + Hkv) * Dh])


@pytest.mark.parametrize("with_wpe", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_embed_positions(with_wpe, dtype):
    g = torch.Generator().manual_seed(6)
    wte = torch.randn(50, 72, generator=g).to(DEV, dtype)
    wpe = torch.randn(16, 72, generator=g).to(DEV, dtype) if with_wpe else None
    idx = torch.tensor([3, 49, 0, 7, 7, 21], device=DEV)
    pos_l = [0, 15, 5, 5, 9, 1]
    got = ops.embed_fwd(idx, wte, wpe, 1, positions=torch.tensor(pos_l, dtype=torch.int32, device=DEV))
    for b, p in enumerate(pos_l):
        assert torch.equal(got[b:b + 1], ops.embed_fwd(idx[b:b + 1], wte, wpe, 1, pos_offset=p)), b


# ------------------------------------------------------------------------- binding checks
def test_bindings_reject_bad_arguments():
    ext = ops.load_ext()
    err = (ValueError, RuntimeError)
    H, Hkv, Dh, Smax, B = 4, 2, 64, 8, 3
    cos, sin = ops.rope_tables(Smax, Dh, 10000.0, DEV)
    qkv = torch.zeros(B, (H + 2 * Hkv) * Dh, device=DEV, dtype=torch.bfloat16)
    kc = torch.zeros(B, Smax, Hkv * Dh, device=DEV, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    act = torch.ones(B, dtype=torch.uint8, device=DEV)

    def append(qkv=qkv, cos=cos, sin=sin, kc=kc, vc=vc, pos=pos, act=act):
        for fn in (ops.rope_kv_append, ext.rope_kv_append):
            with pytest.raises(err):
                fn(qkv, cos, sin, kc, vc, pos, act, H, Hkv, Dh, True)

    append(qkv=qkv.float())                          # wrong dtype
    append(kc=kc.float())
    append(pos=pos.long())
    append(act=act.bool())
    append(pos=pos.cpu())                            # wrong device
    append(act=act.cpu())
    append(pos=pos[:2])                              # wrong length
    append(act=act[:2])
    append(cos=cos[: Smax - 1], sin=sin[: Smax - 1])  # too few table rows
    with pytest.raises(err):
        ext.rope_kv_append(qkv, cos, sin, kc[:2], vc, pos, act, H, Hkv, Dh, True)
    with pytest.raises(err):
        ext.rope_kv_append(qkv, cos, sin, kc, vc, pos, act, H, Hkv, 32, True)
    assert int(kc.float().abs().sum()) == 0 and int(vc.float().abs().sum()) == 0      # nothing was launched

    lg = torch.zeros(B, 64, device=DEV, dtype=torch.bfloat16)
    u = torch.zeros(B, device=DEV)
    out = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    done = torch.zeros(B, dtype=torch.uint8, device=DEV)

    def smp(lg=lg, V=60, u=u, t=1.0, k=0, p=1.0, done=done, out=out):
        with pytest.raises(err):
            ops.sample(lg, V, u, t, k, p, done=done, out=out)
        with pytest.raises(err):
            ext.sample(lg, V, u, t, k, p, done, -1, 0, out)

    smp(lg=lg.half())                                # wrong dtype
    smp(u=u.double())
    smp(done=done.bool())
    smp(u=u.cpu())                                   # wrong device
    smp(lg=lg.cpu())
    smp(u=u[:2])                                     # wrong length
    smp(done=done[:2])
    smp(p=0.0)
    smp(p=1.5)
    smp(V=65)                                        # V > Vp
    smp(t=-1.0)
    smp(k=-1)
    assert out.cpu().tolist() == [-1] * B            # nothing was launched

    wte = torch.zeros(10, 64, device=DEV, dtype=torch.bfloat16)
    idx = torch.zeros(B, dtype=torch.int64, device=DEV)
    for bad in (pos.long(), pos.cpu(), pos[:2]):
        with pytest.raises(err):
            ops.embed_fwd(idx, wte, None, 1, positions=bad)
        with pytest.raises(err):
            ext.embed_pos(idx, bad, wte, None, torch.empty(B, 64, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(err):
        ext.embed_pos(idx, pos, wte.float(), None, torch.empty(B, 64, device=DEV, dtype=torch.bfloat16))
