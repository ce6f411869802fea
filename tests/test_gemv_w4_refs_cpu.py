"""The int4g128 weight-only format, the CPU branches of its ops and the check of gemv_w4_refs.py.

* ``ops.quantize_w4`` equals the independent ``quantize_ref`` bit for bit (zero group, ties,
  bf16 and f32 inputs; CPU against GPU in the one test marked ``gpu``), rejects K % 128 != 0,
  and ``|w - What| <= scale / 2``.
* Packing: hand-written bytes, nibble 0 included, decode as ``nibble - 8`` through
  ``ops.dequant_w4`` and ``ops.linear_w4`` on the CPU.
* The CPU branches of ``ops.linear_skinny_w4`` / ``ops.linear_w4`` against the float64 reference.
* The check of gemv_w4_refs.py passes on the correctly rounded result and fails on six wrong
  ones: the metric on random inputs, bit-exactness on the exact-input case.
* ``gemv_plan`` with the weight code 0, and the codes 1 and 2 as they were before it."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_refs as GR
import gemv_w4_refs as W4

BF16 = torch.bfloat16


# ------------------------------------------------------------------ quantize_w4
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_quantize_w4_equals_reference(dtype):
    g = torch.Generator().manual_seed(1)
    N, K = 40, 384
    w = (torch.randn(N, K, generator=g) * torch.rand(N, 1, generator=g)).to(dtype)
    w[3, 128:256] = 0
    w[5] = 0
    q4, scale = ops.quantize_w4(w)
    assert q4.dtype == torch.uint8 and q4.shape == (N, K // 2) and q4.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (K // 128, N) and scale.is_contiguous()
    q4r, sr = W4.quantize_ref(w)
    assert torch.equal(q4, q4r) and torch.equal(scale, sr)
    wf = w.float()
    assert torch.equal(scale, (wf.view(N, 3, 128).abs().amax(2) / 7.0).t())
    q = W4.unpack(q4)
    # the quantiser never writes nibble 0; a group's maximum maps to +-7 with its sign
    assert float(q.min()) >= -7 and float(q.max()) <= 7
    live = (scale > 0).t()                                            # [N, G]
    assert torch.equal(q.view(N, 3, 128).abs().amax(2)[live], torch.full((int(live.sum()),), 7.0, dtype=torch.float64))
    imax = wf.view(N, 3, 128).abs().argmax(2, keepdim=True)
    assert torch.equal(torch.sign(q.view(N, 3, 128).gather(2, imax)).float(), torch.sign(wf.view(N, 3, 128).gather(2, imax)))
    # the zero groups: scale 0, q 0 (nibble 8)
    assert float(scale[1, 3]) == 0 and float(scale[:, 5].abs().sum()) == 0
    assert bool((q4[3, 64:128] == 0x88).all()) and bool((q4[5] == 0x88).all())
    # |w - What| <= scale / 2: round-to-nearest of w / scale, nothing clamped (|w| <= 7 scale).
    # The f32 roundings of scale and of the quotient move that by at most 2^-22 |w| (half an
    # ulp each of a value of magnitude <= |w|, doubled), as in the int8 test
    err = (wf.double() - W4.what(q4, scale)).abs()
    half = scale.double().t().repeat_interleave(128, dim=1) * 0.5
    assert bool((err <= half + 2.0 ** -22 * wf.double().abs()).all())


def test_quantize_w4_rounds_half_to_even_and_rejects_other_k():
    w = torch.zeros(1, 128)
    w[0, :8] = torch.tensor([7.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5])
    q4, scale = ops.quantize_w4(w)
    assert float(scale) == 1.0
    assert W4.unpack(q4)[0, :8].tolist() == [7, 0, 2, 2, 0, -2, -2, 4]
    assert torch.equal(q4, W4.quantize_ref(w)[0])
    for K in (64, 96, 192, 130):
        with pytest.raises(ValueError):
            ops.quantize_w4(torch.zeros(4, K))
    with pytest.raises(ValueError):
        ops.quantize_w4(torch.zeros(128))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_quantize_w4_same_on_cpu_and_gpu(dtype):
    assert torch.cuda.is_available(), "marked gpu: runs where there is one"
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(264, 2176, generator=g) * 0.02).to(dtype)
    w[5, 256:384] = 0
    q, s = ops.quantize_w4(w)
    qg, sg = ops.quantize_w4(w.cuda())
    assert torch.equal(q, qg.cpu()) and torch.equal(s, sg.cpu())


# ------------------------------------------------------------------ packing
def test_hand_built_bytes_decode_as_nibble_minus_8():
    """byte 0x0F is k = 0 -> nibble 15 (+7), k = 1 -> nibble 0 (-8); 0x80 is (-8, 0); ..."""
    N, K = 2, 128
    q4 = torch.full((N, K // 2), 0x88, dtype=torch.uint8)
    q4[0, 0], q4[0, 1], q4[0, 2], q4[0, 63] = 0x0F, 0x80, 0x79, 0xF0
    q4[1, 0] = 0x00
    scale = torch.tensor([[0.5, 2.0]])
    want = torch.zeros(N, K)
    want[0, 0:6] = torch.tensor([7.0, -8.0, -8.0, 0.0, 1.0, -1.0]) * 0.5
    want[0, 126:128] = torch.tensor([-8.0, 7.0]) * 0.5
    want[1, 0:2] = torch.tensor([-8.0, -8.0]) * 2.0
    assert torch.equal(ops.dequant_w4(q4, scale), want)
    assert torch.equal(W4.what(q4, scale), want.double())
    x = torch.arange(K, dtype=torch.float32)[None, :] / 4
    y = ops.linear_w4(x, q4, scale)
    assert torch.equal(y, x @ want.t())
    assert torch.equal(ops.linear_skinny_w4(x, q4, scale), y)


# ------------------------------------------------------------------ CPU branches
@pytest.mark.parametrize("epi", W4.EPIS)
@pytest.mark.parametrize("M", [1, 5, 16, 40])
def test_cpu_branches_match_reference(M, epi):
    N, K = 40, 384
    c = W4.randn_case(M, N, K, seed=M)
    x, bias, r = c.x.float(), c.bias.float(), c.r.float()
    kw = dict(bias=bias if "bias" in epi else None, act="gelu_tanh" if epi == "bias_gelu" else "none",
              residual=r if "res" in epi else None)
    ref = W4.w4_ref(x, c.q4, c.scale, epi, bias, r)
    outs = [ops.linear_w4(x, c.q4, c.scale, **kw)]
    if M <= 16:
        outs.append(ops.linear_skinny_w4(x, c.q4, c.scale, **kw))
    for y in outs:
        assert y.shape == (M, N) and y.dtype == torch.float32
        torch.testing.assert_close(y.double(), ref.out, atol=1e-5, rtol=1e-5)


def test_ops_argument_checks():
    c = W4.randn_case(17, 16, 128)
    x = c.x.float()
    with pytest.raises(ValueError):
        ops.linear_skinny_w4(x, c.q4, c.scale)                               # M > 16
    with pytest.raises(ValueError):
        ops.linear_w4(x[:, :64], c.q4[:, :32].contiguous(), c.scale)         # K % 128
    with pytest.raises(ValueError):
        ops.linear_w4(x, c.q4, c.scale.t().contiguous().view(-1))            # scale not [K / 128, N]
    with pytest.raises(ValueError):
        ops.linear_w4(x, c.q4.to(torch.int8), c.scale)                       # not packed uint8
    with pytest.raises(ValueError):
        ops.linear_w4(x, c.q4, c.scale, act="relu", bias=c.bias.float())
    with pytest.raises(ValueError):
        ops.dequant_w4(c.q4, c.scale[:, :8])
    assert torch.equal(ops.dequant_w4(c.q4, c.scale).double(), W4.what(c.q4, c.scale).float().double())


# ------------------------------------------------------------------ the check sees wrong results
def _fin(pre, epi, c):
    v = pre
    if "bias" in epi:
        v = v + c.bias.double()[None, :]
    if epi == "bias_gelu":
        v = GR.gelu_parts(v.to(BF16).double())[0]
    if "res" in epi:
        v = v + c.r.double()
    return v.to(BF16)


def _variants(c, epi):
    """name -> bf16 output: the right result and the six wrong ones"""
    x, q, s = c.x.double(), W4.unpack(c.q4), c.scale.double()         # s [G, N]
    M, K = x.shape
    N, G = q.shape[0], K // 128

    def grouped(qq, ss, groups=G):
        part = torch.einsum("mgk,ngk->gmn", x.view(M, G, 128)[:, :groups], qq.view(N, G, 128)[:, :groups])
        return (part * ss[:groups, None, :]).sum(0)

    out = {"right": _fin(grouped(q, s), epi, c)}
    out["nibbles_swapped"] = _fin(grouped(q.view(N, K // 2, 2).flip(2).reshape(N, K), s), epi, c)
    out["neighbour_group_scale"] = _fin(grouped(q, torch.roll(s, 1, 0)), epi, c)
    out["scale_indexed_n_g"] = _fin(grouped(q, s.reshape(-1).view(N, G).t()), epi, c)
    out["unsigned_nibble"] = _fin(grouped(q + 8.0, s), epi, c)
    out["last_group_dropped"] = _fin(grouped(q, s, G - 1), epi, c)
    out["scale_once_after_sum"] = _fin((x @ q.t()) * s[0][None, :], epi, c)
    return out


MUTATIONS = (("nibbles_swapped", "none"), ("neighbour_group_scale", "bias"), ("scale_indexed_n_g", "none"),
             ("unsigned_nibble", "bias"), ("last_group_dropped", "res"), ("scale_once_after_sum", "bias_res"),
             ("neighbour_group_scale", "bias_gelu"), ("last_group_dropped", "bias_gelu"), ("nibbles_swapped", "bias_gelu"))


def _passes(got, cr, ce, epi, which):
    """the whole check: the metric on the random case, bit-exactness on the exact one"""
    if which == "randn":
        return W4.check(got, W4.w4_ref(cr.x, cr.q4, cr.scale, epi, cr.bias, cr.r), epi)[2]
    wrong, safe = W4.check_exact(got, ce.v[epi], epi)
    assert safe > 0.9 * got.numel()
    return wrong == 0


@pytest.mark.parametrize("epi", W4.EPIS)
def test_check_passes_on_the_right_result(epi):
    M, N, K = 5, 40, 384
    cr, ce = W4.randn_case(M, N, K), W4.exact_case(M, N, K)
    assert _passes(_variants(cr, epi)["right"], cr, ce, epi, "randn")
    assert _passes(_variants(ce, epi)["right"], cr, ce, epi, "exact")
    err = W4.check(_variants(cr, epi)["right"], W4.w4_ref(cr.x, cr.q4, cr.scale, epi, cr.bias, cr.r), epi)[0]
    assert err <= 0.5 + 1e-9, err         # a correctly rounded result costs at most half a unit


@pytest.mark.parametrize("name,epi", MUTATIONS)
def test_check_fails_on_wrong_results(name, epi):
    M, N, K = 5, 40, 384
    cr, ce = W4.randn_case(M, N, K), W4.exact_case(M, N, K)
    ok_r = _passes(_variants(cr, epi)[name], cr, ce, epi, "randn")
    ok_e = _passes(_variants(ce, epi)[name], cr, ce, epi, "exact")
    print(f"\n{name} / {epi}: random-input metric {'passes' if ok_r else 'fails'}, "
          f"exact-input case {'passes' if ok_e else 'fails'}")
    assert not ok_r and not ok_e, f"{name} ({epi}) is not seen by both kinds of input"


def test_cases_have_what_they_promise():
    for (N, K) in W4.SHAPES:
        G = K // 128
        zr, zg = W4.zero_group(N, K)
        c = W4.randn_case(16, N, K)
        q = W4.unpack(c.q4).view(N, G, 128)
        live = (c.scale > 0).t()
        assert float(c.scale[zg, zr]) == 0 and int(live.sum()) == N * G - 1 and float(q[zr, zg].abs().sum()) == 0
        assert bool((q.abs().amax(2)[live] == 7).all()) and float(q.min()) == -7       # +-7 in every live group
        assert float(q[0].max()) == 7 and float(q[0].min()) == -7                      # both signs in row 0
        # the exact case: sums that do not fit bf16, an exact bf16 effective weight, scales
        # that differ per group and per row, O(1..64) values, and a GELU share of undetermined
        # elements under 10 %
        e = W4.exact_case(16, N, K)
        v = e.v["bias"]
        assert float((v.to(BF16).double() != v).double().mean()) > 0.25
        assert e.w_exact and float(e.scale[zg, zr]) == 0
        assert 1.0 <= float(v.abs().max()) <= 64.0
        assert len(set(e.scale[0, :6].tolist()) - {0.0}) >= 2 and (G == 1 or len(set(e.scale[:, 2].tolist())) >= 2)
        safe = W4.exact_expected(e.v["bias_gelu"], "bias_gelu")[1]
        assert float(safe.double().mean()) > 0.9, (N, K, float(safe.double().mean()))


# ------------------------------------------------------------------ the plan
def _plan():
    e = ops.load_ext()
    if e is None or not hasattr(e, "gemv_plan"):
        pytest.fail("the extension with gemv_plan must be built (python tools/build_ext.py)")
    return ops.gemv_plan


def test_gemv_plan_code_0():
    plan = _plan()
    for N, K in list(W4.SHAPES) + [W4.DEQUANT_SHAPE, (128256, 2048), (4096, 14336)]:
        rows, split = plan(N, K, 0)
        assert rows in (16, 32, 64) and 1 <= split <= (16 if rows == 16 else 8), (N, K, rows, split)
        assert (split - 1) * (rows // 16) * 1024 <= 64 * 1024          # the reduction's LDS
        assert plan(N, K, 0) == (rows, split)                          # nothing but (N, K)
        for f in W4.SPLITS:
            if f:
                assert plan(N, K, 0, f)[1] == f
    for args in ((16, 32, 0), (16, 96, 0), (16, 192, 0), (16, 0, 0), (0, 128, 0), (16, 128, 0, 17), (16, 128, 0, -1),
                 (16, 128, 3), (16, 128, -1)):
        with pytest.raises(RuntimeError):
            plan(*args)


def test_gemv_plan_codes_1_and_2_are_unchanged():
    """(rows, ksplit) of the int8 and bf16 instantiations as they were before the 4-bit code:
    literals, so a change of the planner for code 0 cannot move them unseen"""
    plan = _plan()
    want = {(16, 32): (16, 1), (8, 32): (16, 1), (40, 96): (16, 1), (264, 2080): (16, 8), (2304, 768): (16, 3),
            (768, 3072): (16, 12), (50304, 768): (64, 3), (3072, 2048): (16, 8), (16384, 2048): (32, 8),
            (2048, 8192): (16, 16), (128256, 2048): (64, 8), (28672, 4096): (32, 8), (4096, 14336): (16, 8),
            (16, 128): (16, 1), (40, 384): (16, 1), (264, 2176): (16, 8)}
    for (N, K), w in want.items():
        for code in (1, 2):
            assert plan(N, K, code) == w, (N, K, code, plan(N, K, code), w)
    assert plan(264, 2080, 1, 3) == (16, 3) and plan(128256, 2048, 2, 16) == (16, 16)
