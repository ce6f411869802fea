"""The int8 weight-only format, the CPU branches of its ops and the check of gemv_w8_refs.py.

* ``ops.quantize_w8``: the properties of the format, bf16 and f32 inputs, CPU against GPU
  (that one test is marked ``gpu``).
* The CPU branches of ``ops.linear_skinny`` / ``ops.linear_w8`` against the float64 reference.
* The check of gemv_w8_refs.py passes on the correctly rounded result and fails on eight
  wrong ones: the metric on random inputs, bit-exactness on the exact-input case.
* ``gemv_plan``: valid for every shape the GPU tests and tools/w8_time.py use, a function of
  its arguments only, ``force_split`` honoured."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_refs as GR
import gemv_w8_refs as WR

BF16 = torch.bfloat16


# ------------------------------------------------------------------ quantize_w8
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_quantize_w8_properties(dtype):
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(40, 96, generator=g) * torch.rand(40, 1, generator=g)).to(dtype)
    w[3] = 0
    q, scale = ops.quantize_w8(w)
    assert q.dtype == torch.int8 and q.shape == w.shape and q.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (40,)
    wf = w.float()
    assert torch.equal(scale, wf.abs().amax(1) / 127.0)
    # |w - q scale| <= scale / 2, to the f32 rounding of scale and of the quotient w / scale
    # (each half an ulp of a value of magnitude <= |w|: together 2^-23 |w|, doubled here)
    err = (wf.double() - q.double() * scale.double()[:, None]).abs()
    assert bool((err <= scale.double()[:, None] * 0.5 + 2.0 ** -22 * wf.double().abs()).all())
    # the row maximum maps to +-127, nothing leaves [-127, 127]
    imax = wf.abs().argmax(1)
    rows = torch.arange(40)
    live = scale > 0
    assert torch.equal(q[rows, imax][live].int().abs(), torch.full((int(live.sum()),), 127, dtype=torch.int32))
    assert torch.equal(torch.sign(q[rows, imax].float()), torch.sign(wf[rows, imax]))
    assert int(q.int().abs().max()) == 127 and int(q.int().min()) >= -127
    # the zero row
    assert float(scale[3]) == 0 and int(q[3].int().abs().sum()) == 0
    # the independent reference quantiser agrees
    q2, s2 = WR.quantize_ref(w)
    assert torch.equal(q, q2) and torch.equal(scale, s2)


def test_quantize_w8_rounds_half_to_even():
    w = torch.tensor([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5]])
    q, scale = ops.quantize_w8(w)
    assert float(scale) == 1.0
    assert q.tolist() == [[127, 0, 2, 2, 0, -2, -2, 64]]
    with pytest.raises(ValueError):
        ops.quantize_w8(torch.zeros(8))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_quantize_w8_same_on_cpu_and_gpu(dtype):
    assert torch.cuda.is_available(), "marked gpu: runs where there is one"
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(264, 2080, generator=g) * 0.02).to(dtype)
    w[5] = 0
    q, s = ops.quantize_w8(w)
    qg, sg = ops.quantize_w8(w.cuda())
    assert torch.equal(q, qg.cpu()) and torch.equal(s, sg.cpu())


# ------------------------------------------------------------------ CPU branches
@pytest.mark.parametrize("epi", WR.EPIS)
@pytest.mark.parametrize("M", [1, 5, 16, 40])
def test_cpu_branches_match_reference(M, epi):
    N, K = 40, 96
    c = WR.randn_case(M, N, K, seed=M)
    x, bias, r = c.x.float(), c.bias.float(), c.r.float()
    kw = dict(bias=bias if "bias" in epi else None, act="gelu_tanh" if epi == "bias_gelu" else "none",
              residual=r if "res" in epi else None)
    ref = WR.w8_ref(x, c.q, c.scale, epi, bias, r)
    outs = [ops.linear_w8(x, c.q, c.scale, **kw)]
    if M <= 16:
        outs.append(ops.linear_skinny(x, c.q, c.scale, **kw))
        refb = WR.bf16_ref(x, c.w, epi, bias, r)
        yb = ops.linear_skinny(x, c.w.float(), None, **kw)
        assert yb.shape == (M, N)
        torch.testing.assert_close(yb.double(), refb.out, atol=1e-5, rtol=1e-5)
    for y in outs:
        assert y.shape == (M, N) and y.dtype == torch.float32
        torch.testing.assert_close(y.double(), ref.out, atol=1e-5, rtol=1e-5)
        # the zero-scale row: exactly bias + residual
        z = min(1, N - 1)
        want = torch.zeros(M)
        if "bias" in epi:
            want = want + bias[z]
        if epi == "bias_gelu":
            want = torch.nn.functional.gelu(want, approximate="tanh")
        if "res" in epi:
            want = want + r[:, z]
        assert torch.equal(y[:, z], want)


def test_ops_argument_checks():
    c = WR.randn_case(17, 16, 32)
    x = c.x.float()
    with pytest.raises(ValueError):
        ops.linear_skinny(x, c.q, c.scale)                          # M > 16
    with pytest.raises(ValueError):
        ops.linear_skinny(x[:4, :24], c.q[:, :24].contiguous(), c.scale)      # K % 32
    with pytest.raises(ValueError):
        ops.linear_skinny(x[:4], c.q)                               # int8 without a scale
    with pytest.raises(ValueError):
        ops.linear_skinny(x[:4], c.w.float(), c.scale)              # a scale without int8
    with pytest.raises(ValueError):
        ops.linear_w8(x, c.q, c.scale, act="relu", bias=c.bias.float())
    assert ops.W8_SKINNY_MAX_M >= 16 and ops.SKINNY_MAX_M == 16
    w = ops.dequant_w8(c.q, c.scale)
    assert torch.equal(w, c.q.float() * c.scale[:, None])


# ------------------------------------------------------------------ the check sees wrong results
def _epilogue(pre, epi, bias, r, round_pre=True, add_bias=True):
    """float64 epilogue of a pre-bias value, as the kernel orders it"""
    v = pre
    if "bias" in epi and add_bias:
        v = v + bias.double()[None, :]
    if epi == "bias_gelu":
        v = GR.gelu_parts(v.to(BF16).double() if round_pre else v)[0]
    if "res" in epi:
        v = v + r.double()
    return v


def _variants(c, epi):
    """name -> bf16 output: the right result and the eight wrong ones"""
    x, q, s, K = c.x.double(), c.q.double(), c.scale.double(), c.x.shape[1]
    M = x.shape[0]
    acc = x @ q.t()
    fin = lambda pre, **k: _epilogue(pre, epi, c.bias, c.r, **k).to(BF16)   # noqa: E731
    out = {"right": fin(acc * s)}
    out["neighbour_scale"] = fin(acc * torch.roll(s, 1))
    out["uint8"] = fin((x @ (q + 256.0 * (q < 0)).t()) * s)
    out["last_kstep_dropped"] = fin((x[:, : K - 32] @ q[:, : K - 32].t()) * s)
    out["bias_before_scale"] = fin((acc + c.bias.double()[None, :]) * s, add_bias=False)
    out["residual_twice"] = (_epilogue(acc * s, epi, c.bias, c.r) + c.r.double()).to(BF16)
    out["next_x_row"] = fin(torch.roll(x, -1, 0) @ q.t() * s) if M > 1 else None
    out["scale_after_rounding"] = fin(acc.to(BF16).double() * s)
    out["gelu_unrounded"] = fin(acc * s, round_pre=False)
    return out


# which epilogue shows which mutation (a residual mutation needs a residual, ...)
MUTATIONS = (("neighbour_scale", "none"), ("uint8", "bias"), ("last_kstep_dropped", "res"),
             ("bias_before_scale", "bias"), ("bias_before_scale", "bias_res"), ("residual_twice", "bias_res"),
             ("residual_twice", "res"), ("next_x_row", "none"), ("scale_after_rounding", "bias"),
             ("gelu_unrounded", "bias_gelu"), ("neighbour_scale", "bias_gelu"), ("last_kstep_dropped", "bias_gelu"))


def _passes(got, c_rand, c_exact, epi, which):
    """the whole check: the metric on the random case, bit-exactness on the exact one"""
    if which == "randn":
        return WR.check(got, WR.w8_ref(c_rand.x, c_rand.q, c_rand.scale, epi, c_rand.bias, c_rand.r), epi)[2]
    wrong, safe = WR.check_exact(got, c_exact.v[epi], epi)
    assert safe > 0.9 * got.numel()
    return wrong == 0


@pytest.mark.parametrize("epi", WR.EPIS)
def test_check_passes_on_the_right_result(epi):
    M, N, K = 5, 40, 96
    cr, ce = WR.randn_case(M, N, K), WR.exact_case(M, N, K)
    assert _passes(_variants(cr, epi)["right"], cr, ce, epi, "randn")
    assert _passes(_variants(ce, epi)["right"], cr, ce, epi, "exact")
    err = WR.check(_variants(cr, epi)["right"], WR.w8_ref(cr.x, cr.q, cr.scale, epi, cr.bias, cr.r), epi)[0]
    assert err <= 0.5 + 1e-9, err         # a correctly rounded result costs at most half a unit


@pytest.mark.parametrize("name,epi", MUTATIONS)
def test_check_fails_on_wrong_results(name, epi):
    M, N, K = 5, 40, 96
    cr, ce = WR.randn_case(M, N, K), WR.exact_case(M, N, K)
    ok_r = _passes(_variants(cr, epi)[name], cr, ce, epi, "randn")
    ok_e = _passes(_variants(ce, epi)[name], cr, ce, epi, "exact")
    print(f"\n{name} / {epi}: random-input metric {'passes' if ok_r else 'fails'}, "
          f"exact-input case {'passes' if ok_e else 'fails'}")
    assert not (ok_r and ok_e), f"{name} ({epi}) is not seen"
    if name in ("scale_after_rounding", "gelu_unrounded"):
        assert not ok_e, "a second rounding must show in the exact-input case"


def test_exact_case_needs_more_than_eight_bits():
    """the exact case is only a test of the rounding order if its sums do not fit bf16"""
    for (N, K) in WR.SHAPES:
        c = WR.exact_case(16, N, K)
        v = c.v["bias"]
        assert float((v.to(BF16).double() != v).double().mean()) > 0.25      # plenty of sums are rounded
        assert c.w_exact and float(c.scale[min(1, N - 1)]) == 0
        assert 1.0 <= float(v.abs().max()) <= 64.0


# ------------------------------------------------------------------ the plan
def _plan():
    e = ops.load_ext()
    if e is None or not hasattr(e, "gemv_plan"):
        pytest.fail("the extension with gemv_plan must be built (python tools/build_ext.py)")
    return ops.gemv_plan


def test_gemv_plan_valid_for_every_shape_in_use():
    plan = _plan()
    shapes = list(WR.SHAPES) + [WR.DEQUANT_SHAPE] + [s for v in WR.MODEL_SHAPES.values() for s in v]
    for N, K in shapes:
        for wbytes in (1, 2):
            rows, split = plan(N, K, wbytes)
            assert rows in (16, 32, 64) and 1 <= split <= (16 if rows == 16 else 8), (N, K, rows, split)
            assert 64 * split <= (1024 if rows == 16 else 512)
            assert (split - 1) * (rows // 16) * 1024 <= 64 * 1024          # the reduction's LDS
            assert plan(N, K, wbytes) == (rows, split)                      # nothing but its arguments
            for f in WR.SPLITS:
                if f:
                    assert plan(N, K, wbytes, f)[1] == f
    # large N takes whole 64-row workgroups, small N 16-row ones
    assert plan(128256, 2048, 1)[0] == 64 and plan(768, 768, 1)[0] == 16


def test_gemv_plan_rejects_what_the_kernel_cannot_run():
    plan = _plan()
    for args in ((16, 48, 1), (16, 0, 1), (0, 32, 1), (16, 32, 4), (16, 32, 1, 17), (16, 32, 1, -1)):
        with pytest.raises(RuntimeError):
            plan(*args)
