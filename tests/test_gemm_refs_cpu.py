"""The float64 GEMM reference of gemm_refs.py and the teeth of its check, on the CPU.

1. The reference against torch.matmul in float64 with torch.nn.functional.gelu(approximate=
   "tanh") and its autograd derivatives, for every epilogue, layout, alpha, accumulate and
   column sum, from row-strided views; and against the CPU branches of ops.linear, linear_dx,
   linear_dw and run_wjobs within the recorded bounds.
2. Twelve mutations of a correct result (a dropped K element or K-tile, a slab added twice,
   alpha missing on one split, a shifted bias, swapped rows, a transposed sub-block, a lost C0,
   a pre-activation rounded after the activation, column sums short of a row, truncated f32
   inputs, a residual read with the wrong row stride): each must fail at the recorded BOUND,
   and the unmutated result must pass.
3. The inputs the GPU test uses keep ReLU's sign-uncertain elements under UNSURE_CAP, the exact
   inputs are exact, and the tables are complete: every key a case can reach has a BOUND and
   an OLD_TOL, the one-rounding bf16 keys are <= 1.0."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_refs as R

BF16, F32 = torch.bfloat16, torch.float32
F = torch.nn.functional


def strided(t, pad=8):
    """the same values as a column slice of a wider tensor"""
    wide = torch.full((t.shape[0], t.shape[1] + 2 * pad), 99.0, dtype=t.dtype)
    wide[:, pad: pad + t.shape[1]] = t
    return wide[:, pad: pad + t.shape[1]]


# ------------------------------------------------------------------ 1. the reference
def test_gelu_parts_match_autograd():
    x = torch.linspace(-9, 9, 2001, dtype=torch.float64, requires_grad=True)
    g = F.gelu(x, approximate="tanh")
    (d1,) = torch.autograd.grad(g.sum(), x, create_graph=True)
    (d2,) = torch.autograd.grad(d1.sum(), x)
    mine = R.gelu_parts(x.detach())
    for a, b in zip(mine, (g, d1, d2)):
        torch.testing.assert_close(a, b.detach(), atol=1e-13, rtol=1e-12)
    big = torch.tensor([R.BF16_MAX, -R.BF16_MAX, 1e30, -1e30], dtype=torch.float64)
    g, d1, d2 = R.gelu_parts(big)
    assert torch.equal(g, torch.tensor([R.BF16_MAX, 0.0, 1e30, 0.0], dtype=torch.float64).abs() * (big > 0))
    assert torch.equal(d1, (big > 0).double()) and torch.equal(d2, torch.zeros(4, dtype=torch.float64))


@pytest.mark.parametrize("tA,tB", [(False, False), (False, True), (True, True), (True, False)])
@pytest.mark.parametrize("alpha", [1.0, 0.5, -2.0])
def test_ref_matches_matmul(tA, tB, alpha):
    M, N, K = 24, 40, 64
    x = R.randn_inputs(M, N, K, 1)
    A = strided(x.a.t().contiguous()) if tA else strided(x.a)
    B = strided(x.b.t().contiguous()) if tB else strided(x.b)
    a, b, bias, r, aux, c0 = (t.double() for t in (x.a, x.b, x.bias, x.r, x.aux, x.c0))
    lin = alpha * torch.matmul(a, b.t())
    keep = (torch.rand(M, N, generator=torch.Generator().manual_seed(2)) > 0.25).double() / 0.75
    cs0 = torch.full((N,), 0.5)
    for epi in R.EPI:
        for kp in ((None, keep) if epi in R.DROP_EPIS else (None,)):
            ref = R.gemm_ref(A, B, tA, tB, alpha, epi, bias=x.bias, R=strided(x.r, 16), aux=strided(x.aux, 24), keep=kp,
                             colsum0=cs0)
            pre = lin + (bias if "bias" in epi else 0)
            k = 1.0 if kp is None else kp
            if epi == "bias_gelu":
                p = pre.clone().requires_grad_(True)
                g = F.gelu(p, approximate="tanh")
                (d,) = torch.autograd.grad(g.sum(), p)
                want, want_aux = g.detach() * k, d
            elif epi == "bias_relu":
                want, want_aux = torch.relu(pre) * k, pre
            elif epi in ("res", "bias_res"):
                want, want_aux = pre + r, None
            elif epi == "dgelu":
                want, want_aux = pre * aux * k, None
            elif epi == "drelu":
                want, want_aux = pre * (aux > 0) * k, None
            else:
                want, want_aux = pre, None
            torch.testing.assert_close(ref.out, want, atol=1e-12, rtol=1e-12)
            torch.testing.assert_close(ref.pre, pre, atol=1e-12, rtol=1e-12)
            if want_aux is not None:
                torch.testing.assert_close(ref.aux, want_aux, atol=1e-12, rtol=1e-12)
            torch.testing.assert_close(ref.colsum, 0.5 + want.sum(0), atol=1e-10, rtol=1e-12)
            assert bool((ref.A_out >= ref.out.abs() * (1 - 1e-12)).all()) or epi == "bias_gelu"
    ref = R.gemm_ref(A, B, tA, tB, alpha, C0=x.c0)
    torch.testing.assert_close(ref.out, lin + c0, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(ref.A_out, abs(alpha) * a.abs() @ b.abs().t() + c0.abs(), atol=1e-12, rtol=1e-12)
    # the f32 epilogues: v = alpha acc (+ C0) + bias, ReLU / dReLU (R = pre-activation), + R
    xf = R.randn_inputs(M, N, K, 3, F32)
    af, bf, biasf, rf, c0f = (t.double() for t in (xf.a, xf.b, xf.bias, xf.r, xf.c0))
    for epi in R.F32_EPI:
        ref = R.gemm_ref(xf.a, xf.b, alpha=alpha, epi=epi, bias=xf.bias, R=xf.r, C0=xf.c0, f32=True,
                         keep=keep if epi in ("bias_relu", "drelu") else None)
        v = alpha * af @ bf.t() + c0f + (biasf if "bias" in epi else 0)
        want = {"none": v, "bias": v, "bias_relu": torch.relu(v) * keep, "res": v + rf, "bias_res": v + rf,
                "drelu": v * (rf > 0) * keep}[epi]
        torch.testing.assert_close(ref.out, want, atol=1e-12, rtol=1e-12)


def test_ref_matches_ops_cpu_branches():
    """ops.linear / linear_dx / linear_dw / run_wjobs on CPU tensors (f32 products, the same
    bf16-rounded pre-activation) are within the bounds recorded for the GPU engines."""
    rep = R.Report("ops-cpu")
    T, N, K = 72, 40, 64
    x = R.randn_inputs(T, N, K, 4)
    for act, epi in (("none", "bias"), ("gelu_tanh", "bias_gelu"), ("relu", "bias_relu")):
        y, aux = ops.linear(x.a, x.b, x.bias, act=act)
        R.check_outputs(rep, "v1", R.gemm_ref(x.a, x.b, epi=epi, bias=x.bias), dict(out=y, aux=aux), epi)
    y, _ = ops.linear(x.a, x.b, None)
    R.check_outputs(rep, "v1", R.gemm_ref(x.a, x.b), dict(out=y))
    y, _ = ops.linear(x.a, x.b, x.bias, residual=x.r)
    R.check_outputs(rep, "v1", R.gemm_ref(x.a, x.b, epi="bias_res", bias=x.bias, R=x.r), dict(out=y), "bias_res")
    y, _ = ops.linear(x.a, x.b, None, residual=x.r)
    R.check_outputs(rep, "v1", R.gemm_ref(x.a, x.b, epi="res", R=x.r), dict(out=y), "res")
    # dx = dy @ w, dy [T, N], w [N, K]: the reference's transB form
    dy, w = x.r, x.b
    gd = (torch.randn(T, K, generator=torch.Generator().manual_seed(5)) * 0.5).to(BF16)
    for act, epi, saved in (("none", "none", None), ("gelu_tanh", "dgelu", gd), ("relu", "drelu", gd)):
        for res in (None, x.a) if act == "none" else (None,):
            cs = torch.full((K,), 0.5)
            dx = ops.linear_dx(dy, w, act_input=saved, act=act, residual=res, colsum=cs)
            e = "res" if res is not None else epi
            ref = R.gemm_ref(dy, w, transB=True, epi=e, aux=saved, R=res, colsum0=torch.full((K,), 0.5), stored=dx)
            R.check_outputs(rep, "v1", ref, dict(out=dx), e)
            torch.testing.assert_close(cs.double(), ref.colsum, atol=1e-3, rtol=1e-5)
    dw0 = torch.randint(-8, 9, (N, K), generator=torch.Generator().manual_seed(6)).float()
    for alpha in (1.0, 0.5):
        dw = ops.linear_dw(dy, x.a, dw0.clone(), alpha=alpha)
        R.check_outputs(rep, "stt", R.gemm_ref(dy, x.a, True, True, alpha, C0=dw0), dict(out=dw))
    g1, g2 = dw0.clone(), dw0.clone()
    ops.kernels.run_wjobs([ops.kernels.DW(dy, x.a, g1, 0.5), ops.kernels.DW(dy, x.a, g2, 0.5)])
    ref = R.gemm_ref(dy, x.a, True, True, 0.5, C0=dw0)
    R.check_outputs(rep, "grouped", ref, dict(out=g1))
    R.check_outputs(rep, "grouped", ref, dict(out=g2))
    rep.finish()


# ------------------------------------------------------------------ 2. mutations
M_, N_, K_ = 136, 72, 320     # kt = 5 (odd), an edge tile of 8 rows / 8 columns behind 128 / 64
SPLIT = 2                      # uneven: K-tiles [0, 2) and [2, 5)


def _problem(dtype=BF16, seed=9):
    return R.randn_inputs(M_, N_, K_, seed, dtype)


def _passes(cls, ref, got, epi="none"):
    rep = R.Report("mutation")
    R.check_outputs(rep, cls, ref, got, epi)
    return not rep.fails


def _slab(x, k0, k1):
    return x.a[:, k0:k1].double() @ x.b[:, k0:k1].double().t()


def _mutations():
    """name -> (engine class, epilogue, reference, correct outputs, mutated outputs)"""
    x = _problem()
    out = {}
    full = R.gemm_ref(x.a, x.b)
    good = dict(out=full.out.to(BF16))
    out["last K element dropped"] = ("g2", "none", full, good, dict(out=_slab(x, 0, K_ - 1).to(BF16)))
    out["last K-tile dropped (kt odd)"] = ("g3nt", "none", full, good, dict(out=_slab(x, 0, K_ - 64).to(BF16)))
    cut = (SPLIT - 1) * (K_ // 64) // SPLIT * 64
    s0, s1 = _slab(x, 0, cut), _slab(x, cut, K_)
    out["one split's slab added twice"] = ("skepi", "none", full, good, dict(out=(s0 + s0 + s1).to(BF16)))
    half = R.gemm_ref(x.a, x.b, alpha=0.5)
    out["alpha missing on one split"] = ("skepi", "none", half, dict(out=half.out.to(BF16)),
                                         dict(out=(0.5 * s0 + s1).to(BF16)))
    b = R.gemm_ref(x.a, x.b, epi="bias", bias=x.bias)
    out["bias shifted by 8 columns"] = ("g2", "bias", b, dict(out=b.out.to(BF16)),
                                        dict(out=(full.out + x.bias.double().roll(8)[None, :]).to(BF16)))
    sw = full.out.clone()
    sw[[M_ - 8, M_ - 7]] = sw[[M_ - 7, M_ - 8]]
    out["two rows swapped in an edge tile"] = ("g2", "none", full, good, dict(out=sw.to(BF16)))
    tr = full.out.clone()
    tr[32:64, 32:64] = tr[32:64, 32:64].t().clone()
    out["a 32x32 sub-block written transposed"] = ("g2", "none", full, good, dict(out=tr.to(BF16)))
    acc = R.gemm_ref(x.a, x.b, alpha=0.5, C0=x.c0)
    out["accumulate without C0"] = ("skred", "none", acc, dict(out=acc.out.float()), dict(out=(0.5 * full.out).float()))
    # ReLU saves its pre-activation: activation first, rounding after, loses every negative one.
    # (For GELU the same slip moves the saved derivative by at most the half-ulp step of the
    # pre-activation that the check must allow, so no check of this kind can see it.)
    g = R.gemm_ref(x.a, x.b, epi="bias_relu", bias=x.bias)
    pre16 = g.pre.to(BF16)
    out["pre-activation rounded after the activation (aux only)"] = (
        "g2", "bias_relu", g, dict(out=torch.relu(pre16), aux=pre16), dict(out=torch.relu(pre16), aux=torch.relu(g.pre).to(BF16)))
    stored = full.out.to(BF16)
    cs = R.gemm_ref(x.a, x.b, colsum0=torch.full((N_,), 0.5), stored=stored)
    out["column sums missing the last row"] = ("g2", "none", cs, dict(out=stored, colsum=(0.5 + stored.double().sum(0)).float()),
                                               dict(out=stored, colsum=(0.5 + stored.double()[:-1].sum(0)).float()))
    r = R.gemm_ref(x.a, x.b, epi="res", R=x.r)
    wrong = torch.cat([x.r.reshape(-1), x.r.reshape(-1)])[: M_ * (N_ + 8)].reshape(M_, N_ + 8)[:, :N_]   # rows at stride N + 8
    out["residual read with ldc instead of ldr"] = ("g2", "res", r, dict(out=r.out.to(BF16)),
                                                    dict(out=(full.out + wrong.double()).to(BF16)))
    xf = R.make_inputs(next(c for c in R.F32_CASES if c.kind == "mant24"))
    f = R.gemm_ref(xf.a, xf.b, f32=True)
    trunc = lambda t: (t.view(torch.int32) & ~((1 << 13) - 1)).view(F32)   # noqa: E731  10 mantissa bits kept
    out["f32 inputs truncated to 10 mantissa bits"] = ("f32.64", "none", f, dict(out=f.out.float()),
                                                       dict(out=(trunc(xf.a).double() @ trunc(xf.b).double().t()).float()))
    return out


MUTATIONS = _mutations()


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_fails_the_check(name):
    cls, epi, ref, good, bad = MUTATIONS[name]
    assert _passes(cls, ref, good, epi), "the correct result does not pass"
    assert not _passes(cls, ref, bad, epi), "the mutated result passes"


def test_twelve_mutations():
    assert len(MUTATIONS) == 12


# ------------------------------------------------------------------ 3. inputs and tables
def test_relu_sign_exclusions_stay_under_the_cap():
    """the bias offset of randn_inputs keeps the elements whose ReLU branch the reference cannot
    decide under 0.1 % in every bias+ReLU case the GPU test runs (bf16 and f32)"""
    worst = 0.0
    for c in R.CASES + R.F32_CASES:
        if c.epi != "bias_relu" or c.M > 600:
            continue
        x = R.make_inputs(c)
        ref = R.gemm_ref(x.a, x.b, alpha=c.alpha, epi="bias_relu", bias=x.bias, C0=x.c0 if c.acc else None,
                         f32=c.prec == "f32")
        frac = float(ref.unsure.double().mean())
        worst = max(worst, frac)
        assert frac <= R.UNSURE_CAP, (c.id, frac)
    print("largest unsure fraction", worst)


def test_exact_inputs_are_exact():
    for K, split in ((64, 1), (192, 1), (320, 1), (704, 3), (832, 3), (4160, 8)):
        for kind in ("select", "twohot"):
            a, b, want = R.exact_inputs(kind, 40, 24, K, split)
            assert torch.equal(a.double() @ b.double().t(), want)
            hot = a.double().sum(1)
            assert bool((hot == (2 if kind == "twohot" and K >= 128 else 1)).all())
            for alpha in R.ALPHAS:
                assert torch.equal((alpha * want).to(BF16).double(), alpha * want)
            if kind == "twohot" and K >= 128:
                kt = K // 64
                cols = a.double().nonzero()[:, 1].reshape(40, 2)
                tiles = cols // 64
                assert bool((tiles[:, 0] != tiles[:, 1]).all()), "the two hot columns share a K-tile"
                if split > 1:
                    own = lambda t: sum(1 for y in range(1, split) if y * kt // split <= t)   # noqa: E731
                    assert all(own(int(t0)) != own(int(t1)) for t0, t1 in tiles), "the two hot columns share a split"
    # the selection touches every K-tile within one 32-row tile
    assert len({R.pi(m, 448) // 64 for m in range(32)}) == 7


def test_tables_cover_every_case():
    keys = set()
    for c in R.CASES + R.F32_CASES:
        out = "acc" if (c.acc or c.prec == "f32") else ("out" if c.epi in R.ONE_ROUNDING else "act")
        keys.add(f"{c.cls}.{out}")
        if c.epi in ("bias_gelu", "bias_relu"):
            keys.add(f"{c.cls}.aux")
        if c.colsum:
            fused = c.prec == "bf16" and not c.v1 and not c.acc and c.split == 1
            keys.add(f"{c.cls}." + (("colsum_act" if c.epi in ("bias_gelu", "bias_relu") else "colsum") if fused else "colsum_sep"))
    keys |= {"grouped.acc", "f32.128.acc"}
    assert keys <= set(R.BOUND), sorted(keys - set(R.BOUND))
    assert keys <= set(R.OLD_TOL), sorted(keys - set(R.OLD_TOL))
    for k, v in R.BOUND.items():
        if k.endswith(".out"):
            assert v <= 1.0, f"{k}: a bf16 output that is one f32 sum rounded once may not exceed 1.0"
    assert len({c.id for c in R.CASES}) == len(R.CASES) and len({c.id for c in R.F32_CASES}) == len(R.F32_CASES)
    classes = {c.cls for c in R.CASES + R.F32_CASES}
    assert {"g2", "g3nt", "g3tt", "g6", "g8", "snt", "stt", "v1", "skepi", "skred", "f32.64", "f32.128", "f32.split",
            "f32.sk"} <= classes
    for c in R.CASES:
        if c.group == "splitk" and c.split > 1:
            assert (c.K // R.BK) % c.split != 0, c.id
