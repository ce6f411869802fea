"""Edge cases of the memory-bound, loss and optimizer HIP kernels against float64 references
(membound_refs.py, themselves checked on the CPU in test_membound_refs_cpu.py).

Shapes are the smallest that reach each launcher branch: every cross-entropy kernel
(512 x 4 / x 13 / x 16, 1024 x 16, streaming, scalar tails), every MAXJ of the norm kernels,
partly filled 64-lane slabs, the per-block partial-sum paths with a short last block, the
atomic paths next to them, second grid-stride passes and scalar tails of the flat kernels.

Tolerances.  bf16 outputs are one f32 computation rounded once: rtol 2^-8 (a bf16 half-ulp at
the bottom of a binade) plus atol 1e-6 x the input scale for cancelling values.  f32 outputs and
reductions are bounded by twice the error measured on an MI355X against the float64 reference
(``BOUND``: the measured value stands next to each bound), never looser than what the older
test of the same kernel allows.  The error of an f32 tensor is
max |got - ref| / (|ref| + min(1, max |ref|))."""
import math

import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import membound_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
RTOL_BF16 = 2.0 ** -8
BF16_MAX = 3.3895313892515355e38

# bound = 2 x the largest error measured on an MI355X over two runs of this file (the measured
# value in the comment; sums that end in f32 atomics vary a little with the order of arrival)
BOUND = {
    "xent.loss.bf16": 2.1e-7,      # 1.009e-07 (older test: atol 2e-3, rtol 1e-3)
    "xent.loss.f32": 1.5e-7,       # 7.110e-08
    "xent.grad.f32": 1.7e-7,       # 8.092e-08
    "norm.bf16.mean": 1.1e-7,      # 5.452e-08
    "norm.bf16.rstd": 6.4e-7,      # 3.166e-07
    "norm.bf16.dw": 1.8e-5,        # 8.861e-06
    "norm.bf16.dbias": 4.8e-6,     # 2.365e-06
    "norm.bf16.colsum": 5.9e-6,    # 2.929e-06
    "norm.f32.y": 3.7e-5,          # 1.845e-05 (rows offset by 100; older f32 norm test: 1e-4)
    "norm.f32.mean": 3.4e-7,       # 1.685e-07
    "norm.f32.rstd": 1.9e-7,       # 9.110e-08
    "norm.f32.ds": 7.2e-6,         # 3.578e-06
    "norm.f32.dw": 2.1e-5,         # 1.001e-05
    "norm.f32.dbias": 1.3e-5,      # 6.136e-06
    "norm.f32.colsum": 1.9e-5,     # 9.324e-06
    "colsum.bf16": 1.5e-5,         # 7.041e-06
    "colsum.f32": 4.6e-5,          # 2.294e-05
    "act_bwd.dbias": 5.0e-5,       # 2.470e-05
    "embed.bwd": 1.8e-5,           # 8.988e-06
    "adamw.p": 2.3e-7,             # 1.141e-07 (older test: 1e-5)
    "adamw.m": 3.3e-7,             # 1.604e-07
    "adamw.v": 3.8e-7,             # 1.875e-07
    "sumsq": 1.2e-6,               # 5.972e-07 (older test: 1e-4)
    "lane_merge.sumsq": 4.6e-6,    # 2.264e-06
    "mean": 1.0e-7,                # 4.935e-08
}


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, g, scale=1.0, dtype=BF16):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def dev(t):
    return None if t is None else t.to(DEV, copy=True)


def amax(*ts):
    return max(float(t.detach().double().abs().max()) for t in ts if t is not None and t.numel())


def check_f32(key, got, ref, what=""):
    """f32 output / reduction against float64: the documented error metric within BOUND[key]."""
    got, ref = R.f64(got).reshape(-1), ref.double().reshape(-1)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{key} {what}: non-finite output"
    floor = max(min(1.0, float(ref.abs().max())), 1e-30)
    err = float(((got - ref).abs() / (ref.abs() + floor)).max())
    print(f"MEASURE {key} {err:.3e} {what}")
    assert err <= BOUND[key], f"{key} {what}: error {err:.3e} > bound {BOUND[key]:.3e}"


def check_bf16(key, got, ref, scale, what="", rtol=RTOL_BF16, atol_unit=1e-6):
    """bf16 output against the unrounded float64 value: |got - ref| <= atol + 2^-8 |ref|."""
    got, ref = R.f64(got).reshape(-1), ref.double().reshape(-1)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{key} {what}: non-finite output"
    ratio = float(((got - ref).abs() / (atol_unit * scale + rtol * ref.abs())).max())
    print(f"MEASURE-BF16 {key} {ratio:.3f} of the allowed error {what}")
    assert ratio <= 1.0, f"{key} {what}: {ratio:.3f} x the allowed bf16 error"


def check_out(key, got, ref, scale, what=""):
    """An output in the storage dtype: the bf16 rule, or the measured f32 bound."""
    if got.dtype == BF16:
        check_bf16(key, got, ref, scale, what)
    else:
        check_f32(key, got, ref, what)


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = torch.int16 if a.dtype == BF16 else torch.int32
    return torch.equal(a.view(view), b.view(view))


# ====================================================================== cross-entropy
XENT = [(5, 8),               # one partial chunk only (512 x 4)
        (1000, 1024),         # 512 x 4, whole padding chunks
        (4093, 4096),         # 512 x 4, partial last chunk
        (50257, 50304),       # 512 x 13, partial chunk + padding chunks (GPT-2)
        (65536, 65536),       # 512 x 16
        (128256, 128256),     # 1024 x 16 (Llama-3)
        (151936, 151936),     # streaming kernel
        (151931, 151936)]     # streaming kernel with a scalar tail


def xent_rows(V, Vp, ignore_index, dtype, seed=0):
    """Eight hand-made rows: 0 all-equal logits (loss = ln V); 1 -80 everywhere, +80 at the
    target V-1; 2 uniform in [-80, 80], target 0; 3 target on the last element of the last full
    8-wide chunk (0 when V < 8: no full chunk); 4 target V-1; 5 target on the first element of
    the partial chunk (if there is one); 6 ignore_index; 7 random.  Padding columns hold +100:
    a kernel that let them into the softmax would be far off."""
    g = gen(seed)
    x = torch.randn(8, Vp, generator=g) * 3
    tgt = torch.randint(0, V, (8,), generator=g)
    x[0] = 1.25
    tgt[0] = V // 2
    x[1] = -80.0
    x[1, V - 1] = 80.0
    tgt[1] = V - 1
    x[2] = torch.rand(Vp, generator=g) * 160 - 80
    tgt[2] = 0
    tgt[3] = max(8 * (V // 8) - 1, 0)
    tgt[4] = V - 1
    if 8 * (V // 8) < V:
        tgt[5] = 8 * (V // 8)
    tgt[6] = ignore_index
    x[:, V:] = 100.0
    return x.to(dtype), tgt


def run_xent(V, Vp, ignore_index, dtype):
    x, tgt = xent_rows(V, Vp, ignore_index, dtype)
    name = "bf16" if dtype == BF16 else "f32"
    what = f"V={V} Vp={Vp} ii={ignore_index}"
    gs = 1.0
    ref_loss, ref_grad = R.xent(x, tgt, V, gs, ignore_index)
    gl = dev(x)
    loss = ops.xent_fwd_bwd(gl, dev(tgt), V, gs, ignore_index=ignore_index)
    check_f32(f"xent.loss.{name}", loss, ref_loss, what)
    ign = tgt == ignore_index
    assert ign[6] and (ignore_index != 0 or ign[2])
    assert abs(float(loss[0]) - math.log(V)) <= BOUND[f"xent.loss.{name}"] * (1 + math.log(V))
    grad = R.f64(gl)
    if dtype == BF16:
        check_bf16("xent.grad", gl, ref_grad, gs, what, atol_unit=2e-6)
    else:
        check_f32("xent.grad.f32", gl, ref_grad, what)
    assert torch.count_nonzero(grad[:, V:]) == 0, "padding columns must be exactly 0"
    assert torch.count_nonzero(grad[ign]) == 0 and torch.count_nonzero(R.f64(loss)[ign]) == 0, "ignored rows"
    rowsum = grad[:, :V].sum(-1).abs()[~ign]
    print(f"MEASURE-ROWSUM xent.{name} {float(rowsum.max()):.3e} {what}")
    assert float(rowsum.max()) <= 2.0 ** -8 * gs
    return x, tgt, ref_loss


@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("V,Vp", XENT)
def test_xent_bf16_edges(V, Vp, ignore_index):
    x, tgt, ref_loss = run_xent(V, Vp, ignore_index, BF16)
    if Vp in (1024, 151936) and V == Vp - (24 if Vp == 1024 else 0):
        # write_grad=False: the same loss, the logits untouched
        gl = dev(x)
        loss = ops.xent_fwd_bwd(gl, dev(tgt), V, 1.0, ignore_index=ignore_index, write_grad=False)
        check_f32("xent.loss.bf16", loss, ref_loss, f"V={V} write_grad=False")
        assert bits_equal(gl, x), "write_grad=False must leave the logits bit-identical"


@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_xent_f32_edges(ignore_index):
    """f32 logits always take the streaming kernel: here with the scalar tail (4093 % 8 = 5)."""
    x, tgt, ref_loss = run_xent(4093, 4096, ignore_index, F32)
    gl = dev(x)
    loss = ops.xent_fwd_bwd(gl, dev(tgt), 4093, 1.0, ignore_index=ignore_index, write_grad=False)
    check_f32("xent.loss.f32", loss, ref_loss, "write_grad=False")
    assert bits_equal(gl, x)


# ====================================================================== LayerNorm / RMSNorm
def norm_shapes():
    out = []
    for D in (8, 520, 1544, 5120, 6152, 8192):    # MAXJ 1, 2, 4, 10, 16, 16; 520 / 1544 / 6152: part slab
        rows = [1, 3]
        if D in (8, 520, 5120):
            rows.append(257)
        if D in (8, 520, 1544):
            rows += [2048, 2050]                  # 256 / 257 blocks: per-block partials + reduce
        out += [(r, D) for r in rows]
    out.append((5000, 64))                        # 500 blocks of 10 rows
    return out


NORM_SHAPES = norm_shapes()


def norm_variant(i):
    """Deterministic spread of the options over the shape list: eps, branch, dres, dbias
    (LayerNorm bias), the +100 row offset, the constant row."""
    return dict(eps=(1e-5, 1e-6)[i % 2], branch=i % 3 != 0, dres=i % 4 != 1, bias=i % 5 != 2,
                offset=i % 4 == 2, const=i % 3 == 1)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind", ["layernorm", "rmsnorm"])
@pytest.mark.parametrize("case", range(len(NORM_SHAPES)), ids=[f"{r}x{d}" for r, d in NORM_SHAPES])
def test_norm_edges(case, kind, dtype):
    rows, D = NORM_SHAPES[case]
    o = norm_variant(case + (kind == "rmsnorm"))
    name = "bf16" if dtype == BF16 else "f32"
    what = f"{kind} {rows}x{D} {o}"
    g = gen(case)
    x = torch.randn(rows, D, generator=g)
    if o["offset"]:
        x += 100.0
    br = rnd(rows, D, g=g, dtype=dtype) if o["branch"] else None
    crow = rows // 2
    if o["const"]:
        x[crow] = 1.5
        if br is not None:
            br[crow] = 0.25
    x = x.to(dtype)
    w = (torch.randn(D, generator=g) * 0.5 + 1).to(dtype)
    ln = kind == "layernorm"
    bias = rnd(D, g=g, scale=0.1, dtype=dtype) if (ln and o["bias"]) else None
    dy = rnd(rows, D, g=g, dtype=dtype)
    dres = rnd(rows, D, g=g, dtype=dtype) if o["dres"] else None

    y, s, mean, rstd = ops.norm_fwd(dev(x), dev(w), dev(bias), dev(br), kind=kind, eps=o["eps"])
    ry, rmean, rrstd, rs = R.norm_fwd(x, w, bias, br, kind, o["eps"])
    scale = amax(x, br, w, bias)
    if br is not None:
        assert bits_equal(s, rs.to(dtype)), "stored residual must be round(a + b)"
    else:
        assert s.data_ptr() != y.data_ptr()
    check_out(f"norm.{name}.y", y, ry, scale, what)
    check_f32(f"norm.{name}.rstd", rstd, rrstd, what)
    if ln:
        check_f32(f"norm.{name}.mean", mean, rmean, what)
    else:
        assert mean is None
    if o["const"] and ln:
        # variance exactly 0: y is the bias (or 0), rstd = eps^-1/2
        want = bias.double() if bias is not None else torch.zeros(D, dtype=torch.float64)
        assert torch.equal(R.f64(y)[crow], want), "constant row: y must equal the bias"
        assert abs(float(rstd[crow]) * math.sqrt(o["eps"]) - 1.0) <= BOUND[f"norm.{name}.rstd"]

    # backward from the kernel's own saved s / mean / rstd
    dw0 = torch.randn(D, generator=g)
    db0 = torch.randn(D, generator=g) if (ln and o["bias"]) else None
    dw, db = dev(dw0.clone()), dev(None if db0 is None else db0.clone())
    ds, _ = ops.norm_bwd(dev(dy), s, dev(w), mean, rstd, kind=kind, dres=dev(dres), dw=dw, dbias=db)
    rds, rdw, rdb, _, _ = R.norm_bwd(dy, s, w, mean, rstd, kind, dres)
    check_out(f"norm.{name}.ds", ds, rds, amax(dy, w, dres) * max(1.0, amax(rstd)), what)
    check_f32(f"norm.{name}.dw", dw, rdw + dw0.double(), what)
    if db is not None:
        check_f32(f"norm.{name}.dbias", db, rdb + db0.double(), what)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,D,mode", [(2048, 520, "res_ds"), (2050, 1544, "res_ds"), (2050, 1544, "branch"),
                                         (2048, 520, "ds_only"), (257, 5120, "res_ds")])
def test_norm_fused_colsums(rows, D, mode, dtype, monkeypatch):
    """colsum_dres / colsum_ds / colsum_branch accumulate onto non-zero starts: on the
    per-block partial-sum path (>= 256 blocks), and at D = 5120 through the documented
    fallback (the extension answers -3, the wrapper sums in separate passes)."""
    name = "bf16" if dtype == BF16 else "f32"
    what = f"{rows}x{D} {mode}"
    g = gen(rows + D)
    x, w, bias = rnd(rows, D, g=g, dtype=dtype), rnd(D, g=g, scale=0.5, dtype=dtype), rnd(D, g=g, scale=0.1, dtype=dtype)
    dy = rnd(rows, D, g=g, dtype=dtype)
    dres = rnd(rows, D, g=g, dtype=dtype) if mode != "ds_only" else None
    ext = ops.load_ext()
    rcs = []
    real = ext.norm_bwd
    monkeypatch.setattr(ext, "norm_bwd", lambda *a: rcs.append(real(*a)) or rcs[-1])
    y, s, mean, rstd = ops.norm_fwd(dev(x), dev(w), dev(bias))
    dw0, db0, c10, c20 = (torch.randn(D, generator=g) for _ in range(4))
    dw, db, c1, c2 = (dev(t.clone()) for t in (dw0, db0, c10, c20))
    kw = dict(dres=dev(dres), dw=dw, dbias=db)
    if mode == "res_ds":
        kw.update(colsum_dres=c1, colsum_ds=c2)
    elif mode == "ds_only":
        kw.update(colsum_ds=c2)
    else:
        kw.update(colsum_dres=c1, colsum_branch=c2, want_branch=True)
    ds, dbr = ops.norm_bwd(dev(dy), s, dev(w), mean, rstd, **kw)
    assert rcs == [-3 if D > 2048 else 0], rcs
    rds, rdw, rdb, rcr, rcd = R.norm_bwd(dy, s, w, mean, rstd, "layernorm", dres)
    check_out(f"norm.{name}.ds", ds, rds, amax(dy, w, dres) * max(1.0, amax(rstd)), what)
    if mode == "branch":
        assert dbr is ds
    check_f32(f"norm.{name}.dw", dw, rdw + dw0.double(), what)
    check_f32(f"norm.{name}.dbias", db, rdb + db0.double(), what)
    # the kernel sums the ds it stored: take the stored values, so only the f32 summation is measured
    check_f32(f"norm.{name}.colsum", c2, R.f64(ds).sum(0) + c20.double(), what + " ds")
    if mode != "ds_only":
        check_f32(f"norm.{name}.colsum", c1, rcr + c10.double(), what + " dres")
    else:
        assert torch.equal(c1.cpu(), c10), "unused accumulator must stay untouched"


@pytest.mark.parametrize("D", [100, 8200])
def test_norm_rejects(D):
    x, w = torch.zeros(4, D, dtype=BF16, device=DEV), torch.ones(D, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.norm_fwd(x, w)
    mean, rstd = torch.zeros(4, device=DEV), torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError):
        ops.norm_bwd(x, x, w, mean, rstd, dw=torch.zeros(D, device=DEV))


# ====================================================================== colsum / act_bwd(dbias)
COLSUM = [(1, 8), (333, 520),
          (8192, 64),      # 256 blocks: per-block partials + reduce
          (8500, 136),     # 266 blocks, short last block
          (8192, 2056)]    # ny = 5, nx = 204 < 256: atomics


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", COLSUM)
def test_colsum_edges(rows, cols, dtype):
    g = gen(rows)
    x = rnd(rows, cols, g=g, dtype=dtype)
    acc0 = torch.randn(cols, generator=g)
    acc = dev(acc0.clone())
    ops.colsum(dev(x), acc)
    check_f32("colsum.bf16" if dtype == BF16 else "colsum.f32", acc, R.colsum(x) + acc0.double(), f"{rows}x{cols}")


@pytest.mark.parametrize("act", ["gelu_tanh", "relu"])
@pytest.mark.parametrize("rows,cols", COLSUM)
def test_act_bwd_dbias_edges(rows, cols, act):
    g = gen(rows + 1)
    dg, a = rnd(rows, cols, g=g), rnd(rows, cols, g=g, scale=2.0)
    acc0 = torch.randn(cols, generator=g)
    acc = dev(acc0.clone())
    da = ops.act_bwd(dev(dg), dev(a), act, dbias=acc)
    rda, _ = R.act_bwd(dg, a, act)
    check_bf16("act_bwd.da", da, rda, amax(dg), f"{act} {rows}x{cols}")
    # the kernel sums the bf16 values it stored
    check_f32("act_bwd.dbias", acc, R.f64(da).sum(0) + acc0.double(), f"{act} {rows}x{cols}")
    if (rows, cols) == (8500, 136):
        da2 = ops.act_bwd(dev(dg), dev(a), act)
        assert bits_equal(da2, da), "act_bwd without dbias must give the same da"


# ====================================================================== act_fwd / act_bwd values
def act_inputs():
    x = torch.cat([torch.linspace(-12, 12, 4083), torch.tensor([30.0, -30.0, 0.0, -0.0, BF16_MAX, -BF16_MAX])])
    return torch.cat([x, torch.zeros(-x.numel() % 8)]).to(BF16)


@pytest.mark.parametrize("act", ["gelu_tanh", "relu"])
def test_act_values(act):
    """Dense grid over [-12, 12] (through the fast sigmoid's saturation), +-30, +-0 and the
    largest finite bf16: no NaN anywhere, GELU(30) = 30, GELU(-30) = -0 or 0, derivative 1 / 0."""
    x = act_inputs()
    assert x.numel() % 8 == 0 and float(x.max()) == BF16_MAX
    y = ops.act_fwd(dev(x), act)
    check_bf16(f"act_fwd.{act}", y, R.act(x, act), 1.0)
    dg = torch.ones_like(x)
    d = ops.act_bwd(dev(dg), dev(x), act)
    assert torch.isfinite(d.float()).all(), f"{act}' is not finite at {x[~torch.isfinite(d.float().cpu())].tolist()}"
    check_bf16(f"act_bwd.{act}", d, R.act_grad(x, act), 1.0)
    i30 = int((x.float() == 30.0).nonzero()[0])
    yc, dc = y.float().cpu(), d.float().cpu()
    assert yc[i30] == 30.0 and yc[i30 + 1] == 0.0 and dc[i30] == 1.0 and dc[i30 + 1] == 0.0
    ibig = int((x.float() == BF16_MAX).nonzero()[0])
    assert yc[ibig] == BF16_MAX and yc[ibig + 1] == 0.0 and dc[ibig] == 1.0 and dc[ibig + 1] == 0.0
    with pytest.raises(RuntimeError):
        ops.act_fwd(dev(x[:12]), act)


def test_act_grid_stride():
    """4100 x 2048 elements: more than 4096 x 256 vectors, so every kernel loops twice."""
    g = gen(7)
    a, dg = rnd(4100, 2048, g=g, scale=2.0), rnd(4100, 2048, g=g)
    y = ops.act_fwd(dev(a), "gelu_tanh")
    check_bf16("act_fwd.gelu_tanh", y, R.act(a, "gelu_tanh"), amax(a), "grid-stride")
    del y
    da = ops.act_bwd(dev(dg), dev(a), "gelu_tanh")
    check_bf16("act_bwd.da", da, R.act_bwd(dg, a, "gelu_tanh")[0], amax(dg), "grid-stride")


# ====================================================================== SwiGLU
@pytest.mark.parametrize("T,F", [(1, 8), (130, 136), (1030, 8192)], ids=["1x8", "130x136", "grid-stride"])
def test_swiglu_edges(T, F):
    g = gen(T)
    gu, dy = rnd(T, 2 * F, g=g, scale=3.0), rnd(T, F, g=g)
    gu[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0]).to(BF16)
    gu[-1, F - 4:F] = torch.tensor([-100.0, 100.0, -30.0, 30.0]).to(BF16)
    y = ops.swiglu_fwd(dev(gu))
    check_bf16("swiglu_fwd", y, R.swiglu_fwd(gu), amax(gu))
    del y
    d = ops.swiglu_bwd(dev(gu), dev(dy))
    ref = R.swiglu_bwd(gu, dy)
    scale = amax(gu) * amax(dy)
    check_bf16("swiglu_bwd.dgate", d[:, :F], ref[:, :F], scale)
    check_bf16("swiglu_bwd.dup", d[:, F:], ref[:, F:], scale)


# ====================================================================== RoPE
@pytest.mark.parametrize("Dh", [8, 64, 128])
@pytest.mark.parametrize("T,S,pos", [(130, 65, 0), (3, 1, 17), (8, 4, 60)])
def test_rope_edges(Dh, T, S, pos):
    H, Hkv = 6, 2
    g = gen(Dh + T)
    qkv = rnd(T, (H + 2 * Hkv) * Dh, g=g)
    cs, sn = ops.rope_tables(min(T, S) + pos, Dh, 500000.0, "cpu")
    out = ops.rope_(dev(qkv.clone()), dev(cs), dev(sn), S, H, Hkv, Dh, pos_offset=pos)
    ref = R.rope(qkv, cs, sn, S, H, Hkv, Dh, pos)
    nrot = (H + Hkv) * Dh
    # each output is a two-term sum a c -+ b s: the scale of the cancelling terms is the pair's norm
    check_bf16("rope", out[:, :nrot], ref[:, :nrot], amax(qkv))
    assert bits_equal(out[:, nrot:], qkv[:, nrot:]), "v heads must pass through bit-identical"
    back = ops.rope_(out.clone(), dev(cs), dev(sn), S, H, Hkv, Dh, pos_offset=pos, inverse=True)
    assert bits_equal(back[:, nrot:], qkv[:, nrot:])
    # two bf16 roundings: the forward's (<= 2^-8 per component of a pair, sqrt(2) 2^-8 |pair| after
    # the inverse rotation) and the inverse's own (2^-8 |x|)
    x = qkv.double().reshape(T, H + 2 * Hkv, Dh)[:, : H + Hkv]
    pair = (x[..., : Dh // 2] ** 2 + x[..., Dh // 2:] ** 2).sqrt()
    allowed = (2 ** 0.5 + 1) * RTOL_BF16 * torch.cat([pair, pair], -1) + 1e-6
    err = (R.f64(back).reshape(T, H + 2 * Hkv, Dh)[:, : H + Hkv] - x).abs()
    assert bool((err <= allowed).all()), float((err / allowed).max())


# ====================================================================== embedding
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("with_pe", [True, False], ids=["wpe", "nowpe"])
@pytest.mark.parametrize("S,pos", [(64, 0), (1, 17), (16, 48)])
@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("D", [8, 520, 768])
def test_embedding_edges(D, T, S, pos, with_pe, dtype):
    V = 37
    g = gen(D + T + S)
    wte = rnd(V, D, g=g, dtype=dtype)
    wpe = rnd(min(T, S) + pos, D, g=g, dtype=dtype) if with_pe else None
    dout = rnd(T, D, g=g, dtype=dtype)
    alt = torch.where(torch.arange(T) % 2 == 0, 0, V - 1)
    for pat, idx in (("equal", torch.full((T,), 5)), ("ends", alt), ("random", torch.randint(0, V, (T,), generator=g))):
        out = ops.embed_fwd(dev(idx), dev(wte), dev(wpe), S, pos_offset=pos)
        want = wte.float()[idx]
        if with_pe:
            want = want + wpe.float()[R.positions(T, S, pos)]
        assert bits_equal(out, want.to(dtype)), f"forward not bit-exact ({pat})"
        a0 = torch.randn(V, D, generator=g)
        b0 = torch.randn(wpe.shape, generator=g) if with_pe else None
        a, b = dev(a0.clone()), dev(None if b0 is None else b0.clone())
        ops.embed_bwd(dev(idx), dev(dout), a, b, S, pos_offset=pos)
        ra, rb = R.embed_bwd(idx, dout, a0, b0, S, pos)
        check_f32("embed.bwd", a, ra, f"dwte {pat} T={T} D={D}")
        if with_pe:
            check_f32("embed.bwd", b, rb, f"dwpe {pat} T={T} D={D}")


def test_embedding_rejects_d12():
    wte = torch.zeros(4, 12, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.embed_fwd(torch.zeros(2, dtype=torch.int64, device=DEV), wte, None, 2)


# ====================================================================== AdamW
HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)
BIG = 2 * 1024 * 1024 + 1027     # 2048 blocks x 256 x 4 = 2M: a second grid-stride pass + a 3-element tail


def adamw_grad(n, g):
    """randn with a slice scaled by 1e-8 (|g| ~ eps: a misplaced eps shows) and a slice of zeros."""
    x = torch.randn(n, generator=g)
    x[n // 2: n // 2 + max(1, n // 8)] *= 1e-8
    if n >= 3:
        x[n // 4: n // 4 + max(1, n // 8)] = 0.0
    return x


def adamw_check(gp, gm, gv, ref, what):
    check_f32("adamw.p", gp, ref.p, what)
    check_f32("adamw.m", gm, ref.m, what)
    check_f32("adamw.v", gv, ref.v, what)


ADAMW_MODES = [("below", 0.125, True, True), ("above", 1.0, False, False), ("ignored", 1.0, True, True)]
ADAMW_CASES = [(n, nd) + mode for n, nd in [(1, 1), (1, 0), (3, 2), (4, 3), (10007, 5003)] for mode in ADAMW_MODES]
ADAMW_CASES.append((BIG, 1000003) + ADAMW_MODES[0])     # the one grid-stride case


@pytest.mark.parametrize("n,n_decay,clip,grad_scale,zero_grad,with_w16", ADAMW_CASES)
def test_adamw_edges(n, n_decay, clip, grad_scale, zero_grad, with_w16):
    """Three consecutive steps against torch.optim.AdamW in float64.  clip: max_norm below the
    gradient norm (clipping active), far above it (coefficient 1), or 0 with a sumsq buffer
    that must then be ignored.  n_decay is no multiple of 4: the boundary falls inside a float4."""
    g = gen(n + n_decay)
    p0 = torch.randn(n, generator=g)
    ref = R.AdamW(p0, n_decay, **HP)
    p, m, v = dev(p0.clone()), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    w16 = torch.zeros(n, dtype=BF16, device=DEV) if with_w16 else None
    for step in (1, 2, 3):
        gr = adamw_grad(n, g)
        norm = math.sqrt(R.sumsq(gr)) * grad_scale
        max_norm = {"below": 0.5 * norm + 1e-3, "above": 100.0 * norm + 1.0, "ignored": 0.0}[clip]
        ss = torch.tensor([R.sumsq(gr) if clip != "ignored" else 1e12], dtype=F32, device=DEV)
        gg = dev(gr.clone())
        ops.adamw_(p, gg, m, v, w16, n_decay, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], step,
                   sumsq_buf=ss, max_norm=max_norm, grad_scale=grad_scale, zero_grad=zero_grad)
        ref.step(gr, max_norm, grad_scale)
        adamw_check(p, m, v, ref, f"n={n} step={step} clip={clip}")
        if zero_grad:
            assert torch.count_nonzero(gg) == 0, "zero_grad=True must leave g all zero"
        else:
            assert bits_equal(gg, gr), "zero_grad=False must leave g bit-identical"
        if with_w16:
            assert bits_equal(w16, p.to(BF16)), "w16 must be the bf16 rounding of the updated p"


def test_adamw_step_1000():
    """One step number 1000 from given moments (bias corrections ~ 1), w16=None."""
    n, nd = 10007, 5003
    g = gen(3)
    p0, gr = torch.randn(n, generator=g), adamw_grad(n, g)
    m0, v0 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.1
    ref = R.AdamW(p0, nd, first_step=1000, m0=m0, v0=v0, **HP)
    ref.step(gr)
    p, m, v = dev(p0.clone()), dev(m0.clone()), dev(v0.clone())
    ops.adamw_(p, dev(gr.clone()), m, v, None, nd, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], 1000)
    adamw_check(p, m, v, ref, "step=1000")


# ====================================================================== sumsq / lane_merge / cast / mean
@pytest.mark.parametrize("n", [1, 3, 10007, BIG])
def test_sumsq_edges(n):
    g = gen(n)
    x = torch.randn(n, generator=g)
    out = torch.tensor([3.5], device=DEV)
    ops.sumsq(dev(x), out)
    check_f32("sumsq", out, torch.tensor([R.sumsq(x) + 3.5]), f"n={n}")


LANE_N = 8192 * 1024 + 1027     # 8192 blocks x 256 x 4 = 8M: a second grid-stride pass + a 3-element tail
LANE_CASES = [(n, k, sq) for n in (1, 3, 1027, 4096) for k in (1, 2, 3) for sq in (False, True)]
LANE_CASES.append((LANE_N, 3, True))


@pytest.mark.parametrize("n,lanes,with_sumsq", LANE_CASES)
def test_lane_merge_edges(n, lanes, with_sumsq):
    """g0 <- ((g0 + g1) + g2) + g3 in f32, bit for bit (adds only, in that order); every lane
    buffer zeroed; sumsq accumulates |merged g0|^2 onto a non-zero start."""
    g = gen(n + lanes)
    bufs = [torch.randn(n, generator=g) for _ in range(lanes + 1)]
    want = bufs[0].clone()
    for b in bufs[1:]:
        want = want + b
    gb = [dev(b.clone()) for b in bufs]
    ss = torch.tensor([2.25], device=DEV) if with_sumsq else None
    ops.load_ext().lane_merge(gb[0], gb[1:], ss)
    assert bits_equal(gb[0], want), "merged g0 is not the f32 sum in lane order"
    for b in gb[1:]:
        assert torch.count_nonzero(b) == 0, "lane buffers must be zeroed"
    if with_sumsq:
        check_f32("lane_merge.sumsq", ss, torch.tensor([R.sumsq(want) + 2.25]), f"n={n} lanes={lanes}")


@pytest.mark.parametrize("n", [1, 524288 + 77])
def test_cast_f32_bf16_edges(n):
    """Bit-equal to torch's round-to-nearest-even cast: +-0, +-inf, NaN (stays NaN), f32
    denormals, exact ties (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6) and f32 max (-> inf)."""
    g = gen(n)
    x = torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 1.4e-45,
                            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 3.4028234663852886e38,
                            -3.4028234663852886e38, BF16_MAX, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134])
    if n > special.numel():
        x[-special.numel():] = special      # the tail of the buffer
        x[: special.numel()] = special
    else:
        x[0] = 1 + 2.0 ** -8
    dst = torch.full((n,), 7.0, dtype=BF16, device=DEV)
    ops.cast_f32_bf16(dev(x), dst)
    want, got = x.to(BF16), dst.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN must stay NaN (and only NaN)"
    assert bits_equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))


@pytest.mark.parametrize("n", [1, 255, 100003])
def test_mean_edges(n):
    g = gen(n)
    x = dev(torch.randn(n, generator=g) + 3.0)
    a, b = ops.mean(x), ops.mean(x)
    assert bits_equal(a.reshape(1), b.reshape(1)), "the one-workgroup mean must be deterministic"
    check_f32("mean", a.reshape(1), R.f64(x).mean().reshape(1), f"n={n}")


# ====================================================================== transpose
@pytest.mark.parametrize("R_,C", [(8, 8), (70, 136), (1000, 72)])
def test_transpose_edges(R_, C):
    g = gen(R_)
    x = rnd(R_, C, g=g)
    assert bits_equal(ops.transpose(dev(x)), x.t().contiguous())
    wide = rnd(R_, 88, g=g)
    view = dev(wide)[:, 8:80]       # row-strided view
    assert not view.is_contiguous() or R_ == 1
    assert bits_equal(ops.transpose(view), wide[:, 8:80].t().contiguous())


# ====================================================================== argument checks of the bindings
# Every bad argument would stay in bounds even if its check were missing: a wrong dtype with at
# least as many bytes, a strided view into a large enough buffer, a table with enough storage
# but too few declared rows.
def strided(n, dtype):
    """[n] view with stride 2 into a [n, 2] buffer."""
    return torch.zeros(n, 2, dtype=dtype, device=DEV).t()[0]


def bad_args(dtype, n):
    """(wrong dtype with more bytes, non-contiguous view) stand-ins for a contiguous [n] ``dtype`` tensor."""
    return [torch.zeros(n, dtype=torch.float64, device=DEV), strided(n, dtype)]


def test_binding_checks_adamw_cast_sumsq():
    n = 64
    z = lambda dt=F32: torch.zeros(n, dtype=dt, device=DEV)
    args = (8, 1e-3, 0.9, 0.95, 1e-8, 0.1, 1)
    ops.adamw_(z(), z(), z(), z(), z(BF16), *args)
    for bad in bad_args(F32, n):
        with pytest.raises(RuntimeError):
            ops.adamw_(z(), z(), bad, z(), z(BF16), *args)
        with pytest.raises(RuntimeError):
            ops.adamw_(z(), z(), z(), bad, z(BF16), *args)
    for bad in [z(F32), strided(n, BF16)]:
        with pytest.raises(RuntimeError):
            ops.adamw_(z(), z(), z(), z(), bad, *args)
        with pytest.raises(RuntimeError):
            ops.cast_f32_bf16(z(), bad)
    for bad in (torch.zeros(1, dtype=torch.float64, device=DEV), strided(2, F32)):
        with pytest.raises(RuntimeError):
            ops.sumsq(z(), bad)


def test_binding_checks_act_swiglu():
    rows, cols = 4, 16
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)
    tview = z(cols, rows).t()                               # [rows, cols] transposed view
    f32 = z(rows, cols, dt=F32)
    for bad in (f32, tview):
        with pytest.raises(RuntimeError):
            ops.act_fwd(z(rows, cols), "relu", out=bad)
        with pytest.raises(RuntimeError):
            ops.act_bwd(z(rows, cols), bad, "relu")
        with pytest.raises(RuntimeError):
            ops.act_bwd(z(rows, cols), z(rows, cols), "relu", out=bad)
    for bad in bad_args(F32, cols):
        with pytest.raises(RuntimeError):
            ops.act_bwd(z(rows, cols), z(rows, cols), "relu", dbias=bad)
    F = cols
    gu_bad = [z(rows, 2 * F, dt=F32), z(2 * F, rows).t()]
    y_bad = [z(rows, F, dt=F32), z(F, rows).t()]
    for gb, yb in zip(gu_bad, y_bad):
        with pytest.raises(RuntimeError):
            ops.swiglu_fwd(gb, out=z(rows, F))
        with pytest.raises(RuntimeError):
            ops.swiglu_fwd(z(rows, 2 * F), out=yb)
        with pytest.raises(RuntimeError):
            ops.swiglu_bwd(gb, z(rows, F), out=z(rows, 2 * F))
        with pytest.raises(RuntimeError):
            ops.swiglu_bwd(z(rows, 2 * F), yb, out=z(rows, 2 * F))
        with pytest.raises(RuntimeError):
            ops.swiglu_bwd(z(rows, 2 * F), z(rows, F), out=gb)


def test_binding_checks_rope_and_position_tables():
    T, S, H, Hkv, Dh, pos = 8, 4, 2, 1, 16, 5
    W = (H + 2 * Hkv) * Dh
    need = min(T, S) + pos
    cs, sn = (dev(t) for t in ops.rope_tables(64, Dh, 10000.0, "cpu"))
    qkv = torch.zeros(T, W, dtype=BF16, device=DEV)
    ops.rope_(qkv, cs[:need], sn[:need], S, H, Hkv, Dh, pos_offset=pos)             # exactly enough rows
    with pytest.raises(RuntimeError):
        ops.rope_(qkv, cs[: need - 1], sn, S, H, Hkv, Dh, pos_offset=pos)           # storage for 64 rows, 8 declared
    with pytest.raises(RuntimeError):
        ops.rope_(qkv, cs, sn[: need - 1], S, H, Hkv, Dh, pos_offset=pos)
    with pytest.raises(RuntimeError):
        ops.rope_(qkv, cs.double(), sn, S, H, Hkv, Dh, pos_offset=pos)
    with pytest.raises(RuntimeError):
        ops.rope_(torch.zeros(T, W, dtype=F32, device=DEV), cs, sn, S, H, Hkv, Dh, pos_offset=pos)
    with pytest.raises(RuntimeError):
        ops.rope_(torch.zeros(W, T, dtype=BF16, device=DEV).t(), cs, sn, S, H, Hkv, Dh, pos_offset=pos)
    with pytest.raises(RuntimeError):
        # 7 x 72 elements: no whole number of 64-wide rows
        ops.rope_(torch.zeros(T - 1, W + 8, dtype=BF16, device=DEV), cs, sn, S, H, Hkv, Dh, pos_offset=pos)
    D, V = 16, 10
    idx = torch.zeros(T, dtype=torch.int64, device=DEV)
    wte = torch.zeros(V, D, dtype=BF16, device=DEV)
    wpe = torch.zeros(64, D, dtype=BF16, device=DEV)
    ops.embed_fwd(idx, wte, wpe[:need], S, pos_offset=pos)
    with pytest.raises(RuntimeError):
        ops.embed_fwd(idx, wte, wpe[: need - 1], S, pos_offset=pos)
    dwte, dwpe = torch.zeros(V, D, device=DEV), torch.zeros(64, D, device=DEV)
    dout = torch.zeros(T, D, dtype=BF16, device=DEV)
    ops.embed_bwd(idx, dout, dwte, dwpe[:need], S, pos_offset=pos)
    with pytest.raises(RuntimeError):
        ops.embed_bwd(idx, dout, dwte, dwpe[: need - 1], S, pos_offset=pos)
