"""The in-flight GEMM epilogue (csrc/kernels/gemm2.hip g2::epilogue): bias chunk loaded once,
a pass's row-input loads (residual / saved activation input) issued before the staging
barrier, chunk loop unrolled -- on whole tiles; tiles on the M / N edge keep the rolled loop.
Every fused epilogue, on the engines that take the new loop (forced cfg 0, 2, 3, 5) and on
those that keep the rolled one (cfg 1, 9 and 15: BN = 192), against the f32 torch path with
test_gemm2_configs' tolerances.

Shapes: (512, 768) is whole tiles on every engine; (1000, 776) mixes whole tiles with a
partial last tile in both dimensions, so one launch runs both loops.  (300, 136), (129, 264)
and M = 1 (partial row tile with N < 256, one row into the second pass, a single row) are
refused by the v2 engine, which takes only M % 8 == 0: they run on the v1 fallback of
``_gemm`` and must stay correct there.  (304, 136), (136, 264) and M = 8 are the same edges
at sizes the v2 engine accepts.

Run as a script (``python tests/test_gemm_epilogue_inflight_gpu.py OUT.pt``) it saves the
outputs of the bitwise cases; the bitwise test starts it with MIPIPE_EXT_VARIANT=rolled."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mipipe  # noqa: E402,F401
from mipipe import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPIS = dict(bias=1, bias_gelu=2, bias_relu=3, bias_res=4, res=5, dgelu=6, drelu=7)
CFGS = [0, 2, 3, 5, 15, 1, 9]
SHAPES = [(300, 136), (1000, 776), (129, 264), (512, 768), (1, 264),
          (304, 136), (136, 264), (8, 264)]
K = 128
PAD = 24   # extra leading columns of the wide tensors the strided cases slice (keeps 16-byte alignment)


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def rnd(*shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape) * scale).to(dtype)


def gelu_grad_ref(a):
    k0, k1 = 0.7978845608028654, 0.044715
    t = torch.tanh(k0 * (a + k1 * a ** 3))
    return 0.5 * (1 + t) + 0.5 * a * (1 - t * t) * k0 * (1 + 3 * k1 * a * a)


def close(a, b, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol, rtol=rtol)


_PROBLEMS = {}


def problem(M, N):
    """Inputs (CPU bf16 + device copies) and the f32 product of one shape, made once."""
    key = (M, N)
    if key not in _PROBLEMS:
        g = torch.Generator().manual_seed(1000 * M + N)
        mk = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16)  # noqa: E731
        p = dict(x=mk(M, K), w=mk(N, K, scale=K ** -0.5), b=mk(N, scale=0.1), r=mk(M, N), aux=mk(M, N))
        p["acc"] = p["x"].float() @ p["w"].float().t()
        p["dev"] = {k: p[k].to(DEV) for k in ("x", "w", "b", "r", "aux")}
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def reference(p, epi):
    """(C, AUX or None) of the f32 torch path."""
    ref, aux = p["acc"], None
    if "bias" in epi:
        ref = ref + p["b"].float()
    if epi == "bias_gelu":
        pre = ref.to(torch.bfloat16).float()
        aux = gelu_grad_ref(pre).to(torch.bfloat16)
        ref = torch.nn.functional.gelu(pre, approximate="tanh")
    if epi == "bias_relu":
        pre = ref.to(torch.bfloat16).float()
        aux = pre.to(torch.bfloat16)
        ref = torch.relu(pre)
    if epi in ("bias_res", "res"):
        ref = ref + p["r"].float()
    if epi == "dgelu":
        ref = ref * p["aux"].float()
    if epi == "drelu":
        ref = ref * (p["aux"].float() > 0).float()
    return ref, aux


def widen(t, fill=0.0):
    """``t`` as a column slice of a wider tensor (row stride != N), same values."""
    wide = torch.full((t.shape[0], t.shape[1] + 2 * PAD), fill, dtype=t.dtype, device=t.device)
    view = wide[:, PAD:PAD + t.shape[1]]
    view.copy_(t)
    return wide, view


def run(p, epi, cfg, strided=False, inplace=False, **kw):
    """One GEMM through ``_gemm``; returns (C, AUX written or None, wide C or None)."""
    from mipipe.ops import kernels as _k
    d = p["dev"]
    M, N = p["r"].shape
    y_wide = None
    if inplace:
        y = d["r"].clone()
        res = y
    else:
        y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        res = d["r"]
        if strided:
            y_wide, y = widen(y, fill=7.0)
            res = widen(res)[1]
    aux = None
    if epi in ("dgelu", "drelu"):
        aux = widen(d["aux"])[1] if strided else d["aux"]
    elif epi in ("bias_gelu", "bias_relu"):
        aux = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        if strided:
            aux = widen(aux)[1]
    w, trans_b = d["w"], False
    if epi in ("dgelu", "drelu") and M % 8:
        # the v1 fallback has the dX epilogues in linear_dx's form only: B = w^T [K, N], transB
        w, trans_b = d["w"].t().contiguous(), True
    _k._gemm(d["x"], w, y, bias=d["b"] if "bias" in epi else None,
             residual=res if epi in ("bias_res", "res") else None, aux=aux, transB=trans_b, epi=EPIS[epi], cfg=cfg,
             **kw)
    return y, (aux if epi in ("bias_gelu", "bias_relu") else None), y_wide


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("epi", list(EPIS))
def test_epilogue_matches_f32(epi, M, N, cfg):
    p = problem(M, N)
    y, aux, _ = run(p, epi, cfg)
    ref, aux_ref = reference(p, epi)
    if aux_ref is not None:
        close(aux, aux_ref)
    close(y, ref)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M,N", [(1000, 776), (304, 136)])
@pytest.mark.parametrize("epi", list(EPIS))
def test_epilogue_strided_row_inputs_and_output(epi, M, N, cfg):
    """R / AUX read from, and C / AUX written into, column slices of wider tensors
    (ldr, ldx, ldc != N); the columns outside the C slice stay untouched."""
    p = problem(M, N)
    y, aux, y_wide = run(p, epi, cfg, strided=True)
    ref, aux_ref = reference(p, epi)
    if aux_ref is not None:
        close(aux, aux_ref)
    close(y, ref)
    assert bool((y_wide[:, :PAD] == 7.0).all()) and bool((y_wide[:, PAD + N:] == 7.0).all())


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("M,N", [(1000, 776), (512, 768), (136, 264)])
@pytest.mark.parametrize("epi", ["bias_res", "res"])
def test_epilogue_inplace_residual(epi, M, N, cfg):
    """R aliasing C, as the cross-attention backward's linear_dx(residual=dh, out=dh) does."""
    p = problem(M, N)
    y, _, _ = run(p, epi, cfg, inplace=True)
    close(y, reference(p, epi)[0])


def _masks(shape, p_drop, seed):
    """The scaled keep mask act_fwd and act_bwd regenerate for a contiguous [M, N] output."""
    one = torch.ones(*shape, dtype=torch.bfloat16, device=DEV)
    return ops.act_fwd(one, "relu", p_drop=p_drop, seed=seed), ops.act_bwd(one, one, "relu", p_drop=p_drop, seed=seed)


@pytest.mark.parametrize("cfg", [0, 2, 3, 5, 1])
@pytest.mark.parametrize("epi", ["bias_gelu", "dgelu", "dgelu_colsum"])
def test_epilogue_dropout_mask(epi, cfg):
    """p_drop = 0.1 in the bias+GELU and dGELU epilogues (one branch per chunk): the output
    is the undropped output times the mask act_fwd / act_bwd regenerate from (seed, element
    index, step counter), and it is zero exactly where that mask is; with the fused column
    sums, those are the sums of the dropped output."""
    M, N, pd, seed = 1000, 776, 0.1, 4321
    p = problem(M, N)
    ops.set_dropout_step(3, torch.device(DEV))
    cs = torch.full((N,), 0.5, device=DEV) if epi == "dgelu_colsum" else None
    e = epi.split("_colsum")[0]
    y0, aux0, _ = run(p, e, cfg)
    kw = dict(colsum=cs) if cs is not None else {}
    y, aux, _ = run(p, e, cfg, p_drop=pd, seed=seed, **kw)
    m_f, m_b = _masks((M, N), pd, seed)
    assert torch.equal(m_f, m_b)
    mask = m_f.float()
    keep = mask != 0
    assert 0.88 < keep.float().mean().item() < 0.92
    if aux0 is not None:
        assert torch.equal(aux, aux0), "the saved derivative is taken before the dropout"
    # bf16(v * s) against bf16(v) * s: two bf16 roundings apart
    close(y, y0.float() * mask, atol=2e-2, rtol=2e-2)
    live = y0.float().abs() > 1e-3
    assert torch.equal((y != 0)[live], keep[live]), "dropout mask differs from act_fwd / act_bwd"
    assert bool((y[~keep] == 0).all())
    if cs is not None:
        close(cs, y.float().cpu().sum(0) + 0.5, atol=0.05 * (M ** 0.5), rtol=2e-2)


# ---- bitwise: the default build against the `rolled` variant build of the same tree
BITWISE_SHAPE = (1000, 776)
BITWISE_CFG = 5


def _bitwise_outputs():
    p = problem(*BITWISE_SHAPE)
    out = {}
    for epi in EPIS:
        y, aux, _ = run(p, epi, BITWISE_CFG)
        out[epi] = y.cpu()
        if aux is not None:
            out[epi + ".aux"] = aux.cpu()
    return out


@pytest.fixture(scope="module")
def rolled_outputs(tmp_path_factory):
    from mipipe.ops import kernels as _k
    so = os.path.join(os.path.dirname(os.path.abspath(_k.__file__)), os.pardir, "_C_rolled.so")
    if os.environ.get("MIPIPE_EXT_VARIANT") or not os.path.exists(so):
        pytest.skip("needs the default build loaded and the variant built: "
                    "python tools/build_ext.py --variant rolled -DMP_EPI_ROLLED")
    path = str(tmp_path_factory.mktemp("rolled") / "out.pt")
    env = dict(os.environ, MIPIPE_EXT_VARIANT="rolled")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return torch.load(path)


@pytest.fixture(scope="module")
def default_outputs():
    return _bitwise_outputs()


@pytest.mark.parametrize("epi", list(EPIS))
def test_epilogue_bitwise_equals_rolled_build(epi, rolled_outputs, default_outputs):
    new = default_outputs
    for k in (epi, epi + ".aux"):
        if k in new:
            assert torch.equal(new[k].view(torch.int16), rolled_outputs[k].view(torch.int16)), k


if __name__ == "__main__":
    assert os.environ.get("MIPIPE_EXT_VARIANT"), "the child runs a variant build"
    torch.save(_bitwise_outputs(), sys.argv[1])
