"""Edge cases of the GEMM engines (gemm.hip; gemm2.hip with its engines in
csrc/include/mp_gemm_*.h; gemm_f32.hip) against the float64 reference of gemm_refs.py (itself
checked on the CPU in test_gemm_refs_cpu.py, together with the teeth of the error metric used
here).

The cases (gemm_refs.CASES / F32_CASES) are the smallest shapes that reach each engine and each
ragged edge; the launcher branch is the last part of a case id: cfg<k>.s<split> exactly as the
binding ``gemm2_plan`` (mp_gemm_plan.h) reports it for the case (asserted, so a planner change fails the case
instead of silently moving the coverage), v1 (the fallback for M % 8 != 0: gemm2 must refuse
the call), f32.64 / f32.128 (+ .s<split>) and f32.sk as ``gemm_f32_plan`` reports them.

Every tensor of a call is a view into a sentinel-padded buffer (guard columns left and right,
guard rows below; vectors have guard elements on both sides), so every operand is row-strided;
only the dropout cases use a contiguous C, which the mask index needs.  Inputs and all padding
must be bit-identical afterwards.  Outputs start as NaN.  Every call runs twice and C / aux
must repeat bit for bit; only the fused column sums end in f32 atomics and are compared within
their bound alone.  Exact-input cases (selection, two-hot) must match exactly (every value is
an integer or half of one; only the sign of a zero is left open).

Large row strides ('stride' cases, ids end in -bigld<x>): one operand at a time lives in a buffer
whose rows are 2^23 + 8 elements apart, at 264 rows (320 for the k-major operands), with the
same guards around the rows used.  Read for 32-bit row x stride products before these ran:
gemm.hip (v1), the gemm2 tile family (src_of), gemm3 NT / TT, gemm6, the small NT / TT and
grouped engines, the shared epilogue, both split-K passes and gemm_f32.hip (both tile sizes,
stream-K, epi_store) form them in int64_t; only gemm8's operand loads use 32-bit buffer
offsets, and its launcher hands such A / B back, so v1 computes them (run here too); gemm8's
ldc / ldr / ldx go through the shared 64-bit epilogue and run.  The 128x128 f32 engine runs its
stride cases in the child process (in process its smallest grid has 2044 rows).

Bounds: gemm_refs.BOUND, 2 x the largest error of two MI355X runs, next to the older tests'
atol / rtol (gemm_refs.OLD_TOL).  The non-default MFMA builds (MIPIPE_GEMM_M16=0,
MIPIPE_GEMM_M16T=1) and the forced 128x128 f32 engine (MIPIPE_F32_TILE=128) are read once per
process: they run in three child processes, one after the other (see the end of the file)."""
import os
import subprocess
import sys

import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import gemm_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENT_IN, SENT_OUT = 512.0, -77.0     # padding of inputs; padding of outputs
PAD_ROWS = 3
COLSUM0 = 0.5
DROP_STEP = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"
    ops.set_dropout_step(DROP_STEP, torch.device(DEV))


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32),
                       b.view(torch.int16 if a.dtype == BF16 else torch.int32))


class Region:
    """One view into a sentinel-padded buffer, with the index expressions of its padding."""

    def __init__(self, buf, view, guards, pad):
        self.buf, self.view, self.guards, self.pad = buf, view, guards, pad

    def snap(self):
        return [self.buf[g].clone() for g in self.guards] + [self.view.clone()]

    def padding_intact(self):
        return all(bool((self.buf[g] == self.pad).all()) for g in self.guards)

    def same(self, snap):
        return all(bits_equal(a, b) for a, b in zip([self.buf[g] for g in self.guards] + [self.view], snap))


def matrix(rows, cols, dtype, pad, init=None, side=8):
    """[rows + PAD_ROWS, side + cols + side] of ``pad``; the view holds ``init`` (a CPU tensor) or NaN"""
    buf = torch.full((rows + PAD_ROWS, cols + 2 * side), pad, dtype=dtype, device=DEV)
    view = buf[:rows, side: side + cols]
    guards = [(slice(None), slice(0, side)), (slice(None), slice(side + cols, None)), (slice(rows, None), slice(None))]
    r = Region(buf, view, guards, pad)
    view.copy_(init.to(DEV)) if init is not None else view.fill_(float("nan"))
    return r


BIG_COL = 4104     # first column of the view inside a BIG_LD-wide buffer (16-byte aligned)


def big_matrix(rows, cols, dtype, pad, init=None):
    """the same view as ``matrix`` inside an uninitialised [rows + 1, BIG_LD] buffer: the rows are
    BIG_LD elements apart; the 8 columns on either side and the row below hold ``pad``"""
    buf = torch.empty(rows + 1, R.BIG_LD, dtype=dtype, device=DEV)
    c0, c1 = BIG_COL, BIG_COL + cols
    buf[:, c0 - 8: c1 + 8] = pad
    view = buf[:rows, c0:c1]
    guards = [(slice(None), slice(c0 - 8, c0)), (slice(None), slice(c1, c1 + 8)), (slice(rows, None), slice(c0 - 8, c1 + 8))]
    r = Region(buf, view, guards, pad)
    view.copy_(init.to(DEV)) if init is not None else view.fill_(float("nan"))
    return r


def place(c, which, rows, cols, dtype, pad, init=None, side=8):
    """operand ``which`` ('lda' ...) of case c: in the large-stride buffer if the case names it"""
    return big_matrix(rows, cols, dtype, pad, init) if c.stride == which else matrix(rows, cols, dtype, pad, init, side)


def vector(n, dtype, pad, init):
    buf = torch.full((n + 16,), pad, dtype=dtype, device=DEV)
    r = Region(buf, buf[8: 8 + n], [slice(0, 8), slice(8 + n, None)], pad)
    r.view.copy_(init.to(DEV)) if torch.is_tensor(init) else r.view.fill_(init)
    return r


def keep_mask(M, N, p, seed):
    """the keep mask act_fwd regenerates for a contiguous [M, N] output (act_bwd: the same; it
    takes rows of a multiple of 8), scaled by exactly 1 / (1 - p)"""
    one = torch.ones(M, N, dtype=BF16, device=DEV)
    kept = ops.act_fwd(one, "relu", p_drop=p, seed=seed) != 0
    if N % 8 == 0:
        assert torch.equal(kept, ops.act_bwd(one, one, "relu", p_drop=p, seed=seed) != 0)
    return kept.double().cpu() / (1.0 - p)


def guarded(fn, what):
    try:
        return fn()
    except RuntimeError as e:
        if "HIP error" in str(e):   # a fault poisons the context: nothing more may run on this GPU
            pytest.exit(f"GPU fault in {what}: {e}", returncode=3)
        raise


# ====================================================================== bf16 engines
def run_bf16(c, plan_check=True):
    """Runs one bf16 case on the GPU and checks everything; returns the Report (call .finish())."""
    e = ops.kernels._ext()
    rep = R.Report(c.id)
    M, N, K, epi = c.M, c.N, c.K, c.epi
    if not c.v1 and plan_check:
        k, s = e.gemm2_plan(M, N, K, c.tA, c.tB, c.acc, c.cfg)
        assert f"cfg{k}.s{s}" == c.path, f"gemm2_plan answers cfg{k}.s{s}"
        if c.group == "splitk" and s > 1:
            assert (K // R.BK) % s != 0, "the split is meant to be uneven"
    x = R.make_inputs(c)
    # dropout indexes its mask, and the separate column-sum pass reads C, as a contiguous [M, N]
    side = 0 if c.p or (c.colsum and (c.acc or c.split > 1 or c.v1)) else 8
    rA = place(c, "lda", *((K, M) if c.tA else (M, K)), BF16, SENT_IN, x.a.t() if c.tA else x.a)
    rB = place(c, "ldb", *((K, N) if c.tB else (N, K)), BF16, SENT_IN, x.b.t() if c.tB else x.b)
    ins, outs = [rA, rB], []
    rC = place(c, "ldc", M, N, F32 if c.acc else BF16, SENT_OUT, x.c0 if c.acc else None, side=side)
    outs.append(rC)
    bias = res = aux = cs = None
    if "bias" in epi:
        rb = vector(N, BF16, SENT_IN, x.bias)
        bias = rb.view
        ins.append(rb)
    if epi in ("res", "bias_res"):
        rr = place(c, "ldr", M, N, BF16, SENT_IN, x.r, side=16)
        res = rr.view
        ins.append(rr)
    if epi in ("dgelu", "drelu"):
        rx = matrix(M, N, BF16, SENT_IN, x.aux, side=24)
        aux = rx.view
        ins.append(rx)
    if epi in ("bias_gelu", "bias_relu"):
        rx = place(c, "ldx", M, N, BF16, SENT_OUT, None, side=24)
        aux = rx.view
        outs.append(rx)
    if c.colsum:
        rcs = vector(N, F32, SENT_OUT, COLSUM0)
        cs = rcs.view
    seed = 4321 + c.seed
    keep = keep_mask(M, N, c.p, seed) if c.p else None
    snap = [r.snap() for r in ins]
    code = R.EPI[epi]

    def call():
        if c.v1:
            assert e.gemm2(rA.view, rB.view, rC.view, bias, res, aux, c.tA, c.tB, code, c.acc, c.alpha, c.cfg, cs,
                           c.p, seed) == 0, "gemm2 took a call with M % 8 != 0"
            e.gemm(rA.view, rB.view, rC.view, bias, res, aux, c.tA, c.tB, code, c.acc, c.alpha)
            rc = 2
        else:
            rc = e.gemm2(rA.view, rB.view, rC.view, bias, res, aux, c.tA, c.tB, code, c.acc, c.alpha, c.cfg, cs, c.p, seed)
            assert rc in (1, 2), f"gemm2 refused the call ({rc})"
            fused = cs is not None and not c.acc and c.split == 1
            assert rc == (1 if cs is None or fused else 2), f"gemm2 answered {rc}"
        if rc == 2 and cs is not None:
            e.colsum(rC.view, cs)

    call()
    first = [r.view.clone() for r in outs]
    cs_got = None if cs is None else cs.to("cpu", copy=True)
    for r in outs:
        r.view.copy_(x.c0.to(DEV)) if (r is rC and c.acc) else r.view.fill_(float("nan"))
    if cs is not None:
        cs.fill_(COLSUM0)
    call()
    torch.cuda.synchronize()
    rep.expect(all(bits_equal(a, r.view) for a, r in zip(first, outs)), "second run differs")
    rep.expect(all(r.same(s) for r, s in zip(ins, snap)), "an input or its padding changed")
    rep.expect(all(r.padding_intact() for r in outs), "padding of an output was written")
    if cs is not None:
        rep.expect(rcs.padding_intact(), "padding of colsum was written")

    got = dict(out=rC.view.cpu(), aux=aux.cpu() if epi in ("bias_gelu", "bias_relu") else None, colsum=cs_got)
    fused = cs is not None and not c.v1 and not c.acc and c.split == 1
    got["colsum_key"] = ("colsum_act" if epi in ("bias_gelu", "bias_relu") else "colsum") if fused else "colsum_sep"
    ref = R.gemm_ref(rA.view, rB.view, c.tA, c.tB, c.alpha, epi, bias=bias, R=res, aux=aux if code >= 6 else None,
                     C0=x.c0 if c.acc else None, keep=keep,
                     stored=got["out"] if cs is not None and got["colsum_key"] != "colsum" else None,
                     colsum0=torch.full((N,), COLSUM0) if cs is not None else None)
    if keep is not None:
        zero_ok = bool((got["out"].double()[keep == 0] == 0).all())
        rep.expect(zero_ok, "a dropped element is not 0: the mask differs from act_fwd's")
        rate = float((keep != 0).double().mean())
        rep.expect(abs(rate - (1 - c.p)) < 5 * (c.p * (1 - c.p) / keep.numel()) ** 0.5, f"keep rate {rate:.4f}")
    R.check_outputs(rep, c.cls, ref, got, epi, old=c.kind not in ("big", "tiny", "gelumax"))
    if x.want is not None and epi == "none":
        want = c.alpha * x.want + (x.c0.double() if c.acc else 0)
        rep.exact("exact inputs", got["out"], want.to(got["out"].dtype))
    return rep


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_gemm_bf16_edges(c):
    guarded(lambda: run_bf16(c), c.id).finish()


# ====================================================================== f32 engines
def f32_plan_path(M, N, K, ks):
    big, split, sk_grid, sk_chunk = ops.kernels._ext().gemm_f32_plan(M, N, K, ks)
    if sk_grid > 0:
        return "f32.sk", sk_chunk
    return ("f32.128" if big else "f32.64") + (f".s{split}" if split > 1 else ""), 0


def run_f32(c, path=None):
    e = ops.kernels._ext()
    rep = R.Report(c.id)
    M, N, K, epi = c.M, c.N, c.K, c.epi
    got_path, chunk = f32_plan_path(M, N, K, c.ks)
    assert got_path == (path or c.path), f"gemm_f32_plan answers {got_path}"
    npairs = -(-K // 64)
    if c.ks == -2:   # a chunk ends inside a tile; one of npairs + 2 units or more spans three tiles
        assert chunk % npairs != 0 and (npairs > chunk or chunk >= npairs + 2), (chunk, npairs)
    if c.ks > 1:
        assert npairs >= 2 * c.ks, "a split the planner itself could not choose"
    x = R.make_inputs(c)
    # A [M, K] / B [K, N] views: 'n' = K-contiguous A / N-contiguous B as torch.mm sees them
    rA = place(c, "lda", *((M, K) if c.layout[0] == "n" else (K, M)), F32, SENT_IN, x.a if c.layout[0] == "n" else x.a.t())
    rB = place(c, "ldb", *((N, K) if c.layout[1] == "t" else (K, N)), F32, SENT_IN, x.b if c.layout[1] == "t" else x.b.t())
    A = rA.view if c.layout[0] == "n" else rA.view.t()
    B = rB.view.t() if c.layout[1] == "t" else rB.view
    rC = place(c, "ldc", M, N, F32, SENT_OUT, x.c0 if c.acc else None)
    ins, outs = [rA, rB], [rC]
    bias = res = X = None
    if "bias" in epi:
        rb = vector(N, F32, SENT_IN, x.bias)
        bias = rb.view
        ins.append(rb)
    if epi in ("res", "bias_res", "drelu"):
        rr = place(c, "ldr", M, N, F32, SENT_IN, x.r, side=16)
        res = rr.view
        ins.append(rr)
    if epi == "bias_relu":
        rx = place(c, "ldx", M, N, F32, SENT_OUT, None, side=24)
        X = rx.view
        outs.append(rx)
    seed = 4321 + c.seed
    # the f32 epilogues hash (seed, row * N + col) as act_fwd does for a contiguous [M, N]:
    # the mask is regenerated independently of the path under test
    keep = keep_mask(M, N, c.p, seed) if c.p else None
    snap = [r.snap() for r in ins]

    def call():
        assert e.gemm_f32_ex(A, B, rC.view, bias, res, X, R.F32_EPI[epi], c.alpha, c.acc, c.p, seed, c.ks) == 1

    call()
    first = [r.view.clone() for r in outs]
    for r in outs:
        r.view.copy_(x.c0.to(DEV)) if (r is rC and c.acc) else r.view.fill_(float("nan"))
    call()
    torch.cuda.synchronize()
    rep.expect(all(bits_equal(a, r.view) for a, r in zip(first, outs)), "second run differs")
    rep.expect(all(r.same(s) for r, s in zip(ins, snap)), "an input or its padding changed")
    rep.expect(all(r.padding_intact() for r in outs), "padding of an output was written")
    got = dict(out=rC.view.cpu(), aux=None if X is None else X.cpu())
    if c.p:
        rep.expect(bool((got["out"].double()[keep == 0] == 0).all()), "a dropped element is not 0: the mask differs from act_fwd's")
    ref = R.gemm_ref(A, B.t(), alpha=c.alpha, epi=epi, bias=bias, R=res, C0=x.c0 if c.acc else None, keep=keep, f32=True)
    cls = path or c.cls
    R.check_outputs(rep, "f32.128" if cls.startswith("f32.128") else cls, ref, got, epi, old=c.kind not in ("big", "tiny"))
    if x.want is not None and epi == "none":
        want = c.alpha * (A.double().cpu() @ B.double().cpu()) + (x.c0.double() if c.acc else 0)
        rep.exact("exact inputs", got["out"], want.float())
    return rep


@pytest.mark.parametrize("c", R.F32_CASES, ids=lambda c: c.id)
def test_gemm_f32_edges(c):
    guarded(lambda: run_f32(c), c.id).finish()


def test_gemm_f32_dropout_mask_fwd_bwd():
    """bias+ReLU and dReLU regenerate one mask from (seed, row * N + col) on the tiled, the split
    and the stream-K path at one (M, N), the mask act_fwd makes for a contiguous [M, N]; the
    128x128 engine's is compared in its child process through the cases with p > 0."""
    e = ops.kernels._ext()
    M, N = 264, 136
    want = keep_mask(M, N, 0.25, 99) != 0
    for K, ks, path in ((100, 1, "f32.64"), (420, 3, "f32.64.s3"), (4132, -2, "f32.sk")):
        assert f32_plan_path(M, N, K, ks)[0] == path
        A, B = torch.ones(M, K, device=DEV), torch.ones(K, N, device=DEV)
        bias, pre = torch.ones(N, device=DEV), torch.ones(M, N, device=DEV)
        y, X, dx = (torch.full((M, N), float("nan"), device=DEV) for _ in range(3))
        assert e.gemm_f32_ex(A, B, y, bias, None, X, 2, 1.0, False, 0.25, 99, ks) == 1
        assert e.gemm_f32_ex(A, B, dx, None, pre, None, 5, 1.0, False, 0.25, 99, ks) == 1
        assert torch.equal((y != 0).cpu(), want), f"{path}: forward mask differs from act_fwd's"
        assert torch.equal((dx != 0).cpu(), want), f"{path}: backward mask differs from act_fwd's"


# ====================================================================== grouped TT
GROUPED = {
    "one-smallest": [(8, 8, 64)],
    "two-ragged": [(136, 200, 192), (200, 136, 320)],
    "eight": [(64, 64, 64), (8, 8, 64), (136, 200, 192), (72, 8, 320), (8, 8, 64), (200, 136, 64), (8, 72, 192),
              (64, 128, 320)],
    # value ranges (see gemm_refs.make_inputs) and one operand at a time with rows BIG_LD apart
    # (dy / x have T = 320 rows, C 264: row x stride leaves 32 bits)
    "ranges": [(136, 200, 192, "big"), (136, 200, 192, "tiny"), (136, 200, 192, "zerorow")],
    "stride-dy": [(72, 136, 320, "lda"), (8, 8, 64)],
    "stride-x": [(72, 136, 320, "ldb"), (8, 8, 64)],
    "stride-c": [(264, 72, 192, "ldc"), (8, 8, 64)],
}


@pytest.mark.parametrize("name", list(GROUPED))
def test_gemm_tt_grouped_edges(name):
    """gemms_tt_grouped_kernel: C_g [N, K] += alpha dy_g^T x_g for 1, 2 and 8 problems in one
    launch, row-strided dy / x / C, the smallest problem (one 8x8 corner of one tile) between
    larger ones, alpha = 0.5; plus two jobs into the halves of one gradient."""
    e = ops.kernels._ext()
    rep = R.Report(f"grouped-{name}")
    probs = GROUPED[name]
    regs, ins, outs, c0s = [], [], [], []
    old = True
    for i, (N, K, T, *kind) in enumerate(probs):
        kind = kind[0] if kind else "randn"
        g = torch.Generator().manual_seed(i)
        dy, xx = torch.randn(T, N, generator=g), torch.randn(T, K, generator=g) * (T ** -0.5)
        if kind in ("big", "tiny"):
            dy, xx, old = dy * 2.0 ** (60 if kind == "big" else -50), xx * 2.0 ** (62 if kind == "big" else -50), False
        if kind == "zerorow":
            dy[:, 3] = 0       # a zero row of A = dy^T
        dy, xx = dy.to(BF16), xx.to(BF16)
        c0 = torch.randint(-8, 9, (N, K), generator=g).float()
        c = R.NS(stride=kind if kind.startswith("ld") else None)
        rdy, rx = place(c, "lda", T, N, BF16, SENT_IN, dy), place(c, "ldb", T, K, BF16, SENT_IN, xx, side=16)
        rc = place(c, "ldc", N, K, F32, SENT_OUT, c0)
        ins += [rdy, rx]
        outs.append(rc)
        c0s.append(c0)
        regs.append((rdy, rx, rc))
    snap = [r.snap() for r in ins]

    def call():
        e.gemm_tt_grouped([r[0].view for r in regs], [r[1].view for r in regs], [r[2].view for r in regs], 0.5)

    guarded(call, name)
    first = [r.view.clone() for r in outs]
    for r, c0 in zip(outs, c0s):
        r.view.copy_(c0.to(DEV))
    guarded(call, name)
    torch.cuda.synchronize()
    rep.expect(all(bits_equal(a, r.view) for a, r in zip(first, outs)), "second run differs")
    rep.expect(all(r.same(s) for r, s in zip(ins, snap)), "an input or its padding changed")
    rep.expect(all(r.padding_intact() for r in outs), "padding of an output was written")
    for (rdy, rx, rc), c0 in zip(regs, c0s):
        ref = R.gemm_ref(rdy.view, rx.view, True, True, 0.5, C0=c0)
        R.check_outputs(rep, "grouped", ref, dict(out=rc.view.cpu()), old=old)
    rep.finish()


def test_gemm_tt_grouped_halves_of_one_gradient():
    """two jobs write the upper and the lower half of one [2 N, K] gradient (a fused QKV-style
    weight): neither touches the other's rows; exact inputs, bit for bit"""
    e = ops.kernels._ext()
    N, K, T = 136, 200, 192
    rc = matrix(2 * N, K, F32, SENT_OUT, torch.zeros(2 * N, K))
    wants, dys, xs = [], [], []
    for h in range(2):
        a, b, want = R.exact_inputs("twohot", N, K, T)      # a [N, T] one/two-hot, b [K, T]
        dys.append(matrix(T, N, BF16, SENT_IN, a.t()).view)
        xs.append(matrix(T, K, BF16, SENT_IN, b.t() if h == 0 else -b.t()).view)
        wants.append(want if h == 0 else -want)
    guarded(lambda: e.gemm_tt_grouped(dys, xs, [rc.view[:N], rc.view[N:]], 0.5), "halves")
    torch.cuda.synchronize()
    assert rc.padding_intact()
    assert torch.equal(rc.view.cpu().double(), 0.5 * torch.cat(wants))


# ====================================================================== wrappers
def test_wrappers_dispatch():
    """ops.linear, linear_dx (with and without wt, with colsum, and the few-tiles-long-K split
    branch) and linear_dw once each through the same check: the dispatch of ops/kernels.py."""
    rep = R.Report("wrappers")
    T, N, K = 320, 192, 128
    x = R.randn_inputs(T, N, K, 77)
    xg, wg, bg, rg = (t.to(DEV) for t in (x.a, x.b, x.bias, x.r))
    plan = ops.kernels._ext().gemm2_plan
    assert plan(T, N, K, False, False, False, -1) == (12, 1)      # linear: the small NT engine
    assert plan(T, K, N, False, False, False, -1) == (12, 1)      # linear_dx with wt
    assert plan(N, K, T, True, True, True, -1) == (13, 1)         # linear_dw: the small TT engine
    # linear_dx without wt is A @ B with B [K, N] (transB): no v2 engine is instantiated for it,
    # so gemm2 must hand it back (0) and the wrapper's v1 fallback computes it
    assert ops.kernels._ext().gemm2(x.r.to(DEV), wg, torch.empty(T, K, dtype=BF16, device=DEV), None, None, None, False,
                                    True, 0, False, 1.0, -1, None, 0.0, 0) == 0
    y, aux = ops.linear(xg, wg, bg, act="gelu_tanh")
    ref = R.gemm_ref(x.a, x.b, epi="bias_gelu", bias=x.bias)
    R.check_outputs(rep, "snt", ref, dict(out=y.cpu(), aux=aux.cpu()), "bias_gelu")
    y, _ = ops.linear(xg, wg, bg, residual=rg)
    R.check_outputs(rep, "snt", R.gemm_ref(x.a, x.b, epi="bias_res", bias=x.bias, R=x.r), dict(out=y.cpu()), "bias_res")
    # dx = dy @ w: dy [T, N], w [N, K]
    dy, w = x.r.to(DEV), x.b.to(DEV)
    wt = w.t().contiguous()
    dx = ops.linear_dx(dy, w)                                 # transB on v1
    ref = R.gemm_ref(x.r, x.b, transB=True)
    R.check_outputs(rep, "v1", ref, dict(out=dx.cpu()))
    cs = torch.full((K,), COLSUM0, device=DEV)
    gd = (torch.randn(T, K, generator=torch.Generator().manual_seed(5)) * 0.5).to(BF16)
    dx = ops.linear_dx(dy, w, act_input=gd.to(DEV), act="gelu_tanh", wt=wt, colsum=cs)
    ref = R.gemm_ref(x.r, wt.cpu(), epi="dgelu", aux=gd, colsum0=torch.full((K,), COLSUM0))
    R.check_outputs(rep, "snt", ref, dict(out=dx.cpu(), colsum=cs.cpu()), "dgelu")
    # few output tiles, long reduction: f32 split-K accumulate, then one cast
    Tn, Nl, Kd = 64, 4160, 128
    g = torch.Generator().manual_seed(6)
    dl, wl = torch.randn(Tn, Nl, generator=g).to(BF16), (torch.randn(Nl, Kd, generator=g) * Nl ** -0.5).to(BF16)
    wlt = wl.t().contiguous().to(DEV)
    assert plan(Tn, Kd, Nl, False, False, True, -1) == (2, 13)    # 65 K-tiles in 13 splits
    dx = ops.linear_dx(dl.to(DEV), wl.to(DEV), wt=wlt)
    R.check_outputs(rep, "skepi", R.gemm_ref(dl, wlt.cpu()), dict(out=dx.cpu()))   # f32 slabs, one cast: one rounding
    dw0 = torch.randint(-8, 9, (N, K), generator=g).float()
    dw = ops.linear_dw(dy, xg, dw0.to(DEV).clone(), alpha=0.5)   # dy [T, N], x [T, K]
    R.check_outputs(rep, "stt", R.gemm_ref(x.r, x.a, True, True, 0.5, C0=dw0), dict(out=dw.cpu()))
    # two groupable jobs of one alpha go out as one grouped launch
    g1, g2 = dw0.to(DEV).clone(), dw0.to(DEV).clone()
    jobs = [ops.kernels.DW(dy, xg, g1, 0.5), ops.kernels.DW(xg, dy, g2.t().contiguous(), 0.5)]
    assert all(j.groupable() for j in jobs)
    ops.kernels.run_wjobs(jobs)
    R.check_outputs(rep, "grouped", R.gemm_ref(x.r, x.a, True, True, 0.5, C0=dw0), dict(out=g1.cpu()))
    R.check_outputs(rep, "grouped", R.gemm_ref(x.a, x.r, True, True, 0.5, C0=dw0.t()), dict(out=jobs[1].dw.cpu()))
    rep.finish()


# ====================================================================== argument checks
def _bf(*s, fill=1.0):
    return torch.full(s, fill, dtype=BF16, device=DEV)


def test_binding_checks_gemm():
    """gemm / gemm2 look at every tensor on the host before any launch; each bad call raises,
    names the argument, and leaves the sentinel-filled C untouched."""
    e = ops.kernels._ext()
    M, N, K = 64, 72, 128

    def args():
        return dict(A=_bf(M, K), B=_bf(N, K), C=_bf(M, N, fill=SENT_OUT), bias=_bf(N), residual=_bf(M, N), aux=_bf(M, N),
                    transA=False, transB=False, epilogue=0, accum=False, alpha=1.0)

    wide = lambda t: torch.full((t.shape[0], 2 * t.shape[1]), SENT_OUT, dtype=t.dtype, device=DEV)[:, ::2]   # noqa: E731
    odd = lambda t: torch.full((t.shape[0], t.shape[1] + 4), SENT_OUT, dtype=t.dtype, device=DEV)[:, :t.shape[1]]   # noqa: E731
    off = lambda t: torch.full((t.shape[0], t.shape[1] + 8), SENT_OUT, dtype=t.dtype, device=DEV)[:, 4:4 + t.shape[1]]   # noqa: E731
    bad = []    # (edits, extra gemm2 keywords, word the message must hold)
    for name in ("A", "B", "C"):
        word = f": {name} "     # as in "gemm2: A must be ...": not any message that happens to hold the letter
        bad += [({name: lambda t: t.float()}, {}, word), ({name: lambda t: t.cpu()}, {}, word),
                ({name: lambda t: t.reshape(-1)}, {}, word), ({name: lambda t: t[None]}, {}, word),
                ({name: wide}, {}, word), ({name: odd}, {}, word), ({name: off}, {}, word)]
    bad += [({"accum": lambda _: True}, {}, "accumulate needs f32 C"),
            ({"A": lambda t: t[:0]}, {}, ": A is empty"), ({"B": lambda t: t[:0]}, {}, ": B is empty"),
            ({"A": lambda t: t[:, :0], "B": lambda t: t[:, :0]}, {}, ": A is empty"),
            ({"A": lambda t: t[:M - 8]}, {}, "A/M mismatch"), ({"B": lambda t: t[:N - 8]}, {}, "B mismatch"),
            ({"epilogue": lambda _: 8}, {}, "epilogue"), ({"epilogue": lambda _: -1}, {}, "epilogue")]
    for epi, name in ((1, "bias"), (2, "bias"), (3, "bias"), (4, "bias"), (4, "residual"), (5, "residual"), (2, "aux"),
                      (3, "aux"), (6, "aux"), (7, "aux")):
        ed = {"epilogue": lambda _, v=epi: v}
        bad += [(dict(ed, **{name: lambda t: None}), {}, name), (dict(ed, **{name: lambda t: t.float()}), {}, name),
                (dict(ed, **{name: lambda t: t.cpu()}), {}, name)]
        if name == "bias":
            bad += [(dict(ed, bias=lambda t: t[: N - 8]), {}, "bias"), (dict(ed, bias=lambda t: _bf(2 * N)[::2]), {}, "bias"),
                    (dict(ed, bias=lambda t: _bf(N + 8)), {}, "bias")]
        else:
            bad += [(dict(ed, **{name: lambda t: t[: M - 8]}), {}, name), (dict(ed, **{name: lambda t: t.reshape(-1)}), {}, name),
                    (dict(ed, **{name: wide}), {}, name), (dict(ed, **{name: odd}), {}, name)]
    strided_c = lambda t: torch.full((M, N + 8), SENT_OUT, dtype=BF16, device=DEV)[:, :N]   # noqa: E731
    bad += [({"epilogue": lambda _: 3, "C": strided_c}, {"p_drop": 0.1}, "contiguous C"),
            ({"epilogue": lambda _: 1}, {"p_drop": 0.1}, "p_drop"), ({"epilogue": lambda _: 5}, {"p_drop": 0.1}, "p_drop"),
            ({"epilogue": lambda _: 3}, {"p_drop": 1.0}, "p_drop"), ({"epilogue": lambda _: 3}, {"p_drop": -0.1}, "p_drop"),
            ({}, {"colsum": torch.zeros(N)}, "colsum"), ({}, {"colsum": torch.zeros(N, device=DEV, dtype=torch.float64)}, "colsum"),
            ({}, {"colsum": torch.zeros(N - 8, device=DEV)}, "colsum"), ({}, {"colsum": torch.zeros(2 * N, device=DEV)[::2]}, "colsum")]
    if torch.cuda.device_count() > 1:
        for name in ("B", "C"):
            bad.append(({name: lambda t: t.to("cuda:1")}, {}, f": {name} "))
    for edits, kw, word in bad:
        for fn in ("gemm2", "gemm"):
            if fn == "gemm" and kw:
                continue
            a = args()
            for name, f in edits.items():
                a[name] = f(a[name])
            what = f"{fn} {sorted(edits)} {sorted(kw)}"
            with pytest.raises(RuntimeError) as ei:
                if fn == "gemm":
                    e.gemm(*a.values())
                else:
                    e.gemm2(*a.values(), force_cfg=-1, colsum=kw.get("colsum"), p_drop=kw.get("p_drop", 0.0), seed=1)
                pytest.fail(f"accepted: {what}")
            assert word in str(ei.value), f"{what}: message does not name it ({word!r}): {ei.value}"
            torch.cuda.synchronize()
            C = a["C"]
            if C.is_cuda and C.dtype == BF16:
                assert bool((C == SENT_OUT).all()), f"{what}: C was written"
    # valid neighbours of the refused calls still run: a [1, K] row with any row stride, an unused bias
    e.gemm2(_bf(8, K), _bf(N, K), _bf(8, N), _bf(3).float(), None, None, False, False, 0, False, 1.0, -1, None, 0.0, 0)
    torch.cuda.synchronize()


def test_binding_checks_grouped_f32_transpose():
    e = ops.kernels._ext()
    T, N, K = 64, 8, 16
    dy, x, C = _bf(T, N), _bf(T, K), torch.zeros(N, K, device=DEV)
    for bad in ((dy.float(), x, C), (dy, x.float(), C), (dy, x, C.to(BF16)), (dy.cpu(), x, C), (dy, x.cpu(), C),
                (dy, x, C.cpu()), (dy.reshape(-1), x, C), (dy, x, C.reshape(-1)), (dy[:0], x[:0], C),
                (_bf(T, 2 * N)[:, ::2], x, C), (dy, _bf(T, K + 4)[:, :K], C), (dy, x, torch.zeros(N, K + 2, device=DEV)[:, :K]),
                (dy[:32], x, C), (dy, x, torch.zeros(N, K + 4, device=DEV)[:, 1:K + 1])):
        with pytest.raises(RuntimeError, match="gemm_tt_grouped"):
            e.gemm_tt_grouped([bad[0]], [bad[1]], [bad[2]], 1.0)
    with pytest.raises(RuntimeError, match="gemm_tt_grouped"):
        e.gemm_tt_grouped([dy] * 9, [x] * 9, [C] * 9, 1.0)
    torch.cuda.synchronize()
    assert bool((C == 0).all())
    M, N, K = 8, 12, 16
    A, B, Cf = torch.ones(M, K, device=DEV), torch.ones(K, N, device=DEV), torch.full((M, N), SENT_OUT, device=DEV)
    b, Rr = torch.ones(N, device=DEV), torch.ones(M, N, device=DEV)
    ok = dict(A=A, B=B, C=Cf, bias=None, R=None, X=None, epi=0, alpha=1.0, accumulate=False, p_drop=0.0, seed=0, force_ks=1)
    for ed in (dict(A=A.cpu()), dict(B=B.cpu()), dict(C=Cf.cpu()), dict(A=A.double()), dict(B=B.to(BF16)), dict(A=A.reshape(-1)),
               dict(C=Cf[None]), dict(A=A[:0], C=Cf[:0]), dict(A=A[:, :0], B=B[:0]), dict(epi=1), dict(epi=1, bias=b.cpu()),
               dict(epi=1, bias=b.double()), dict(epi=1, bias=b[:8]), dict(epi=3), dict(epi=3, R=Rr.cpu()), dict(epi=3, R=Rr[:4]),
               dict(epi=2, bias=b), dict(epi=2, bias=b, X=Rr.cpu()), dict(epi=6), dict(epi=-1), dict(p_drop=0.1),
               dict(epi=1, bias=b, p_drop=0.1), dict(epi=2, bias=b, X=Rr, p_drop=1.0), dict(epi=2, bias=b, X=Rr, p_drop=-0.5)):
        with pytest.raises(RuntimeError, match="gemm_f32_ex"):
            e.gemm_f32_ex(**dict(ok, **ed))
    for bad in ((A.cpu(), B, Cf), (A, B.cpu(), Cf), (A, B, Cf.cpu()), (A.double(), B, Cf), (A.reshape(-1), B, Cf), (A[:0], B, Cf[:0])):
        with pytest.raises(RuntimeError, match="gemm_f32"):
            e.gemm_f32(*bad, None, 1.0, False)
    with pytest.raises(RuntimeError, match="gemm_f32"):
        e.gemm_f32(A, B, Cf, b.cpu(), 1.0, False)
    torch.cuda.synchronize()
    assert bool((Cf == SENT_OUT).all())
    t_in, t_out = _bf(16, 24), _bf(24, 16, fill=SENT_OUT)
    for bad in ((t_in.cpu(), t_out), (t_in, t_out.cpu()), (t_in.float(), t_out), (t_in, t_out.float()), (t_in.reshape(-1), t_out),
                (t_in, _bf(16, 24)), (t_in[:0], t_out[:, :0]), (_bf(16, 48)[:, ::2], t_out)):
        with pytest.raises(RuntimeError, match="transpose"):
            e.transpose(*bad)
    torch.cuda.synchronize()
    assert bool((t_out == SENT_OUT).all())


def test_gemm8_refuses_row_strides_beyond_32_bits():
    """gemm8 (cfg 15 / 16) addresses a tile's 256 rows through 32-bit buffer offsets.  A row
    stride of 2^23 + 8 elements at 264 rows passes 2^31 bytes: its launcher hands the call back
    (gemm2 answers 0, the caller's v1 fallback takes it) before any launch, for A and for B
    alike, and takes the same shapes at an ordinary stride.  The buffer is never touched."""
    e = ops.kernels._ext()
    M = N = 264
    K, ld = 64, (1 << 23) + 8
    big = torch.empty(M, ld, dtype=BF16, device=DEV)[:, 8: 8 + K]
    small = _bf(M, K)
    for cfg in (15, 16):
        for A, B in ((big, small), (small, big)):
            C = _bf(M, N, fill=SENT_OUT)
            assert e.gemm2(A, B, C, None, None, None, False, False, 0, False, 1.0, cfg, None, 0.0, 0) == 0
            torch.cuda.synchronize()
            assert bool((C == SENT_OUT).all())
        C = _bf(M, N, fill=SENT_OUT)
        assert e.gemm2(small, small, C, None, None, None, False, False, 0, False, 1.0, cfg, None, 0.0, 0) == 1
        torch.cuda.synchronize()
        assert bool((C == K).all())


# ====================================================================== non-default builds
CHILDREN = {
    # name: (environment, cases).  The 32x32x16 build of the gemm2 tile family (NT), its
    # 16x16x32 build for the k-major (TT) operands, and the 128x128 f32 engine forced on
    # small and ragged grids and on its split.
    "m16-0": ({"MIPIPE_GEMM_M16": "0"}, [c for c in R.CASES if not c.v1 and not c.tA and c.engine in (0, 1, 2, 3)
                                         and c.group in ("shape", "epi", "exact", "splitk")]),
    "m16t-1": ({"MIPIPE_GEMM_M16T": "1"}, [c for c in R.CASES if not c.v1 and c.tA and c.engine in (0, 2, 3)]),
    "f32-tile128": ({"MIPIPE_F32_TILE": "128"}, [c for c in R.F32_CASES if c.ks in (0, 1, 2, 3) and c.group != "big"]),
}


def f32_big_path(c):
    """the path of an f32 case under MIPIPE_F32_TILE=128: the 128x128 engine, split only where
    its own rule (nkt >= 2 s) allows the forced factor"""
    return "f32.128" + (f".s{c.ks}" if c.ks > 1 else "")


@pytest.fixture(scope="module")
def child_runs():
    res = {}
    for name, (envs, _) in CHILDREN.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith(("MIPIPE_GEMM", "MIPIPE_F32"))}
        env.update(envs)
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), name]
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as ex:
            res[name] = (None, f"timed out: {ex}")
            break
        print(p.stdout)
        res[name] = (p.returncode, p.stdout[-4000:] + p.stderr[-4000:])
        if p.returncode != 0:
            break
    return res


@pytest.mark.parametrize("name", list(CHILDREN))
def test_nondefault_builds(child_runs, name):
    assert name in child_runs, "not started: the child before it failed"
    rc, out = child_runs[name]
    assert rc == 0, out
    assert f"child {name}: {len(CHILDREN[name][1])} cases ok" in out, out


if __name__ == "__main__":
    assert torch.cuda.is_available() and ops.ext_available()
    which = sys.argv[1]
    envs, cases = CHILDREN[which]
    assert all(os.environ.get(k) == v for k, v in envs.items()), "start me with the child's environment"
    ops.set_dropout_step(DROP_STEP, torch.device(DEV))
    fails = []
    for case in cases:
        # forced cfgs plan alike in these builds; the f32 planner is asked again in run_f32
        rep_ = run_bf16(case) if case.prec == "bf16" else run_f32(case, f32_big_path(case))
        fails += rep_.fails
    torch.cuda.synchronize()
    if fails:
        print("\n".join(fails))
        sys.exit(1)
    print(f"child {which}: {len(cases)} cases ok")
