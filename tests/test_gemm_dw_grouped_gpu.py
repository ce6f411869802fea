"""Edge cases of the grouped long-token weight-gradient engine (csrc/kernels/gemm2.hip
gemm3_tt_grouped_kernel + splitk_reduce_grouped_kernel, binding ``gemm_dw_grouped``) against the
float64 reference of gemm_refs.py, at the binding level.

C_g [M_g, N_g] (f32) += alpha dy_g^T x_g for up to 8 problems over one token count T, 256x256
tiles, one split-K factor S for the group.  Every operand is a view into a sentinel-padded,
row-strided buffer (the helpers of test_gemm_edges_gpu.py, re-implemented here); every call runs
twice from the same C0 and must repeat bit for bit, leave its inputs and all padding alone, and
stay inside gemm_refs.BOUND: 'g3tt.acc' where the engine ran with S = 1 (gemm3's TT tile with the
read-modify-write epilogue), 'skred.acc' where it went through slabs and the reduce pass --
the bounds the one-problem engine has for the same two paths; only the summation order differs.

K-loop: T = 64 with S forced to 2 (clamps to 1), T = 128 / S = 2 (one K-tile per split, the
nk == 1 prologue), T = 192 / S = 2 (1 + 2 K-tiles), T = 320 / S = 3, T = 320 / S = 1 (direct
epilogue onto a non-zero integer C0), T = 320 with the planner's own S.
Tiles: (8, 8) one corner of one tile, (264, 264) 2 x 2 tiles with 8-wide ragged edges,
(256, 512) exact tiles, (136, 200).  Groups: 1, 2, 3 and 8 problems of mixed shapes, the 8 x 8
problem between larger ones; two problems into the halves of one gradient with exact inputs.
Strides: one operand at a time with rows BIG_LD elements apart.

The fused bias column sum of the issue is not built (the kernel has 236 of 256 VGPRs in use and
the sum needs 32 more), so it has no cases here."""
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
BIG_COL = 4104


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
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


def matrix(rows, cols, dtype, pad, init, side=8, big=False):
    """the view [rows, cols] holding ``init`` as a column slice of a wider buffer of ``pad``
    (``big``: of an uninitialised buffer whose rows are BIG_LD elements apart)"""
    if big:
        buf = torch.empty(rows + 1, R.BIG_LD, dtype=dtype, device=DEV)
        c0, c1 = BIG_COL, BIG_COL + cols
        buf[:, c0 - 8: c1 + 8] = pad
        view = buf[:rows, c0:c1]
        guards = [(slice(None), slice(c0 - 8, c0)), (slice(None), slice(c1, c1 + 8)),
                  (slice(rows, None), slice(c0 - 8, c1 + 8))]
    else:
        buf = torch.full((rows + PAD_ROWS, cols + 2 * side), pad, dtype=dtype, device=DEV)
        view = buf[:rows, side: side + cols]
        guards = [(slice(None), slice(0, side)), (slice(None), slice(side + cols, None)),
                  (slice(rows, None), slice(None))]
    view.copy_(init.to(DEV))
    return Region(buf, view, guards, pad)


def guarded(fn, what):
    try:
        return fn()
    except RuntimeError as e:
        if "HIP error" in str(e):   # a fault poisons the context: nothing more may run on this GPU
            pytest.exit(f"GPU fault in {what}: {e}", returncode=3)
        raise


# name: (T, forced S (0: the planner's), S the binding must report, alpha, [(M, N[, big operand])])
EIGHT = [(136, 200), (8, 8), (264, 264), (72, 8), (256, 512), (8, 72), (200, 136), (64, 128)]
CASES = {
    "T64-S2-clamps-to-1": (64, 2, 1, 1.0, [(136, 200), (8, 8)]),
    "T128-S2-one-ktile-each": (128, 2, 2, 1.0, [(264, 264), (8, 8), (136, 200)]),
    "T192-S2-uneven-one-problem": (192, 2, 2, 1.0, [(256, 512)]),
    "T320-S3-eight": (320, 3, 3, 0.5, EIGHT),
    "T320-S1-direct": (320, 1, 1, 0.5, [(264, 264), (8, 8), (136, 200)]),
    "T320-S1-eight": (320, 1, 1, 1.0, EIGHT),
    "T320-planner": (320, 0, 1, 1.0, [(136, 200), (264, 264)]),
    "T1024-planner": (1024, 0, None, 1.0, [(264, 264), (8, 8)]),
    "T320-S2-one-smallest": (320, 2, 2, 1.0, [(8, 8)]),
    "stride-dy": (320, 2, 2, 0.5, [(72, 136, "dy"), (8, 8)]),
    "stride-x": (320, 2, 2, 0.5, [(72, 136, "x"), (8, 8)]),
    "stride-c-S2": (192, 2, 2, 0.5, [(264, 72, "c"), (8, 8)]),
    "stride-c-S1": (192, 1, 1, 0.5, [(264, 72, "c"), (8, 8)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_dw_grouped_edges(name):
    e = ops.kernels._ext()
    T, force, want_s, alpha, probs = CASES[name]
    rep = R.Report(f"dwgroup-{name}")
    regs, c0s = [], []
    for i, (M, N, *big) in enumerate(probs):
        big = big[0] if big else ""
        g = torch.Generator().manual_seed(100 + i)
        dy, xx = torch.randn(T, M, generator=g).to(BF16), (torch.randn(T, N, generator=g) * (T ** -0.5)).to(BF16)
        c0 = torch.randint(-8, 9, (M, N), generator=g).float()
        regs.append((matrix(T, M, BF16, SENT_IN, dy, big=big == "dy"),
                     matrix(T, N, BF16, SENT_IN, xx, side=16, big=big == "x"),
                     matrix(M, N, F32, SENT_OUT, c0, big=big == "c")))
        c0s.append(c0)
    ins = [r for t in regs for r in t[:2]]
    outs = [t[2] for t in regs]
    snap = [r.snap() for r in ins]

    def call():
        return e.gemm_dw_grouped([t[0].view for t in regs], [t[1].view for t in regs], [t[2].view for t in regs],
                                 alpha, force)

    s_used = guarded(call, name)
    first = [r.view.clone() for r in outs]
    for r, c0 in zip(outs, c0s):
        r.view.copy_(c0.to(DEV))
    s_again = guarded(call, name)
    torch.cuda.synchronize()
    print(f"MEASURE split {s_used} dwgroup-{name}")
    rep.expect(s_used == s_again, "the planner changed its mind between two calls")
    if want_s is not None:
        rep.expect(s_used == want_s, f"split {s_used}, expected {want_s}")
    rep.expect(1 <= s_used <= T // 64, f"split {s_used} outside 1..{T // 64}")
    rep.expect(all(bits_equal(a, r.view) for a, r in zip(first, outs)), "second run differs")
    rep.expect(all(r.same(s) for r, s in zip(ins, snap)), "an input or its padding changed")
    rep.expect(all(r.padding_intact() for r in outs), "padding of an output was written")
    cls = "g3tt" if s_used == 1 else "skred"
    for (rdy, rx, rc), c0 in zip(regs, c0s):
        ref = R.gemm_ref(rdy.view, rx.view, True, True, alpha, C0=c0)
        R.check_outputs(rep, cls, ref, dict(out=rc.view.cpu()))
    rep.finish()


@pytest.mark.parametrize("split", (1, 2))
def test_gemm_dw_grouped_halves_of_one_gradient(split):
    """two problems write the upper and the lower half of one [2 M, N] gradient (a fused
    QKV-style weight): neither touches the other's rows; exact two-hot inputs whose two hot
    columns lie in different splits, bit for bit"""
    e = ops.kernels._ext()
    M, N, T = 136, 200, 192
    rc = matrix(2 * M, N, F32, SENT_OUT, torch.zeros(2 * M, N))
    wants, dys, xs = [], [], []
    for h in range(2):
        a, b, want = R.exact_inputs("twohot", M, N, T, split)      # a [M, T] one/two-hot, b [N, T]
        dys.append(matrix(T, M, BF16, SENT_IN, a.t()).view)
        xs.append(matrix(T, N, BF16, SENT_IN, b.t() if h == 0 else -b.t()).view)
        wants.append(want if h == 0 else -want)
    s = guarded(lambda: e.gemm_dw_grouped(dys, xs, [rc.view[:M], rc.view[M:]], 0.5, split), "halves")
    torch.cuda.synchronize()
    assert s == split
    assert rc.padding_intact()
    assert torch.equal(rc.view.cpu().double(), 0.5 * torch.cat(wants))


def test_gemm_dw_grouped_refusals():
    """unequal T, T % 64 != 0, M % 8 != 0, N % 8 != 0, a wrong dtype, a CPU operand, a wrong C
    shape, too many problems: each raises from the binding before any launch"""
    e = ops.kernels._ext()

    def mk(T, M, N, dt=BF16, cdt=F32, dev=DEV):
        up = lambda n: (n + 7) // 8 * 8   # noqa: E731  (rows stay 16-byte aligned: column slices)
        return (torch.ones(T, up(M), dtype=dt, device=dev)[:, :M], torch.ones(T, up(N), dtype=dt, device=dev)[:, :N],
                torch.full((M, up(N)), 3.0, dtype=cdt, device=dev)[:, :N])

    good = mk(128, 16, 24)
    bad = {
        "unequal T": ([good, mk(192, 16, 24)], "same token count"),
        "T % 64": ([mk(96, 16, 24)], "multiple of 64"),
        "M % 8": ([good, mk(128, 12, 24)], "multiples of 8"),
        "N % 8": ([good, mk(128, 16, 20)], "multiples of 8"),
        "f32 dy": ([good, mk(128, 16, 24, dt=F32)], "must be"),
        "bf16 C": ([good, mk(128, 16, 24, cdt=BF16)], "must be"),
        "cpu x": ([good, (good[0], torch.ones(128, 24, dtype=BF16), good[2].clone())], "GPU"),
        "C shape": ([good, (good[0], good[1], torch.full((24, 16), 3.0, device=DEV))], "C["),
        "nine problems": ([good] * 9, "1..8 problems"),
    }
    for what, (probs, msg) in bad.items():
        cs = [p[2] for p in probs]
        before = [c.clone() for c in cs]
        with pytest.raises(RuntimeError, match=msg.replace("[", r"\[").replace("..", r"\.\.")):
            e.gemm_dw_grouped([p[0] for p in probs], [p[1] for p in probs], cs, 1.0, 0)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, cs)), f"{what}: an output was written"
    with pytest.raises(RuntimeError, match="split"):
        e.gemm_dw_grouped([good[0]], [good[1]], [good[2]], 1.0, -1)
    assert bool((good[2] == 3.0).all())


@pytest.mark.parametrize("group3", (True, False))
def test_run_wjobs_long_token_group(monkeypatch, group3):
    """one layer's job list (QKV dW + its bias sum, wo dW, the halves of a fused gradient, a
    plain callable) through ops.run_wjobs with the long-token threshold down at T = 320: through
    the grouped 256x256 engine, and with it switched off (MIPIPE_WGRAD_GROUP3=0's behaviour).
    Both stay inside the bound of the float64 reference; the bias sum lands in its own vector."""
    K = ops.kernels
    monkeypatch.setattr(ops.wgrad, "_GROUP3_MIN_T", 256)      # the module that owns the switches
    monkeypatch.setattr(ops.wgrad, "_WGRAD_GROUP3", group3)
    rep = R.Report(f"dwgroup-wrapper-{int(group3)}")
    T = 320
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    dqkv, h1, dx2, o = mk(T, 264).to(BF16), (mk(T, 136) / 18).to(BF16), mk(T, 136).to(BF16), (mk(T, 136) / 18).to(BF16)
    c_qkv, c_wo, c_two = (torch.randint(-8, 9, s, generator=g).float() for s in ((264, 136), (136, 136), (272, 136)))
    b0 = torch.full((264,), 0.5)
    dev = lambda t: t.to(DEV)   # noqa: E731
    d = dict(dqkv=dev(dqkv), h1=dev(h1), dx2=dev(dx2), o=dev(o), qkv=dev(c_qkv), wo=dev(c_wo), two=dev(c_two),
             b=dev(b0), called=[])
    jobs = [K.DW(d["dqkv"], d["h1"], d["qkv"]), K.ColSum(d["dqkv"], d["b"]), K.DW(d["dx2"], d["o"], d["wo"]),
            K.DW(d["dx2"], d["h1"], d["two"][:136]), K.DW(d["dx2"], d["o"], d["two"][136:]),
            lambda: d["called"].append(1)]
    small, long_, rest = K.plan_wjobs(jobs)
    if group3:
        assert [len(p) for p in long_] == [4] and not small and rest == [jobs[1], jobs[5]]
        assert long_[0] == [jobs[0], jobs[2], jobs[3], jobs[4]]
    else:
        assert not long_ and [len(p) for p in small] == [4] and rest == [jobs[1], jobs[5]]
    guarded(lambda: K.run_wjobs(jobs), "run_wjobs")
    torch.cuda.synchronize()
    assert d["called"] == [1]
    cls = "g3tt" if group3 else "grouped"
    for key, dy, x, c0 in (("qkv", dqkv, h1, c_qkv), ("wo", dx2, o, c_wo)):
        R.check_outputs(rep, cls, R.gemm_ref(dy, x, True, True, 1.0, C0=c0), dict(out=d[key].cpu()))
    for half, x in ((slice(0, 136), h1), (slice(136, 272), o)):
        R.check_outputs(rep, cls, R.gemm_ref(dx2, x, True, True, 1.0, C0=c_two[half]), dict(out=d["two"][half].cpu()))
    ref = R.gemm_ref(dqkv, h1, True, True, colsum0=b0, stored=dqkv)
    rep.value("g2.colsum_sep", d["b"].cpu(), ref.colsum, ref.A_colsum)
    rep.finish()
