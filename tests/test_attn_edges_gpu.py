"""Edge cases of the attention kernels (attention.hip, attention_f32.hip), forward and backward,
against the float64 reference of attn_refs.py (itself checked on the CPU in
test_attn_refs_cpu.py, together with the teeth of the error metric used here).

The cases (attn_refs.CASES) are the smallest shapes that reach each launcher branch and each
ragged edge; the branch is the last part of a case id, `forward+backward`:

  ks2-1iter / ks2-loop      key-split forward (non-causal, < 256 blocks), one / several iterations
  fwd2xNpair{odd,even}      forward v2 (d_h <= 64), causal: N paired 128-query blocks, odd / even count
  fwd1dpX                   forward v1 (head dim padded to X = 128 / 256; X = 64 only with 64-bit offsets)
  shortM+N                  one-launch short backward, M query-role + N key-role blocks
  dq3.. / dkdv3..           dQ v3 / dK dV v3 (d_h <= 64), xN blocks or paired as above
  dq1dpX / dkdv1dpX         dQ v1 / dK dV v1
  f32                       the f32 kernels
  (dq2 / dkdv2 and the v1 kernels at d_h 64 run in child processes, see the end of the file)

Every case runs with all tensors as column slices of wider buffers with extra rows, the
padding holding a sentinel: inputs and all padding must be bit-identical afterwards.  Forward
and backward run twice and must agree bit for bit: no attention kernel accumulates a gradient
or an output with atomics on any path (v1, v2, v3, short, key-split, f32).  Only ``dbias``
ends in f32 atomics (wg_colsum_atomic), on every bf16 backward path; it starts at 0.25, is
compared with the reference sums within a measured bound, and a third backward without it
must reproduce the gradients bit for bit.  The short backward takes no ``delta``: there it
must stay untouched, everywhere else it is checked, which also shows which path ran.

Bounds: see attn_refs.BOUND (2 x the largest error of two MI355X runs; every bf16 ratio
measured is near 1, i.e. one bf16 ulp of what was summed).  The LSE of forward v2 without
dropout is the log of a sum of bf16-rounded probabilities and is about 4000 x less accurate
than every other kernel's (1.5e-3 against 3.5e-7): it has a key of its own, 'lse_v2'.
Every comparison also asserts the older tests' atol / rtol."""
import math
import os
import subprocess
import sys

import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

import attn_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENT_IN, SENT_OUT = 512.0, -77.0     # padding of inputs; padding and starting content of outputs
PAD_ROWS = 3
DBIAS0 = 0.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = torch.int16 if a.dtype == BF16 else torch.int32
    return torch.equal(a.view(view), b.view(view))


class Region:
    """Views into one sentinel-padded buffer, with the index expressions of its padding."""

    def __init__(self, buf, views, guards, fill):
        self.buf, self.views, self.guards, self.fill = buf, views, guards, fill

    def snap(self):
        return [self.buf[g].clone() for g in self.guards] + [v.clone() for v in self.views]

    def padding_intact(self):
        return all(bool((self.buf[g] == self.fill).all()) for g in self.guards)

    def same(self, snap):
        now = [self.buf[g] for g in self.guards] + list(self.views)
        return all(bits_equal(a, b) for a, b in zip(now, snap))

    def reset(self):
        for v in self.views:
            v.fill_(self.fill)


def region(rows, widths, dtype, fill, left=8, right=8):
    """[rows + PAD_ROWS, left + sum(widths) + right] filled with ``fill``; one view per width, side by side."""
    buf = torch.full((rows + PAD_ROWS, left + sum(widths) + right), fill, dtype=dtype, device=DEV)
    views, c0 = [], left
    for w in widths:
        views.append(buf[:rows, c0: c0 + w])
        c0 += w
    guards = [(slice(None), slice(0, left)), (slice(None), slice(c0, None)), (slice(rows, None), slice(None))]
    return Region(buf, views, guards, fill)


def vector(n, fill):
    buf = torch.full((n + 16,), fill, dtype=F32, device=DEV)
    return Region(buf, [buf[8: 8 + n]], [slice(0, 8), slice(8 + n, None)], fill)


class Layout:
    """The tensors of one case on the GPU.  ``ins`` / ``outs``: the regions of inputs / outputs."""

    def __init__(self, c):
        B, Sq, Sk, H, Hkv, D = c.shape()
        Tq, Tk, wq, wk, dt = B * Sq, B * Sk, H * D, Hkv * D, c.dtype
        lay = c.layout
        if lay == "bigstride":
            # every tensor a column slice of one uninitialised buffer whose row stride needs 64-bit offsets
            big = torch.empty(Tq + 1, R.BIG_STRIDE, dtype=dt, device=DEV)
            cols = [8 + 500000 * i for i in range(8)]
            regs = []
            for i, c0 in enumerate(cols):
                fill = SENT_IN if i in (0, 1, 2, 4) else SENT_OUT
                big[:, c0 - 8: c0 + wq + 8] = fill
                guards = [(slice(None), slice(c0 - 8, c0)), (slice(None), slice(c0 + wq, c0 + wq + 8)),
                          (slice(Tq, None), slice(c0, c0 + wq))]
                regs.append(Region(big, [big[:Tq, c0: c0 + wq]], guards, fill))
            rq, rk, rv, ro, rdo, rdq, rdk, rdv = regs
            self.q, self.k, self.v, self.o, self.do = (r.views[0] for r in (rq, rk, rv, ro, rdo))
            self.dq, self.dk, self.dv = (r.views[0] for r in (rdq, rdk, rdv))
            self.ins, self.outs = [rq, rk, rv, rdo], [ro, rdq, rdk, rdv]
        else:
            if lay == "packed":
                rin, rg = region(Tq, [wq, wk, wk], dt, SENT_IN), region(Tq, [wq, wk, wk], dt, SENT_OUT)
                (self.q, self.k, self.v), (self.dq, self.dk, self.dv) = rin.views, rg.views
                ins, outs = [rin], [rg]
            elif lay == "q_kv":
                r1, r2 = region(Tq, [wq], dt, SENT_IN, right=16), region(Tk, [wk, wk], dt, SENT_IN)
                g1, g2 = region(Tq, [wq], dt, SENT_OUT, right=16), region(Tk, [wk, wk], dt, SENT_OUT)
                self.q, (self.k, self.v), self.dq, (self.dk, self.dv) = r1.views[0], r2.views, g1.views[0], g2.views
                ins, outs = [r1, r2], [g1, g2]
            elif lay in ("sep", "gradstride"):
                pads = (8, 16, 24)
                gpads = pads if lay == "sep" else (24, 32, 8)
                ins = [region(T, [w], dt, SENT_IN, right=p) for T, w, p in zip((Tq, Tk, Tk), (wq, wk, wk), pads)]
                outs = [region(T, [w], dt, SENT_OUT, right=p) for T, w, p in zip((Tq, Tk, Tk), (wq, wk, wk), gpads)]
                self.q, self.k, self.v = (r.views[0] for r in ins)
                self.dq, self.dk, self.dv = (r.views[0] for r in outs)
                assert len({t.stride(0) for t in (self.k, self.v, self.dk, self.dv)}) == (2 if lay == "sep" else 4)
            else:
                raise ValueError(lay)
            ro, rdo = region(Tq, [wq], dt, SENT_OUT, right=16), region(Tq, [wq], dt, SENT_IN, right=16)
            self.o, self.do = ro.views[0], rdo.views[0]
            self.ins, self.outs = ins + [rdo], outs + [ro]
        n = B * H * Sq
        self.rlse, self.rdelta, self.rdbias = vector(n, SENT_OUT), vector(n, SENT_OUT), vector((H + 2 * Hkv) * D, DBIAS0)
        self.lse, self.delta, self.dbias = self.rlse.views[0], self.rdelta.views[0], self.rdbias.views[0]
        self.outs += [self.rlse, self.rdelta, self.rdbias]
        self.fwd_outs = [r for r in self.outs if any(v is self.o or v is self.lse for v in r.views)]

    def load(self, q, k, v, do):
        for dst, src in ((self.q, q), (self.k, k), (self.v, v), (self.do, do)):
            dst.copy_(src.to(DEV))


def fwd(c, L, seed):
    ops.attn_fwd(L.q, L.k, L.v, L.o, L.lse, *c.shape(), c.causal, scale=c.scale, p_drop=c.p, seed=seed)


def bwd(c, L, seed, dbias):
    ops.attn_bwd(L.q, L.k, L.v, L.o, L.do, L.lse, L.dq, L.dk, L.dv, *c.shape(), c.causal, scale=c.scale,
                 p_drop=c.p, seed=seed, delta=L.delta, dbias=dbias)


def recover_mask(c, L, seed, rep):
    """The kernels' dropout mask for this case, [B, H, Sq, Sk] bool, through the same launcher
    branch and buffers: q = k = 0 makes P uniform over the visible keys, V = a D-column window
    of the identity turns O into P o keep over those D keys (ceil(Sk / D) forward passes), and
    dO = such a window in one query head per KV head turns dV into its transpose
    (H / Hkv x ceil(Sq / D) backward passes).  Forward and backward must agree."""
    B, Sq, Sk, H, Hkv, D = c.shape()
    g = H // Hkv
    zq, zk = torch.zeros(B * Sq, H * D, dtype=c.dtype), torch.zeros(B * Sk, Hkv * D, dtype=c.dtype)
    kept_f = torch.zeros(B, H, Sq, Sk, dtype=torch.bool)
    kept_b = torch.zeros(B, H, Sq, Sk, dtype=torch.bool)
    for w in range((Sk + D - 1) // D):
        L.load(zq, zk, R.identity_window(Sk, D, w, Hkv, B, c.dtype), zq)
        fwd(c, L, seed)
        n = min(D, Sk - w * D)
        kept_f[..., w * D: w * D + n] = R.heads(L.o, B, Sq, H, D)[..., :n] > 0
    for r in range(g):
        for w in range((Sq + D - 1) // D):
            do = zq.clone()
            win = R.identity_window(Sq, D, w, 1, B, c.dtype)
            for hk in range(Hkv):
                h = hk * g + r
                do[:, h * D: (h + 1) * D] = win
            L.do.copy_(do.to(DEV))
            bwd(c, L, seed, None)
            n = min(D, Sq - w * D)
            kept_b[:, r::g, w * D: w * D + n, :] = (R.heads(L.dv, B, Sk, Hkv, D)[..., :n] > 0).transpose(-1, -2)
    vis = R.visible(Sq, Sk, c.causal)
    rep.expect(torch.equal(kept_f & vis, kept_b & vis), "forward and backward dropout masks differ")
    rep.expect(not (kept_f & ~vis).any() and not (kept_b & ~vis).any(), "weight on a masked key")
    nvis = int(vis.sum()) * B * H
    rate = float((kept_f & vis).sum()) / nvis
    rep.expect(abs(rate - (1 - c.p)) < 5 * math.sqrt(c.p * (1 - c.p) / nvis), f"keep rate {rate:.4f} at p = {c.p}")
    rep.expect(not torch.equal(kept_f[:, 0], kept_f[:, 1]), "two heads share one dropout mask")
    return kept_f.double() / (1.0 - c.p)


def run_case(c, env=R.DEFAULT_ENV):
    """Runs one case on the GPU and checks everything; returns the Report (call .finish())."""
    B, Sq, Sk, H, Hkv, D = c.shape()
    path = R.path(c, env)
    rep = R.Report(f"{c.id} [{'+'.join(path)}]")
    L = Layout(c)
    if c.prec == "bf16":   # the label this case's result is filed under is what will run
        plan = ops.attn_plan(B, Sq, Sk, H, Hkv, D, *(t.stride(0) for t in (L.q, L.k, L.v, L.o)), c.causal, c.p > 0,
                             env=R.plan_env(env))
        assert R.planned_kernels(plan) == R.path_kernels(path), (c.id, path, plan)
    seed = 4321 + c.seed
    q, k, v, do = R.make_inputs(c)
    keep = recover_mask(c, L, seed, rep) if c.p else None
    L.load(q, k, v, do)
    for r in L.outs:
        r.reset()
    snap_in = [r.snap() for r in L.ins]
    bf = c.prec == "bf16"

    # forward, twice
    fwd(c, L, seed)
    o1, lse1 = L.o.clone(), L.lse.clone()
    for r in L.fwd_outs:
        r.reset()
    fwd(c, L, seed)
    rep.expect(bits_equal(o1, L.o) and bits_equal(lse1, L.lse), "forward: second run differs")
    # backward: twice with dbias (bf16; the f32 kernels have none), once more without
    runs = []
    for dbias in ((L.dbias, L.dbias, None) if bf else (None, None)):
        for r in L.outs:
            if r not in L.fwd_outs:
                r.reset()
        bwd(c, L, seed, dbias)
        runs.append(tuple(t.clone() for t in (L.dq, L.dk, L.dv, L.delta)))
        if dbias is not None:
            dbias_got = L.dbias.to("cpu", copy=True)
    for i, other in enumerate(runs[1:]):
        same = all(bits_equal(a, b) for a, b in zip(runs[0], other))
        rep.expect(same, f"backward: run {i + 2} differs from run 1" + (" (run 3 is without dbias)" if bf else ""))
    if bf:
        rep.expect(bool((L.dbias == DBIAS0).all()), "dbias written by a backward that was given none")
    torch.cuda.synchronize()
    rep.expect(all(r.same(s) for r, s in zip(L.ins, snap_in)), "an input or its padding changed")
    rep.expect(all(r.padding_intact() for r in L.outs), "padding of an output was written")

    got = dict(o=L.o.cpu(), lse=L.lse.cpu(), dq=L.dq.cpu(), dk=L.dk.cpu(), dv=L.dv.cpu())
    if path[1].startswith("short"):
        rep.expect(bool((L.delta == SENT_OUT).all()), "delta written on the short path (which takes none)")
    else:
        got["delta"] = L.delta.cpu()
    if bf:
        got.update(dbias=dbias_got, dbias0=DBIAS0)
    f = R.attn_fwd_ref(q, k, v, B, Sq, Sk, H, Hkv, D, c.causal, c.scale, keep)
    b = R.attn_bwd_ref(q, k, v, got["o"], do, B, Sq, Sk, H, Hkv, D, c.causal, c.scale, keep)
    lse_key = "lse_v2" if path[0].startswith("fwd2") and not c.p else "lse"
    R.check_outputs(rep, c.prec, f, b, got, B, Sq, H, Hkv, D, lse_key)
    return rep


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_attention_edges(c):
    try:
        rep = run_case(c)
    except RuntimeError as e:
        if "HIP error" in str(e):   # a fault poisons the context: nothing more may run on this GPU
            pytest.exit(f"GPU fault in {c.id}: {e}", returncode=3)
        raise
    rep.finish()


# ====================================================================== argument checks
def test_binding_checks_attention():
    """Every tensor of attn_fwd / attn_bwd is checked on the host before any launch: one dtype,
    unit inner stride, enough rows and columns, f32 contiguous lse / delta of B*H*Sq, sane
    sizes.  Each bad call raises and leaves the sentinel-filled outputs untouched.  (Only
    arguments the host-side checks refuse are passed here.)"""
    B, S, H, Hkv, D = 2, 40, 4, 4, 64
    T, wq, wk, n = B * S, H * D, Hkv * D, B * H * S

    def args(dt=BF16):
        mk = lambda w, fill: torch.full((T, w), fill, dtype=dt, device=DEV)   # noqa: E731
        a = dict(q=mk(wq, 1.0), k=mk(wk, 1.0), v=mk(wk, 1.0), o=mk(wq, SENT_OUT), do=mk(wq, 1.0), dq=mk(wq, SENT_OUT),
                 dk=mk(wk, SENT_OUT), dv=mk(wk, SENT_OUT), lse=torch.full((n,), SENT_OUT, device=DEV),
                 delta=torch.full((n,), SENT_OUT, device=DEV), dbias=torch.full(((H + 2 * Hkv) * D,), SENT_OUT, device=DEV))
        return a

    def other(t):
        return torch.full(t.shape, 1.0, dtype=F32 if t.dtype == BF16 else BF16, device=DEV)

    def strided(t):
        return torch.full((t.shape[0], 2 * t.shape[1]), SENT_OUT, dtype=t.dtype, device=DEV)[:, ::2]

    dims = dict(B=B, Sq=S, Sk=S, H=H, Hkv=Hkv, D=D)
    bad = []   # (which call, tensor edits, dim edits)
    for name in ("k", "v", "o"):
        bad.append(("fwd", {name: other}, {}))
    for name in ("k", "v", "o", "do", "dq", "dk", "dv"):
        bad.append(("bwd", {name: other}, {}))
    for name in ("q", "k", "v", "o"):
        bad.append(("fwd", {name: strided}, {}))
    for name in ("do", "dq", "dk", "dv", "k"):
        bad.append(("bwd", {name: strided}, {}))
    short_rows, short_cols = (lambda t: t[: T - 1]), (lambda t: t[:, : t.shape[1] - 8])
    for name in ("q", "k", "v", "o"):
        bad += [("fwd", {name: short_rows}, {}), ("fwd", {name: short_cols}, {})]
    for name in ("q", "k", "v", "o", "do", "dq", "dk", "dv"):
        bad += [("bwd", {name: short_rows}, {}), ("bwd", {name: short_cols}, {})]
    for call, name in (("fwd", "lse"), ("bwd", "lse"), ("bwd", "delta")):
        bad += [(call, {name: lambda t: t[: n - 1]}, {}), (call, {name: lambda t: t.double()}, {}),
                (call, {name: lambda t: torch.full((2 * n,), SENT_OUT, device=DEV)[::2]}, {})]
    for call in ("fwd", "bwd"):
        bad += [(call, {}, {"B": 0}), (call, {}, {"Sq": 0}), (call, {}, {"Sk": 0}), (call, {}, {"H": 0}),
                (call, {}, {"Hkv": 0}), (call, {}, {"H": 3}), (call, {}, {"D": 60}), (call, {}, {"D": 4}),
                (call, {}, {"Sk": S + 1}), (call, {}, {"Sq": S + 1}), (call, {}, {"B": B + 1}), (call, {}, {"Hkv": 8}),
                (call, {}, {"H": 8, "Hkv": 4})]
    bad.append(("bwd", {"dbias": lambda t: t[:-1]}, {}))
    bad.append(("bwd", {"dbias": lambda t: t.double()}, {}))
    for dt in (BF16, F32):
        for call, edits, dim_edits in bad:
            a = args(dt)
            if dt == F32 and "dbias" in edits:
                continue
            for name, fn in edits.items():
                a[name] = fn(a[name])
            d = dict(dims, **dim_edits)
            shape = (d["B"], d["Sq"], d["Sk"], d["H"], d["Hkv"], d["D"])
            what = f"{dt} {call} {sorted(edits)} {dim_edits}"
            with pytest.raises(RuntimeError):
                if call == "fwd":
                    ops.attn_fwd(a["q"], a["k"], a["v"], a["o"], a["lse"], *shape, False)
                else:
                    ops.attn_bwd(a["q"], a["k"], a["v"], a["o"], a["do"], a["lse"], a["dq"], a["dk"], a["dv"], *shape,
                                 False, delta=a["delta"], dbias=a["dbias"] if dt == BF16 else None)
                pytest.fail(f"accepted: {what}")
            torch.cuda.synchronize()
            for name in ("o", "dq", "dk", "dv", "lse", "delta", "dbias"):
                t = a[name]
                if t.dtype in (BF16, F32, torch.float64) and name not in edits:
                    assert bool((t == SENT_OUT).all()), f"{what}: {name} was written"
                elif name in edits and edits[name] is strided:
                    assert bool((t == SENT_OUT).all()), f"{what}: {name} was written"


# ====================================================================== non-default kernels
@pytest.fixture(scope="module")
def nondefault_runs():
    """The MIPIPE_ATTN_* switches are read once per process, so the v1 kernels at d_h 64 (with
    the key-split forward and the short backward off) and the v2 backward kernels run
    attn_refs.CHILD_CASES through run_case in two fresh child processes, one after the
    other; the second starts only if the first exited 0."""
    res = {}
    for name in ("v1", "v2"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MIPIPE_ATTN_")}
        env.update(R.CHILD_ENVS[name])
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired as e:
            res[name] = (None, f"timed out: {e}")
            break
        print(p.stdout)
        res[name] = (p.returncode, p.stdout[-4000:] + p.stderr[-4000:])
        if p.returncode != 0:
            break
    return res


@pytest.mark.parametrize("name", ["v1", "v2"])
def test_nondefault_kernels(nondefault_runs, name):
    assert name in nondefault_runs, "not started: the child before it failed"
    rc, out = nondefault_runs[name]
    assert rc == 0, out
    assert f"child {name}: {len(R.CHILD_CASES)} cases ok" in out, out


if __name__ == "__main__":
    assert torch.cuda.is_available() and ops.ext_available()
    flags = R.env_flags(os.environ)
    which = [n for n, e in R.CHILD_ENVS.items() if R.env_flags(e) == flags]
    fails = []
    for case in R.CHILD_CASES:
        fails += run_case(case, flags).fails
    torch.cuda.synchronize()
    if fails:
        print("\n".join(fails))
        sys.exit(1)
    print(f"child {which[0] if which else flags}: {len(R.CHILD_CASES)} cases ok")
