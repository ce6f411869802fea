"""ops.run_wjobs / ops.plan_wjobs on the CPU: which weight-gradient jobs of a mixed list go to
the grouped launches (short-token 64x64 engine, long-token 256x256 split-K engine), how a
deferred list that spans layers and token counts is cut into chunks, and that the result of the
whole list equals running every job alone.  The two grouped launchers and the per-job GEMM are
replaced by float32 CPU arithmetic that records what it was given; ``_gpu`` answers yes, so the
planner sees the tensors as it would on the GPU.  Every stand-in is installed in the module that
owns the name (``ops.wgrad`` looks the foreign ones up there when it runs); ``rec`` and the plans
show that the stand-ins are what ran."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops

K = ops.kernels
W, G = ops.wgrad, ops.gemm
BF16, F32 = torch.bfloat16, torch.float32


def _cpu_dw(dy, x, dw, alpha=1.0):
    dw += alpha * (dy.float().t() @ x.float())
    return dw


@pytest.fixture
def rec(monkeypatch):
    log = dict(small=[], long=[], single=[])
    monkeypatch.setattr(ops._base, "_gpu", lambda t: True)
    monkeypatch.setattr(W, "_WGRAD_GROUP", True)
    monkeypatch.setattr(W, "_WGRAD_GROUP3", True)
    monkeypatch.setattr(G, "GEMM_BACKEND", "hip")
    monkeypatch.setattr(W, "_GROUP3_MIN_T", 8192)

    def group(kind):
        def run(part):
            assert 2 <= len(part) <= 8
            assert len({j.alpha for j in part}) == 1
            if kind == "long":
                assert len({j.dy.shape[0] for j in part}) == 1
            log[kind].append(list(part))
            for j in part:
                _cpu_dw(j.dy, j.x, j.dw, j.alpha)
        return run

    def single(dy, x, dw, alpha=1.0):
        log["single"].append((dy, x, dw))
        return _cpu_dw(dy, x, dw, alpha)

    monkeypatch.setattr(W, "_run_group_small", group("small"))
    monkeypatch.setattr(W, "_run_group_long", group("long"))
    monkeypatch.setattr(G, "linear_dw", single)
    monkeypatch.setattr(ops.elementwise_optim, "colsum", lambda x, db: db.add_(x.float().sum(0)))
    return log


def _jobs():
    """a deferred list over token counts 8192 (11 long jobs: chunks of 8 + 3), 16384 (2 long, one
    of them alpha = 0.5 -> two singles), 128 (3 short), with bias sums, a callable, an f32 job, a
    job with an odd output width and a transposed (strided) dy."""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.randn(*s, generator=g) / 8).to(BF16)   # noqa: E731
    z = lambda *s: torch.zeros(*s)   # noqa: E731
    d8 = [r(8192, 16) for _ in range(11)]
    x8 = r(8192, 24)
    jobs, kinds = [], []

    def add(j, kind):
        jobs.append(j)
        kinds.append(kind)

    for i, dy in enumerate(d8):
        add(K.DW(dy, x8, z(16, 24)), "long8192")
        if i == 0:
            add(K.ColSum(dy, z(16)), "rest")
    d16, x16 = r(16384, 8), r(16384, 8)
    add(K.DW(d16, x16, z(8, 8)), "single")
    add(K.DW(d16, x16, z(8, 8), 0.5), "single")
    for _ in range(3):
        add(K.DW(r(128, 16), r(128, 8), z(16, 8)), "short")
    hits = []
    add(lambda: hits.append(1), "rest")
    add(K.DW(r(8192, 16).float(), x8.float(), z(16, 24)), "single")                 # f32 operands
    add(K.DW(r(8192, 12), x8, z(12, 24)), "single")                                  # M % 8 != 0
    add(K.DW(r(16, 8192).t(), x8, z(16, 24)), "single")                              # dy without a unit inner stride
    return jobs, kinds, hits


def test_plan_and_results(rec):
    jobs, kinds, hits = _jobs()
    small, long_, rest = K.plan_wjobs(jobs)
    by = lambda k: [j for j, kk in zip(jobs, kinds) if kk == k]   # noqa: E731
    assert [len(p) for p in long_] == [8, 3]
    assert [j for p in long_ for j in p] == by("long8192")
    assert small == [by("short")]
    assert rest == [j for j, kk in zip(jobs, kinds) if kk in ("rest", "single")]

    K.run_wjobs(jobs)
    assert hits == [1]
    assert rec["long"] == long_ and rec["small"] == small
    assert len(rec["single"]) == len(by("single"))
    # every job alone on fresh gradients gives the same bits
    jobs2, _, _ = _jobs()
    for j, j2 in zip(jobs, jobs2):
        if isinstance(j2, K.DW):
            _cpu_dw(j2.dy, j2.x, j2.dw, j2.alpha)
            assert torch.equal(j.dw, j2.dw) and bool(j.dw.abs().sum() > 0)
        elif isinstance(j2, K.ColSum):
            j2.dbias.add_(j2.x.float().sum(0))
            assert torch.equal(j.dbias, j2.dbias) and bool(j.dbias.abs().sum() > 0)


def test_switches(rec, monkeypatch):
    jobs, kinds, _ = _jobs()
    monkeypatch.setattr(W, "_WGRAD_GROUP3", False)
    small, long_, rest = K.plan_wjobs(jobs)
    assert not long_ and [len(p) for p in small] == [3]
    assert len(rest) == len(jobs) - 3
    monkeypatch.setattr(W, "_WGRAD_GROUP", False)
    assert K.plan_wjobs(jobs) == ([], [], jobs)
    monkeypatch.setattr(W, "_WGRAD_GROUP", True)
    monkeypatch.setattr(G, "GEMM_BACKEND", "blas")
    assert K.plan_wjobs(jobs) == ([], [], jobs)


def test_threshold_is_inclusive_and_lone_jobs_stay_single(rec):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16)   # noqa: E731
    below = [K.DW(r(8128, 8), r(8128, 8), torch.zeros(8, 8)) for _ in range(2)]
    at = [K.DW(r(8192, 8), r(8192, 8), torch.zeros(8, 8)) for _ in range(2)]
    lone = K.DW(r(8256, 8), r(8256, 8), torch.zeros(8, 8))
    # an output of >= 256 tiles (the LM head's) fills the chip alone: never grouped (shapes only)
    m = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device="meta")   # noqa: E731
    head = [K.DW(m(8192, 4096), m(8192, 4096), m(4096, 4096, dt=F32)) for _ in range(2)]
    small, long_, rest = K.plan_wjobs(below + at + [lone] + head)
    assert long_ == [at] and not small and rest == below + [lone] + head
