"""Greedy speculative decoding on the CPU (f32 reference paths of the ops): whatever the draft
proposes, ``generate_speculative`` returns the target's own greedy continuation, the tokens
of ``generate_batch``.

The target is the tiny walk model of test_generate_cpu.py's ``trained`` fixture (the recipe
is copied here); the trained draft is a smaller model trained the same way for fewer steps.
Token equality between two code paths (one-row decode steps against T-row extends) only
means something where the reference's own choice is not a near-tie, so the module first
asserts that the target's greedy run has a top-2 logit gap above 1e-3 at every emitted
position."""
import math
import os
import subprocess
import sys

import pytest
import torch

import mipipe
from mipipe.engine import PipelineTrainer
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext
from mipipe.utils.checkpoint import save_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import train as _train  # noqa: E402

CPU = torch.device("cpu")
LENS, N = [1, 6, 3], 24


def _gpt2(vocab=64):
    return NativeConfig.gpt2("tiny", vocab_size=vocab, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32)


def _small():
    return NativeConfig.gpt2("tiny", vocab_size=64, d_model=32, n_layers=1, n_heads=2, d_ff=64, max_seq_len=32)


def _train_walk(cfg, steps):
    m, mbs, seq = 2, 8, 32
    tr = PipelineTrainer(cfg, pp=1, schedule="1F1B", n_microbatches=m, mbs=mbs, seq_len=seq, device=CPU,
                         dtype=torch.float32, lr=3e-3, seed=0, graphs=False)
    data = _train.TokenData("pattern:48", cfg.vocab_size, m * mbs, seq, CPU, 0, 0)
    loss = None
    for s in range(steps):
        loss = tr.train_step(*data.batch(s))
    return tr, float(loss)


@pytest.fixture(scope="module")
def models():
    """(target trainer, target generator, trained draft generator, draft trainer)."""
    tr, loss = _train_walk(_gpt2(), 120)
    assert loss < 0.05
    dtr, _ = _train_walk(_small(), 60)
    return (tr, mipipe.Generator.from_model(tr.stages[0].model), mipipe.Generator.from_model(dtr.stages[0].model),
            dtr)


def _prompts():
    data = _train.TokenData("pattern:48", 64, len(LENS), 32, CPU, 0, 0)
    x, _ = data.batch(100003)        # a step no training batch used
    return [x[b, :n].contiguous() for b, n in enumerate(LENS)]


@pytest.fixture(scope="module")
def greedy(models):
    """generate_batch's tokens and lengths, with the check that makes equality meaningful:
    the target's top-2 logit gap at every emitted position."""
    gen = models[1]
    out, lengths = gen.generate_batch(_prompts(), N)
    assert lengths.tolist() == [n + N for n in LENS]
    gap = math.inf
    for b, n in enumerate(LENS):
        row = out[b:b + 1, : n + N]
        lg = gen.model.forward(row, MBContext(0, 0), 1, n + N, target=None).view(n + N, -1)[:, : gen.cfg.vocab_size]
        top = lg[n - 1:n + N - 1].topk(2, -1)
        assert torch.equal(top.indices[:, 0], row[0, n:])        # the run is the full forward's argmax
        gap = min(gap, float((top.values[:, 0] - top.values[:, 1]).min()))
    assert gap > 1e-3, gap
    return out, lengths


def _same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_trained_draft_gives_the_targets_tokens(models, greedy):
    gen, draft = models[1], models[2]
    out, lengths, stats = gen.generate_speculative(_prompts(), N, draft, lookahead=4)
    assert _same((out, lengths), greedy)
    # the prefill yields one token, every round at most lookahead + 1
    assert stats["rounds"] >= math.ceil((N - 1) / 5) and 0 <= stats["accepted"] <= stats["drafted"]


def test_untrained_draft_gives_the_targets_tokens(models, greedy):
    gen = models[1]
    draft = mipipe.Generator(_small(), CPU, dtype=torch.float32, seed=11)
    out, lengths, stats = gen.generate_speculative(_prompts(), N, draft, lookahead=4)
    assert _same((out, lengths), greedy)
    assert stats["accepted"] < stats["drafted"]


def test_target_as_its_own_draft_accepts_everything(models, greedy):
    gen = models[1]
    out, lengths, stats = gen.generate_speculative(_prompts(), N, gen, lookahead=4)
    assert _same((out, lengths), greedy)
    assert stats["rounds"] == math.ceil(N / 5) and stats["accepted"] == stats["drafted"] > 0


@pytest.mark.parametrize("lookahead,n", [(1, N), (4, 7), (3, 1), (2, 0)])
def test_lookahead_and_lengths(models, greedy, lookahead, n):
    gen, draft = models[1], models[2]
    out, lengths, _ = gen.generate_speculative(_prompts(), n, draft, lookahead=lookahead)
    want, want_len = gen.generate_batch(_prompts(), n)
    assert torch.equal(out, want) and torch.equal(lengths, want_len)
    if n == N:
        assert _same((out, lengths), greedy)


def test_argument_errors(models):
    gen, draft = models[1], models[2]
    other = mipipe.Generator(NativeConfig.gpt2("tiny", vocab_size=60, d_model=32, n_layers=1, n_heads=2, d_ff=64,
                                               max_seq_len=32), CPU, dtype=torch.float32)
    with pytest.raises(ValueError, match="vocabulary"):
        gen.generate_speculative(_prompts(), 4, other)
    with pytest.raises(ValueError, match="lookahead"):
        gen.generate_speculative(_prompts(), 4, draft, lookahead=0)
    with pytest.raises(ValueError, match="max_seq_len"):
        gen.generate_speculative(_prompts(), 27, draft)          # 6 + 27 > 32


def test_cli_with_a_draft_prints_the_api_rows(models, greedy, tmp_path):
    tr, dtr = models[0], models[3]
    tpath, dpath = str(tmp_path / "target"), str(tmp_path / "draft")
    save_checkpoint(tr, tpath)
    save_checkpoint(dtr, dpath)
    arg = ";".join(",".join(str(int(t)) for t in row) for row in _prompts())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint", tpath, "--draft-checkpoint",
                        dpath, "--lookahead", "4", "--prompt", arg, "--max-new-tokens", str(N), "--device", "cpu"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = [[int(t) for t in line.split(",")] for line in r.stdout.strip().splitlines()]
    out, lengths = greedy
    assert got == [row[:n] for row, n in zip(out.tolist(), lengths.tolist())]
    assert "accepted" in r.stderr
