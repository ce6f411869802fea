"""Ragged-batch generation on the CPU (f32 reference paths of the ops): prefill(lens=) and
the device-position decode step compute, for every row, what the full forward of that
sequence alone computes; generate_batch follows a learned permutation walk from prompts of
different lengths, honours a stop token, reproduces ``generate`` on equal-length prompts, is
a function of the seed, never emits a padded vocabulary column, and the CLI prints what the
API returns."""
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


def _gpt2(vocab=64):
    return NativeConfig.gpt2("tiny", vocab_size=vocab, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32)


def _llama():
    return NativeConfig.llama3("tiny", vocab_size=64, d_model=64, n_layers=2, n_heads=4, n_kv_heads=2, d_ff=128,
                               max_seq_len=32)


def _alone(model, seq: torch.Tensor) -> torch.Tensor:
    """Last-position logits of the full forward of one sequence on its own."""
    S = seq.numel()
    return model.forward(seq.view(1, S), MBContext(0, 0), 1, S, target=None).view(S, -1)[-1]


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_ragged_incremental_equals_full(family):
    cfg = _gpt2() if family == "gpt2" else _llama()
    gen = mipipe.Generator(cfg, CPU, dtype=torch.float32, seed=3)
    lens, steps = [1, 5, 16, 9], 12
    B, S0 = len(lens), max(lens)
    g = torch.Generator().manual_seed(1)
    seqs = [torch.randint(0, cfg.vocab_size, (n + steps,), generator=g) for n in lens]
    prompt = torch.randint(0, cfg.vocab_size, (B, S0), generator=g)          # the padding is arbitrary tokens
    for b, n in enumerate(lens):
        prompt[b, :n] = seqs[b][:n]
    cache = mipipe.KVCache(cfg, B, S0 + steps, CPU, torch.float32)
    got = gen.prefill(prompt, cache, lens=lens)
    assert cache.ragged and cache.lens.tolist() == lens and cache.pos == S0
    for b, n in enumerate(lens):
        torch.testing.assert_close(got[b], _alone(gen.model, seqs[b][:n]), atol=1e-4, rtol=1e-4)
    for li in range(cfg.n_layers):                    # rows at and beyond lens[b] must not matter
        for b, n in enumerate(lens):
            cache.k[li][b, n:] = float("nan")
            cache.v[li][b, n:] = float("nan")
    for t in range(steps):
        tok = torch.stack([seqs[b][n + t] for b, n in enumerate(lens)])
        got = gen.decode(tok, cache)
        assert cache.lens.tolist() == [n + t + 1 for n in lens]
        for b, n in enumerate(lens):
            torch.testing.assert_close(got[b], _alone(gen.model, seqs[b][: n + t + 1]), atol=1e-4, rtol=1e-4)


def test_inactive_rows_keep_their_cache_and_length():
    cfg = _llama()
    gen = mipipe.Generator(cfg, CPU, dtype=torch.float32, seed=3)
    lens = [3, 6]
    g = torch.Generator().manual_seed(2)
    seq = torch.randint(0, cfg.vocab_size, (2, 12), generator=g)
    cache = gen.new_cache(2, 12)
    gen.prefill(seq[:, :6], cache, lens=lens)
    k0 = [k.clone() for k in cache.k]
    v0 = [v.clone() for v in cache.v]
    active = torch.tensor([1, 0], dtype=torch.uint8)
    got = gen.decode(torch.stack([seq[0, 3], seq[1, 6]]), cache, active=active)
    assert cache.lens.tolist() == [4, 6]
    for li in range(cfg.n_layers):
        assert torch.equal(cache.k[li][1], k0[li][1]) and torch.equal(cache.v[li][1], v0[li][1])
        assert not torch.equal(cache.k[li][0, 3], k0[li][0, 3])
    torch.testing.assert_close(got[0], _alone(gen.model, seq[0, :4]), atol=1e-4, rtol=1e-4)
    got = gen.decode(torch.stack([seq[0, 4], seq[1, 6]]), cache)           # row 1 resumes where it was
    assert cache.lens.tolist() == [5, 7]
    torch.testing.assert_close(got[1], _alone(gen.model, seq[1, :7]), atol=1e-4, rtol=1e-4)
    with pytest.raises(ValueError):
        gen.prefill(seq[:, :6], gen.new_cache(2, 12), lens=[0, 6])
    with pytest.raises(ValueError):
        gen.prefill(seq[:, :6], gen.new_cache(2, 12), lens=[3, 7])
    plain = gen.new_cache(2, 12)
    gen.prefill(seq[:, :6], plain)
    with pytest.raises(ValueError):
        gen.decode(seq[:, 6], plain, active=active)                        # active needs a ragged cache


# ---------------------------------------------------------------------------- trained model
@pytest.fixture(scope="module")
def trained():
    """The tiny GPT-2 of test_generate_cpu / test_learning.test_learns_pattern_pp1_cpu, trained
    the same way."""
    cfg = _gpt2()
    m, mbs, seq = 2, 8, 32
    tr = PipelineTrainer(cfg, pp=1, schedule="1F1B", n_microbatches=m, mbs=mbs, seq_len=seq, device=CPU,
                         dtype=torch.float32, lr=3e-3, seed=0, graphs=False)
    data = _train.TokenData("pattern:48", cfg.vocab_size, m * mbs, seq, CPU, 0, 0)
    loss = None
    for s in range(120):
        loss = tr.train_step(*data.batch(s))
    assert float(loss) < 0.05
    return tr, data.perm


def _held_out(n=4, S0=8):
    data = _train.TokenData("pattern:48", 64, n, 32, CPU, 0, 0)
    x, _ = data.batch(100003)        # a step no training batch used
    return x[:, :S0].contiguous()


def _walk(perm, start: int, n: int):
    out = []
    for _ in range(n):
        start = int(perm[start])
        out.append(start)
    return out


def test_learned_walk_ragged_and_stop_token(trained):
    tr, perm = trained
    gen = mipipe.Generator.from_model(tr.stages[0].model)
    lens, N = [4, 8, 6, 5], 16
    held = _held_out()
    prompts = [held[b, :n].clone() for b, n in enumerate(lens)]
    out, lengths = gen.generate_batch(prompts, N, pad_token=63)
    assert out.shape == (4, 8 + N) and lengths.tolist() == [n + N for n in lens]
    walks = [_walk(perm, int(p[-1]), N) for p in prompts]
    for b, n in enumerate(lens):
        assert out[b, :n].tolist() == prompts[b].tolist()
        assert out[b, n:n + N].tolist() == walks[b], (b, out[b])
        assert bool((out[b, n + N:] == 63).all())

    stop = walks[0][4]                               # the 5th new token of row 0
    assert stop not in walks[0][:4]
    out2, lengths2 = gen.generate_batch(prompts, N, stop_token=stop, pad_token=63)
    want_new = [w.index(stop) + 1 if stop in w else N for w in walks]        # from perm alone
    assert want_new[0] == 5
    assert lengths2.tolist() == [n + k for n, k in zip(lens, want_new)]
    assert int(lengths2[0]) == 4 + 5
    for b, (n, k) in enumerate(zip(lens, want_new)):
        assert out2[b, :n + k].tolist() == prompts[b].tolist() + walks[b][:k]
        assert bool((out2[b, n + k:] == 63).all())


def test_equal_lengths_greedy_matches_generate(trained):
    tr, _ = trained
    gen = mipipe.Generator.from_model(tr.stages[0].model)
    prompt = _held_out(3, 8)
    out, lengths = gen.generate_batch(list(prompt), 20)
    assert torch.equal(out, gen.generate(prompt, 20)) and lengths.tolist() == [28] * 3
    out0, lengths0 = gen.generate_batch(list(prompt), 0)
    assert torch.equal(out0, prompt) and lengths0.tolist() == [8] * 3


def test_seeds_and_sampling_switches():
    cfg = _gpt2(vocab=60)            # padded to 64 columns: ids 60..63 must never come out
    assert cfg.vocab_padded == 64
    gen = mipipe.Generator(cfg, CPU, dtype=torch.float32, seed=5)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, 60, (n,), generator=g) for n in (8, 3, 5)]
    # make the padded columns attractive: only the vocabulary bound keeps them out
    gen.arena.master_view("tok_embeddings.weight")[60:] *= 50.0
    gen.arena.sync_w16()
    a, la = gen.generate_batch(prompts, 24, temperature=1.5, seed=11)
    b, _ = gen.generate_batch(prompts, 24, temperature=1.5, seed=11)
    c, _ = gen.generate_batch(prompts, 24, temperature=1.5, seed=12)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert la.tolist() == [32, 27, 29]
    assert int(a.max()) < 60 and int(c.max()) < 60
    greedy, _ = gen.generate_batch(prompts, 24)
    assert int(greedy.max()) < 60
    k1, _ = gen.generate_batch(prompts, 24, temperature=1.5, top_k=1, seed=3)
    assert torch.equal(k1, greedy)                   # top-1 sampling is greedy
    # a nucleus below the top token's probability (>= 1 / 60) holds that token alone
    p0, _ = gen.generate_batch(prompts, 24, temperature=1.5, top_p=1e-3, seed=3)
    assert torch.equal(p0, greedy)
    kp, _ = gen.generate_batch(prompts, 24, temperature=1.5, top_k=40, top_p=0.9, seed=3)
    assert int(kp.max()) < 60 and not torch.equal(kp, greedy)


def test_argument_errors():
    gen = mipipe.Generator(_gpt2(), CPU, dtype=torch.float32, seed=5)
    ok = [torch.tensor([1, 2, 3]), torch.tensor([7, 8])]
    with pytest.raises(ValueError):
        gen.generate_batch([torch.tensor([1, 2]), torch.tensor([], dtype=torch.int64)], 4)      # an empty prompt
    with pytest.raises(ValueError):
        gen.generate_batch([], 4)
    with pytest.raises(ValueError, match="max_seq_len"):
        gen.generate_batch(ok, 30)                   # 3 + 30 > 32
    assert gen.generate_batch(ok, 29)[0].shape == (2, 32)
    with pytest.raises(ValueError, match="pad_token"):
        gen.generate_batch(ok, 4, pad_token=64)
    with pytest.raises(ValueError, match="stop_token"):
        gen.generate_batch(ok, 4, stop_token=64)
    with pytest.raises(ValueError):
        gen.generate_batch(ok, 4, temperature=1.0, top_p=0.0)
    with pytest.raises(ValueError):
        gen.generate_batch(ok, 4, graphs=True)       # graphs need a GPU
    with pytest.raises(ValueError):
        gen.generate_batch([torch.tensor([1, 64])], 4)


def test_cli_ragged_matches_api(trained, tmp_path):
    tr, perm = trained
    path = str(tmp_path / "ckpt")
    save_checkpoint(tr, path)
    gen = mipipe.Generator.from_model(tr.stages[0].model)
    prompts = [torch.tensor([1, 2, 3]), torch.tensor([7, 8])]
    stop = int(gen.generate_batch(prompts, 12)[0][0, 3 + 3])      # row 0's 4th new token
    out, lengths = gen.generate_batch(prompts, 12, stop_token=stop)
    want = [r[:n] for r, n in zip(out.tolist(), lengths.tolist())]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint", path, "--prompt",
                        "1,2,3;7,8", "--max-new-tokens", "12", "--stop-token", str(stop), "--device", "cpu"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = [[int(t) for t in line.split(",")] for line in r.stdout.strip().splitlines()]
    assert got == want and len(got[0]) < 3 + 12
