"""KV-cache generation on the CPU (f32 reference paths of the ops): the incremental
prefill / decode path computes what the full forward computes, the decode attention op
agrees with ``attn_fwd`` at ``Sq = 1``, a model trained on the ``pattern`` stream reproduces
the permutation walk when sampled, checkpoints written at PP = 1 and PP = 2 load by FQN, and
the CLI prints what the API returns."""
import os
import subprocess
import sys

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.engine import PipelineTrainer
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext, NativeModel
from mipipe.utils.checkpoint import load_weights, save_checkpoint

from dist_utils import run_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import train as _train  # noqa: E402

CPU = torch.device("cpu")


def _gpt2(vocab=64):
    return NativeConfig.gpt2("tiny", vocab_size=vocab, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32)


def _llama():
    return NativeConfig.llama3("tiny", vocab_size=64, d_model=64, n_layers=2, n_heads=4, n_kv_heads=2, d_ff=128,
                               max_seq_len=32)


def _full_last_logits(model: NativeModel, tokens: torch.Tensor) -> torch.Tensor:
    B, S = tokens.shape
    logits = model.forward(tokens, MBContext(0, 0), B, S, target=None)
    return logits.view(B, S, -1)[:, -1]


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_incremental_equals_full(family):
    cfg = _gpt2() if family == "gpt2" else _llama()
    if family == "llama":
        assert cfg.head_dim == 16 and cfg.pos == "rope" and cfg.activation == "swiglu"
    gen = mipipe.Generator(cfg, CPU, dtype=torch.float32, seed=3)
    B, S0, steps = 3, 5, 11
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, cfg.vocab_size, (B, S0 + steps), generator=g)
    cache = mipipe.KVCache(cfg, B, S0 + steps, CPU, torch.float32)
    got = gen.prefill(tokens[:, :S0], cache)
    torch.testing.assert_close(got, _full_last_logits(gen.model, tokens[:, :S0]), atol=1e-4, rtol=1e-4)
    for t in range(S0, S0 + steps):
        got = gen.decode(tokens[:, t], cache)
        assert cache.pos == t + 1 and cache.lens.tolist() == [t + 1] * B
        torch.testing.assert_close(got, _full_last_logits(gen.model, tokens[:, : t + 1]), atol=1e-4, rtol=1e-4)


def test_attn_decode_op_matches_attn_fwd_ragged():
    H, Hkv, D, Smax = 4, 2, 16, 24
    lens = [1, 7, 20]
    B = len(lens)
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, generator=g)
    q = qkv[:, : H * D]                                  # a strided slice, as in the model
    kc = torch.randn(B, Smax, Hkv * D, generator=g)
    vc = torch.randn(B, Smax, Hkv * D, generator=g)
    for b, n in enumerate(lens):                         # stale rows must not matter
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
    o = torch.zeros(B, H * D)
    ops.attn_decode(q, kc, vc, torch.tensor(lens, dtype=torch.int32), o, H, Hkv, D)
    for b, n in enumerate(lens):
        ref = torch.zeros(1, H * D)
        lse = torch.zeros(H)
        ops.attn_fwd(q[b:b + 1], kc[b, :n], vc[b, :n], ref, lse, 1, 1, n, H, Hkv, D, True)
        torch.testing.assert_close(o[b:b + 1], ref, atol=1e-6, rtol=1e-6)
    with pytest.raises(ValueError):
        ops.attn_decode(q, kc, vc, torch.tensor(lens, dtype=torch.int64), o, H, Hkv, D)


# ---------------------------------------------------------------------------- trained model
@pytest.fixture(scope="module")
def trained():
    """The tiny GPT-2 of test_learning.test_learns_pattern_pp1_cpu, trained the same way."""
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


def _held_out_prompts(n=4, S0=8):
    data = _train.TokenData("pattern:48", 64, n, 32, CPU, 0, 0)
    x, _ = data.batch(100003)        # a step no training batch used
    return x[:, :S0].contiguous()


def test_learned_walk(trained):
    tr, perm = trained
    gen = mipipe.Generator.from_model(tr.stages[0].model)
    assert gen.arena is tr.stages[0].model.arena          # shared, not copied
    prompt = _held_out_prompts()
    out = gen.generate(prompt, 24)
    assert out.shape == (4, 32) and torch.equal(out[:, :8], prompt)
    assert torch.equal(out[:, 8:], perm[out[:, 7:-1]]), out


@pytest.fixture(scope="module")
def saved(trained, tmp_path_factory):
    tr, _ = trained
    path = str(tmp_path_factory.mktemp("ckpt") / "pp1")
    save_checkpoint(tr, path)
    return path


def _probe_logits(gen):
    """Prefill + two decode steps on a fixed prompt."""
    prompt = _held_out_prompts(2, 6)
    cache = gen.new_cache(2, 8)
    out = [gen.prefill(prompt, cache)]
    for _ in range(2):
        out.append(gen.decode(out[-1][:, : gen.cfg.vocab_size].argmax(-1), cache))
    return torch.stack(out)


def test_checkpoint_round_trip_pp1(trained, saved):
    tr, _ = trained
    ref = _probe_logits(mipipe.Generator.from_model(tr.stages[0].model))
    gen = mipipe.Generator.load(saved, device="cpu")
    assert gen.dtype == torch.float32 and gen.cfg.vocab_size == 64
    assert torch.equal(_probe_logits(gen), ref)
    # the building block on its own: strict load into a fresh arena, and a missing tensor raises
    fresh = mipipe.Generator(_gpt2(), CPU, dtype=torch.float32, seed=9)
    load_weights([fresh.arena], saved)
    assert torch.equal(_probe_logits(fresh), ref)
    other = mipipe.Generator(NativeConfig.gpt2("tiny", vocab_size=64, d_model=64, n_layers=3, n_heads=4, d_ff=256,
                                               max_seq_len=32), CPU, dtype=torch.float32)
    with pytest.raises(KeyError):
        load_weights([other.arena], saved, strict=True)


def _pp2_save_worker(rank, world, path):
    tr = PipelineTrainer(_gpt2(), pp=2, schedule="1F1B", n_microbatches=2, mbs=8, seq_len=32, device=CPU,
                         dtype=torch.float32, lr=3e-3, seed=0, graphs=False)
    save_checkpoint(tr, path)
    return tr.head is not None


def test_checkpoint_round_trip_pp2_gloo(tmp_path):
    path = str(tmp_path / "pp2")
    res = run_world(_pp2_save_worker, 2, path)
    # PP = 2 keeps the tied vocabulary matrix in the distributed head's shard
    assert all(res.values()) and os.path.exists(os.path.join(path, "head.safetensors"))
    gen = mipipe.Generator.load(path, device="cpu")
    # the same seed at PP = 1: parameters are initialised per FQN, so the weights agree
    tr1 = PipelineTrainer(_gpt2(), pp=1, schedule="1F1B", n_microbatches=2, mbs=8, seq_len=32, device=CPU,
                          dtype=torch.float32, lr=3e-3, seed=0, graphs=False)
    ref = _probe_logits(mipipe.Generator.from_model(tr1.stages[0].model))
    assert torch.equal(_probe_logits(gen), ref)


def test_limits_and_sampling():
    cfg = _gpt2(vocab=60)            # padded to 64 columns: ids 60..63 must never come out
    assert cfg.vocab_padded == 64
    gen = mipipe.Generator(cfg, CPU, dtype=torch.float32, seed=5)
    prompt = torch.randint(0, 60, (2, 8), generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="max_seq_len"):
        gen.generate(prompt, 25)     # 8 + 25 > 32
    assert gen.generate(prompt, 24).shape == (2, 32)
    with pytest.raises(ValueError):
        mipipe.Generator(NativeConfig.reference(n_layers=2, n_heads=4, vocab_size=64, dim=64, dim_feedforward=128),
                         CPU, dtype=torch.float32)
    with pytest.raises(ValueError):
        mipipe.Generator(NativeConfig.gpt2("tiny", vocab_size=64, causal=False), CPU, dtype=torch.float32)
    # make the padded columns attractive: only the mask keeps them out
    gen.arena.master_view("tok_embeddings.weight")[60:] *= 50.0
    gen.arena.sync_w16()
    a = gen.generate(prompt, 24, temperature=1.5, seed=11)
    b = gen.generate(prompt, 24, temperature=1.5, seed=11)
    c = gen.generate(prompt, 24, temperature=1.5, seed=12)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.max()) < 60 and int(c.max()) < 60
    k = gen.generate(prompt, 24, temperature=1.5, top_k=1, seed=3)
    assert torch.equal(k, gen.generate(prompt, 24))      # top-1 sampling is greedy
    assert int(gen.generate(prompt, 24).max()) < 60


def test_cli_matches_api(trained, saved):
    tr, _ = trained
    prompt = _held_out_prompts(2, 8)
    want = mipipe.Generator.from_model(tr.stages[0].model).generate(prompt, 12)
    arg = ";".join(",".join(str(t) for t in row) for row in prompt.tolist())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint", saved, "--prompt", arg,
                        "--max-new-tokens", "12", "--device", "cpu"], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = [[int(t) for t in line.split(",")] for line in r.stdout.strip().splitlines()]
    assert got == want.tolist()
