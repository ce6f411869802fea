"""KV-cache generation on the GPU (bf16 HIP kernels).

* The incremental path (prefill on 16 tokens, 48 teacher-forced decode steps) against the
  CPU f32 path of the same (bf16-rounded) weights.  The bound comes from what the existing
  kernels already do: ``e_full`` is the largest absolute logit difference between the GPU
  full forward and the CPU path over the same 64 tokens, and the incremental logits must be
  within ``2 * e_full`` of the CPU path -- the decode step rounds through a second,
  different set of bf16 kernels (M = B row GEMMs, split-KV attention).  Both numbers are
  printed.
* A GPT-2 trained on the ``pattern`` stream (the test_learns_pattern_gpu recipe) reproduces
  the permutation walk when sampled greedily through the KV cache.
"""
import math
import os
import sys

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.engine import PipelineTrainer
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import train as _train  # noqa: E402

pytestmark = pytest.mark.gpu


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _cfg(family):
    if family == "gpt2":     # head_dim 64
        return NativeConfig.gpt2("tiny", vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024,
                                 max_seq_len=128)
    return NativeConfig.llama3("tiny", vocab_size=512, d_model=1024, n_layers=2, n_heads=8, n_kv_heads=2, d_ff=2048,
                               max_seq_len=128)    # head_dim 128, rep 4


def _full_logits(model, tokens):
    B, S = tokens.shape
    lg = model.forward(tokens.to(model.device), MBContext(0, 0), B, S, target=None)
    return lg.view(B, S, -1)[..., : model.cfg.vocab_size].float().cpu()


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_incremental_matches_cpu_within_twice_full_forward_error(family):
    cfg = _cfg(family)
    assert cfg.head_dim == (64 if family == "gpt2" else 128)
    dev = torch.device("cuda", 0)
    gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4)
    # the CPU f32 path of the same weights: the bf16 values the kernels read
    ref = mipipe.Generator(cfg, "cpu", dtype=torch.float32, init=False)
    ref.arena.load_state_dict({n: gen.arena.w(n).float().cpu() for n in gen.arena.order})
    B, S0, steps = 2, 16, 48
    S = S0 + steps
    tokens = torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(5))
    cpu_full = _full_logits(ref.model, tokens)
    e_full = float((_full_logits(gen.model, tokens) - cpu_full).abs().max())

    cache = gen.new_cache(B, S)
    rows = [gen.prefill(tokens[:, :S0].to(dev), cache)]
    for t in range(S0, S):
        rows.append(gen.decode(tokens[:, t].to(dev), cache))
    inc = torch.stack(rows, 1)[..., : cfg.vocab_size].float().cpu()          # positions S0-1 .. S-1
    e_inc = float((inc - cpu_full[:, S0 - 1:]).abs().max())
    print(f"\n[{family}] e_full = {e_full:.6f}  e_incremental = {e_inc:.6f}  bound = {2 * e_full:.6f}")
    assert math.isfinite(e_inc) and e_full > 0
    assert e_inc <= 2 * e_full, (e_inc, e_full)


def test_learned_walk_gpu():
    dev = torch.device("cuda", 0)
    cfg = NativeConfig.gpt2("tiny", vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024, max_seq_len=128)
    m, mbs, seq = 4, 8, 128
    tr = PipelineTrainer(cfg, pp=1, schedule="1F1B", n_microbatches=m, mbs=mbs, seq_len=seq, device=dev,
                         dtype=torch.bfloat16, lr=2e-3, seed=0, graphs=True)
    data = _train.TokenData("pattern:256", cfg.vocab_size, m * mbs, seq, dev, 0, 0)
    tr.capture_graphs(*data.batch(0))
    losses = [float(tr.train_step(*data.batch(s))) for s in range(200)]
    tail = sorted(losses[-10:])
    assert tail[len(tail) // 2] < 0.1, losses[::20]

    model = tr.stages[0].model
    gen = mipipe.Generator.from_model(model)
    held = _train.TokenData("pattern:256", cfg.vocab_size, 8, seq, dev, 0, 0)
    prompt = held.batch(100003)[0][:, :16].contiguous()
    out = gen.generate(prompt, 64)
    assert out.shape == (8, 80) and torch.equal(out[:, :16], prompt)
    walk = torch.equal(out[:, 16:], data.perm[out[:, 15:-1]])
    if not walk:
        # does the trained model's own full-forward greedy decoding miss the walk too?  Then
        # the generator is held to that sequence instead (and the run says so)
        full = prompt.clone()
        for _ in range(64):
            Bf, Sf = full.shape
            lg = model.forward(full, MBContext(0, 0), Bf, Sf, target=None).view(Bf, Sf, -1)
            full = torch.cat([full, lg[:, -1, : cfg.vocab_size].float().argmax(-1, keepdim=True)], 1)
        full_walk = torch.equal(full[:, 16:], data.perm[full[:, 15:-1]])
        print(f"\nfull-forward greedy follows the permutation: {full_walk}")
        assert not full_walk, "the full forward follows the walk but the KV-cache generator does not"
        assert torch.equal(out, full), "generator differs from the model's own full-forward greedy sequence"
