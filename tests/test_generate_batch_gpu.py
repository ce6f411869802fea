"""Ragged-batch generation on the GPU (bf16 HIP kernels), on the two configurations of
test_generate_gpu.py (head dims 64 and 128, rep 4).

* Teacher-forced ragged logits (prompt lengths [1, 16, 7], 32 decode steps) against the CPU
  f32 generator of the same bf16-rounded weights, with that file's own bound: ``e_full`` is
  the largest absolute logit difference between the GPU full forward and the CPU path on
  the same tokens, and the ragged incremental logits must be within ``2 * e_full`` of the
  CPU path.  Both numbers are printed.
* The graph-replayed step against the eager one, on the same inputs and seed: equal tokens
  (greedy, and top_k = 40 with top_p = 0.9), bit-equal teacher-forced logits, and equal
  ``lengths`` with a stop token.  Both modes run the same kernels on the same grids.
"""
import math

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext
from mipipe.parallel.graphs import GraphCache

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


LENS, STEPS = [1, 16, 7], 32


def _setup(family):
    cfg = _cfg(family)
    dev = torch.device("cuda", 0)
    gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4)
    tokens = torch.randint(0, cfg.vocab_size, (len(LENS), max(LENS) + STEPS), generator=torch.Generator().manual_seed(5))
    return cfg, dev, gen, tokens


def _teacher_forced(gen, tokens, dev, graph: bool):
    """Logits [B, STEPS + 1, vocab_padded] of the ragged run: row b is tokens[b, : LENS[b] +
    STEPS], teacher-forced.  ``graph``: the first decode step eager, the second captured,
    the rest replayed."""
    B, S0 = len(LENS), max(LENS)
    cache = gen.new_cache(B, S0 + STEPS)
    rows = [gen.prefill(tokens[:, :S0].to(dev), cache, lens=LENS).clone()]
    tok = torch.empty(B, dtype=torch.int64, device=dev)
    act = torch.ones(B, dtype=torch.uint8, device=dev)
    logits = torch.empty_like(rows[0])
    gc = GraphCache("T")
    for t in range(STEPS):
        tok.copy_(torch.stack([tokens[b, n + t] for b, n in enumerate(LENS)]))
        if graph and t > 0:
            gc.run("step", (), lambda _: gen.decode(tok, cache, active=act, out=logits))
        else:
            gen.decode(tok, cache, active=act, out=logits)
        rows.append(logits.clone())
    assert not graph or (gc.captures == 1 and gc.replays == STEPS - 2)
    assert cache.lens.tolist() == [n + STEPS for n in LENS]
    return torch.stack(rows, 1)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_ragged_incremental_within_twice_full_forward_error_and_graph_equal(family):
    cfg, dev, gen, tokens = _setup(family)
    assert cfg.head_dim == (64 if family == "gpt2" else 128)
    ref = mipipe.Generator(cfg, "cpu", dtype=torch.float32, init=False)
    ref.arena.load_state_dict({n: gen.arena.w(n).float().cpu() for n in gen.arena.order})
    cpu_full = _full_logits(ref.model, tokens)
    e_full = float((_full_logits(gen.model, tokens) - cpu_full).abs().max())

    eager = _teacher_forced(gen, tokens, dev, graph=False)
    inc = eager[..., : cfg.vocab_size].float().cpu()
    e_inc = 0.0
    for b, n in enumerate(LENS):                     # row b, step t: the logits of position n - 1 + t
        e_inc = max(e_inc, float((inc[b] - cpu_full[b, n - 1:n + STEPS]).abs().max()))
    print(f"\n[{family}] e_full = {e_full:.6f}  e_ragged_incremental = {e_inc:.6f}  bound = {2 * e_full:.6f}")
    assert math.isfinite(e_inc) and e_full > 0
    assert e_inc <= 2 * e_full, (e_inc, e_full)

    replayed = _teacher_forced(gen, tokens, dev, graph=True)
    assert torch.equal(replayed, eager)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_graphs_on_and_off_give_the_same_tokens(family):
    cfg, dev, gen, tokens = _setup(family)
    prompts = [tokens[b, :n] for b, n in enumerate(LENS)]
    N = 40
    for kw in (dict(), dict(temperature=0.9, top_k=40, top_p=0.9, seed=7)):
        off, l_off = gen.generate_batch(prompts, N, graphs=False, **kw)
        on, l_on = gen.generate_batch(prompts, N, graphs=True, **kw)
        assert torch.equal(on, off) and torch.equal(l_on, l_off), kw
        assert l_off.tolist() == [n + N for n in LENS] and int(off.max()) < cfg.vocab_size
        for b, n in enumerate(LENS):
            assert torch.equal(off[b, :n].cpu(), prompts[b])
    sampled, _ = gen.generate_batch(prompts, N, temperature=0.9, top_k=40, top_p=0.9, seed=8)     # graphs=None
    assert not torch.equal(sampled, on)

    # a stop token through the graph path: the same lengths as the eager path
    free, _ = gen.generate_batch(prompts, N, graphs=False)
    stop = int(free[0, LENS[0] + 5])
    off, l_off = gen.generate_batch(prompts, N, stop_token=stop, pad_token=3, graphs=False)
    on, l_on = gen.generate_batch(prompts, N, stop_token=stop, pad_token=3, graphs=True)
    assert torch.equal(l_on, l_off) and torch.equal(on, off)
    first = (free[0, LENS[0]:] == stop).nonzero()[0, 0].item() + 1
    assert int(l_off[0]) == LENS[0] + first <= LENS[0] + 6
    assert bool((off[0, int(l_off[0]):] == 3).all()) and int(off[0, int(l_off[0]) - 1]) == stop
    for b in range(len(LENS)):                       # up to its end every row is the free run
        n = int(l_off[b])
        assert torch.equal(off[b, :n], free[b, :n])
