"""Generator.extend and greedy speculative decoding on the GPU (bf16 HIP kernels), on the two
configurations of test_generate_batch_gpu.py (head dims 64 and 128, rep 4) with that file's
own bound: ``e_full`` is the largest absolute logit difference between the GPU full forward
and the CPU f32 generator on the same bf16-rounded weights and tokens.

* Teacher-forced logits from a mix of calls -- ``prefill(lens=[1, 16, 7])``, ``extend`` with
  T = 5 and counts [5, 2, 0], ``decode``, ``extend`` with T = 8 and ``all_logits=True`` --
  must be within ``2 * e_full`` of the CPU path.  Both numbers are printed.
* ``generate_speculative`` with ``lookahead = 4`` and the target as its own draft: every
  emitted token's CPU-reference logit is within ``4 * e_full`` of that position's reference
  maximum (each of the two logits compared may be off by ``2 * e_full``), ``lengths`` are
  ``len + N``, the prompts are reproduced, and two runs give equal tokens.

Exact token equality with ``generate_batch`` is not asserted here: the one-row and T-row
GEMM paths may round a near-tie differently."""
import math

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext

pytestmark = pytest.mark.gpu

LENS = [1, 16, 7]
COUNTS, T1, T2 = [5, 2, 0], 5, 8
S_ALL = 16 + 2 + 1 + T2                    # the longest row after every call


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


_SETUP = {}


def _setup(family):
    """(cfg, device, GPU generator, CPU f32 generator on the same weights, tokens, the CPU
    full-forward logits of the tokens, e_full), built once per family."""
    if family not in _SETUP:
        cfg = _cfg(family)
        dev = torch.device("cuda", 0)
        gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4)
        ref = mipipe.Generator(cfg, "cpu", dtype=torch.float32, init=False)
        ref.arena.load_state_dict({n: gen.arena.w(n).float().cpu() for n in gen.arena.order})
        tokens = torch.randint(0, cfg.vocab_size, (len(LENS), S_ALL), generator=torch.Generator().manual_seed(5))
        cpu_full = _full_logits(ref.model, tokens)
        e_full = float((_full_logits(gen.model, tokens) - cpu_full).abs().max())
        assert math.isfinite(e_full) and e_full > 0
        _SETUP[family] = (cfg, dev, gen, ref, tokens, cpu_full, e_full)
    return _SETUP[family]


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_mixed_calls_within_twice_full_forward_error(family):
    cfg, dev, gen, _, tokens, cpu_full, e_full = _setup(family)
    assert cfg.head_dim == (64 if family == "gpt2" else 128)
    B, V = len(LENS), cfg.vocab_size
    at = list(LENS)                                  # tokens consumed per row
    cache = gen.new_cache(B, max(LENS) + T1 + 1 + T2)       # cache.pos is a bound: it counts T per extend
    err = 0.0

    def check(lg, b, pos):                           # lg: the logits of position pos of row b
        nonlocal err
        err = max(err, float((lg[:V].float().cpu() - cpu_full[b, pos]).abs().max()))

    lg = gen.prefill(tokens[:, : max(LENS)].to(dev), cache, lens=LENS)
    for b in range(B):
        check(lg[b], b, at[b] - 1)
    new = torch.stack([tokens[b, n:n + T1] for b, n in enumerate(at)]).to(dev)
    lg = gen.extend(new, cache, counts=COUNTS)
    assert bool(torch.isfinite(lg.float()).all())
    at = [n + c for n, c in zip(at, COUNTS)]
    assert cache.lens.tolist() == at and cache.ragged
    for b in range(B):
        if COUNTS[b]:
            check(lg[b], b, at[b] - 1)
    lg = gen.decode(torch.stack([tokens[b, n] for b, n in enumerate(at)]).to(dev), cache)
    at = [n + 1 for n in at]
    for b in range(B):
        check(lg[b], b, at[b] - 1)
    new = torch.stack([tokens[b, n:n + T2] for b, n in enumerate(at)]).to(dev)
    lg = gen.extend(new, cache, all_logits=True)
    assert lg.shape == (B, T2, cfg.vocab_padded)
    for b in range(B):
        for t in range(T2):
            check(lg[b, t], b, at[b] + t)
    at = [n + T2 for n in at]
    assert cache.lens.tolist() == at and max(at) == S_ALL
    print(f"\n[{family}] e_full = {e_full:.6f}  e_mixed_calls = {err:.6f}  bound = {2 * e_full:.6f}")
    assert math.isfinite(err)
    assert err <= 2 * e_full, (err, e_full)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_speculative_emits_near_maximal_tokens_and_is_deterministic(family):
    cfg, dev, gen, ref, tokens, _, e_full = _setup(family)
    N, V = 24, cfg.vocab_size
    prompts = [tokens[b, :n] for b, n in enumerate(LENS)]
    out, lengths, stats = gen.generate_speculative(prompts, N, gen, lookahead=4)
    again, lengths2, _ = gen.generate_speculative(prompts, N, gen, lookahead=4)
    assert torch.equal(out, again) and torch.equal(lengths, lengths2)
    assert lengths.tolist() == [n + N for n in LENS] and int(out.max()) < V
    assert stats["rounds"] >= math.ceil((N - 1) / 5) and 0 <= stats["accepted"] <= stats["drafted"]
    out = out.cpu()
    worst = 0.0
    for b, n in enumerate(LENS):
        assert torch.equal(out[b, :n], prompts[b])
        row = out[b:b + 1, : n + N]
        lg = _full_logits(ref.model, row)[0, n - 1:n + N - 1]           # the positions that emitted row[n:]
        short = lg.max(-1).values - lg.gather(1, row[0, n:, None])[:, 0]
        worst = max(worst, float(short.max()))
    print(f"\n[{family}] e_full = {e_full:.6f}  worst shortfall of an emitted token = {worst:.6f}  "
          f"bound = {4 * e_full:.6f}  accepted {stats['accepted']} of {stats['drafted']} in {stats['rounds']} rounds")
    assert worst <= 4 * e_full, (worst, e_full)
