"""Generation with an int8 KV cache on the GPU (csrc/kernels/attention_kv8.hip), the tiny GPT-2
(head_dim 64) and Llama (head_dim 128, rep 4) configs of test_generate_gpu.py.

The logit bound.  The int8-cache decode logits on the GPU differ from the GPU bf16-cache logits
for two reasons only, which at worst add: the quantisation of the cache, measured on the CPU as
``e_quant`` (int8 against float cache, same weights and tokens, f32 paths), and the rounding of
the bf16 kernels, measured as test_generate_gpu.py measures it: ``e_full``, the GPU full forward
against the CPU path.  With that test's own factor two as the margin:
``max |gpu_int8 - gpu_bf16| <= 2 * (e_quant + e_full)``.  All three numbers are printed."""
import math

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext

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


def _incremental(gen, tokens, S0, kv):
    """teacher-forced logits of positions S0 - 1 .. S - 1: a prefill, then decode steps"""
    B, S = tokens.shape
    cache = gen.new_cache(B, S, kv=kv)
    rows = [gen.prefill(tokens[:, :S0].to(gen.device), cache)]
    for t in range(S0, S):
        rows.append(gen.decode(tokens[:, t].to(gen.device), cache))
    return torch.stack(rows, 1)[..., : gen.cfg.vocab_size].float().cpu(), cache


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_int8_cache_logits_within_quantisation_plus_kernel_error(family):
    cfg = _cfg(family)
    dev = torch.device("cuda", 0)
    gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4)
    ref = mipipe.Generator(cfg, "cpu", dtype=torch.float32, init=False)
    ref.arena.load_state_dict({n: gen.arena.w(n).float().cpu() for n in gen.arena.order})
    B, S0, steps = 2, 16, 32
    S = S0 + steps
    tokens = torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(5))
    e_full = float((_full_logits(gen.model, tokens) - _full_logits(ref.model, tokens)).abs().max())
    cpu_f, _ = _incremental(ref, tokens, S0, "bf16")
    cpu_8, _ = _incremental(ref, tokens, S0, "int8")
    e_quant = float((cpu_8 - cpu_f).abs().max())
    gpu_f, _ = _incremental(gen, tokens, S0, "bf16")
    gpu_8, c8 = _incremental(gen, tokens, S0, "int8")
    e = float((gpu_8 - gpu_f).abs().max())
    bound = 2 * (e_quant + e_full)
    print(f"\n[{family}] e_quant(cpu) = {e_quant:.6f}  e_full = {e_full:.6f}  |gpu int8 - gpu bf16| = {e:.6f}  "
          f"bound = {bound:.6f}")
    assert math.isfinite(e) and e_quant > 0 and e_full > 0
    assert e <= bound, (e, e_quant, e_full)
    assert c8.k[0].dtype == torch.int8 and c8.nbytes == 2 * cfg.n_layers * B * S * ops.generate.kv8_row_bytes(
        cfg.n_kv_heads, cfg.head_dim)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_batch_graphs_and_speculative(family):
    cfg = _cfg(family)
    dev = torch.device("cuda", 0)
    gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4, kv_cache="int8")
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (1, 9, 4)]
    eager, le = gen.generate_batch(prompts, 24, graphs=False)
    graph, lg = gen.generate_batch(prompts, 24, graphs=True)
    assert torch.equal(eager, graph) and torch.equal(le, lg)
    s1, _ = gen.generate_batch(prompts, 24, temperature=0.8, top_k=40, top_p=0.9, seed=3, graphs=False)
    s2, _ = gen.generate_batch(prompts, 24, temperature=0.8, top_k=40, top_p=0.9, seed=3, graphs=True)
    assert torch.equal(s1, s2)
    # a bf16-cache target with an int8-cache draft of the same weights completes with the target's
    # tokens: every emitted token's CPU-reference logit is within 4 * e_full of that position's
    # maximum (the measure and margin of test_generate_extend_gpu.py: the one-row and T-row paths
    # may round a near-tie differently, so generate_batch's tokens are not the yardstick)
    target = mipipe.Generator.from_model(gen.model)
    assert target.kv_cache == "bf16" and gen.kv_cache == "int8"
    ref = mipipe.Generator(cfg, "cpu", dtype=torch.float32, init=False)
    ref.arena.load_state_dict({n: gen.arena.w(n).float().cpu() for n in gen.arena.order})
    N, V = 24, cfg.vocab_size
    out, lens, stats = target.generate_speculative(prompts, N, gen, lookahead=4)
    assert lens.tolist() == [int(p.numel()) + N for p in prompts] and int(out.max()) < V
    assert stats["rounds"] > 0 and 0 < stats["accepted"] <= stats["drafted"]
    out = out.cpu()
    worst, e_full = 0.0, 0.0
    for b, p in enumerate(prompts):
        n = int(p.numel())
        assert torch.equal(out[b, :n], p)
        row = out[b:b + 1, : n + N]
        cpu = _full_logits(ref.model, row)
        e_full = max(e_full, float((_full_logits(gen.model, row) - cpu).abs().max()))
        lg = cpu[0, n - 1:n + N - 1]
        worst = max(worst, float((lg.max(-1).values - lg.gather(1, row[0, n:, None])[:, 0]).max()))
    print(f"\n[{family}] e_full = {e_full:.6f}  worst shortfall of an emitted token = {worst:.6f}  "
          f"bound = {4 * e_full:.6f}  accepted {stats['accepted']} of {stats['drafted']} in {stats['rounds']} rounds")
    assert worst <= 4 * e_full, (worst, e_full)
    # and the int8-cache generator as the target of a bf16-cache draft
    out8, l8, _ = gen.generate_speculative(prompts, N, target, lookahead=3)
    assert out8.shape == eager.shape and torch.equal(l8, le)
