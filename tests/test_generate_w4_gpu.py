"""int4g128 weight-only generation on the GPU, on the tiny models of test_generate_w4_cpu.py.

* The recipe of test_generate_w8_gpu.py: prefill on 16 tokens (32 rows: the dequantising
  route), then 48 teacher-forced decode steps (2 rows: the 4-bit skinny kernel), B = 2, both
  families.  The oracle is the CPU f32 generator holding ``What = q * scale``; ``e_b`` is the
  error of the bf16 GPU generator loaded with ``bf16(What)``, and the int4g128 generator must
  satisfy ``e_q <= 2 e_b``, that file's margin for a second, different set of bf16 kernels.
  The test prints the figures (profiles/r13_w4_decode.md records a run on an MI355X).
* ``generate_batch`` on three ragged prompts: graph replay gives the eager tokens.
* ``generate_speculative`` of a bf16 target with its own int4g128 draft: every emitted token is
  the target's greedy choice -- its CPU-reference logit is within ``4 e_full`` of the position's
  maximum, as test_generate_extend_gpu.py asserts it -- and the tokens equal the target's
  ``generate_batch`` up to the first position whose reference top-2 gap is below ``4 e_full``
  (where the one-row and T-row paths of the target may round a near-tie differently).
* The dequantisation scratch holds N * K values of the largest matrix and is allocated by the
  first eager call of more than 16 rows; later prefills reuse it."""
import math

import pytest
import torch

import mipipe
from mipipe import ops

from test_generate_w4_cpu import W4, _cfg, dense_oracle

pytestmark = pytest.mark.gpu


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _incremental(gen, tokens, S0):
    dev = gen.device
    B, S = tokens.shape
    cache = gen.new_cache(B, S)
    rows = [gen.prefill(tokens[:, :S0].to(dev), cache)]
    for t in range(S0, S):
        rows.append(gen.decode(tokens[:, t].to(dev), cache))
    return torch.stack(rows, 1)[..., : gen.cfg.vocab_size].float().cpu()


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_int4_within_twice_the_bf16_error(family):
    cfg = _cfg(family)
    dev = torch.device("cuda", 0)
    q = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4, weights=W4)
    head = q.arena.q[q.arena.head_name]
    assert head.dtype == torch.uint8 and head.is_cuda and head.shape == (cfg.vocab_padded, cfg.d_model // 2)
    oracle = dense_oracle(q)                                   # CPU f32, holds What
    base = dense_oracle(q, dev, torch.bfloat16)                # the bf16 path on bf16(What)
    B, S0, steps = 2, 16, 48
    tokens = torch.randint(0, cfg.vocab_size, (B, S0 + steps), generator=torch.Generator().manual_seed(5))
    want = _incremental(oracle, tokens, S0)
    e_b = float((_incremental(base, tokens, S0) - want).abs().max())
    got = _incremental(q, tokens, S0)
    e_q = float((got - want).abs().max())
    e_prefill = float((got[:, 0] - want[:, 0]).abs().max())
    print(f"\n[{family}] e_bf16 = {e_b:.6f}  e_int4g128 = {e_q:.6f} (prefill row {e_prefill:.6f})  bound = {2 * e_b:.6f}")
    assert math.isfinite(e_q) and e_b > 0
    assert e_q <= 2 * e_b, (e_q, e_b)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_batch_graphs_equal_eager_on_int4(family):
    cfg = _cfg(family)
    q = mipipe.Generator(cfg, torch.device("cuda", 0), dtype=torch.bfloat16, seed=4, weights=W4)
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (3, 17, 9)]
    eager, le = q.generate_batch(prompts, 24, graphs=False)
    replay, lr = q.generate_batch(prompts, 24, graphs=True)
    assert torch.equal(eager, replay) and torch.equal(le, lr)
    # up to 16 rows every linear layer is the skinny kernel, whose rows are independent
    x = torch.randn(15, cfg.d_model, device="cuda", dtype=torch.bfloat16)
    name = "layers.0.attn.wqkv.weight"
    many = q._linear(x, name)
    for m in (0, 7, 14):
        assert torch.equal(q._linear(x[m: m + 1], name), many[m: m + 1])


def test_speculative_with_int4_draft_returns_the_targets_greedy_tokens():
    cfg = _cfg("gpt2")
    dev = torch.device("cuda", 0)
    target = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4)
    draft = mipipe.Generator.from_model(target.model, weights=W4)
    ref = mipipe.Generator(cfg, "cpu", dtype=torch.float32, init=False)
    ref.arena.load_state_dict({n: target.arena.w(n).float().cpu() for n in target.arena.order})
    lens, N, V = [1, 16, 7], 24, cfg.vocab_size
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, V, (n,), generator=g) for n in lens]
    out, lengths, stats = target.generate_speculative(prompts, N, draft, lookahead=4)
    again, lengths2, _ = target.generate_speculative(prompts, N, draft, lookahead=4)
    assert torch.equal(out, again) and torch.equal(lengths, lengths2)
    assert lengths.tolist() == [n + N for n in lens] and int(out.max()) < V
    assert stats["drafted"] > 0 and 0 <= stats["accepted"] <= stats["drafted"]
    greedy, gl = target.generate_batch(prompts, N, graphs=False)
    assert torch.equal(gl.cpu(), lengths.cpu())
    out, greedy = out.cpu(), greedy.cpu()
    worst, e_full, checked = 0.0, 0.0, 0
    for b, n in enumerate(lens):
        assert torch.equal(out[b, :n], prompts[b])
        row = out[b:b + 1, : n + N]
        cache_r, cache_t = ref.new_cache(1, n + N), target.new_cache(1, n + N)
        lg = ref.extend(row, cache_r, all_logits=True)[0, :, :V].float()
        lt = target.extend(row.to(dev), cache_t, all_logits=True)[0, :, :V].float().cpu()
        e_full = max(e_full, float((lt - lg).abs().max()))
        lg = lg[n - 1:n + N - 1]                                          # the positions that emitted row[n:]
        short = lg.max(-1).values - lg.gather(1, row[0, n:, None])[:, 0]
        worst = max(worst, float(short.max()))
    for b, n in enumerate(lens):
        row = out[b:b + 1, : n + N]
        lg = ref.extend(row, ref.new_cache(1, n + N), all_logits=True)[0, n - 1:n + N - 1, :V].float()
        top2 = lg.topk(2, -1).values
        close = ((top2[:, 0] - top2[:, 1]) < 4 * e_full).nonzero()
        upto = int(close[0]) if close.numel() else N               # tokens before the first near-tie
        assert torch.equal(out[b, n:n + upto], greedy[b, n:n + upto]), (b, upto)
        checked += upto
    print(f"\ne_full = {e_full:.6f}  worst shortfall of an emitted token = {worst:.6f}  bound = {4 * e_full:.6f}  "
          f"accepted {stats['accepted']} of {stats['drafted']}; {checked} of {3 * N} tokens before a near-tie equal "
          f"generate_batch")
    assert e_full > 0 and worst <= 4 * e_full, (worst, e_full)


def test_prefill_of_more_than_16_rows_uses_an_n_times_k_scratch():
    cfg = _cfg("llama")
    dev = torch.device("cuda", 0)
    q = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4, weights=W4)
    oracle = dense_oracle(q)
    A = q.arena
    tok = torch.randint(0, cfg.vocab_size, (2, 20), generator=torch.Generator().manual_seed(8))
    cache = q.new_cache(2, 64)
    q.prefill(tok[:, :4].to(dev), cache)                      # 8 rows: the skinny kernel, no scratch
    q.decode(tok[:, 4].to(dev), cache)
    assert q._scratch is None
    # 40 rows: dequantise into the scratch, which must hold N * K of the largest matrix (the
    # packed tensor has half as many elements)
    big = max(A.specs[n].shape[0] * A.specs[n].shape[1] for n in A.q)
    cache = q.new_cache(2, 64)
    lg = q.prefill(tok.to(dev), cache)
    assert q._scratch is not None and q._scratch.numel() == big == A.max_matrix_numel()
    ptr = q._scratch.data_ptr()
    want = oracle.prefill(tok, oracle.new_cache(2, 64))
    base = dense_oracle(q, dev, torch.bfloat16)
    e_b = float((base.prefill(tok.to(dev), base.new_cache(2, 64)).float().cpu() - want).abs().max())
    e_q = float((lg.float().cpu() - want).abs().max())
    print(f"\nprefill of 40 rows: e_bf16 = {e_b:.6f}  e_int4g128 = {e_q:.6f}  bound = {2 * e_b:.6f}")
    assert e_q <= 2 * e_b, (e_q, e_b)
    # a later, larger prefill and a graph-replayed generation find the scratch in place
    q.prefill(torch.cat([tok, tok], 0).to(dev), q.new_cache(4, 64))
    out, _ = q.generate_batch([tok[0, :18], tok[1, :3]], 8, graphs=True)
    assert q._scratch.data_ptr() == ptr and out.shape[0] == 2
