"""int8 weight-only generation on the CPU (f32 reference paths of the ops).

A ``weights="int8"`` generator computes with ``What = q * scale``.  Its oracle is a bf16-mode
(dense) CPU generator whose arena was loaded with exactly those values
(``QuantWeights.effective_state_dict``); with tied embeddings the head's ``What`` differs from
the embedding table, so the oracle is the same model with the tie cut (``output.weight`` =
the head's ``What``).  The two run the same f32 arithmetic up to ``(x q^T) scale`` against
``x (q scale)^T``: logits agree at ``torch.testing.assert_close``'s f32 defaults through
prefill, decode, ragged decode, extend and generate_batch.  The configs are the tiny GPT-2
and Llama of test_generate_gpu.py."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

import mipipe
from mipipe.engine import PipelineTrainer
from mipipe.models.config import NativeConfig
from mipipe.models.generate import QUANTIZED, QuantWeights
from mipipe.utils.checkpoint import save_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
F32 = torch.float32


def _cfg(family):
    if family == "gpt2":
        return NativeConfig.gpt2("tiny", vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024,
                                 max_seq_len=128)
    return NativeConfig.llama3("tiny", vocab_size=512, d_model=1024, n_layers=2, n_heads=8, n_kv_heads=2, d_ff=2048,
                               max_seq_len=128)


def dense_oracle(qgen, device="cpu", dtype=F32):
    """the dense generator that holds the quantised generator's effective weights"""
    sd = qgen.arena.effective_state_dict()
    cfg = qgen.cfg
    if cfg.tie_embeddings:
        cfg = dataclasses.replace(cfg, tie_embeddings=False)
        sd["output.weight"] = sd.pop("lm_head")
    ref = mipipe.Generator(cfg, device, dtype=dtype, init=False)
    ref.arena.load_state_dict(sd)
    return ref


@pytest.fixture(scope="module", params=["gpt2", "llama"])
def pair(request):
    cfg = _cfg(request.param)
    q = mipipe.Generator(cfg, CPU, dtype=F32, seed=4, weights="int8")
    return q, dense_oracle(q)


def _tokens(B, S, seed=5):
    return torch.randint(0, 512, (B, S), generator=torch.Generator().manual_seed(seed))


def test_quantised_generator_holds_int8_only(pair):
    q, ref = pair
    A = q.arena
    assert isinstance(A, QuantWeights) and q.model is None and q.weights == "int8" and ref.weights == "bf16"
    for name in A.order:
        block_matrix = name.endswith(QUANTIZED)
        head = name == A.head_name
        assert (name in A.q) == (block_matrix or head)
        if name in A.q:
            assert A.q[name].dtype == torch.int8 and A.scale[name].dtype == F32
            assert A.q[name].shape == A.specs[name].shape and A.scale[name].shape == (A.specs[name].shape[0],)
        # no dense copy of a quantised matrix; a tied head keeps the embedding table
        assert (name in A.dense) == (not block_matrix and (not head or q.cfg.tie_embeddings))
    assert not hasattr(A, "master") and not hasattr(A, "grad") and not hasattr(A, "wt16")
    with pytest.raises(ValueError):
        mipipe.Generator(q.cfg, CPU, dtype=F32, weights="int4")
    with pytest.raises(ValueError):
        mipipe.Generator(q.cfg, CPU, dtype=F32, weights="int8", skinny=True)


def test_logits_match_dense_oracle(pair):
    q, ref = pair
    B, S0 = 2, 16
    tok = _tokens(B, S0 + 6)
    cq, cr = q.new_cache(B, 64), ref.new_cache(B, 64)
    torch.testing.assert_close(q.prefill(tok[:, :S0], cq), ref.prefill(tok[:, :S0], cr))
    for t in range(S0, S0 + 3):                                     # uniform decode
        torch.testing.assert_close(q.decode(tok[:, t], cq), ref.decode(tok[:, t], cr))
    # extend, all logits, then per-row counts (the cache turns ragged)
    ext = _tokens(B, 4, seed=6)
    torch.testing.assert_close(q.extend(ext, cq, all_logits=True), ref.extend(ext, cr, all_logits=True))
    torch.testing.assert_close(q.extend(ext, cq, counts=[3, 1]), ref.extend(ext, cr, counts=[3, 1]))
    assert cq.ragged and torch.equal(cq.lens, cr.lens)
    out_q, out_r = torch.empty(B, q.cfg.vocab_padded), torch.empty(B, q.cfg.vocab_padded)
    active = torch.tensor([1, 0], dtype=torch.uint8)
    for t in range(3):                                              # ragged decode with active / out
        a = q.decode(tok[:, S0 + 3 + t], cq, active=active if t == 2 else None, out=out_q)
        b = ref.decode(tok[:, S0 + 3 + t], cr, active=active if t == 2 else None, out=out_r)
        assert a is out_q and b is out_r
        torch.testing.assert_close(a[:1] if t == 2 else a, b[:1] if t == 2 else b)
    assert torch.equal(cq.lens, cr.lens)


def test_ragged_prefill_and_generate_batch(pair):
    q, ref = pair
    tok = _tokens(3, 9, seed=7)
    lens = [9, 4, 1]
    cq, cr = q.new_cache(3, 32), ref.new_cache(3, 32)
    torch.testing.assert_close(q.prefill(tok, cq, lens), ref.prefill(tok, cr, lens))
    nxt = _tokens(3, 1, seed=8)[:, 0]
    torch.testing.assert_close(q.decode(nxt, cq), ref.decode(nxt, cr))
    prompts = [tok[b, : lens[b]] for b in range(3)]
    oq, lq = q.generate_batch(prompts, 12)
    orf, lr = ref.generate_batch(prompts, 12)
    assert torch.equal(oq, orf) and torch.equal(lq, lr)
    oq, _ = q.generate_batch(prompts, 12, temperature=0.9, top_k=50, top_p=0.9, seed=3, stop_token=7)
    orf, _ = ref.generate_batch(prompts, 12, temperature=0.9, top_k=50, top_p=0.9, seed=3, stop_token=7)
    assert torch.equal(oq, orf)
    assert torch.equal(q.generate(tok[:, :5], 6), ref.generate(tok[:, :5], 6))


def test_speculative_with_quantised_draft_returns_the_targets_tokens():
    """the int8 generator of the same weights drafts for its own dense target (and the other
    way round): the tokens are the target's greedy continuation either way"""
    cfg = _cfg("gpt2")
    target = mipipe.Generator(cfg, CPU, dtype=F32, seed=11)
    draft = mipipe.Generator.from_model(target.model, weights="int8")
    prompts = [_tokens(1, n, seed=20 + n)[0] for n in (1, 6, 3)]
    want, wl = target.generate_batch(prompts, 16)
    # token equality across code paths only means something away from near-ties
    cache = target.new_cache(3, 64)
    lg = target.extend(want, cache, all_logits=True)[..., : cfg.vocab_size]
    top2 = lg.topk(2, -1).values
    gap = (top2[..., 0] - top2[..., 1])
    emitted = torch.arange(want.shape[1])[None, :] >= (torch.tensor([1, 6, 3])[:, None] - 1)
    emitted &= torch.arange(want.shape[1])[None, :] < (wl[:, None] - 1)
    assert float(gap[emitted].min()) > 1e-4, "a near-tie: pick another seed"
    out, lens, stats = target.generate_speculative(prompts, 16, draft, lookahead=4)
    assert torch.equal(out, want) and torch.equal(lens, wl)
    assert stats["drafted"] > 0 and stats["accepted"] > 0          # the int8 draft does agree with its target
    want_q, wl_q = draft.generate_batch(prompts, 16)
    out, lens, _ = draft.generate_speculative(prompts, 16, target, lookahead=3)
    assert torch.equal(out, want_q) and torch.equal(lens, wl_q)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_from_model_leaves_the_model_untouched(family):
    cfg = _cfg(family)
    base = mipipe.Generator(cfg, CPU, dtype=F32, seed=2)
    A = base.arena
    before = {k: getattr(A, k).clone() for k in ("master", "grad", "w16", "wt16")}
    q = mipipe.Generator.from_model(base.model, weights="int8")
    for k, v in before.items():
        assert torch.equal(getattr(A, k), v), k
    assert q.arena is not A and q.model is None and base.model.arena is A
    # the same quantised values as a generator built with the same seed
    q2 = mipipe.Generator(cfg, CPU, dtype=F32, seed=2, weights="int8")
    for n in q.arena.q:
        assert torch.equal(q.arena.q[n], q2.arena.q[n]) and torch.equal(q.arena.scale[n], q2.arena.scale[n])
    # a snapshot: a later change of the model is not seen
    tok = _tokens(1, 4)
    lg = q.prefill(tok, q.new_cache(1, 8)).clone()
    A.master.mul_(0.5)
    A.sync_w16()
    assert torch.equal(q.prefill(tok, q.new_cache(1, 8)), lg)


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    cfg = NativeConfig.gpt2("tiny", vocab_size=64, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32)
    tr = PipelineTrainer(cfg, pp=1, schedule="1F1B", n_microbatches=2, mbs=2, seq_len=32, device=CPU, dtype=F32,
                         lr=1e-3, seed=0, graphs=False)
    path = str(tmp_path_factory.mktemp("ckpt_w8") / "pp1")
    save_checkpoint(tr, path)
    return tr, path


def test_load_int8_equals_from_model(saved):
    tr, path = saved
    a = mipipe.Generator.load(path, device="cpu", weights="int8")
    b = mipipe.Generator.from_model(tr.stages[0].model, weights="int8")
    assert a.weights == "int8" and a.dtype == F32
    for n in b.arena.q:
        assert torch.equal(a.arena.q[n], b.arena.q[n]) and torch.equal(a.arena.scale[n], b.arena.scale[n])
    for n in b.arena.dense:
        assert torch.equal(a.arena.dense[n], b.arena.dense[n])


def test_cli_weights_int8(saved):
    tr, path = saved
    prompt = _tokens(2, 5, seed=9) % 64
    want = mipipe.Generator.from_model(tr.stages[0].model, weights="int8").generate(prompt, 8)
    arg = ";".join(",".join(str(t) for t in row) for row in prompt.tolist())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint", path, "--prompt", arg,
                        "--max-new-tokens", "8", "--device", "cpu", "--weights", "int8"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = [[int(t) for t in line.split(",")] for line in r.stdout.strip().splitlines()]
    assert got == want.tolist()
