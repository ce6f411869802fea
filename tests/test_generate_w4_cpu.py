"""int4g128 weight-only generation on the CPU (f32 reference paths of the ops).

A ``weights="int4g128"`` generator computes with ``What[n, k] = q[n, k] * scale[k // 128, n]``.
Its oracle, as in test_generate_w8_cpu.py, is a dense CPU generator loaded with exactly those
values (``QuantWeights.effective_state_dict``; with tied embeddings the tie is cut and
``output.weight`` is the head's ``What``).  The two run the same f32 arithmetic up to
``sum_g scale_g (x_g q_g^T)`` against ``x What^T``: logits agree at
``torch.testing.assert_close``'s f32 defaults, the tolerance of the int8 file's equivalent test.
The models are a tiny GPT-2 and a tiny Llama-3 with d = 128 and 2 layers, so every quantised
matrix has K % 128 == 0."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.engine import PipelineTrainer
from mipipe.models.config import NativeConfig
from mipipe.models.generate import QUANTIZED, QuantWeights
from mipipe.utils.checkpoint import save_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
F32 = torch.float32
W4 = "int4g128"


def _cfg(family):
    if family == "gpt2":
        return NativeConfig.gpt2("tiny", vocab_size=512, d_model=128, n_layers=2, n_heads=2, d_ff=512, max_seq_len=128)
    # head_dim 64 (what the GPU attention kernels take), rep 2
    return NativeConfig.llama3("tiny", vocab_size=512, d_model=128, n_layers=2, n_heads=2, n_kv_heads=1, d_ff=256,
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
    q = mipipe.Generator(_cfg(request.param), CPU, dtype=F32, seed=4, weights=W4)
    return q, dense_oracle(q)


def _tokens(B, S, seed=5):
    return torch.randint(0, 512, (B, S), generator=torch.Generator().manual_seed(seed))


def test_quantised_generator_holds_packed_4bit_only(pair):
    q, ref = pair
    A = q.arena
    assert isinstance(A, QuantWeights) and A.fmt == W4 and q.model is None and q.weights == W4 and ref.weights == "bf16"
    for name in A.order:
        block_matrix = name.endswith(QUANTIZED)
        head = name == A.head_name
        assert (name in A.q) == (block_matrix or head)
        if name in A.q:
            N, K = A.specs[name].shape
            assert A.q[name].dtype == torch.uint8 and A.q[name].shape == (N, K // 2)
            assert A.scale[name].dtype == F32 and A.scale[name].shape == (K // 128, N)
        # no dense copy of a quantised matrix; a tied head keeps the embedding table
        assert (name in A.dense) == (not block_matrix and (not head or q.cfg.tie_embeddings))
    assert not hasattr(A, "master") and not hasattr(A, "grad") and not hasattr(A, "wt16")
    # the scratch of the dequantising route holds N * K bf16 values, not the packed count
    assert A.max_matrix_numel() == max(A.specs[n].shape[0] * A.specs[n].shape[1] for n in A.q)
    assert A.max_matrix_numel() == 2 * max(t.numel() for t in A.q.values())
    # the effective weights are q * scale per group
    sd = A.effective_state_dict()
    n = "layers.0.attn.wqkv.weight"
    assert torch.equal(sd[n], ops.dequant_w4(A.q[n], A.scale[n]))
    with pytest.raises(ValueError):
        mipipe.Generator(q.cfg, CPU, dtype=F32, weights="int4")
    with pytest.raises(ValueError):
        mipipe.Generator(q.cfg, CPU, dtype=F32, weights=W4, skinny=True)
    with pytest.raises(ValueError):
        QuantWeights(q.cfg, CPU, F32, "int4")


def test_k_not_a_multiple_of_128_is_refused():
    cfg = NativeConfig.gpt2("tiny", vocab_size=512, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32)
    with pytest.raises(ValueError, match="128"):
        mipipe.Generator(cfg, CPU, dtype=F32, weights=W4)
    mipipe.Generator(cfg, CPU, dtype=F32, weights="int8")                # int8 takes it


def test_logits_match_dense_oracle(pair):
    q, ref = pair
    B, S0 = 2, 16
    tok = _tokens(B, S0 + 6)
    cq, cr = q.new_cache(B, 64), ref.new_cache(B, 64)
    torch.testing.assert_close(q.prefill(tok[:, :S0], cq), ref.prefill(tok[:, :S0], cr))
    for t in range(S0, S0 + 3):                                     # uniform decode
        torch.testing.assert_close(q.decode(tok[:, t], cq), ref.decode(tok[:, t], cr))
    ext = _tokens(B, 4, seed=6)
    torch.testing.assert_close(q.extend(ext, cq, all_logits=True), ref.extend(ext, cr, all_logits=True))
    torch.testing.assert_close(q.extend(ext, cq, counts=[3, 1]), ref.extend(ext, cr, counts=[3, 1]))
    assert cq.ragged and torch.equal(cq.lens, cr.lens)
    for t in range(2):                                              # ragged decode
        torch.testing.assert_close(q.decode(tok[:, S0 + 3 + t], cq), ref.decode(tok[:, S0 + 3 + t], cr))


def test_generate_batch_matches_dense_oracle(pair):
    q, ref = pair
    tok = _tokens(3, 9, seed=7)
    lens = [9, 4, 1]
    prompts = [tok[b, : lens[b]] for b in range(3)]
    oq, lq = q.generate_batch(prompts, 12)
    orf, lr = ref.generate_batch(prompts, 12)
    assert torch.equal(oq, orf) and torch.equal(lq, lr)
    assert torch.equal(q.generate(tok[:, :5], 6), ref.generate(tok[:, :5], 6))


def test_speculative_with_int4_draft_returns_the_targets_tokens():
    cfg = _cfg("gpt2")
    target = mipipe.Generator(cfg, CPU, dtype=F32, seed=11)
    draft = mipipe.Generator.from_model(target.model, weights=W4)
    prompts = [_tokens(1, n, seed=20 + n)[0] for n in (1, 6, 3)]
    want, wl = target.generate_batch(prompts, 16)
    out, lens, stats = target.generate_speculative(prompts, 16, draft, lookahead=4)
    assert torch.equal(out, want) and torch.equal(lens, wl)
    assert stats["drafted"] > 0
    # ... and drafting for an int8 target
    t8 = mipipe.Generator.from_model(target.model, weights="int8")
    want8, wl8 = t8.generate_batch(prompts, 16)
    out, lens, _ = t8.generate_speculative(prompts, 16, draft, lookahead=3)
    assert torch.equal(out, want8) and torch.equal(lens, wl8)


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    cfg = NativeConfig.gpt2("tiny", vocab_size=128, d_model=128, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32)
    tr = PipelineTrainer(cfg, pp=1, schedule="1F1B", n_microbatches=2, mbs=2, seq_len=32, device=CPU, dtype=F32,
                         lr=1e-3, seed=0, graphs=False)
    path = str(tmp_path_factory.mktemp("ckpt_w4") / "pp1")
    save_checkpoint(tr, path)
    return tr, path


def test_load_from_model_and_seed_give_the_same_values(saved):
    tr, path = saved
    a = mipipe.Generator.load(path, device="cpu", weights=W4)
    b = mipipe.Generator.from_model(tr.stages[0].model, weights=W4)
    assert a.weights == W4 and a.dtype == F32 and b.weights == W4
    assert set(a.arena.q) == set(b.arena.q) and len(a.arena.q) > 0
    for n in b.arena.q:
        assert a.arena.q[n].dtype == torch.uint8
        assert torch.equal(a.arena.q[n], b.arena.q[n]) and torch.equal(a.arena.scale[n], b.arena.scale[n])
    for n in b.arena.dense:
        assert torch.equal(a.arena.dense[n], b.arena.dense[n])
    # the random-init constructor against from_model of a dense generator with the same seed
    for family in ("gpt2", "llama"):
        cfg = _cfg(family)
        base = mipipe.Generator(cfg, CPU, dtype=F32, seed=2)
        before = base.arena.master.clone()
        q1 = mipipe.Generator.from_model(base.model, weights=W4)
        q2 = mipipe.Generator(cfg, CPU, dtype=F32, seed=2, weights=W4)
        assert torch.equal(base.arena.master, before)
        for n in q1.arena.q:
            assert torch.equal(q1.arena.q[n], q2.arena.q[n]) and torch.equal(q1.arena.scale[n], q2.arena.scale[n])


def test_cli_weights_int4g128(saved):
    tr, path = saved
    prompt = _tokens(2, 5, seed=9) % 128
    want = mipipe.Generator.from_model(tr.stages[0].model, weights=W4).generate(prompt, 8)
    arg = ";".join(",".join(str(t) for t in row) for row in prompt.tolist())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint", path, "--prompt", arg,
                        "--max-new-tokens", "8", "--device", "cpu", "--weights", W4], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = [[int(t) for t in line.split(",")] for line in r.stdout.strip().splitlines()]
    assert got == want.tolist()
