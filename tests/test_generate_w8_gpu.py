"""int8 weight-only generation on the GPU.

* The recipe of test_generate_gpu.test_incremental_matches_cpu_within_twice_full_forward_error:
  prefill on 16 tokens, then 48 teacher-forced decode steps, B = 2, both families.  The oracle
  is the CPU f32 generator holding ``What = q * scale``.  ``e_b`` is the error of today's bf16
  GPU generator loaded with ``bf16(What)``; the int8 generator must satisfy ``e_q <= 2 e_b``
  (that test's margin for "a second, different set of bf16 kernels"), and so must the bf16
  generator with ``skinny=True``.  All three figures are printed.
* ``generate_batch`` on three ragged prompts: graph replay gives the eager tokens.
* Memory of ``Generator.load(path, weights="int8")``: at most the int8 matrices, their f32
  scales, two bytes for every other parameter, and 1 MiB -- a condition derived from the
  format, not a measurement (taken in a fresh process: see the test)."""
import math

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.engine import PipelineTrainer
from mipipe.utils.checkpoint import save_checkpoint

from test_generate_w8_cpu import _cfg, dense_oracle

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
def test_int8_and_skinny_within_twice_the_bf16_error(family):
    cfg = _cfg(family)
    dev = torch.device("cuda", 0)
    q = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4, weights="int8")
    assert q.arena.q[q.arena.head_name].dtype == torch.int8 and q.arena.q[q.arena.head_name].is_cuda
    oracle = dense_oracle(q)                                   # CPU f32, holds What
    base = dense_oracle(q, dev, torch.bfloat16)                # today's bf16 path on bf16(What)
    skinny = mipipe.Generator.from_model(base.model, skinny=True)
    assert base.weights == "bf16" and not base.skinny and skinny.skinny and skinny.arena is base.arena
    B, S0, steps = 2, 16, 48
    tokens = torch.randint(0, cfg.vocab_size, (B, S0 + steps), generator=torch.Generator().manual_seed(5))
    want = _incremental(oracle, tokens, S0)
    e_b = float((_incremental(base, tokens, S0) - want).abs().max())
    e_q = float((_incremental(q, tokens, S0) - want).abs().max())
    e_s = float((_incremental(skinny, tokens, S0) - want).abs().max())
    print(f"\n[{family}] e_bf16 = {e_b:.6f}  e_int8 = {e_q:.6f}  e_bf16_skinny = {e_s:.6f}  bound = {2 * e_b:.6f}")
    assert math.isfinite(e_q) and math.isfinite(e_s) and e_b > 0
    assert e_q <= 2 * e_b, (e_q, e_b)
    assert e_s <= 2 * e_b, (e_s, e_b)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_generate_batch_graphs_equal_eager_on_int8(family):
    cfg = _cfg(family)
    q = mipipe.Generator(cfg, torch.device("cuda", 0), dtype=torch.bfloat16, seed=4, weights="int8")
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (3, 17, 9)]
    eager, le = q.generate_batch(prompts, 24, graphs=False)
    replay, lr = q.generate_batch(prompts, 24, graphs=True)
    assert torch.equal(eager, replay) and torch.equal(le, lr)
    # the decode step and a verifying extend of the same rows run bit-identical linear layers:
    # B (lookahead + 1) <= 16 rows all go through the skinny kernel, whose rows are independent
    x = torch.randn(15, cfg.d_model, device="cuda", dtype=torch.bfloat16)
    name = "layers.0.attn.wqkv.weight"
    many = q._linear(x, name)
    for m in (0, 7, 14):
        assert torch.equal(q._linear(x[m: m + 1], name), many[m: m + 1])


_LOAD_PROBE = """
import json, math, sys, torch
sys.path.insert(0, sys.argv[1])
import mipipe
dev = torch.device("cuda", 0)
torch.cuda.init()
torch.cuda.synchronize()
before = torch.cuda.memory_allocated(dev)
gen = mipipe.Generator.load(sys.argv[2], device=dev, weights="int8")
torch.cuda.synchronize()
used = torch.cuda.memory_allocated(dev) - before
A = gen.arena
out = gen.generate(torch.randint(0, gen.cfg.vocab_size, (1, 4)), 4)
print(json.dumps({"used": used, "quant": sum(q.numel() for q in A.q.values()),
                  "scales": 4 * sum(q.shape[0] for q in A.q.values()),
                  "other": 2 * sum(math.prod(A.specs[n].shape) for n in A.order if n not in A.q),
                  "generated": list(out.shape)}))
"""


def test_int8_load_memory(tmp_path):
    """``memory_allocated`` counts whole allocator blocks, and a block cached by an earlier
    test is handed out unsplit when it is up to 1 MiB larger than the request: what a load
    allocates is therefore measured in a fresh process, which is what a user's is."""
    import json
    import os
    import subprocess
    import sys
    cfg = _cfg("llama")
    tr = PipelineTrainer(cfg, pp=1, schedule="1F1B", n_microbatches=1, mbs=1, seq_len=32, device=torch.device("cpu"),
                         dtype=torch.float32, lr=1e-3, seed=0, graphs=False)
    path = str(tmp_path / "ckpt")
    save_checkpoint(tr, path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _LOAD_PROBE, root, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout.strip().splitlines()[-1])
    bound = m["quant"] + m["scales"] + m["other"] + (1 << 20)
    print(f"\nint8 load: {m['used']} bytes allocated, bound {bound} (int8 {m['quant']}, scales {m['scales']}, "
          f"other {m['other']})")
    assert m["quant"] == 2 * (1536 * 1024 + 1024 * 1024 + 4096 * 1024 + 1024 * 2048) + 512 * 1024
    assert 0 < m["used"] <= bound, (m["used"], bound)
    assert m["generated"] == [1, 8]
