"""``weights="mxfp4"`` generation on the GPU, on the tiny models of test_generate_w4_cpu.py: a prefill
of 16 tokens (B = 2, 32 rows: dequant_mx4 + the GEMM) and 8 teacher-forced decode steps (2 rows:
gemv_mx4_kernel).  The GPU logits are held against the CPU f32 mxfp4 generator with the same bytes; the
bound is 2 x the error of the bf16 GPU generator on the same effective weights against its CPU f32 twin,
measured here from that existing path.  ``generate_batch(graphs=True)`` returns the eager tokens."""
import math

import pytest
import torch

import mipipe
from mipipe import ops

from test_generate_w4_cpu import _cfg, dense_oracle
from test_generate_w4_gpu import _incremental

pytestmark = pytest.mark.gpu


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_mxfp4_within_twice_the_bf16_error_and_graphs_equal_eager(family):
    cfg = _cfg(family)
    dev = torch.device("cuda", 0)
    q = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=4, weights="mxfp4")
    A = q.arena
    head = A.q[A.head_name]
    assert head.dtype == torch.uint8 and head.is_cuda and A.scale[A.head_name].shape == (cfg.vocab_padded, cfg.d_model // 32)
    twin = mipipe.Generator(cfg, "cpu", dtype=torch.float32, init=False, weights="mxfp4")       # the same bytes on the CPU
    twin.arena.q = {n: t.cpu() for n, t in A.q.items()}
    twin.arena.scale = {n: t.cpu() for n, t in A.scale.items()}
    twin.arena.dense = {n: t.float().cpu() for n, t in A.dense.items()}
    B, S0, steps = 2, 16, 8
    tokens = torch.randint(0, cfg.vocab_size, (B, S0 + steps), generator=torch.Generator().manual_seed(5))
    e_q = float((_incremental(q, tokens, S0) - _incremental(twin, tokens, S0)).abs().max())
    # the yardstick: the bf16 kernels on bf16(What) (exactly What) against their CPU f32 twin
    e_b = float((_incremental(dense_oracle(q, dev, torch.bfloat16), tokens, S0)
                 - _incremental(dense_oracle(q), tokens, S0)).abs().max())
    print(f"\n[{family}] e_bf16 = {e_b:.6f}  e_mxfp4 = {e_q:.6f}  bound = {2 * e_b:.6f}")
    assert math.isfinite(e_q) and e_b > 0
    assert e_q <= 2 * e_b, (e_q, e_b)

    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g) for n in (3, 17, 9)]
    eager, le = q.generate_batch(prompts, 24, graphs=False)
    replay, lr = q.generate_batch(prompts, 24, graphs=True)
    assert torch.equal(eager, replay) and torch.equal(le, lr)
