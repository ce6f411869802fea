"""Generation with an int8 KV cache (``kv_cache="int8"``) on the CPU: the f32 reference paths of
the ops over int8 rows, through every Generator method.

Exact checks use layer 0, whose K / V rows do not depend on the cache: they must be
``kv_quantize`` of the float-cache generator's rows, byte for byte.  Later layers see attention
outputs that differ by the quantisation error, so logits are compared only for finiteness and
their error is printed (profiles/r14_kv8_decode.md records it).  Tiny GPT-2 and Llama configs,
2 layers, head_dim 64."""
import os
import subprocess
import sys

import pytest
import torch

import mipipe
from mipipe import ops
from mipipe.engine import PipelineTrainer
from mipipe.models.config import NativeConfig
from mipipe.models.generate import KVCache
from mipipe.utils.checkpoint import save_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
F32 = torch.float32
G = ops.generate


def _cfg(family):
    if family == "gpt2":
        return NativeConfig.gpt2("tiny", vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024,
                                 max_seq_len=128)
    return NativeConfig.llama3("tiny", vocab_size=512, d_model=512, n_layers=2, n_heads=8, n_kv_heads=2, d_ff=1024,
                               max_seq_len=128)


@pytest.fixture(scope="module", params=["gpt2", "llama"])
def pair(request):
    """(int8-cache generator, float-cache generator) over the same weights"""
    cfg = _cfg(request.param)
    assert cfg.head_dim == 64
    ref = mipipe.Generator(cfg, CPU, dtype=F32, seed=4)
    gen = mipipe.Generator.from_model(ref.model, kv_cache="int8")
    return gen, ref


def _tokens(B, S, seed=5):
    return torch.randint(0, 512, (B, S), generator=torch.Generator().manual_seed(seed))


def _layer0_equal(gen, c8, cf):
    """layer 0's valid int8 rows are kv_quantize of the float cache's rows"""
    KV, Dh = gen.cfg.n_kv_heads, gen.cfg.head_dim
    for b, n in enumerate(cf.lens.tolist()):
        assert torch.equal(c8.k[0][b, :n], G.kv_quantize(cf.k[0][b, :n], KV, Dh)), "K rows of layer 0"
        assert torch.equal(c8.v[0][b, :n], G.kv_quantize(cf.v[0][b, :n], KV, Dh)), "V rows of layer 0"


def test_cache_allocation_and_choice(pair):
    gen, ref = pair
    cfg = gen.cfg
    L, KV, Dh = cfg.n_layers, cfg.n_kv_heads, cfg.head_dim
    W = G.kv8_row_bytes(KV, Dh)
    assert gen.kv_cache == "int8" and ref.kv_cache == "bf16" and gen.arena is ref.arena
    c8, cf = gen.new_cache(3, 40), ref.new_cache(3, 40)
    assert c8.kv == "int8" and cf.kv == "bf16"
    assert all(t.dtype == torch.int8 and t.shape == (3, 40, W) for t in c8.k + c8.v)
    assert c8.nbytes == 2 * L * 3 * 40 * W
    assert cf.nbytes == 2 * L * 3 * 40 * KV * Dh * 4                 # f32 rows on the CPU
    assert gen.new_cache(1, 8, kv="bf16").kv == "bf16" and ref.new_cache(1, 8, kv="int8").kv == "int8"
    assert KVCache(cfg, 1, 8, CPU, F32).kv == "bf16"
    for bad in ("int4", "fp8", ""):
        with pytest.raises(ValueError):
            mipipe.Generator(cfg, CPU, dtype=F32, kv_cache=bad)
        with pytest.raises(ValueError):
            KVCache(cfg, 1, 8, CPU, F32, kv=bad)
        with pytest.raises(ValueError):
            gen.new_cache(1, 8, kv=bad)
        with pytest.raises(ValueError):
            mipipe.Generator.from_model(ref.model, kv_cache=bad)
    # independent of weights= and skinny=
    q = mipipe.Generator(cfg, CPU, dtype=F32, seed=4, weights="int8", kv_cache="int8")
    assert q.weights == "int8" and q.new_cache(1, 8).kv == "int8"
    assert torch.isfinite(q.prefill(_tokens(1, 4), q.new_cache(1, 8))).all()


def test_every_mode_writes_quantised_rows(pair):
    gen, ref = pair
    B, S0 = 2, 16
    tok = _tokens(B, S0 + 8)
    c8, cf = gen.new_cache(B, 64), ref.new_cache(B, 64)
    errs = {}

    def both(name, f):
        a, b = f(gen, c8), f(ref, cf)
        assert a.shape == b.shape and bool(torch.isfinite(a).all())
        errs[name] = max(errs.get(name, 0.0), float((a - b).abs().max()))
        assert torch.equal(c8.lens, cf.lens) and c8.pos == cf.pos and c8.ragged == cf.ragged
        _layer0_equal(gen, c8, cf)
        return a, b

    a, b = both("prefill", lambda g, c: g.prefill(tok[:, :S0], c))
    assert torch.equal(a, b), "a prefill attends to its own exact K / V: the logits do not see the cache format"
    for t in range(S0, S0 + 3):                                     # uniform decode
        both("decode", lambda g, c: g.decode(tok[:, t], c))
    ext = _tokens(B, 4, seed=6)
    both("extend", lambda g, c: g.extend(ext, c, all_logits=True))
    both("extend_counts", lambda g, c: g.extend(ext, c, counts=[3, 1]))
    assert c8.ragged
    active = torch.tensor([1, 0], dtype=torch.uint8)
    rows8 = c8.k[0].clone()
    for t in range(3):                                              # ragged decode, the last with a mask
        both("decode_ragged", lambda g, c: g.decode(tok[:, S0 + 3 + t], c, active=active if t == 2 else None)[:1])
    n1 = int(c8.lens[1])
    assert torch.equal(c8.k[0][1, n1:], rows8[1, n1:]), "an inactive row's cache was touched"
    scale = float(ref.prefill(tok[:, :S0], ref.new_cache(B, 64)).abs().max())
    print("\n[%s] max |logit(int8 cache) - logit(float cache)| on the CPU, logits up to %.3f: %s"
          % (gen.cfg.name, scale, ", ".join(f"{k} {v:.2e}" for k, v in errs.items())))
    # truncate + reset leave the format alone
    c8.truncate([5, 3])
    assert c8.lens.tolist() == [5, 3] and c8.kv == "int8"
    c8.reset()
    assert c8.pos == 0 and not c8.ragged and c8.k[0].dtype == torch.int8


def test_extend_from_an_empty_cache_attends_to_quantised_rows(pair):
    """the documented difference: prefill attends to exact K / V, extend to the stored rows"""
    gen, ref = pair
    tok = _tokens(2, 12, seed=8)
    c_pre, c_ext = gen.new_cache(2, 32), gen.new_cache(2, 32)
    lp, le = gen.prefill(tok, c_pre), gen.extend(tok, c_ext)
    assert torch.equal(c_pre.k[0][:, :12], c_ext.k[0][:, :12]) and torch.equal(c_pre.v[0][:, :12], c_ext.v[0][:, :12])
    assert not torch.equal(lp, le) and bool(torch.isfinite(le).all())
    # on a float cache the two agree to rounding
    lpf, lef = ref.prefill(tok, ref.new_cache(2, 32)), ref.extend(tok, ref.new_cache(2, 32))
    torch.testing.assert_close(lpf, lef, atol=1e-4, rtol=1e-4)


def test_truncate_then_extend_reproduces_a_fresh_cache(pair):
    gen, _ = pair
    tok = _tokens(2, 14, seed=9)
    a = gen.new_cache(2, 32)
    gen.extend(tok[:, :6], a)
    gen.extend(tok[:, 6:12], a)                  # rows that the truncation drops
    a.truncate([6, 6])
    la = gen.extend(tok[:, 10:14], a)
    b = gen.new_cache(2, 32)
    gen.extend(tok[:, :6], b)
    lb = gen.extend(tok[:, 10:14], b)
    assert torch.equal(la, lb)
    assert torch.equal(a.k[1][:, :10], b.k[1][:, :10]) and torch.equal(a.v[1][:, :10], b.v[1][:, :10])


def test_generate_methods_run_and_speculative_returns_the_targets_tokens(pair):
    gen, ref = pair
    cfg = gen.cfg
    prompts = [_tokens(1, n, seed=20 + n)[0] for n in (1, 6, 3)]
    want, wl = gen.generate_batch(prompts, 12)
    assert want.shape == (3, 18) and wl.tolist() == [13, 18, 15]
    # token equality across code paths only means something away from near-ties
    cache = gen.new_cache(3, 64)
    lg = gen.extend(want, cache, all_logits=True)[..., : cfg.vocab_size]
    top2 = lg.topk(2, -1).values
    emitted = torch.arange(want.shape[1])[None, :] >= (torch.tensor([1, 6, 3])[:, None] - 1)
    emitted &= torch.arange(want.shape[1])[None, :] < (wl[:, None] - 1)
    assert float((top2[..., 0] - top2[..., 1])[emitted].min()) > 1e-4, "a near-tie: pick another seed"
    # an int8-cache target with a float-cache draft, an int8-cache draft, and both
    draft8 = mipipe.Generator.from_model(ref.model, kv_cache="int8")
    for draft in (ref, draft8):
        out, lens, stats = gen.generate_speculative(prompts, 12, draft, lookahead=3)
        assert torch.equal(out, want) and torch.equal(lens, wl)
        assert stats["drafted"] > 0 and stats["accepted"] > 0
    # a float-cache target with an int8-cache draft returns the float target's tokens
    want_f, wl_f = ref.generate_batch(prompts, 12)
    out, lens, _ = ref.generate_speculative(prompts, 12, draft8, lookahead=4)
    assert torch.equal(out, want_f) and torch.equal(lens, wl_f)
    # sampling, a stop token, generate()
    o1, l1 = gen.generate_batch(prompts, 10, temperature=0.9, top_k=50, top_p=0.9, seed=3, stop_token=7)
    o2, l2 = gen.generate_batch(prompts, 10, temperature=0.9, top_k=50, top_p=0.9, seed=3, stop_token=7)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    tok = _tokens(2, 5, seed=7)
    out = gen.generate(tok, 6)
    assert out.shape == (2, 11) and torch.equal(out[:, :5], tok)
    assert torch.equal(out, gen.generate(tok, 6))


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    cfg = NativeConfig.gpt2("tiny", vocab_size=64, d_model=128, n_layers=2, n_heads=2, d_ff=256, max_seq_len=32)
    tr = PipelineTrainer(cfg, pp=1, schedule="1F1B", n_microbatches=2, mbs=2, seq_len=32, device=CPU, dtype=F32,
                         lr=1e-3, seed=0, graphs=False)
    path = str(tmp_path_factory.mktemp("ckpt_kv8") / "pp1")
    save_checkpoint(tr, path)
    return tr, path


def test_load_and_cli_kv_cache_int8(saved):
    tr, path = saved
    a = mipipe.Generator.load(path, device="cpu", kv_cache="int8")
    assert a.kv_cache == "int8" and a.weights == "bf16" and a.new_cache(1, 8).kv == "int8"
    b = mipipe.Generator.load(path, device="cpu", weights="int8", kv_cache="int8")
    assert b.kv_cache == "int8" and b.weights == "int8"
    prompt = _tokens(2, 5, seed=9) % 64
    want = mipipe.Generator.from_model(tr.stages[0].model, kv_cache="int8").generate(prompt, 8)
    arg = ";".join(",".join(str(t) for t in row) for row in prompt.tolist())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint", path, "--prompt", arg,
                        "--max-new-tokens", "8", "--device", "cpu", "--kv-cache", "int8"], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = [[int(t) for t in line.split(",")] for line in r.stdout.strip().splitlines()]
    assert got == want.tolist()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--checkpoint", path, "--prompt", arg,
                        "--kv-cache", "int4"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--kv-cache" in r.stderr
