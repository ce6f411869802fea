"""Generator.extend and KVCache.truncate on the CPU (f32 reference paths of the ops), on the
tiny gpt2 / llama configurations of test_generate_cpu.py at that file's tolerance: a chunked
extend computes what prefill computes, per-position logits are the full forward's, rows of a
ragged extend match the same sequence run alone, a row with nothing to append keeps its
cache bit for bit, and truncate + extend equals never having appended the dropped tokens."""
import pytest
import torch

import mipipe
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext

CPU = torch.device("cpu")
TOL = dict(atol=1e-4, rtol=1e-4)


def _cfg(family):
    if family == "gpt2":
        return NativeConfig.gpt2("tiny", vocab_size=64, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32)
    return NativeConfig.llama3("tiny", vocab_size=64, d_model=64, n_layers=2, n_heads=4, n_kv_heads=2, d_ff=128,
                               max_seq_len=32)


def _gen(family):
    return mipipe.Generator(_cfg(family), CPU, dtype=torch.float32, seed=3)


def _full_logits(gen, tokens):
    B, S = tokens.shape
    return gen.model.forward(tokens, MBContext(0, 0), B, S, target=None).view(B, S, -1)


def _tokens(B, S, seed=1):
    return torch.randint(0, 64, (B, S), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_chunked_extend_equals_prefill(family):
    gen = _gen(family)
    B = 3
    tokens = _tokens(B, 13)
    ref_cache = gen.new_cache(B, 16)
    want = gen.prefill(tokens[:, :12], ref_cache)
    cache = gen.new_cache(B, 16)
    gen.extend(tokens[:, :5], cache)
    assert cache.pos == 5 and cache.lens.tolist() == [5] * B and not cache.ragged
    got = gen.extend(tokens[:, 5:12], cache)
    assert cache.pos == 12 and cache.lens.tolist() == [12] * B and not cache.ragged
    torch.testing.assert_close(got, want, **TOL)
    for li in range(gen.cfg.n_layers):
        torch.testing.assert_close(cache.k[li][:, :12], ref_cache.k[li][:, :12], **TOL)
        torch.testing.assert_close(cache.v[li][:, :12], ref_cache.v[li][:, :12], **TOL)
    torch.testing.assert_close(gen.decode(tokens[:, 12], cache), gen.decode(tokens[:, 12], ref_cache), **TOL)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_all_logits_are_the_full_forward(family):
    gen = _gen(family)
    B = 2
    tokens = _tokens(B, 12, seed=2)
    full = _full_logits(gen, tokens)
    cache = gen.new_cache(B, 12)
    a = gen.extend(tokens[:, :4], cache, all_logits=True)
    b = gen.extend(tokens[:, 4:], cache, all_logits=True)
    assert a.shape == (B, 4, gen.cfg.vocab_padded) and b.shape == (B, 8, gen.cfg.vocab_padded)
    torch.testing.assert_close(torch.cat([a, b], 1), full, **TOL)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_ragged_counts_match_each_sequence_alone(family):
    gen = _gen(family)
    lens, counts, T = [4, 9, 2], [3, 0, 5], 5
    B = len(lens)
    tokens = _tokens(B, 20, seed=4)
    cache = gen.new_cache(B, 20)
    gen.prefill(tokens[:, :9], cache, lens=lens)
    before_k = [k.clone() for k in cache.k]
    before_v = [v.clone() for v in cache.v]
    new = torch.stack([tokens[b, n:n + T] for b, n in enumerate(lens)])
    last = gen.extend(new, cache, counts=counts)
    assert cache.ragged and cache.pos == 9 + T and cache.lens.tolist() == [7, 9, 7]
    for li in range(gen.cfg.n_layers):                  # the counts = 0 row: bit for bit
        assert torch.equal(cache.k[li][1], before_k[li][1]) and torch.equal(cache.v[li][1], before_v[li][1])
    assert bool(torch.isfinite(last).all())
    # the per-position variant on a second cache
    cache2 = gen.new_cache(B, 20)
    gen.prefill(tokens[:, :9], cache2, lens=lens)
    every = gen.extend(new, cache2, counts=counts, all_logits=True)
    assert bool(torch.isfinite(every).all())
    for b in (0, 2):
        n, c = lens[b], counts[b]
        alone = _full_logits(gen, tokens[b:b + 1, : n + c])[0]
        torch.testing.assert_close(last[b], alone[-1], **TOL)
        torch.testing.assert_close(every[b, :c], alone[n:], **TOL)
    # the cache goes on: one ragged decode step matches the sequences alone
    nxt = torch.stack([tokens[b, n + c] for b, (n, c) in enumerate(zip(lens, counts))])
    got = gen.decode(nxt, cache)
    for b, (n, c) in enumerate(zip(lens, counts)):
        alone = _full_logits(gen, tokens[b:b + 1, : n + c + 1])[0]
        torch.testing.assert_close(got[b], alone[-1], **TOL)


@pytest.mark.parametrize("family", ["gpt2", "llama"])
def test_truncate_then_extend_is_a_rollback(family):
    gen = _gen(family)
    B = 2
    tokens = _tokens(B, 16, seed=5)
    other = _tokens(B, 6, seed=6)
    cache = gen.new_cache(B, 24)
    gen.prefill(tokens[:, :6], cache)
    gen.extend(other, cache)                             # six tokens that will be dropped in part
    keep = [8, 6]                                        # row 0 keeps two of them, row 1 none
    cache.truncate(keep)
    assert cache.ragged and cache.pos == 8 and cache.lens.tolist() == keep
    rest = torch.stack([tokens[0, 8:12], tokens[1, 6:10]])
    got = gen.extend(rest, cache)
    seq0 = torch.cat([tokens[0, :6], other[0, :2], tokens[0, 8:12]])[None]
    seq1 = tokens[1:2, :10]
    torch.testing.assert_close(got[0], _full_logits(gen, seq0)[0, -1], **TOL)
    torch.testing.assert_close(got[1], _full_logits(gen, seq1)[0, -1], **TOL)
    # a device-side tensor with an explicit host bound
    cache.truncate(torch.tensor([3, 10], dtype=torch.int32), pos=10)
    assert cache.pos == 10 and cache.lens.tolist() == [3, 10]
    with pytest.raises(ValueError):
        cache.truncate([11, 0])                          # above the bound
    with pytest.raises(ValueError):
        cache.truncate([1, 2, 3])


def test_extend_argument_errors():
    gen = _gen("gpt2")
    cache = gen.new_cache(2, 8)
    tokens = _tokens(2, 9)
    with pytest.raises(ValueError, match="exceed"):
        gen.extend(tokens, cache)                        # 9 tokens, 8 rows
    gen.extend(tokens[:, :6], cache)
    with pytest.raises(ValueError, match="exceed"):
        gen.extend(tokens[:, :3], cache)                 # 6 + 3 > 8
    with pytest.raises(ValueError, match="sequences"):
        gen.extend(_tokens(3, 2), cache)                 # wrong B
    with pytest.raises(ValueError, match="counts"):
        gen.extend(tokens[:, :2], cache, counts=[3, 1])
    with pytest.raises(ValueError, match="counts"):
        gen.extend(tokens[:, :2], cache, counts=[-1, 1])
    with pytest.raises(ValueError, match="counts"):
        gen.extend(tokens[:, :2], cache, counts=[1])
    assert cache.pos == 6 and cache.lens.tolist() == [6, 6]
    gen.extend(tokens[:, :2], cache)                     # exactly full
    assert cache.pos == 8
