"""Sample token ids from a mipipe checkpoint.

    python generate.py --checkpoint DIR --prompt "1,2,3" --max-new-tokens 16
    python generate.py --checkpoint DIR --prompt "1,2,3;7,8,9" --max-new-tokens 16 \
        --temperature 0.8 --top-k 40 --seed 1 --device cuda
    python generate.py --checkpoint DIR --prompt "1,2,3;7,8" --max-new-tokens 16 \
        --temperature 0.8 --top-k 40 --top-p 0.9 --stop-token 0
    python generate.py --checkpoint DIR --draft-checkpoint SMALL_DIR --lookahead 4 \
        --prompt "1,2,3;7,8" --max-new-tokens 16
    python generate.py --checkpoint DIR --weights int8 --prompt "1,2,3" --max-new-tokens 16
    python generate.py --checkpoint DIR --kv-cache int8 --prompt "1,2,3" --max-new-tokens 16

The model configuration comes from the checkpoint's manifest; the weights are found by FQN,
so a checkpoint written at any PP / DP degree loads into this single process.  Prompts are
comma-separated token ids (train.py's data are ids; there is no tokenizer), several prompts
separated by ``;``.  Prints the prompt + generated ids, one sequence per line.

Prompts of one shared length with none of ``--top-p`` / ``--stop-token`` / ``--pad-token``
go through ``Generator.generate``.  Prompts of different lengths, or any of those flags, go
through ``Generator.generate_batch`` (positions and sampling on the device): each printed
row then ends with its last valid token -- the stop token if it was produced -- and the
padding is not printed.

``--draft-checkpoint`` routes to ``Generator.generate_speculative`` (greedy only): a smaller
model over the same vocabulary drafts ``--lookahead`` tokens per round and the checkpoint's
model verifies them in one pass.  The printed rows are the model's own greedy continuation;
the acceptance rate goes to stderr.

``--weights int8`` quantises the block matrices and the LM head per output row while loading
(int8 weight-only inference; the draft of ``--draft-checkpoint`` follows ``--draft-weights``).
``--weights int4g128`` stores them as 4-bit values with one scale per 128-element group of K
instead (every such matrix needs K % 128 == 0).

``--kv-cache int8`` keeps the K / V cache as int8 rows with one f32 scale per (token, KV head):
about half the cache bytes, with any ``--weights`` (the draft follows ``--draft-kv-cache``).
"""
from __future__ import annotations

import argparse
import sys


def parse_prompts(text: str):
    rows = [[int(t) for t in row.replace(" ", "").split(",") if t] for row in text.split(";") if row.strip()]
    if not rows or any(not r for r in rows):
        raise ValueError("--prompt: comma-separated token ids, prompts separated by ';'")
    return rows


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True, help="directory written by save_checkpoint / train.py")
    ap.add_argument("--prompt", required=True, help='token ids, e.g. "1,2,3" (";" between prompts; lengths may differ)')
    ap.add_argument("--max-new-tokens", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=0.0, help="0 = greedy")
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--top-p", type=float, default=None, help="nucleus sampling: keep the smallest set of the most "
                    "probable tokens whose mass reaches this value, in (0, 1]")
    ap.add_argument("--stop-token", type=int, default=None, help="a sequence ends once it produces this id")
    ap.add_argument("--pad-token", type=int, default=None, help="id that fills finished rows (default 0; not printed)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--draft-checkpoint", default=None, help="speculative decoding: checkpoint directory of the "
                    "draft model (same vocabulary; greedy only)")
    ap.add_argument("--lookahead", type=int, default=4, help="tokens the draft proposes per round")
    ap.add_argument("--device", choices=("cpu", "cuda"), default=None, help="default: cuda when available")
    ap.add_argument("--weights", choices=("bf16", "int8", "int4g128"), default="bf16",
                    help="int8 / int4g128: weight-only quantisation of the block matrices and the LM head at load "
                    "(per output row / 4-bit with one scale per 128 k)")
    ap.add_argument("--draft-weights", choices=("bf16", "int8", "int4g128"), default="bf16",
                    help="the same for the draft model")
    ap.add_argument("--kv-cache", choices=("bf16", "int8"), default="bf16",
                    help="int8: K / V cache rows as int8 with one f32 scale per (token, KV head)")
    ap.add_argument("--draft-kv-cache", choices=("bf16", "int8"), default="bf16", help="the same for the draft model")
    a = ap.parse_args(argv)

    import torch
    import mipipe

    rows = parse_prompts(a.prompt)
    gen = mipipe.Generator.load(a.checkpoint, device=a.device, weights=a.weights, kv_cache=a.kv_cache)
    bad = [t for r in rows for t in r if not 0 <= t < gen.cfg.vocab_size]
    if bad:
        raise ValueError(f"--prompt: token id {bad[0]} outside the vocabulary [0, {gen.cfg.vocab_size})")
    if a.draft_checkpoint is not None:
        if a.temperature != 0 or a.top_k is not None or a.top_p is not None or a.stop_token is not None:
            raise ValueError("--draft-checkpoint: speculative decoding is greedy only (no --temperature / --top-k / "
                             "--top-p / --stop-token)")
        draft = mipipe.Generator.load(a.draft_checkpoint, device=gen.device, dtype=gen.dtype, weights=a.draft_weights,
                                      kv_cache=a.draft_kv_cache)
        out, lengths, stats = gen.generate_speculative([torch.tensor(r, dtype=torch.int64) for r in rows],
                                                       a.max_new_tokens, draft, lookahead=a.lookahead,
                                                       pad_token=a.pad_token or 0)
        for r, n in zip(out.tolist(), lengths.tolist()):
            print(",".join(str(t) for t in r[:n]))
        rate = stats["accepted"] / stats["drafted"] if stats["drafted"] else 0.0
        print(f"speculative: {stats['rounds']} rounds, {stats['accepted']} of {stats['drafted']} drafted tokens "
              f"accepted ({rate:.1%})", file=sys.stderr)
        return 0
    ragged = len({len(r) for r in rows}) != 1
    if ragged or a.top_p is not None or a.stop_token is not None or a.pad_token is not None:
        out, lengths = gen.generate_batch([torch.tensor(r, dtype=torch.int64) for r in rows], a.max_new_tokens,
                                          temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.seed,
                                          stop_token=a.stop_token, pad_token=a.pad_token or 0)
        for r, n in zip(out.tolist(), lengths.tolist()):
            print(",".join(str(t) for t in r[:n]))
        return 0
    out = gen.generate(torch.tensor(rows, dtype=torch.int64), a.max_new_tokens, temperature=a.temperature,
                       top_k=a.top_k, seed=a.seed)
    for r in out.tolist():
        print(",".join(str(t) for t in r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
