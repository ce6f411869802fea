"""End-to-end tokens/s of generation on one GPU: ``Generator.generate`` (one shared prompt
length, host positions, torch sampling) against ``Generator.generate_batch`` (device
positions, on-device sampling) with the decode step run eagerly and as a replayed HIP graph.

    python tools/generate_time.py                       # the full table (profiles/r10_generate_batch.md)
    python tools/generate_time.py --models gpt2-small --batches 1 --windows 5

Needs a GPU and the built extension: there is no fallback.  Per shape every variant is
warmed, then the three variants alternate inside this one process; a window is one whole call
(prefill of the prompt + ``--new-tokens`` tokens) ending in a synchronise, and the figure is
``B * new_tokens / median(window)``.  The greedy tokens of the three variants are compared on
the timed inputs: graph replay must equal the eager step bit for bit; ``generate`` must equal
them too wherever its ``attn_decode`` calls use the key-split plan of ``generate_batch`` (it
sizes the grid by the current position, ``generate_batch`` by the cache, so at small B the
partial sums may be grouped differently; a mismatch there is reported, not an error).
Launches per token are counted on the host over one decode step: calls into the HIP
extension plus ATen ops that launch a kernel.  Prints one JSON line per shape.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import mipipe  # noqa: E402
from mipipe import ops  # noqa: E402
from mipipe.models.config import NativeConfig  # noqa: E402
from mipipe.ops import _base, kernels as _k  # noqa: E402

_NO_KERNEL = ("empty", "view", "as_strided", "slice", "select", "reshape", "unsqueeze", "squeeze", "expand", "alias",
              "detach", "transpose", "permute", "t.default", "_unsafe_view", "resize", "set_", "lift_fresh",
              "is_pinned", "_local_scalar_dense", "split", "unbind")


class _Count(TorchDispatchMode):
    """ATen ops that launch a kernel (everything that is not a view or an allocation)."""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if not any(s in name for s in _NO_KERNEL):
            self.n += 1
        return func(*args, **(kwargs or {}))


class _ExtProxy:
    """Counts calls into the HIP extension (attn_decode is two launches: splits + combine)."""

    def __init__(self, ext):
        self.ext, self.n = ext, 0

    def __getattr__(self, name):
        fn = getattr(self.ext, name)
        if not callable(fn) or name.endswith("_plan"):
            return fn

        def call(*a, **kw):
            self.n += 2 if name == "attn_decode" else 1
            return fn(*a, **kw)
        return call


def launches_per_token(run) -> dict:
    """Host-side launch count of one decode step: the difference between runs of 4 and 3 new tokens."""
    got = []
    for n in (3, 4):
        real = _k._ext()
        proxy = _ExtProxy(real)
        _base._EXT = proxy         # the loader's cached module: what every op family calls
        try:
            with _Count() as c:
                run(n)
        finally:
            _base._EXT = real
        got.append((proxy.n, c.n))
    return {"hip": got[1][0] - got[0][0], "aten": got[1][1] - got[0][1]}


def _config(name: str) -> NativeConfig:
    if name == "gpt2-small":
        return NativeConfig.gpt2("small")
    if name == "llama3-1b":
        return NativeConfig.llama3("1b", max_seq_len=1024)
    raise ValueError(name)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="gpt2-small,llama3-1b")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available() or not ops.ext_available():
        raise SystemExit("generate_time: needs a GPU and the built HIP extension")
    if a.windows < 5:
        raise SystemExit("generate_time: at least 5 windows")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S0, N = a.prompt, a.new_tokens
    bad = 0
    for mname in a.models.split(","):
        cfg = _config(mname)
        gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0)
        for B in (int(b) for b in a.batches.split(",")):
            prompt = torch.randint(0, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(B))
            rows = list(prompt)
            plans = {ops.attn_decode_plan(B, cfg.n_kv_heads, p) for p in range(S0 + 1, S0 + N)}
            same_plan = plans == {ops.attn_decode_plan(B, cfg.n_kv_heads, S0 + N)}
            for label, kw in (("greedy", {}), ("top_k=40,top_p=0.9", dict(temperature=1.0, top_k=40, top_p=0.9))):
                kw_old = {k: v for k, v in kw.items() if k != "top_p"}        # generate has no top-p
                variants = {
                    "generate": lambda n=N: gen.generate(prompt, n, seed=1, **kw_old),
                    "batch_eager": lambda n=N: gen.generate_batch(rows, n, seed=1, graphs=False, **kw)[0],
                    "batch_graph": lambda n=N: gen.generate_batch(rows, n, seed=1, graphs=True, **kw)[0],
                }
                outs = {}
                for name, fn in variants.items():               # warm every variant of the shape
                    outs[name] = fn()
                torch.cuda.synchronize()
                times = {name: [] for name in variants}
                for _ in range(a.windows):                      # alternate inside the one process
                    for name, fn in variants.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[name].append(time.perf_counter() - t0)
                rec = {"model": mname, "B": B, "prompt": S0, "new_tokens": N, "sampling": label}
                for name in variants:
                    rec[f"{name}_tok_s"] = round(B * N / statistics.median(times[name]), 1)
                rec["graph_vs_eager"] = round(rec["batch_graph_tok_s"] / rec["batch_eager_tok_s"], 3)
                rec["graph_vs_generate"] = round(rec["batch_graph_tok_s"] / rec["generate_tok_s"], 3)
                rec["graph_equals_eager"] = bool(torch.equal(outs["batch_graph"], outs["batch_eager"]))
                bad += not rec["graph_equals_eager"]
                if not kw:
                    rec["generate_equals_batch"] = bool(torch.equal(outs["generate"], outs["batch_eager"]))
                    rec["same_split_plan"] = same_plan
                    if not rec["generate_equals_batch"]:
                        diff = (outs["generate"] != outs["batch_eager"]).any(0).nonzero()
                        rec["first_difference_at_new_token"] = int(diff[0, 0]) - S0
                        bad += same_plan
                rec["launches_generate"] = launches_per_token(variants["generate"])
                rec["launches_batch"] = launches_per_token(variants["batch_eager"])
                print(json.dumps(rec), flush=True)
        del gen
        torch.cuda.empty_cache()
    if bad:
        print(f"generate_time: {bad} token mismatches", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
