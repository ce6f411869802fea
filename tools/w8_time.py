"""Time of the skinny-M kernel (int8, int4g128 and bf16 weights) against ``ops.linear`` per GEMM
shape, and end-to-end tokens/s of bf16, bf16 ``skinny=True``, int8 and int4g128 generators, on
one GPU.

    python tools/w8_time.py                       # both tables (profiles/r12_w8_decode.md, r13_w4_decode.md)
    python tools/w8_time.py --parts gemm --models llama3-1b --rows 1,16
    python tools/w8_time.py --parts e2e --batches 1 --speculative

Needs a GPU and the built extension: there is no fallback.  The protocol is that of
tools/generate_time.py: per shape every variant is warmed, then the variants alternate inside
this one process, and each figure is the median of ``--windows`` (>= 5) windows.

Per GEMM (``--parts gemm``): the layer and head shapes [N, K] of GPT-2 small, Llama-3 1B and
Llama-3 8B at M in {1, 4, 8, 16, 32, 64} rows.  A window is ``--iters`` calls between two
events.  Each call takes the next of several copies of the weight (together at least
``--cold-mb``, 512 MB by default, capped at 64 copies) so the matrix comes from HBM rather
than from the 256 MB Infinity Cache, as it does inside a decode step of a model that does not
fit there; ``copies`` is printed.  Variants: ``w8`` = ops.linear_w8 (the skinny kernel up to
W8_SKINNY_MAX_M rows, dequantise + ops.linear above), ``w4`` = ops.linear_w4 on the int4g128
format of the same weights (the same routes), ``skinny_bf16`` (up to 16 rows),
``linear`` = ops.linear on bf16 weights, ``dequant_linear`` = dequant_w8 + ops.linear at every
M (the crossover).  GB/s counts the weight bytes of the variant's own format once per call
(for ``w4`` the packed nibbles and their group scales: N K / 2 + N K / 32 bytes).

End to end (``--parts e2e``): greedy ``generate_batch`` (eager step) of one set of weights as
a bf16 generator, the same with ``skinny=True`` and quantised to int8 and to int4g128;
``--speculative`` adds ``generate_speculative`` of the bf16 target with its own int8 and
int4g128 generators as the draft.  A
window is one whole call (prefill + new tokens); tok/s = B * new_tokens / median.
Prints one JSON line per shape, then both tables in markdown."""
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

import mipipe  # noqa: E402
from mipipe import ops  # noqa: E402
from mipipe.models.config import NativeConfig  # noqa: E402

# wqkv, wo, w1 / w13, w2, head: [N, K]
MODEL_SHAPES = {
    "gpt2-small": ((2304, 768), (768, 768), (3072, 768), (768, 3072), (50304, 768)),
    "llama3-1b": ((3072, 2048), (2048, 2048), (16384, 2048), (2048, 8192), (128256, 2048)),
    "llama3-8b": ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128256, 4096)),
}
NAMES = ("wqkv", "wo", "w1/w13", "w2", "head")


def _config(name: str) -> NativeConfig:
    if name == "gpt2-small":
        return NativeConfig.gpt2("small")
    if name == "llama3-1b":
        return NativeConfig.llama3("1b", max_seq_len=1024)
    raise ValueError(name)


def _windows(variants, windows, iters):
    """{name: median seconds per call}: warm, then alternate the variants window by window"""
    for fn in variants.values():
        fn(0)
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    call = 1
    for _ in range(windows):
        for name, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                fn(call + i)
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e-3 / iters)
        call += iters
    return {n: statistics.median(t) for n, t in times.items()}


def gemm_part(a, dev):
    recs = []
    for mname in a.models.split(","):
        for lname, (N, K) in zip(NAMES, MODEL_SHAPES[mname]):
            copies = max(2, min(64, -(-a.cold_mb * (1 << 20) // (N * K))))
            w = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * (K ** -0.5) for _ in range(copies)]
            qs = [ops.quantize_w8(t) for t in w]
            q4s = [ops.quantize_w4(t) for t in w]
            scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
            for M in (int(m) for m in a.rows.split(",")):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                variants = {
                    "w8": lambda i: ops.linear_w8(x, *qs[i % copies], out=y, scratch=scratch),
                    "w4": lambda i: ops.linear_w4(x, *q4s[i % copies], out=y, scratch=scratch),
                    "linear": lambda i: ops.linear(x, w[i % copies], out=y),
                    "dequant_linear": lambda i: ops.linear(
                        x, ops.dequant_w8(*qs[i % copies], scratch.view(N, K)), out=y),
                }
                if M <= ops.SKINNY_MAX_M:
                    variants["skinny_bf16"] = lambda i: ops.linear_skinny(x, w[i % copies], out=y)
                t = _windows(variants, a.windows, a.iters)
                rec = {"model": mname, "layer": lname, "N": N, "K": K, "M": M, "copies": copies,
                       "w8_route": "skinny" if M <= ops.W8_SKINNY_MAX_M else "dequant"}
                for name, sec in t.items():
                    wbytes = N * K // 2 + N * K // 32 if name == "w4" else \
                        N * K * (1 if name in ("w8", "dequant_linear") else 2)
                    rec[f"{name}_us"] = round(sec * 1e6, 1)
                    rec[f"{name}_gbs"] = round(wbytes / sec * 1e-9)
                print(json.dumps(rec), flush=True)
                recs.append(rec)
            del w, qs, q4s, scratch
            torch.cuda.empty_cache()
    return recs


def e2e_part(a, dev):
    recs = []
    S0, N = a.prompt, a.new_tokens
    for mname in (m for m in a.models.split(",") if m != "llama3-8b"):
        cfg = _config(mname)
        base = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0)
        gens = {"bf16": base, "bf16_skinny": mipipe.Generator.from_model(base.model, skinny=True),
                "int8": mipipe.Generator.from_model(base.model, weights="int8"),
                "int4g128": mipipe.Generator.from_model(base.model, weights="int4g128")}
        for B in (int(b) for b in a.batches.split(",")):
            prompt = torch.randint(0, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(B))
            rows = list(prompt)
            variants = {n: (lambda g=g: g.generate_batch(rows, N, graphs=False)[0]) for n, g in gens.items()}
            if a.speculative:
                variants["bf16_spec_int8_draft"] = lambda: base.generate_speculative(rows, N, gens["int8"], lookahead=4)
                variants["bf16_spec_int4g128_draft"] = lambda: base.generate_speculative(rows, N, gens["int4g128"],
                                                                                         lookahead=4)
            outs = {n: fn() for n, fn in variants.items()}                  # warm
            torch.cuda.synchronize()
            times = {n: [] for n in variants}
            for _ in range(a.windows):
                for n, fn in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[n].append(time.perf_counter() - t0)
            rec = {"model": mname, "B": B, "prompt": S0, "new_tokens": N}
            for n in variants:
                rec[f"{n}_tok_s"] = round(B * N / statistics.median(times[n]), 1)
            rec["skinny_vs_bf16"] = round(rec["bf16_skinny_tok_s"] / rec["bf16_tok_s"], 3)
            rec["int8_vs_bf16"] = round(rec["int8_tok_s"] / rec["bf16_tok_s"], 3)
            rec["int4g128_vs_bf16"] = round(rec["int4g128_tok_s"] / rec["bf16_tok_s"], 3)
            rec["int4g128_vs_int8"] = round(rec["int4g128_tok_s"] / rec["int8_tok_s"], 3)
            rec["skinny_tokens_equal_bf16"] = bool(torch.equal(outs["bf16"], outs["bf16_skinny"]))
            if a.speculative:
                st = outs["bf16_spec_int8_draft"][2]
                rec["spec_accept_rate"] = round(st["accepted"] / max(1, st["drafted"]), 3)
                rec["spec_equals_bf16"] = bool(torch.equal(outs["bf16_spec_int8_draft"][0], outs["bf16"]))
                st = outs["bf16_spec_int4g128_draft"][2]
                rec["spec4_accept_rate"] = round(st["accepted"] / max(1, st["drafted"]), 3)
            print(json.dumps(rec), flush=True)
            recs.append(rec)
        del base, gens
        torch.cuda.empty_cache()
    return recs


def _markdown(gemm, e2e):
    if gemm:
        print("\n| model | layer | N x K | M | w4 us | w4 GB/s | w8 us | w8 GB/s | skinny bf16 us | GB/s | linear us | GB/s "
              "| dequant+linear us |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for r in gemm:
            sk = (r.get("skinny_bf16_us", "-"), r.get("skinny_bf16_gbs", "-"))
            print(f"| {r['model']} | {r['layer']} | {r['N']} x {r['K']} | {r['M']} | {r['w4_us']} | {r['w4_gbs']} | "
                  f"{r['w8_us']} ({r['w8_route']}) | "
                  f"{r['w8_gbs']} | {sk[0]} | {sk[1]} | {r['linear_us']} | {r['linear_gbs']} | {r['dequant_linear_us']} |")
    if e2e:
        keys = [k for k in e2e[0] if k not in ("model", "B", "prompt", "new_tokens")]
        print("\n| model | B | " + " | ".join(keys) + " |")
        print("|---|---|" + "---|" * len(keys))
        for r in e2e:
            print(f"| {r['model']} | {r['B']} | " + " | ".join(str(r[k]) for k in keys) + " |")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="gemm,e2e")
    ap.add_argument("--models", default="gpt2-small,llama3-1b,llama3-8b")
    ap.add_argument("--rows", default="1,4,8,16,32,64")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cold-mb", type=int, default=512)
    ap.add_argument("--speculative", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available() or not ops.ext_available():
        raise SystemExit("w8_time: needs a GPU and the built HIP extension")
    if a.windows < 5:
        raise SystemExit("w8_time: at least 5 windows")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    parts = a.parts.split(",")
    gemm = gemm_part(a, dev) if "gemm" in parts else []
    e2e = e2e_part(a, dev) if "e2e" in parts else []
    _markdown(gemm, e2e)
    return 0


if __name__ == "__main__":
    sys.exit(main())
