"""Time of the skinny-M kernel (int8, int4g128, mxfp4 and bf16 weights) against ``ops.linear`` per
GEMM shape, and end-to-end tokens/s of bf16, bf16 ``skinny=True``, int8, int4g128 and mxfp4
generators, on one GPU.

    python tools/w8_time.py                       # both tables (profiles/r12_w8_decode.md, r13_w4_decode.md)
    python tools/w8_time.py --parts gemm --models llama3-1b --rows 1,16
    python tools/w8_time.py --parts e2e --batches 1 --speculative
    python tools/w8_time.py --parts mx,mx_e2e --models llama3-1b,llama3-8b --iters 50     # profiles/r17_gemm_mx.md

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
format of the same weights (the same routes), ``mx4`` = ops.quant.linear_mx4 on their MXFP4 format
(profiles/r16_mx4_decode.md), ``skinny_bf16`` (up to 16 rows),
``linear`` = ops.linear on bf16 weights, ``dequant_linear`` = dequant_w8 + ops.linear at every
M (the crossover).  Above 16 and up to 64 rows four more alternate in the same windows:
``rows64`` / ``rows64_w4`` / ``rows64_bf16`` = ops.quant.linear_skinny64 on the int8 / int4g128 /
bf16 weights (csrc/kernels/gemv_rows64.hip) and ``loop`` = ceil(M / 16) ``linear_skinny`` calls
on the int8 weights, which reads and converts them that many times.  Every record also carries
``<variant>_spread_us``, the largest minus the smallest window.  MIPIPE_EXT_VARIANT=xreg (a
``tools/build_ext.py --variant xreg -DMP_ROWS64_XREG`` build) times the register-direct x path
of the 64-row kernel in a process of its own.  GB/s counts the weight bytes of the variant's
own format once per call (for ``w4`` and ``mx4`` the packed nibbles and their scales: N K / 2 +
N K / 32 bytes).

End to end (``--parts e2e``): greedy ``generate_batch`` (eager step) of one set of weights as
a bf16 generator, the same with ``skinny=True`` and quantised to int8 and to int4g128, and the
bf16 and int8 ones again with ``skinny64=True`` (they differ from 17 sequences on);
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
    return {n: statistics.median(t) for n, t in times.items()}, {n: max(t) - min(t) for n, t in times.items()}


def gemm_part(a, dev):
    recs = []
    for mname in a.models.split(","):
        for lname, (N, K) in zip(NAMES, MODEL_SHAPES[mname]):
            copies = max(2, min(64, -(-a.cold_mb * (1 << 20) // (N * K))))
            w = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * (K ** -0.5) for _ in range(copies)]
            qs = [ops.quantize_w8(t) for t in w]
            q4s = [ops.quantize_w4(t) for t in w]
            mxs = [ops.quant.quantize_mx4(t) for t in w]
            scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
            for M in (int(m) for m in a.rows.split(",")):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                variants = {
                    "w8": lambda i: ops.linear_w8(x, *qs[i % copies], out=y, scratch=scratch),
                    "w4": lambda i: ops.linear_w4(x, *q4s[i % copies], out=y, scratch=scratch),
                    "mx4": lambda i: ops.quant.linear_mx4(x, *mxs[i % copies], out=y, scratch=scratch),
                    "linear": lambda i: ops.linear(x, w[i % copies], out=y),
                    "dequant_linear": lambda i: ops.linear(
                        x, ops.dequant_w8(*qs[i % copies], scratch.view(N, K)), out=y),
                }
                if M <= ops.SKINNY_MAX_M:
                    variants["skinny_bf16"] = lambda i: ops.linear_skinny(x, w[i % copies], out=y)
                if ops.SKINNY_MAX_M < M <= ops.quant.SKINNY64_MAX_M:
                    s64 = ops.quant.linear_skinny64
                    variants["rows64"] = lambda i: s64(x, *qs[i % copies], out=y)
                    variants["rows64_w4"] = lambda i: s64(x, *q4s[i % copies], out=y)
                    variants["rows64_bf16"] = lambda i: s64(x, w[i % copies], out=y)
                    variants["loop"] = lambda i: [ops.linear_skinny(x[m: m + 16], *qs[i % copies], out=y[m: m + 16])
                                                  for m in range(0, M, 16)]
                t, spread = _windows(variants, a.windows, a.iters)
                rec = {"model": mname, "layer": lname, "N": N, "K": K, "M": M, "copies": copies,
                       "w8_route": "skinny" if M <= ops.W8_SKINNY_MAX_M else "dequant"}
                for name, sec in t.items():
                    wbytes = N * K // 2 + N * K // 32 if name in ("w4", "mx4", "rows64_w4") else \
                        N * K * (1 if name in ("w8", "dequant_linear", "rows64", "loop") else 2)
                    rec[f"{name}_us"] = round(sec * 1e6, 1)
                    rec[f"{name}_spread_us"] = round(spread[name] * 1e6, 1)
                    rec[f"{name}_gbs"] = round(wbytes / sec * 1e-9)
                print(json.dumps(rec), flush=True)
                recs.append(rec)
            del w, qs, q4s, mxs, scratch
            torch.cuda.empty_cache()
    return recs


def mx_part(a, dev):
    """``--parts mx`` (profiles/r17_gemm_mx.md): per shape and M in ``--mx-rows``, ``mx4a8`` = ops.quant.linear_mx4a8
    (quantiser + the MXFP8 x MXFP4 GEMM), ``mx4a8_gemm`` = the GEMM alone on rows quantised before the window,
    ``mx4`` = ops.quant.linear_mx4 (dequantise + ops.linear above 16 rows) and ``linear`` = ops.linear on bf16
    weights, alternating in the same windows; and the plan's tile."""
    recs = []
    Q = ops.quant
    for mname in a.models.split(","):
        for lname, (N, K) in zip(NAMES, MODEL_SHAPES[mname]):
            copies = max(2, min(64, -(-a.cold_mb * (1 << 20) // (N * K))))
            w = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * (K ** -0.5) for _ in range(copies)]
            mxs = [Q.quantize_mx4(t) for t in w]
            scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
            for M in (int(m) for m in a.mx_rows.split(",")):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                xq = Q.quantize_mx8_rows(x)
                gemm = ops.load_ext().gemv_skinny
                variants = {
                    "mx4a8": lambda i: Q.linear_mx4a8(x, *mxs[i % copies], out=y, xq=xq),
                    "mx4a8_gemm": lambda i: gemm(xq, *mxs[i % copies], y, None, None),
                    "mx4": lambda i: Q.linear_mx4(x, *mxs[i % copies], out=y, scratch=scratch),
                    "linear": lambda i: ops.linear(x, w[i % copies], out=y),
                }
                t, spread = _windows(variants, a.windows, a.iters)
                rec = {"model": mname, "layer": lname, "N": N, "K": K, "M": M, "copies": copies,
                       "tile": "64x32" if M <= 64 else "128x128"}
                for name, sec in t.items():
                    rec[f"{name}_us"] = round(sec * 1e6, 1)
                    rec[f"{name}_spread_us"] = round(spread[name] * 1e6, 1)
                rec["tflops_gemm"] = round(2.0 * M * N * K / t["mx4a8_gemm"] * 1e-12, 1)
                print(json.dumps(rec), flush=True)
                recs.append(rec)
            del w, mxs, scratch
            torch.cuda.empty_cache()
    return recs


def mx_e2e_part(a, dev):
    """``--parts mx_e2e`` (profiles/r17_gemm_mx.md).  Llama-3 1B, ``--mx-prompt`` prompt tokens, ``--mx-new`` new
    tokens, B = ``--mx-batch``: peak allocated bytes of a ``weights="mxfp4"`` generator with and without
    ``activations="mxfp8"`` over one ``generate_batch`` (each alone on the device), then tokens/s of both and of
    the bf16 generator, alternating, one whole call per window.  Then the logit error of a random-init GPT-2
    small against its bf16 generator (B = 4, 96-token prefill, 32 teacher-forced decode steps)."""
    S0, N, B = a.mx_prompt, a.mx_new, a.mx_batch
    cfg = NativeConfig.llama3("1b", max_seq_len=S0 + N + 64)
    rows = list(torch.randint(0, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(B)))
    kinds = {"mxfp4": {"weights": "mxfp4"}, "mxfp4_mxfp8": {"weights": "mxfp4", "activations": "mxfp8"}, "bf16": {}}
    rec = {"model": "llama3-1b", "B": B, "prompt": S0, "new_tokens": N}
    for n in ("mxfp4", "mxfp4_mxfp8"):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        g = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0, **kinds[n])
        rec[f"{n}_weights_bytes"] = torch.cuda.memory_allocated()
        g.generate_batch(rows, N, graphs=False)
        torch.cuda.synchronize()
        rec[f"{n}_peak_bytes"] = torch.cuda.max_memory_allocated()
        rec[f"{n}_scratch"] = None if g._scratch is None else g._scratch.numel() * 2
        del g
    gens = {n: mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0, **kw) for n, kw in kinds.items()}
    times = {n: [] for n in gens}
    for w in range(a.windows + 1):                                      # window 0 warms
        for n, g in gens.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.generate_batch(rows, N, graphs=False)
            torch.cuda.synchronize()
            if w:
                times[n].append(time.perf_counter() - t0)
    for n in gens:
        rec[f"{n}_ms"] = round(statistics.median(times[n]) * 1e3, 1)
        rec[f"{n}_spread_ms"] = round((max(times[n]) - min(times[n])) * 1e3, 1)
        rec[f"{n}_tok_s"] = round(B * N / statistics.median(times[n]), 1)
    # the prefill alone (the part the option changes at B <= 16)
    for n, g in gens.items():
        ts = []
        for _ in range(a.windows):
            cache = g.new_cache(B, S0 + 8)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.prefill(torch.stack(rows).to(dev), cache)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        rec[f"{n}_prefill_ms"] = round(statistics.median(ts) * 1e3, 1)
    print(json.dumps(rec), flush=True)
    del gens
    torch.cuda.empty_cache()
    cfg = NativeConfig.gpt2("small")
    tok = torch.randint(0, cfg.vocab_size, (4, 128), generator=torch.Generator().manual_seed(4)).to(dev)
    lg = {}
    for n, kw in kinds.items():
        g = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0, **kw)
        cache = g.new_cache(4, 128)
        out = [g.prefill(tok[:, :96].contiguous(), cache)] + [g.decode(tok[:, t].contiguous(), cache) for t in range(96, 128)]
        lg[n] = torch.stack(out, 1)[..., : cfg.vocab_size].float()
        del g, cache
    err = {"protocol": "gpt2-small random init, B 4, 96-token prefill + 32 decode steps, against the bf16 generator",
           "logit_rms": round(float(lg["bf16"].pow(2).mean().sqrt()), 3)}
    for n in ("mxfp4", "mxfp4_mxfp8"):
        d = lg[n] - lg["bf16"]
        err[n] = {"max": round(float(d.abs().max()), 3), "rms": round(float(d.pow(2).mean().sqrt()), 3),
                  "same_argmax": round(float((lg[n].argmax(-1) == lg["bf16"].argmax(-1)).float().mean()), 3)}
    print(json.dumps(err), flush=True)


def e2e_part(a, dev):
    recs = []
    S0, N = a.prompt, a.new_tokens
    for mname in (m for m in a.models.split(",") if m != "llama3-8b"):
        cfg = _config(mname)
        base = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0)
        gens = {"bf16": base, "bf16_skinny": mipipe.Generator.from_model(base.model, skinny=True),
                "int8": mipipe.Generator.from_model(base.model, weights="int8"),
                "int4g128": mipipe.Generator.from_model(base.model, weights="int4g128"),
                "mxfp4": mipipe.Generator.from_model(base.model, weights="mxfp4"),
                "bf16_skinny64": mipipe.Generator.from_model(base.model, skinny64=True),
                "int8_skinny64": mipipe.Generator.from_model(base.model, weights="int8", skinny64=True)}
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
            rec["mxfp4_vs_int4g128"] = round(rec["mxfp4_tok_s"] / rec["int4g128_tok_s"], 3)
            rec["mxfp4_vs_int8"] = round(rec["mxfp4_tok_s"] / rec["int8_tok_s"], 3)
            rec["int8_skinny64_vs_int8"] = round(rec["int8_skinny64_tok_s"] / rec["int8_tok_s"], 3)
            rec["int8_skinny64_vs_bf16"] = round(rec["int8_skinny64_tok_s"] / rec["bf16_tok_s"], 3)
            for n in variants:
                rec[f"{n}_spread_ms"] = round((max(times[n]) - min(times[n])) * 1e3, 2)
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
        print("\n| model | layer | N x K | M | mx4 us | mx4 GB/s | w4 us | w4 GB/s | w8 us | w8 GB/s | skinny bf16 us | GB/s | linear us | GB/s "
              "| dequant+linear us | rows64 us | rows64 w4 us | rows64 bf16 us | loop us |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for r in gemm:
            sk = (r.get("skinny_bf16_us", "-"), r.get("skinny_bf16_gbs", "-"))
            print(f"| {r['model']} | {r['layer']} | {r['N']} x {r['K']} | {r['M']} | {r['mx4_us']} | {r['mx4_gbs']} | {r['w4_us']} | "
                  f"{r['w4_gbs']} | "
                  f"{r['w8_us']} ({r['w8_route']}) | "
                  f"{r['w8_gbs']} | {sk[0]} | {sk[1]} | {r['linear_us']} | {r['linear_gbs']} | {r['dequant_linear_us']} | "
                  + " | ".join(str(r.get(f"{n}_us", "-")) for n in ("rows64", "rows64_w4", "rows64_bf16", "loop")) + " |")
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
    ap.add_argument("--batches", default="1,8,32,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cold-mb", type=int, default=512)
    ap.add_argument("--speculative", action="store_true")
    ap.add_argument("--mx-rows", default="32,64,256,2048", help="rows of --parts mx")
    ap.add_argument("--mx-prompt", type=int, default=4096, help="prompt tokens of --parts mx_e2e")
    ap.add_argument("--mx-new", type=int, default=64)
    ap.add_argument("--mx-batch", type=int, default=8)
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
    if "mx" in parts:
        mx_part(a, dev)
    if "mx_e2e" in parts:
        mx_e2e_part(a, dev)
    _markdown(gemm, e2e)
    return 0


if __name__ == "__main__":
    sys.exit(main())
