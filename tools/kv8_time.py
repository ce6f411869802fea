"""Timing of the int8 KV cache (csrc/kernels/attention_kv8.hip) against the bf16 cache, in one run.

    python tools/kv8_time.py --parts decode,append,quant [--out FILE]
    python tools/kv8_time.py --parts e2e --batches 8,32 --weights bf16,int8

The protocol of tools/decode_time.py: every timed call reads the next cache of a rotating set of
at least 1 GiB (so the figure is an HBM stream, not an Infinity Cache replay), a window of calls
is timed with device events on one stream, and the median over the windows is reported.  The
yardstick of every int8 figure is the bf16 kernel in the same run on the same shape; the ideal
ratio is the byte ratio of the formats (W / (2 Hkv D): 0.53 at D = 64, 0.52 at D = 128).

* ``decode``: ``ops.attn_decode`` at B = 1, 8, 64 and L = 1024, 8192 for the GPT-2 small (H 12,
  Hkv 12, D 64) and Llama-3 8B (H 32, Hkv 8, D 128) head layouts: the table of
  profiles/r8_attn_decode.md.  GB/s = the K and V bytes of the format over the time.
* ``append``: ``ops.attn_append`` at T = 5 on the B = 8 and B = 64, L = 8192 rows of that table.
* ``quant``: ``ops.rope_kv_append`` (rope on, T = 1) into int8 against bf16 caches at B = 64.
* ``e2e``: greedy ``generate_batch`` (eager step) of Llama-3 1B, random init, prompt 4096 and 64
  new tokens: tokens/s with a bf16 and an int8 cache.  A window is one whole call."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = [("GPT-2 small", 12, 12, 64), ("Llama-3 8B", 32, 8, 128)]
BATCHES = (1, 8, 64)
LENGTHS = (1024, 8192)
ROTATE_BYTES = 1 << 30
HBM_CEILING = 6.3e12            # bytes/s, streaming ceiling of one MI355X


def _time(fn, n_rot, windows, min_calls):
    """Median per-call microseconds of ``fn(i)`` (i = rotating buffer index)."""
    import torch
    calls = max(min_calls, n_rot)
    for i in range(2 * n_rot if n_rot < 8 else n_rot):
        fn(i % n_rot)
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(calls):
            fn(i % n_rot)
        e.record()
        e.synchronize()
        per_call.append(s.elapsed_time(e) * 1e3 / calls)
    return statistics.median(per_call)


def _cache_sets(B, L, Hkv, D, dev, g):
    """rotating (k, v) caches of both formats, the int8 set quantised from the bf16 set's values;
    both sets rotate over at least ROTATE_BYTES"""
    import torch
    from mipipe import ops
    W = ops.generate.kv8_row_bytes(Hkv, D)
    bf_bytes, i8_bytes = 2 * B * L * Hkv * D * 2, 2 * B * L * W
    n_bf = max(2, min(512, math.ceil(ROTATE_BYTES / bf_bytes)))
    n_i8 = max(2, min(512, math.ceil(ROTATE_BYTES / i8_bytes)))
    bf, i8 = [], []
    for i in range(max(n_bf, n_i8)):
        k = torch.randn(B, L, Hkv * D, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(B, L, Hkv * D, device=dev, generator=g).to(torch.bfloat16)
        if i < n_i8:
            i8.append((ops.generate.kv_quantize(k, Hkv, D), ops.generate.kv_quantize(v, Hkv, D)))
        if i < n_bf:
            bf.append((k, v))
    return bf, i8, bf_bytes, i8_bytes


def part_decode(a, lines):
    import torch
    from mipipe import ops
    dev = torch.device("cuda", 0)
    lines += ["", "## attn_decode, bf16 cache against int8 cache", "",
              "| layout | B | L | splits | bf16 us | bf16 GB/s | int8 us | int8 GB/s | int8 % of ceiling | int8 / bf16 "
              "time | byte ratio | max diff |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, H, Hkv, D in LAYOUTS:
        for B in BATCHES:
            for L in LENGTHS:
                g = torch.Generator(device=dev).manual_seed(B * 131 + L)
                q = torch.randn(B, (H + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)[:, : H * D]
                bf, i8, bf_bytes, i8_bytes = _cache_sets(B, L, Hkv, D, dev, g)
                lens = torch.full((B,), L, device=dev, dtype=torch.int32)
                o, o8 = (torch.empty(B, H * D, device=dev, dtype=torch.bfloat16) for _ in range(2))
                ops.attn_decode(q, bf[0][0], bf[0][1], lens, o, H, Hkv, D)
                ops.attn_decode(q, i8[0][0], i8[0][1], lens, o8, H, Hkv, D)
                diff = float((o.float() - o8.float()).abs().max())
                t_bf = _time(lambda i: ops.attn_decode(q, bf[i][0], bf[i][1], lens, o, H, Hkv, D), len(bf), a.windows,
                             a.calls)
                t_i8 = _time(lambda i: ops.attn_decode(q, i8[i][0], i8[i][1], lens, o8, H, Hkv, D), len(i8),
                             a.windows, a.calls)
                row = dict(part="decode", layout=name, B=B, L=L, splits=ops.attn_decode_plan(B, Hkv, L), bf16_us=t_bf,
                           int8_us=t_i8, bf16_gbps=bf_bytes / t_bf / 1e3, int8_gbps=i8_bytes / t_i8 / 1e3,
                           ratio=t_i8 / t_bf, byte_ratio=i8_bytes / bf_bytes, diff=diff)
                print(json.dumps(row), flush=True)
                lines.append(f"| {name} | {B} | {L} | {row['splits']} | {t_bf:.1f} | {row['bf16_gbps']:.0f} | "
                             f"{t_i8:.1f} | {row['int8_gbps']:.0f} | "
                             f"{100 * i8_bytes / (t_i8 * 1e-6) / HBM_CEILING:.1f} % | {row['ratio']:.2f} | "
                             f"{row['byte_ratio']:.3f} | {diff:.4f} |")
                del bf, i8
                torch.cuda.empty_cache()


def part_append(a, lines):
    import torch
    from mipipe import ops
    dev = torch.device("cuda", 0)
    T = 5
    lines += ["", f"## attn_append at T = {T}, bf16 cache against int8 cache", "",
              "| layout | B | L | splits | bf16 us | int8 us | int8 / bf16 time | byte ratio | max diff |",
              "|---|---|---|---|---|---|---|---|---|"]
    for name, H, Hkv, D in LAYOUTS:
        for B in (8, 64):
            L = 8192
            g = torch.Generator(device=dev).manual_seed(B * 7 + L)
            q = torch.randn(B * T, (H + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)[:, : H * D]
            bf, i8, bf_bytes, i8_bytes = _cache_sets(B, L, Hkv, D, dev, g)
            base = torch.full((B,), L - T, device=dev, dtype=torch.int32)
            o, o8 = (torch.empty(B * T, H * D, device=dev, dtype=torch.bfloat16) for _ in range(2))
            ops.attn_append(q, bf[0][0], bf[0][1], base, None, o, T, H, Hkv, D)
            ops.attn_append(q, i8[0][0], i8[0][1], base, None, o8, T, H, Hkv, D)
            diff = float((o.float() - o8.float()).abs().max())
            t_bf = _time(lambda i: ops.attn_append(q, bf[i][0], bf[i][1], base, None, o, T, H, Hkv, D), len(bf),
                         a.windows, a.calls)
            t_i8 = _time(lambda i: ops.attn_append(q, i8[i][0], i8[i][1], base, None, o8, T, H, Hkv, D), len(i8),
                         a.windows, a.calls)
            row = dict(part="append", layout=name, B=B, L=L, T=T, splits=ops.attn_append_plan(B, T, Hkv, H // Hkv, L),
                       bf16_us=t_bf, int8_us=t_i8, ratio=t_i8 / t_bf, byte_ratio=i8_bytes / bf_bytes, diff=diff)
            print(json.dumps(row), flush=True)
            lines.append(f"| {name} | {B} | {L} | {row['splits']} | {t_bf:.1f} | {t_i8:.1f} | {row['ratio']:.2f} | "
                         f"{row['byte_ratio']:.3f} | {diff:.4f} |")
            del bf, i8
            torch.cuda.empty_cache()


def part_quant(a, lines):
    import torch
    from mipipe import ops
    dev = torch.device("cuda", 0)
    B, L = 64, 1024
    lines += ["", "## rope_kv_append (rope on, T = 1, B = 64), bf16 cache against int8 cache", "",
              "| layout | bf16 us | int8 us | int8 / bf16 time |", "|---|---|---|---|"]
    for name, H, Hkv, D in LAYOUTS:
        g = torch.Generator(device=dev).manual_seed(5)
        W = ops.generate.kv8_row_bytes(Hkv, D)
        cos, sin = ops.rope_tables(L, D, 10000.0, dev)
        n_rot = 8
        qkvs = [torch.randn(B, (H + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16) for _ in range(n_rot)]
        kb, vb = (torch.zeros(B, L, Hkv * D, device=dev, dtype=torch.bfloat16) for _ in range(2))
        k8, v8 = (torch.zeros(B, L, W, device=dev, dtype=torch.int8) for _ in range(2))
        pos = torch.randint(0, L, (B,), device=dev, generator=g).to(torch.int32)
        t_bf = _time(lambda i: ops.rope_kv_append(qkvs[i], cos, sin, kb, vb, pos, None, H, Hkv, D), n_rot, a.windows,
                     a.calls)
        t_i8 = _time(lambda i: ops.rope_kv_append(qkvs[i], cos, sin, k8, v8, pos, None, H, Hkv, D), n_rot, a.windows,
                     a.calls)
        print(json.dumps(dict(part="quant", layout=name, bf16_us=t_bf, int8_us=t_i8)), flush=True)
        lines.append(f"| {name} | {t_bf:.1f} | {t_i8:.1f} | {t_i8 / t_bf:.2f} |")


def part_e2e(a, lines):
    import torch
    import mipipe
    from mipipe.models.config import NativeConfig
    dev = torch.device("cuda", 0)
    S0, N = a.prompt, a.new_tokens
    cfg = NativeConfig.llama3("1b")
    lines += ["", f"## generate_batch, Llama-3 1B (random init), prompt {S0}, {N} new tokens, greedy, eager step", "",
              "| weights | B | cache bytes bf16 | cache bytes int8 | bf16 cache tok/s | int8 cache tok/s | int8 / bf16 |",
              "|---|---|---|---|---|---|---|"]
    base = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0)
    for wname in a.weights.split(","):
        gen = base if wname == "bf16" else mipipe.Generator.from_model(base.model, weights=wname)
        for B in (int(b) for b in a.batches.split(",")):
            rows = list(torch.randint(0, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(B)))
            res, nbytes = {}, {}
            for kv in ("bf16", "int8"):
                gen.kv_cache = kv
                nbytes[kv] = gen.new_cache(1, 1).nbytes * B * (S0 + N)
                gen.generate_batch(rows, N, graphs=False)                  # warm
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.e2e_windows):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    gen.generate_batch(rows, N, graphs=False)
                    e.record()
                    e.synchronize()
                    ts.append(s.elapsed_time(e) * 1e-3)
                res[kv] = B * N / statistics.median(ts)
                torch.cuda.empty_cache()
            gen.kv_cache = "bf16"
            print(json.dumps(dict(part="e2e", weights=wname, B=B, prompt=S0, new=N, bf16_tok_s=res["bf16"],
                                  int8_tok_s=res["int8"], cache_bytes=nbytes)), flush=True)
            lines.append(f"| {wname} | {B} | {nbytes['bf16'] / 2**20:.0f} MiB | {nbytes['int8'] / 2**20:.0f} MiB | "
                         f"{res['bf16']:.0f} | {res['int8']:.0f} | {res['int8'] / res['bf16']:.2f} |")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="decode,append,quant", help="comma-separated: decode, append, quant, e2e")
    ap.add_argument("--out", default="", help="also write the markdown report to this file")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per shape (the median is reported)")
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window (at least)")
    ap.add_argument("--batches", default="8,32", help="e2e: batch sizes")
    ap.add_argument("--weights", default="bf16,int8", help="e2e: weight formats")
    ap.add_argument("--prompt", type=int, default=4096)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--e2e-windows", type=int, default=3)
    a = ap.parse_args(argv)

    import torch
    import mipipe  # noqa: F401
    from mipipe import ops
    if not torch.cuda.is_available() or not ops.ext_available():
        print("kv8_time.py needs a GPU and the built HIP extension", file=sys.stderr)
        return 1
    lines = ["# int8 KV cache against the bf16 cache", "",
             f"Device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}).  Median of "
             f"{a.windows} windows of >= {a.calls} calls, each call on the next cache of a rotating set of >= 1 GiB; us "
             "= call-to-call time on one stream.  GB/s = the K and V bytes of the format (bf16: 2 B L Hkv D 2; int8: "
             "2 B L W) over that time; ceiling = 6.3 TB/s."]
    parts = dict(decode=part_decode, append=part_append, quant=part_quant, e2e=part_e2e)
    for p in a.parts.split(","):
        parts[p](a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
