"""Microbenchmark of the decode attention op (csrc/kernels/attention_decode.hip).

    python tools/decode_time.py [--out profiles/r8_attn_decode.md] [--sweep]

Times ``ops.attn_decode`` at B = 1, 8, 64 and L = 1024, 8192 cached keys for the GPT-2 small
(H 12, Hkv 12, D 64) and Llama-3 8B (H 32, Hkv 8, D 128) head layouts, and next to each row
the only way to compute the same thing without the kernel: ``ops.attn_fwd`` with ``Sq = 1``
on a contiguous token-major copy of the valid cache rows.

Method: every timed call reads a different cache out of a rotating set larger than the
256 MB Infinity Cache, so the figure is an HBM stream, not a cache replay.  After warm-up
runs of every shape, a window of calls is timed with device events (the time is the
call-to-call time on one stream: it includes the launch of the op's two kernels, which
dominates the small shapes); the table gives the median over the windows.  Bandwidth is the
K and V bytes the algorithm must read, 2 * B * L * Hkv * D * 2 bytes, over that time.
``--sweep`` adds forced split counts at B = 1, L = 8192 beside the planner's choice.
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = [("GPT-2 small", 12, 12, 64), ("Llama-3 8B", 32, 8, 128)]
BATCHES = (1, 8, 64)
LENGTHS = (1024, 8192)
ROTATE_BYTES = 1 << 30          # rotating working set: 4 x the Infinity Cache
HBM_CEILING = 6.3e12            # bytes/s, streaming ceiling of one MI355X


def _time(fn, n_rot, windows, min_calls):
    """Median per-call microseconds of ``fn(i)`` (i = rotating buffer index)."""
    import torch
    calls = max(min_calls, n_rot)
    for i in range(2 * n_rot if n_rot < 8 else n_rot):      # warm-up: code objects, allocator blocks, every buffer
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
    return statistics.median(per_call), min(per_call), max(per_call)


def bench_shape(name, H, Hkv, D, B, L, windows, min_calls, sweep):
    import torch
    from mipipe import ops
    dev = torch.device("cuda", 0)
    kv_bytes = 2 * B * L * Hkv * D * 2
    n_rot = max(2, min(512, math.ceil(ROTATE_BYTES / kv_bytes)))
    g = torch.Generator(device=dev).manual_seed(B * 131 + L)
    qkv = torch.randn(B, (H + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
    q = qkv[:, : H * D]
    caches = [(torch.randn(B, L, Hkv * D, device=dev, generator=g).to(torch.bfloat16),
               torch.randn(B, L, Hkv * D, device=dev, generator=g).to(torch.bfloat16)) for _ in range(n_rot)]
    lens = torch.full((B,), L, device=dev, dtype=torch.int32)
    o = torch.empty(B, H * D, device=dev, dtype=torch.bfloat16)
    o_ref = torch.empty_like(o)
    lse = torch.empty(B * H, device=dev, dtype=torch.float32)

    def decode(i, splits=0):
        ops.attn_decode(q, caches[i][0], caches[i][1], lens, o, H, Hkv, D, splits=splits)

    def baseline(i):
        # the cache of full sequences is already the token-major [B*L, Hkv*D] view attn_fwd wants
        ops.attn_fwd(q, caches[i][0].view(B * L, Hkv * D), caches[i][1].view(B * L, Hkv * D), o_ref, lse, B, 1, L, H,
                     Hkv, D, True)

    decode(0)
    baseline(0)
    torch.cuda.synchronize()
    diff = float((o.float() - o_ref.float()).abs().max())
    splits = ops.attn_decode_plan(B, Hkv, L)
    t_dec = _time(decode, n_rot, windows, min_calls)
    t_base = _time(baseline, n_rot, windows, min_calls)
    row = dict(layout=name, B=B, L=L, splits=splits, us=t_dec[0], us_min=t_dec[1], us_max=t_dec[2],
               gbps=kv_bytes / t_dec[0] / 1e3, base_us=t_base[0], base_gbps=kv_bytes / t_base[0] / 1e3,
               ratio=t_base[0] / t_dec[0], frac=kv_bytes / (t_dec[0] * 1e-6) / HBM_CEILING, diff=diff, n_rot=n_rot)
    extra = []
    if sweep:
        for s in sweep:
            if s != splits and s <= L:
                t = _time(lambda i, s=s: decode(i, s), n_rot, windows, min_calls)
                extra.append((s, t[0], kv_bytes / t[0] / 1e3))
    return row, extra


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="", help="also write the markdown report to this file")
    ap.add_argument("--windows", type=int, default=9, help="timed windows per shape (the median is reported)")
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window (at least)")
    ap.add_argument("--sweep", action="store_true", help="forced split counts at B = 1, L = 8192")
    a = ap.parse_args(argv)

    import torch
    import mipipe  # noqa: F401
    from mipipe import ops
    if not torch.cuda.is_available() or not ops.ext_available():
        print("decode_time.py needs a GPU and the built HIP extension", file=sys.stderr)
        return 1
    lines = ["# Decode attention: `ops.attn_decode` vs `ops.attn_fwd` at Sq = 1", "",
             f"Device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}).  bf16, full caches (lens = L), median of {a.windows} windows of "
             f">= {a.calls} calls,",
             "each call on the next cache of a rotating set of >= 1 GiB (n_rot caches).  us = call-to-call time on "
             "one stream",
             "(two launches per decode call).  GB/s = 2 * B * L * Hkv * D * 2 bytes / time.  ceiling = share of the "
             "6.3 TB/s",
             "HBM streaming ceiling.  baseline = `attn_fwd(Sq = 1, Sk = L)` on the same rows as one token-major view.",
             "max diff = largest absolute difference between the two outputs (bf16).", "",
             "| layout | B | L | splits | decode us (min - max) | decode GB/s | ceiling | baseline us | baseline GB/s | "
             "baseline / decode | max diff | n_rot |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    sweeps = []
    for name, H, Hkv, D in LAYOUTS:
        for B in BATCHES:
            for L in LENGTHS:
                sw = (4, 8, 16, 64, 128) if a.sweep and B == 1 and L == 8192 else ()
                r, extra = bench_shape(name, H, Hkv, D, B, L, a.windows, a.calls, sw)
                lines.append(f"| {r['layout']} | {r['B']} | {r['L']} | {r['splits']} | {r['us']:.1f} "
                             f"({r['us_min']:.1f} - {r['us_max']:.1f}) | {r['gbps']:.0f} | {100 * r['frac']:.1f} % | "
                             f"{r['base_us']:.1f} | {r['base_gbps']:.0f} | {r['ratio']:.2f}x | {r['diff']:.4f} | "
                             f"{r['n_rot']} |")
                print(lines[-1], flush=True)
                for s, us, gbps in extra:
                    sweeps.append(f"| {name} | {B} | {L} | {s} | {us:.1f} | {gbps:.0f} |")
    if sweeps:
        lines += ["", "Forced split counts (the planner's row is in the table above):", "",
                  "| layout | B | L | forced splits | decode us | decode GB/s |", "|---|---|---|---|---|---|"] + sweeps
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
