"""Timings of multi-token append attention and of what is built on it.

    python tools/extend_time.py [--out profiles/r11_attn_append.md] [--parts op,prefill,extend,spec]

Four tables, each a median over timed windows after a warm-up of every variant:

``op``       ``ops.attn_append`` (csrc/kernels/attention_append.hip) at T = 1, 4, 8, 16, 64 new
             tokens over L cached keys against T calls of ``ops.attn_decode`` on the same
             cache, for the GPT-2 small (H 12, Hkv 12, D 64) and Llama-3 8B (H 32, Hkv 8,
             D 128) head layouts.  As in decode_time.py every timed call reads the next cache
             of a rotating set larger than the 256 MB Infinity Cache, and the time is the
             call-to-call time on one stream measured with device events.
``prefill``  ``attn_append`` with T = S on an empty cache against ``ops.attn_fwd`` (causal,
             Sq = Sk = S): the same result from the training forward kernel.
``extend``   ``Generator.extend`` of T tokens against T ``Generator.decode`` steps over a
             prefix of cached tokens, for the two models generate_time.py uses.  A window is
             the call(s) plus a synchronise, on a cache rolled back before every window.
``spec``     tokens/s of ``generate_speculative`` with the target as its own draft (the upper
             bound on acceptance, at the price of a draft as slow as the target) against
             ``generate_batch``, greedy.

Needs a GPU and the built extension: there is no fallback.
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = [("GPT-2 small", 12, 12, 64), ("Llama-3 8B", 32, 8, 128)]
TOKENS = (1, 4, 8, 16, 64)
ROTATE_BYTES = 1 << 30          # rotating working set: 4 x the Infinity Cache


def _time_events(fn, n_rot, windows, calls):
    """Median per-call microseconds of ``fn(i)`` (i = rotating buffer index)."""
    import torch
    calls = max(calls, n_rot)
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


def _time_sync(fn, windows, reset=None):
    """Median seconds of ``fn()`` + synchronise (``reset()`` runs untimed before every window)."""
    import torch
    out = []
    for i in range(windows + 2):                     # two warm-up windows
        if reset is not None:
            reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(time.perf_counter() - t0)
    return statistics.median(out)


def part_op(a, lines):
    import torch
    from mipipe import ops
    dev = torch.device("cuda", 0)
    lines += ["## `attn_append` against T calls of `attn_decode`", "",
              f"bf16, median of {a.windows} windows of >= {a.calls} calls, each call on the next cache of a rotating "
              "set of >= 1 GiB.  us = call-to-call time on one stream (append: two launches; decode: two launches "
              "per token).  base = L - T cached keys before the call; the decode calls each read L keys.  GB/s = "
              "2 * B * L * Hkv * D * 2 bytes over the append time.  max diff = largest absolute difference between "
              "the append output's last token and `attn_decode` over the same L keys.", "",
              "| layout | B | L | T | splits | append us | append GB/s | T x decode us | decode / append | max diff |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for name, H, Hkv, D in LAYOUTS:
        for B, L in ((1, 4096), (8, 4096), (1, 8192)):
            kv_bytes = 2 * B * L * Hkv * D * 2
            n_rot = max(2, min(256, math.ceil(ROTATE_BYTES / kv_bytes)))
            g = torch.Generator(device=dev).manual_seed(B * 131 + L)
            caches = [(torch.randn(B, L, Hkv * D, device=dev, generator=g).to(torch.bfloat16),
                       torch.randn(B, L, Hkv * D, device=dev, generator=g).to(torch.bfloat16)) for _ in range(n_rot)]
            lens = torch.full((B,), L, device=dev, dtype=torch.int32)
            for T in TOKENS:
                qkv = torch.randn(B * T, (H + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
                q = qkv[:, : H * D]
                q1 = qkv.view(B, T, -1)[:, -1, : H * D]               # each sequence's last token
                base = torch.full((B,), L - T, device=dev, dtype=torch.int32)
                o = torch.empty(B * T, H * D, device=dev, dtype=torch.bfloat16)
                o1 = torch.empty(B, H * D, device=dev, dtype=torch.bfloat16)

                def append(i):
                    ops.attn_append(q, caches[i][0], caches[i][1], base, None, o, T, H, Hkv, D)

                def decodes(i):
                    for _ in range(T):
                        ops.attn_decode(q1, caches[i][0], caches[i][1], lens, o1, H, Hkv, D)

                append(0)
                decodes(0)
                torch.cuda.synchronize()
                diff = float((o.view(B, T, -1)[:, -1].float() - o1.float()).abs().max())
                t_app = _time_events(append, n_rot, a.windows, a.calls)
                t_dec = _time_events(decodes, n_rot, a.windows, max(8, a.calls // T))
                lines.append(f"| {name} | {B} | {L} | {T} | {ops.attn_append_plan(B, T, Hkv, H // Hkv, L)} | "
                             f"{t_app:.1f} | {kv_bytes / t_app / 1e3:.0f} | {t_dec:.1f} | {t_dec / t_app:.2f}x | "
                             f"{diff:.4f} |")
                print(lines[-1], flush=True)
            del caches
            torch.cuda.empty_cache()
    lines.append("")


def part_prefill(a, lines):
    import torch
    from mipipe import ops
    dev = torch.device("cuda", 0)
    lines += ["## `attn_append` with T = S on an empty cache against `attn_fwd`", "",
              f"B = 1, causal, bf16, median of {a.windows} windows of >= {a.calls} calls on one buffer (the inputs "
              "stay in cache for both).", "",
              "| layout | S | splits | append us | attn_fwd us | append / attn_fwd | max diff |", "|---|---|---|---|---|---|---|"]
    for name, H, Hkv, D in LAYOUTS:
        for S in (512, 2048):
            g = torch.Generator(device=dev).manual_seed(S)
            qkv = torch.randn(S, (H + 2 * Hkv) * D, device=dev, generator=g).to(torch.bfloat16)
            q, k, v = qkv[:, : H * D], qkv[:, H * D:(H + Hkv) * D], qkv[:, (H + Hkv) * D:]
            kc, vc = k.contiguous().view(1, S, -1), v.contiguous().view(1, S, -1)
            base = torch.zeros(1, device=dev, dtype=torch.int32)
            o = torch.empty(S, H * D, device=dev, dtype=torch.bfloat16)
            o2 = torch.empty_like(o)
            lse = torch.empty(H * S, device=dev, dtype=torch.float32)
            app = lambda i: ops.attn_append(q, kc, vc, base, None, o, S, H, Hkv, D)            # noqa: E731
            fwd = lambda i: ops.attn_fwd(q, k, v, o2, lse, 1, S, S, H, Hkv, D, True)           # noqa: E731
            app(0)
            fwd(0)
            torch.cuda.synchronize()
            diff = float((o.float() - o2.float()).abs().max())
            t_app, t_fwd = _time_events(app, 1, a.windows, a.calls), _time_events(fwd, 1, a.windows, a.calls)
            lines.append(f"| {name} | {S} | {ops.attn_append_plan(1, S, Hkv, H // Hkv, S)} | {t_app:.1f} | {t_fwd:.1f} | "
                         f"{t_app / t_fwd:.2f}x | {diff:.4f} |")
            print(lines[-1], flush=True)
    lines.append("")


def _config(name):
    from mipipe.models.config import NativeConfig
    if name == "gpt2-small":
        return NativeConfig.gpt2("small")
    if name == "llama3-1b":
        return NativeConfig.llama3("1b", max_seq_len=1024)
    raise ValueError(name)


def part_extend(a, lines):
    import torch
    import mipipe
    dev = torch.device("cuda", 0)
    P = 512
    lines += ["## `Generator.extend(T)` against T `Generator.decode` steps", "",
              f"B = 1, a prefix of {P} cached tokens, bf16; a window is the call(s) and a synchronise on a cache "
              f"rolled back to the prefix; median of {a.windows} windows after two warm-up windows.", "",
              "| model | T | extend ms | T x decode ms | decode / extend |", "|---|---|---|---|---|"]
    for mname in ("gpt2-small", "llama3-1b"):
        cfg = _config(mname)
        gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0)
        tokens = torch.randint(0, cfg.vocab_size, (1, P + 64), generator=torch.Generator().manual_seed(1)).to(dev)
        cache = gen.new_cache(1, P + 64)
        gen.prefill(tokens[:, :P], cache, lens=[P])

        def reset():
            cache.truncate([P])

        for T in (4, 8, 16, 64):
            new = tokens[:, P:P + T]

            def steps():
                for t in range(T):
                    gen.decode(new[:, t], cache)

            t_ext = _time_sync(lambda: gen.extend(new, cache), a.windows, reset)
            t_dec = _time_sync(steps, a.windows, reset)
            lines.append(f"| {mname} | {T} | {t_ext * 1e3:.2f} | {t_dec * 1e3:.2f} | {t_dec / t_ext:.2f}x |")
            print(lines[-1], flush=True)
        del gen, cache
        torch.cuda.empty_cache()
    lines.append("")


def part_spec(a, lines):
    import torch
    import mipipe
    dev = torch.device("cuda", 0)
    S0, N, K = 128, 128, 4
    lines += ["## `generate_speculative` (target as its own draft) against `generate_batch`", "",
              f"Greedy, prompt {S0}, {N} new tokens, lookahead {K}, bf16; a window is one whole call and a "
              f"synchronise; tokens/s = B * {N} / median of {a.windows} windows after two warm-up windows.  With the "
              "target as its own draft every draft is accepted in exact arithmetic (in bf16 the one-row and T-row "
              "GEMMs can round a near-tie differently), but a drafted token costs a full decode step: the "
              "ratio shows the overhead of the round, not the gain of a small draft.", "",
              "| model | B | generate_batch tok/s | speculative tok/s | speculative / batch | rounds | accepted / drafted | "
              "same tokens |", "|---|---|---|---|---|---|---|---|"]
    for mname in ("gpt2-small", "llama3-1b"):
        cfg = _config(mname)
        gen = mipipe.Generator(cfg, dev, dtype=torch.bfloat16, seed=0)
        for B in (1, 8):
            rows = list(torch.randint(0, cfg.vocab_size, (B, S0), generator=torch.Generator().manual_seed(B)))
            ref = gen.generate_batch(rows, N)[0]
            out, _, stats = gen.generate_speculative(rows, N, gen, lookahead=K)
            t_b = _time_sync(lambda: gen.generate_batch(rows, N), a.windows)
            t_s = _time_sync(lambda: gen.generate_speculative(rows, N, gen, lookahead=K), a.windows)
            lines.append(f"| {mname} | {B} | {B * N / t_b:.1f} | {B * N / t_s:.1f} | {t_b / t_s:.2f}x | {stats['rounds']} | "
                         f"{stats['accepted']} / {stats['drafted']} | {bool(torch.equal(ref, out))} |")
            print(lines[-1], flush=True)
        del gen
        torch.cuda.empty_cache()
    lines.append("")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="", help="also write the markdown report to this file")
    ap.add_argument("--parts", default="op,prefill,extend,spec")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per row (the median is reported)")
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window of the op tables (at least)")
    a = ap.parse_args(argv)

    import torch
    import mipipe  # noqa: F401
    from mipipe import ops
    if not torch.cuda.is_available() or not ops.ext_available():
        print("extend_time.py needs a GPU and the built HIP extension", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    lines = ["# Append attention, `Generator.extend` and speculative decoding", "",
             f"Device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}).  "
             f"Command: `python tools/extend_time.py --parts {a.parts} --windows {a.windows} --calls {a.calls}`.  "
             "Every figure is a median of repeated windows inside this one process.", ""]
    parts = {"op": part_op, "prefill": part_prefill, "extend": part_extend, "spec": part_spec}
    for p in a.parts.split(","):
        parts[p](a, lines)
        if a.out:                                    # keep what is done if a later part is cut short
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
