"""Time of the document-masked attention kernels (attention_doc.hip), forward and backward,
against the plain causal kernels on the same tensors.

    python tools/attn_doc_time.py [--rounds 3] [--out FILE.md]

Two shapes: B 64, S 1024, H 12, D 64 (GPT-2 small microbatch) and B 2, S 8192, H 32, Hkv 8,
D 128 (Llama-3 8B).  Three layouts each: one document per row, and fixed-seed boundaries with a
mean document length of S/4 and of S/16 (every position starts a document with probability
1/mean).  ``sum len^2 / S^2`` is the share of the causal score matrix the documents keep: the
time is expected to follow it.

The causal baselines run twice: with the default dispatch (v2 / v3 kernels at d_h 64) in this
process, and the v1 kernels (MIPIPE_ATTN_FWD=1 MIPIPE_ATTN_BWD_DQ=1 MIPIPE_ATTN_BWD_DKDV=1,
read once per process) in a child process, so the cost of leaving the v2 / v3 path is apart
from the cost of the mask.  Every figure is the median of ``--rounds`` rounds that alternate
all variants; one round times 20 launches replayed from one HIP graph, three times.  Needs a
GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import mipipe  # noqa: E402,F401
from mipipe import ops  # noqa: E402
from tools.gemm_epi_probe import timed  # noqa: E402

SHAPES = [(64, 1024, 12, 12, 64), (2, 8192, 32, 8, 128)]
V1_ENV = {"MIPIPE_ATTN_FWD": "1", "MIPIPE_ATTN_BWD_DQ": "1", "MIPIPE_ATTN_BWD_DKDV": "1"}


def layout(B, S, mean, seed=0):
    """(doc_start, doc_end, sum len^2 / S^2) for B rows; mean None: one document per row."""
    g = torch.Generator().manual_seed(seed)
    start = torch.zeros(B, S, dtype=torch.bool)
    if mean is not None:
        start = torch.rand(B, S, generator=g) < 1.0 / mean
    start[:, 0] = True
    pos = torch.arange(S)[None, :].expand(B, S)
    ds = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 1).values
    end = torch.ones(B, S, dtype=torch.bool)
    end[:, :-1] = start[:, 1:]
    de = torch.cummin(torch.where(end, pos, torch.full_like(pos, S - 1)).flip(1), 1).values.flip(1)
    share = float(((de - ds + 1).double().sum(1) / S / S).mean())   # sum over tokens of len = sum len^2
    return ds.reshape(-1).int().cuda(), de.reshape(-1).int().cuda(), share


def tensors(B, S, H, Hkv, D):
    T = B * S
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(T, (H + 2 * Hkv) * D, device="cuda", generator=g).to(torch.bfloat16)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:(H + Hkv) * D], qkv[:, (H + Hkv) * D:]
    o = torch.empty(T, H * D, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B * H * S, device="cuda")
    do = torch.randn(T, H * D, device="cuda", generator=g).to(torch.bfloat16)
    d = torch.empty_like(qkv)
    return q, k, v, o, lse, do, (d[:, :H * D], d[:, H * D:(H + Hkv) * D], d[:, (H + Hkv) * D:])


def variants(shape, with_docs):
    B, S, H, Hkv, D = shape
    q, k, v, o, lse, do, (dq, dk, dv) = tensors(*shape)
    out = {}

    def add(name, ds, de):
        kw = {} if ds is None else dict(doc_start=ds)
        kb = {} if ds is None else dict(doc_start=ds, doc_end=de)
        fwd = lambda: ops.attn_fwd(q, k, v, o, lse, B, S, S, H, Hkv, D, True, **kw)   # noqa: E731
        bwd = lambda: ops.attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, S, S, H, Hkv, D, True, **kb)   # noqa: E731
        out[name] = (fwd, bwd)

    add("causal", None, None)
    shares = {"causal": 1.0}
    if with_docs:
        for name, mean in (("doc 1/row", None), ("doc S/4", S // 4), ("doc S/16", S // 16)):
            ds, de, share = layout(B, S, mean)
            add(name, ds, de)
            shares[name] = share
    return out, shares


def measure(shape, with_docs, rounds):
    var, shares = variants(shape, with_docs)
    tf = {n: [] for n in var}
    tb = {n: [] for n in var}
    for _ in range(rounds):            # alternate the variants inside every round
        for n, (fwd, bwd) in var.items():
            fwd()                      # the backward reads this variant's o / lse
            tf[n].append(timed(fwd, True))
            tb[n].append(timed(bwd, True))
    return {n: dict(share=shares[n], fwd_us=statistics.median(tf[n]), bwd_us=statistics.median(tb[n]),
                    fwd_spread=max(tf[n]) - min(tf[n]), bwd_spread=max(tb[n]) - min(tb[n])) for n in var}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    ap.add_argument("--causal-only", action="store_true", help="(child) causal baselines only, JSON on stdout")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_doc_time: needs a GPU")
    if a.causal_only:
        print(json.dumps([measure(s, False, a.rounds) for s in SHAPES]))
        return
    res = [measure(s, True, a.rounds) for s in SHAPES]
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--causal-only", "--rounds", str(a.rounds)],
                           capture_output=True, text=True, env=dict(os.environ, **V1_ENV), timeout=600)
    if child.returncode != 0:
        raise SystemExit("v1 baseline run failed:\n" + child.stderr[-2000:])
    v1 = json.loads(child.stdout.strip().splitlines()[-1])
    lines = ["| shape (B, S, H, Hkv, D) | variant | sum len^2 / S^2 | fwd us | bwd us | fwd / causal v1 | bwd / causal v1 |",
             "|---|---|---|---|---|---|---|"]
    for shape, r, r1 in zip(SHAPES, res, v1):
        rows = [("causal, default dispatch", r["causal"]), ("causal, v1 kernels", r1["causal"])]
        rows += [(n, x) for n, x in r.items() if n != "causal"]
        base = r1["causal"]
        for n, x in rows:
            lines.append(f"| {shape} | {n} | {x['share']:.3f} | {x['fwd_us']:.1f} (+-{x['fwd_spread'] / 2:.1f}) | "
                         f"{x['bwd_us']:.1f} (+-{x['bwd_spread'] / 2:.1f}) | {x['fwd_us'] / base['fwd_us']:.3f} | "
                         f"{x['bwd_us'] / base['bwd_us']:.3f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
