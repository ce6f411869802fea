"""A layer's four weight-gradient GEMMs at the GPT-2 small shapes: the per-GEMM split-K plan
(four dW launches + four reduce launches) plus the QKV bias column sum, against ONE grouped
256x256 launch (gemm3_tt_grouped_kernel, + one reduce launch) at each split factor, every
arm replayed from one HIP graph of 20 repetitions.

    python tools/gemm_dw_group_probe.py [--tokens 65536,16384] [--splits 1,2,4,7,9]

--arm single | grouped runs one arm only (results: profiles/r7_dw_group.md)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mipipe  # noqa: E402,F401
from mipipe.ops import kernels as K_  # noqa: E402
from tools.gemm_epi_probe import timed  # noqa: E402

SHAPES = (("qkv", 2304, 768), ("out-proj", 768, 768), ("fc1", 3072, 768), ("fc2", 768, 3072))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="65536,16384")
    ap.add_argument("--splits", default="1,2,4,7,9")
    ap.add_argument("--arm", default="both", choices=["both", "single", "grouped"])
    a = ap.parse_args()
    e = K_._ext()
    out = {}
    for T in (int(t) for t in a.tokens.split(",")):
        dys = [torch.randn(T, n, device="cuda", dtype=torch.bfloat16) for _, n, _ in SHAPES]
        xs = [torch.randn(T, k, device="cuda", dtype=torch.bfloat16) * T ** -0.5 for _, _, k in SHAPES]
        dws = [torch.zeros(n, k, device="cuda", dtype=torch.float32) for _, n, k in SHAPES]
        db = torch.zeros(SHAPES[0][1], device="cuda", dtype=torch.float32)
        flop = sum(2 * T * n * k for _, n, k in SHAPES)
        row = {}

        def single():
            for dy, x, dw in zip(dys, xs, dws):
                K_.linear_dw(dy, x, dw)

        if a.arm in ("both", "single"):
            row["single"] = timed(single, True)
            row["colsum"] = timed(lambda: K_.colsum(dys[0], db), True)
        if a.arm in ("both", "grouped"):
            for s in (int(s) for s in a.splits.split(",")):
                row[f"grouped_S{s}"] = timed(lambda: e.gemm_dw_grouped(dys, xs, dws, 1.0, s), True)
        for k, us in row.items():
            tf = "" if k == "colsum" else f"  {flop / us / 1e6:7.1f} TF"
            print(f"T={T:6d} {k:12s} {us:9.1f} us{tf}", flush=True)
        out[T] = {k: round(v, 1) for k, v in row.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
