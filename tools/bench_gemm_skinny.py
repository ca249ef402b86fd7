#!/usr/bin/env python3
"""Decode GEMM microbenchmark: ops.gemm_skinny (csrc/gemm_skinny.hip) against torch.nn.functional.linear on the
projection shapes of a decode step, M = 1 / 16 / 64. Prints one JSON line.

Per call time from device events around `--iters` back-to-back calls, the two arms alternating, `--rounds` rounds,
the median round reported with the min-max spread. Every call reads a different copy of W out of a pool of at least
`--pool-mb` MB, so W comes from HBM and not from the 256 MB last-level cache. Bytes/s = 2 N K bytes over that time,
stated against the 8 TB/s HBM peak of the MI355X. For kernel times proper run this under
`rocprofv3 --kernel-trace --stats` (the kernels are gemm_skinny_kernel / gemm_skinny_reduce_kernel).

    python tools/bench_gemm_skinny.py [--models smollm3 llama8b] [--ms 1 16 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fine_tune_distributed_amd.ops import _ext  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = {  # name: (N, K)
    "smollm3": {"qkv": (3072, 2048), "o": (2048, 2048), "gate_up": (22016, 2048), "down": (2048, 11008),
                "lm_head": (128256, 2048)},
    "llama8b": {"o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)},
}


def time_arm(fn, ws, x, iters):
    for w in ws[:2]:
        fn(x, w)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(x, ws[i % len(ws)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(SHAPES))
    ap.add_argument("--ms", nargs="+", type=int, default=[1, 16, 64])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pool-mb", type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available() and _ext.load(), "needs the GPU and the built extension"
    skinny, blas = _ext.ops().gemm_skinny, torch.nn.functional.linear
    rows = []
    for model in args.models:
        for name, (N, K) in SHAPES[model].items():
            copies = max(2, -(-args.pool_mb * 2 ** 20 // (2 * N * K)))
            ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) for _ in range(copies)]
            for M in args.ms:
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
                t = {"skinny": [], "blas": []}
                for _ in range(args.rounds):
                    t["skinny"].append(time_arm(skinny, ws, x, args.iters))
                    t["blas"].append(time_arm(blas, ws, x, args.iters))
                row = {"model": model, "proj": name, "M": M, "N": N, "K": K}
                for arm, v in t.items():
                    med = statistics.median(v)
                    row[arm] = {"us": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                                "TBps": round(2 * N * K / med / 1e6, 3),
                                "of_hbm_peak": round(2 * N * K / med / 1e6 / (HBM_PEAK / 1e12), 3)}
                rows.append(row)
            del ws
    print(json.dumps({"bench": "gemm_skinny", "hbm_peak_TBps": HBM_PEAK / 1e12, "iters": args.iters,
                      "rounds": args.rounds, "rows": rows}))


if __name__ == "__main__":
    main()
