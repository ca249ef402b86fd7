#!/usr/bin/env python3
"""Micro-benchmark of the flash-attention kernels (causal forward and backward, the backward with its delta kernel).

    python tools/bench_attention.py                                   # head_dim 64, 32q/8kv against 128, 16q/4kv
    python tools/bench_attention.py --seqs 4 --len 4096
    python tools/bench_attention.py --head-dim 128 --heads 16 --kv-heads 4 --ds-mb "" 0   # the two head_dim-128 dQ paths

--head-dim / --heads / --kv-heads take one value per configuration (a single value is shared), --ds-mb one
SFTAMD_ATTN_DS_MB setting per configuration ("" = the default budget, 0 = the recomputing dQ; head_dim 128 only). The
configurations alternate in one process, --rounds times; every shape is warmed up before its timed window; a time is
the median over the rounds of the median of --calls device-event timings. FLOP/s are computed from the shapes: the
causal forward is 4 nq L^2 d / 2 per sequence (QK^T and PV), the backward 2.5 x that (its five products; what a kernel
recomputes is not counted). --ragged draws the recipe's padding-free lengths (553..754) instead of --len."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(torch, fn, calls):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--head-dim", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--heads", type=int, nargs="+", default=[32, 16])
    ap.add_argument("--kv-heads", type=int, nargs="+", default=[8, 4])
    ap.add_argument("--ds-mb", nargs="+", default=[""])
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--len", type=int, default=512)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    n = max(len(args.head_dim), len(args.heads), len(args.kv_heads), len(args.ds_mb))
    cols = [v * n if len(v) == 1 else v for v in (args.head_dim, args.heads, args.kv_heads, args.ds_mb)]
    assert all(len(v) == n for v in cols), "one value per configuration, or a single shared one"
    assert args.calls >= 20, "the median of at least 20 calls"

    import torch
    from llm_fine_tune_distributed_amd.ops import _ext
    assert torch.cuda.is_available(), "bench_attention needs a GPU"
    assert _ext.load(), _ext.load_error()
    ops = _ext.ops()
    lens = [args.len] * args.seqs
    if args.ragged:
        lens = torch.randint(553, 755, (args.seqs,), generator=torch.Generator().manual_seed(0)).tolist()
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
    M, L = sum(lens), max(lens)
    cfgs = []
    for d, nq, nkv, ds in zip(*cols):
        g = torch.Generator(device="cuda").manual_seed(0)
        cfgs.append(dict(d=d, nq=nq, nkv=nkv, ds=ds, sc=1 / math.sqrt(d),
                         qkv=torch.randn(M, (nq + 2 * nkv) * d, device="cuda", generator=g).to(torch.bfloat16),
                         dout=torch.randn(M, nq * d, device="cuda", generator=g).to(torch.bfloat16),
                         flops=sum(4.0 * nq * l * l * d / 2 for l in lens), t=[]))
    for _ in range(args.rounds):
        for c in cfgs:
            os.environ["SFTAMD_ATTN_DS_MB"] = c["ds"]
            a = (c["qkv"], cu, L, c["nq"], c["nkv"], c["d"], c["sc"], True)
            out, lse = ops.flash_fwd(*a)
            tf = timeit(torch, lambda: ops.flash_fwd(*a), args.calls)
            tb = timeit(torch, lambda: ops.flash_bwd(c["dout"], c["qkv"], out, lse, *a[1:]), args.calls)
            c["t"].append((tf, tb))
    rows = []
    for c in cfgs:
        tf, tb = (statistics.median(x[i] for x in c["t"]) for i in (0, 1))
        rows.append(dict(head_dim=c["d"], heads=c["nq"], kv_heads=c["nkv"], ds_mb=c["ds"], seqs=args.seqs, max_len=L,
                         tokens=M, fwd_us=round(tf * 1e3, 1), bwd_us=round(tb * 1e3, 1),
                         fwd_tflops=round(c["flops"] / tf / 1e9, 1), bwd_tflops=round(2.5 * c["flops"] / tb / 1e9, 1)))
        print(json.dumps(rows[-1]))
    for r in rows[1:]:
        print(f"ratio of configuration 1 to head_dim {r['head_dim']} {r['heads']}q/{r['kv_heads']}kv: "
              f"fwd {rows[0]['fwd_us'] / r['fwd_us']:.2f}, bwd {rows[0]['bwd_us'] / r['bwd_us']:.2f}")


if __name__ == "__main__":
    main()
