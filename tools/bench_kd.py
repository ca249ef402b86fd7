#!/usr/bin/env python3
"""The distillation loss kernel (csrc/distill.hip kd_fwd) at the bench shape, M = 8192 rows x V = 128256 bf16 logits
for the student and for the teacher, in its three instantiations (beta 0 forward KL, beta 1 reverse KL, beta 0.5
mixture), stats only and with the in-place bf16 gradient, next to ce_fwd on the same box. Prints one JSON line: the
median time per call and the rate of the bytes a call has to move at least once (stats: both rows read; grad: both
rows read, the student's written).

SFTAMD_KD_INFLIGHT_MB (read once per process) sets the rows-in-flight budget of the gradient launch."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_fine_tune_distributed_amd.ops import _ext  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=0.9)
    a = ap.parse_args()
    assert _ext.load(), _ext.load_error()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    base = (torch.randn(a.rows, a.vocab, device=dev, generator=g) * 2).to(torch.bfloat16)
    teacher = (torch.randn(a.rows, a.vocab, device=dev, generator=g) * 2).to(torch.bfloat16)
    labels = torch.randint(0, a.vocab, (a.rows,), device=dev, generator=g)
    inv = torch.tensor([1.0 / a.rows], device=dev)
    work = base.clone()
    ops = _ext.ops()

    def timed(fn):
        for _ in range(3):
            work.copy_(base)
            fn()
        ts = []
        for _ in range(a.iters):
            work.copy_(base)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
        return sorted(ts)[len(ts) // 2]

    row = a.rows * a.vocab * 2
    out = {"rows": a.rows, "vocab": a.vocab, "iters": a.iters,
           "inflight_mb": os.environ.get("SFTAMD_KD_INFLIGHT_MB", "default")}
    for write_grad in (False, True):
        key = "grad" if write_grad else "stats"
        ms = timed(lambda: ops.ce_fwd(work, labels, inv, write_grad))
        out[f"ce_{key}"] = {"ms": round(ms, 4), "TB_s": round(row * (2 if write_grad else 1) / ms / 1e9, 2)}
        for name, beta in (("fkl", 0.0), ("rkl", 1.0), ("mix", 0.5)):
            ms = timed(lambda: ops.kd_fwd(work, teacher, labels, inv, write_grad, beta, a.temperature))
            out[f"kd_{name}_{key}"] = {"ms": round(ms, 4), "TB_s": round(row * (3 if write_grad else 2) / ms / 1e9, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
