#!/usr/bin/env python3
"""The distillation loss kernel (csrc/distill.hip kd_fwd) at the bench shape, M = 8192 rows x V = 128256 bf16 logits
for the student and for the teacher, in its three instantiations (beta 0 forward KL, beta 1 reverse KL, beta 0.5
mixture), stats only and with the in-place bf16 gradient, next to ce_fwd on the same box; and the two kernels of
offline distillation (csrc/distill_topk.hip) in the same process: teacher_topk at each --topk K and kd_topk_fwd on its
output. Prints one JSON line: the median time per call and the rate of the bytes a call has to move at least once
(stats: the dense rows read; grad: the dense rows read, the student's written; teacher_topk: the row read).

SFTAMD_KD_INFLIGHT_MB / SFTAMD_KD_TOPK_INFLIGHT_MB (read once per process) set the rows-in-flight budget of kd_fwd's /
kd_topk_fwd's gradient launch, SFTAMD_TEACHER_TOPK_INFLIGHT_MB that of teacher_topk."""
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
    ap.add_argument("--topk", type=int, nargs="*", default=[64, 256], help="the K of teacher_topk / kd_topk_fwd")
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
           "inflight_mb": os.environ.get("SFTAMD_KD_INFLIGHT_MB", "default"),
           "topk_inflight_mb": os.environ.get("SFTAMD_KD_TOPK_INFLIGHT_MB", "default"),
           "teacher_topk_inflight_mb": os.environ.get("SFTAMD_TEACHER_TOPK_INFLIGHT_MB", "default")}
    cached = {}
    for k in a.topk:  # (the teacher's logits are only read: no restore between calls needed, timed() restores anyway)
        ms = timed(lambda: ops.teacher_topk(teacher, k, a.temperature))
        out[f"teacher_topk_k{k}"] = {"ms": round(ms, 4), "TB_s": round(row / ms / 1e9, 2)}
        cached[k] = ops.teacher_topk(teacher, k, a.temperature)
    for write_grad in (False, True):
        key = "grad" if write_grad else "stats"
        ms = timed(lambda: ops.ce_fwd(work, labels, inv, write_grad))
        out[f"ce_{key}"] = {"ms": round(ms, 4), "TB_s": round(row * (2 if write_grad else 1) / ms / 1e9, 2)}
        for name, beta in (("fkl", 0.0), ("rkl", 1.0), ("mix", 0.5)):
            ms = timed(lambda: ops.kd_fwd(work, teacher, labels, inv, write_grad, beta, a.temperature))
            out[f"kd_{name}_{key}"] = {"ms": round(ms, 4), "TB_s": round(row * (3 if write_grad else 2) / ms / 1e9, 2)}
        for k, (ids, lps) in cached.items():
            ms = timed(lambda: ops.kd_topk_fwd(work, ids, lps, labels, inv, write_grad, a.temperature))
            out[f"kd_topk_k{k}_{key}"] = {"ms": round(ms, 4), "TB_s": round(row * (2 if write_grad else 1) / ms / 1e9, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
