#!/usr/bin/env python3
"""What the SFT objectives cost at the bench shapes: ce_fwd (csrc/cross_entropy.hip) at 8192 x 128256 with the gradient
written, in plain, label-smoothing and dft modes, and embedding_noise_fwd against embedding_fwd (csrc/elementwise.hip)
at 8192 x 2048. Every step is a child process of its own under ``timeout``; the first one that fails ends the run.
Prints one JSON line per step (median ms per call, HBM rate). ``--steps ce_plain,emb_plain`` runs on a build without
the objectives (SFTAMD_LIB=<that build's _C.so>), for the A/B of the untouched paths."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["ce_plain", "ce_smooth", "ce_dft", "emb_plain", "emb_noise"]


def _median_ms(fn, iters, before=None):
    import torch
    ts = []
    for i in range(iters + 3):
        if before is not None:
            before()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if i >= 3:  # three warm-up calls
            ts.append(s.elapsed_time(e))
    return sorted(ts)[len(ts) // 2]


def run_step(step, a):
    import torch
    sys.path.insert(0, ROOT)
    from llm_fine_tune_distributed_amd.ops import _ext
    assert _ext.load(), _ext.load_error()
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    if step.startswith("ce_"):
        base = (torch.randn(a.rows, a.vocab, device=dev, generator=g) * 2).to(torch.bfloat16)
        labels = torch.randint(0, a.vocab, (a.rows,), device=dev, generator=g)
        inv = torch.tensor([1.0 / a.rows], device=dev)
        work = base.clone()
        extra = {"ce_plain": (), "ce_smooth": (0.1, 0), "ce_dft": (0.0, 1)}[step]
        ms = _median_ms(lambda: ops.ce_fwd(work, labels, inv, True, *extra), a.iters, lambda: work.copy_(base))
        nbytes = a.rows * a.vocab * 2 * 3  # two reads and one write of the logits
    else:
        w = torch.randn(a.vocab, a.hidden, device=dev, generator=g).to(torch.bfloat16)
        ids = torch.randint(0, a.vocab, (a.rows,), device=dev, generator=g)
        mag = torch.full((a.rows,), 5.0 / (512 * a.hidden) ** 0.5, device=dev)
        fn = (lambda: ops.embedding_fwd(ids, w)) if step == "emb_plain" else \
            (lambda: ops.embedding_noise_fwd(ids, w, mag, 12345))
        ms = _median_ms(fn, a.iters)
        nbytes = a.rows * a.hidden * 2 * 2  # one read and one write of the rows
    print(json.dumps({"step": step, "ms": round(ms, 4), "TB_s": round(nbytes / ms / 1e9, 3), "lib": _ext.lib_path()}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds per step")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_step(a.child, a)
    for step in a.steps.split(","):
        if step not in STEPS:
            raise SystemExit(f"unknown step {step!r}: one of {STEPS}")
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", step,
               "--rows", str(a.rows), "--vocab", str(a.vocab), "--hidden", str(a.hidden), "--iters", str(a.iters)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
            raise SystemExit(f"step {step} ended with status {rc}")


if __name__ == "__main__":
    main()
