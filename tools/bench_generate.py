#!/usr/bin/env python3
"""Decode throughput of batched generation against sequential generation (SmolLM3-3B, random weights).

    python tools/bench_generate.py [--batches 1 4 16 64] [--reps 3] [--out table.md]

For every batch size B two arms are timed, alternating, each as a fresh child process under its own ``timeout``:
``seq`` runs B sequential ``generate`` calls, ``batch`` one ``generate_batch`` of B. Prompt 128 tokens, 128 new
tokens, greedy (no sampling, no repetition penalty), no EOS, so both arms produce exactly B * 128 tokens. Each
child builds the model, warms the timed shape up once (kernels, library algorithm choice, graph capture path) and
reports a host-clock time around a call that ends in a device-to-host read of the tokens.

    python tools/bench_generate.py --arm batch --batch 16          # one arm, one JSON line (what the children run)
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/bench_generate.py --arm batch --batch 16
    python tools/bench_generate.py --kernel-split DIR/.../*_kernel_trace.csv   # GEMMs / attention / sampler per step
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PROMPT, NEW = 128, 128


def run_arm(arm: str, B: int, reps: int) -> dict:
    import torch
    from llm_fine_tune_distributed_amd.inference.generation import generate, generate_batch
    from llm_fine_tune_distributed_amd.models import build_model, smollm3_3b
    from llm_fine_tune_distributed_amd.ops import _ext
    assert torch.cuda.is_available(), "bench_generate needs a GPU"
    assert _ext.load(), _ext.load_error()
    cfg = smollm3_3b()
    model = build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=0)
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (PROMPT,), generator=g).tolist() for _ in range(B)]
    kw = dict(max_new_tokens=NEW, do_sample=False, repetition_penalty=1.0, eos_token_id=None)

    def once():
        if arm == "seq":
            return [generate(model, p, **kw) for p in prompts]
        return generate_batch(model, prompts, **kw)

    # warm-up of the timed shapes: one call (every sequential call has the same shapes, so one of them is enough)
    out = [generate(model, prompts[0], **kw)] if arm == "seq" else once()
    assert all(len(o) == NEW for o in out)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        once()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    best = min(times)
    return {"arm": arm, "batch": B, "new_tokens": B * NEW, "seconds": times, "tokens_per_s": B * NEW / best,
            "device": torch.cuda.get_device_name(0), "layers": cfg.num_hidden_layers}


def kernel_split(path: str) -> str:
    """Per decode step kernel time of one traced ``--arm batch`` run, by class. The window is the span of the batched
    sampler's merge kernel: one dispatch per decode step (graph replays included)."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[1])
    marks = [i for i, r in enumerate(rows) if "final_batched_kernel" in r[0]]
    assert len(marks) > NEW, "no batched decode steps in this trace"
    # the last NEW - 1 steps are the timed call's decode steps (the first token comes from the prefill logits)
    lo, hi = marks[-NEW], marks[-1]
    steps = NEW - 1
    cls = {"GEMMs": 0.0, "decode attention": 0.0, "sampler": 0.0, "other": 0.0}
    names = {}
    for n, s, e in rows[lo + 1:hi + 1]:
        us = (e - s) / 1e3
        if "Cijk" in n or "gemm" in n.lower() or "gemv" in n.lower():
            k = "GEMMs"
        elif "decode::" in n:
            k = "decode attention"
        elif "samp::" in n:
            k = "sampler"
        else:
            k = "other"
        cls[k] += us
        names[n] = names.get(n, 0.0) + us
    total = sum(cls.values())
    span = (rows[hi][2] - rows[lo][2]) / 1e3
    lines = [f"{steps} decode steps, {total / steps:.1f} us of kernel time per step, {span / steps:.1f} us wall per step",
             "", "| class | us / step | % of kernel time |", "|---|---:|---:|"]
    for k, v in cls.items():
        lines.append(f"| {k} | {v / steps:.1f} | {100 * v / total:.1f} |")
    lines += ["", "Largest kernels of the window:", "", "| kernel | us / step |", "|---|---:|"]
    for n, v in sorted(names.items(), key=lambda kv: -kv[1])[:8]:
        lines.append(f"| `{n.split('(')[0][:90]}` | {v / steps:.1f} |")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--arm", choices=["seq", "batch"], help="run one arm in this process and print one JSON line")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=1, help="timed repetitions per arm (best is reported)")
    ap.add_argument("--arm-timeout", type=int, default=300, help="seconds each arm's child may take")
    ap.add_argument("--out", help="write the table as markdown")
    ap.add_argument("--kernel-split", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args(argv)
    if a.kernel_split:
        print(kernel_split(a.kernel_split))
        return
    if a.arm:
        print(json.dumps(run_arm(a.arm, a.batch, a.reps)))
        return
    results = {}
    for B in a.batches:
        for arm in ("seq", "batch"):  # alternate the arms: neighbours in time share the box's condition
            cmd = ["timeout", "-k", "10", str(a.arm_timeout), sys.executable, os.path.abspath(__file__), "--arm", arm,
                   "--batch", str(B), "--reps", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:  # a fault, an abort or the time limit: start nothing more on this GPU
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"arm {arm} B={B} ended with status {r.returncode}")
            results[(B, arm)] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(results[(B, arm)]), flush=True)
    dev = results[(a.batches[0], "seq")]["device"]
    lines = [f"Device: {dev}. SmolLM3-3B ({results[(a.batches[0], 'seq')]['layers']} layers), random bf16 weights, "
             f"prompt {PROMPT}, {NEW} new tokens per sequence, greedy, no EOS.", "",
             "| B | sequential generate: s | tokens/s | generate_batch: s | tokens/s | ratio |",
             "|---:|---:|---:|---:|---:|---:|"]
    def span(t):  # best time, and the slowest repetition when there is more than one
        return f"{min(t):.3f}" + (f" (max {max(t):.3f})" if len(t) > 1 else "")
    for B in a.batches:
        s, b = results[(B, "seq")], results[(B, "batch")]
        lines.append(f"| {B} | {span(s['seconds'])} | {s['tokens_per_s']:.0f} | {span(b['seconds'])} | "
                     f"{b['tokens_per_s']:.0f} | {b['tokens_per_s'] / s['tokens_per_s']:.2f}x |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
