#!/usr/bin/env python3
"""qkv bias + RoPE kernels (csrc/qkv_bias.hip) at a training shape: M = 8192 tokens, 28 q / 4 kv heads x 128
(Qwen2.5-7B). Times forward and backward over rotating buffers larger than the 256 MB last-level cache, next to the
plain in-place RoPE kernel on the same buffers (what a frozen bias costs in the backward), and prints time per call and
the HBM rate from the bytes each one has to move: forward = the whole qkv read + written; backward = the q|k columns
read + written and the v columns read; RoPE = the q|k columns read + written (the cos / sin tables are shared by a
token's heads and not counted).

Each of the three measurements runs in a process of its own under a time limit of its own (--step runs one)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("rope", "fwd", "bwd")


def run_step(a):
    import torch

    sys.path.insert(0, ROOT)
    from llm_fine_tune_distributed_amd.ops import _ext
    from llm_fine_tune_distributed_amd.ops import reference as ref

    assert _ext.load(), _ext.load_error()
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    D, nh = 128, a.n_q + a.n_kv
    ld = (a.n_q + 2 * a.n_kv) * D
    bufs = [torch.randn(a.rows, ld, device=dev, generator=g).bfloat16() for _ in range(a.buffers)]
    bias = torch.randn(ld, device=dev, generator=g).bfloat16()
    cos, sin = ref.rope_cos_sin(torch.arange(a.rows, device=dev) % 512, D, 1e6)
    cos, sin = cos.contiguous(), sin.contiguous()
    qk_bytes, v_bytes = a.rows * nh * D * 2, a.rows * a.n_kv * D * 2
    fn, nbytes = {
        "rope": (lambda i: ops.rope_(bufs[i], cos, sin, a.n_q, a.n_kv, D, True), 2 * qk_bytes),
        "fwd": (lambda i: ops.qkv_bias_rope_fwd(bufs[i], bias, cos, sin, a.n_q, a.n_kv, D), 2 * (qk_bytes + v_bytes)),
        "bwd": (lambda i: ops.qkv_bias_rope_bwd(bufs[i], cos, sin, a.n_q, a.n_kv, D), 2 * qk_bytes + v_bytes),
    }[a.step]
    for i in range(a.buffers):
        fn(i)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(a.iters):
        fn(i % a.buffers)
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / a.iters
    print(json.dumps({"us": round(ms * 1e3, 2), "TB_s": round(nbytes / ms / 1e9, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--n-q", type=int, default=28)
    ap.add_argument("--n-kv", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--step", choices=STEPS, help="run this one measurement in this process")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each measurement may take")
    a = ap.parse_args()
    if a.step:
        return run_step(a)
    out = {"shape": [a.rows, a.n_q, a.n_kv]}
    fwd_args = [x for x in sys.argv[1:]]
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step]
        r = subprocess.run(cmd + fwd_args, capture_output=True, text=True)
        if r.returncode != 0:  # a fault or a time limit: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"bench_qkv_bias: step {step} ended with status {r.returncode}")
        out[step] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
