#!/usr/bin/env python3
"""Per-head QK RMSNorm + RoPE kernels (csrc/qk_norm.hip) at a training shape: M = 8192 tokens, 32 q / 8 kv heads x
128 (Qwen3-4B / 8B). Times forward (with and without the raw q|k copy) and backward over rotating buffers larger than
the 256 MB last-level cache, next to the plain in-place RoPE kernel on the same buffers, and prints time per call and
the HBM rate from the bytes each one has to move (q|k columns read + written, + the raw copy written / read; the
cos / sin tables are shared by a token's heads and not counted)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_fine_tune_distributed_amd.ops import _ext  # noqa: E402
from llm_fine_tune_distributed_amd.ops import reference as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--n-q", type=int, default=32)
    ap.add_argument("--n-kv", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--buffers", type=int, default=4)
    a = ap.parse_args()
    assert _ext.load(), _ext.load_error()
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    D, nh = 128, a.n_q + a.n_kv
    ld = (a.n_q + 2 * a.n_kv) * D
    bufs = [torch.randn(a.rows, ld, device=dev, generator=g).bfloat16() for _ in range(a.buffers)]
    raws = [b[:, : nh * D].contiguous() for b in bufs]
    qw = (1 + 0.1 * torch.randn(D, device=dev, generator=g)).bfloat16()
    kw = (1 + 0.1 * torch.randn(D, device=dev, generator=g)).bfloat16()
    cos, sin = ref.rope_cos_sin(torch.arange(a.rows, device=dev) % 512, D, 1e6)
    cos, sin = cos.contiguous(), sin.contiguous()
    qk_bytes = a.rows * nh * D * 2

    def timed(fn, nbytes):
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
        return {"us": round(ms * 1e3, 2), "TB_s": round(nbytes / ms / 1e9, 2)}

    out = {"shape": [a.rows, a.n_q, a.n_kv]}
    out["rope"] = timed(lambda i: ops.rope_(bufs[i], cos, sin, a.n_q, a.n_kv, D, False), 2 * qk_bytes)
    out["fwd"] = timed(lambda i: ops.qk_norm_rope_fwd(bufs[i], qw, kw, cos, sin, a.n_q, a.n_kv, D, 1e-6, True),
                       3 * qk_bytes)
    out["fwd_nocopy"] = timed(lambda i: ops.qk_norm_rope_fwd(bufs[i], qw, kw, cos, sin, a.n_q, a.n_kv, D, 1e-6,
                                                             False), 2 * qk_bytes)
    out["bwd"] = timed(lambda i: ops.qk_norm_rope_bwd(bufs[i], raws[i], qw, kw, cos, sin, a.n_q, a.n_kv, D, 1e-6),
                       3 * qk_bytes)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
