#!/usr/bin/env python3
"""Distillation step throughput on one GPU: a SmolLM3-3B student (random weights, full fine-tuning) learning from a
frozen Llama-3-8B teacher (random weights, bf16), 16 x 512 tokens per optimizer step — the tokens, the trainer settings
and the GEMM selection of ``bench.py --gpus 1``, so the two step times compare directly.

The teacher's forward (``CausalLM.logits_rows`` under no_grad, part of every step) is also timed on its own, on one
batch of the same shape, to report its share of the step. Prints one JSON line.

``--teacher-topk K`` (with ``--beta 0``) measures offline distillation: the teacher's caching pass over the dataset is
timed on its own (``cache_s``, ``cache_tokens_per_sec``), the teacher is released, and the steps run from the cache
(``peak_mem_gb`` is then the steps' peak, counted from after the release; ``cache_peak_mem_gb`` the caching pass's).

    python tools/bench_distill.py --steps 10 --warmup 3
    python tools/bench_distill.py --beta 0 --teacher-topk 64
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="smollm3-3b", help="the student")
    ap.add_argument("--teacher", default="llama3-8b")
    ap.add_argument("--micro-batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=0.9)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "outputs", "bench_distill"))
    ap.add_argument("--teacher-topk", type=int, default=None, help="K: train from the teacher's cached top-K")
    a = ap.parse_args()

    import torch
    from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
    from llm_fine_tune_distributed_amd.models import build_model, get_config
    from llm_fine_tune_distributed_amd.ops import _ext
    from llm_fine_tune_distributed_amd.train import GKDConfig, GKDTrainer

    assert torch.cuda.is_available(), "bench_distill needs a GPU"
    assert _ext.load(), _ext.load_error()
    if "PYTORCH_TUNABLEOP_ENABLED" not in os.environ:  # the measured GEMM selections bench.py runs with
        from llm_fine_tune_distributed_amd.utils.gemm_tuning import enable_tuned_gemms
        enable_tuned_gemms(tune=False, verbose=False)
    cfg = get_config(a.model)
    model = build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=0)
    teacher = build_model(get_config(a.teacher), device="cuda", dtype=torch.bfloat16, seed=1)
    ds = TokenizedDataset.synthetic(a.micro_batch * (a.steps + a.warmup + 2), cfg.vocab_size, a.seq, a.seq, seed=1)
    args = GKDConfig(output_dir=a.out_dir, per_device_train_batch_size=a.micro_batch, learning_rate=5e-5,
                     max_grad_norm=1.0, bf16=True, gradient_checkpointing=False, max_length=a.seq,
                     dataloader_drop_last=True, jsonl_log=False, logging_steps=0, save_strategy="no", gemm_tuning=False,
                     beta=a.beta, temperature=a.temperature, teacher_topk=a.teacher_topk)
    if a.teacher_topk is not None:  # a directory of its own: a cache file of an earlier run would skip the pass
        import tempfile
        os.makedirs(a.out_dir, exist_ok=True)
        args.output_dir = tempfile.mkdtemp(prefix="topk-", dir=a.out_dir)
    trainer = GKDTrainer(model=model, args=args, train_dataset=ds, teacher_model=teacher)
    it = iter(trainer.get_train_dataloader())

    cache = {}
    if a.teacher_topk is not None:
        # (the loader of a trainer without its cache cannot collate: the teacher is timed on tokens of the same shape)
        ids = ds.tokens[: a.micro_batch * a.seq].to("cuda", torch.int64).view(a.micro_batch, a.seq)
        ts = []
        with torch.no_grad():
            for i in range(a.steps + 2):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                logits = trainer.teacher.logits_rows(ids)
                e.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(s.elapsed_time(e))
                del logits
        teacher_ms = sorted(ts)[len(ts) // 2]
        del teacher  # the trainer's reference is the last one
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.precompute_teacher_topk()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n_tok = int(ds.offsets[-1])
        cache = {"teacher_topk": a.teacher_topk, "cache_s": round(dt, 3), "cache_tokens": n_tok,
                 "cache_tokens_per_sec": round(n_tok / dt, 1),
                 "cache_file_mb": round(os.path.getsize(trainer.teacher_topk_path()) / 1e6, 2),
                 "cache_peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
        assert trainer.teacher is None
        torch.cuda.reset_peak_memory_stats()
        it = iter(trainer.get_train_dataloader())

    def step():
        return trainer.optimizer_step([next(it)], lr=args.learning_rate)

    for _ in range(a.warmup):
        r = step()
    trainer.optimizer.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        r = step()
    trainer.optimizer.synchronize()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss = float(r["acc"][0])

    if a.teacher_topk is None:
        # the teacher's forward on its own: one batch of the step's shape, the median of --steps calls
        kw = trainer._model_inputs(next(it))
        kw.pop("labels")
        kw.pop("shift_labels", None)
        ts = []
        with torch.no_grad():
            for i in range(a.steps + 2):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                logits = trainer.teacher.logits_rows(**kw)
                e.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(s.elapsed_time(e))
                del logits
        teacher_ms = sorted(ts)[len(ts) // 2]
    ms = dt / a.steps * 1e3
    tokens = a.micro_batch * a.seq
    rec = {"bench": "distill", "student": a.model, "teacher": a.teacher, "beta": a.beta, "temperature": a.temperature,
           "tokens_per_step": tokens, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 3),
           "tokens_per_sec": round(tokens * a.steps / dt, 1), "teacher_fwd_ms": round(teacher_ms, 3),
           "teacher_fwd_share": round(teacher_ms / ms, 4), "final_loss": round(loss, 5),
           "loss_finite": math.isfinite(loss), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2),
           **cache}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
