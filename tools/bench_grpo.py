#!/usr/bin/env python3
"""GRPO step on one GPU, rollout and update timed separately: SmolLM3-3B with random weights, full fine-tuning,
8 prompts x 8 generations per optimizer step, 256-token prompts, 256 new tokens (no EOS, so every completion is full
length): 64 x 512 tokens per optimizer step, in 4 micro-batches of 16 sequences — the tokens of
``bench.py --gpus 1 --micro-batch 16 --ga 4``, so the update time compares with that step time directly.

The rollout runs ``rollout_batch`` with ``top_k=0``: the batched graph decoder with the full-vocabulary HIP sampler.
``--host-rollouts N`` also times N rollouts of one micro-batch forced onto the host loop (Python per row,
``multinomial``, a host sync per token), the path those rollouts took before the sampler existed.
Prints one JSON line.

    python tools/bench_grpo.py --steps 5 --warmup 2 --host-rollouts 1
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
    ap.add_argument("--model", default="HuggingFaceTB/SmolLM3-3B")
    ap.add_argument("--prompts", type=int, default=8, help="prompts per optimizer step")
    ap.add_argument("--generations", type=int, default=8)
    ap.add_argument("--micro", type=int, default=16, help="completions per micro-batch (a multiple of --generations)")
    ap.add_argument("--prompt", type=int, default=256, help="prompt tokens")
    ap.add_argument("--new", type=int, default=256, help="new tokens per completion")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--host-rollouts", type=int, default=0, help="also time this many host-loop rollouts of one micro-batch")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "outputs", "bench_grpo"))
    a = ap.parse_args()

    import torch
    from llm_fine_tune_distributed_amd.models import build_model, get_config
    from llm_fine_tune_distributed_amd.ops import _ext
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer

    assert torch.cuda.is_available(), "bench_grpo needs a GPU"
    assert _ext.load(), _ext.load_error()
    total = a.prompts * a.generations
    assert a.micro % a.generations == 0 and total % a.micro == 0, "--micro: a multiple of --generations dividing the step"
    ga = total // a.micro
    cfg = get_config(a.model)
    model = build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=0)
    V = cfg.vocab_size
    g = torch.Generator().manual_seed(1)
    n_prompts = a.prompts * (a.steps + a.warmup + 1)
    ds = [{"prompt_ids": torch.randint(0, V, (a.prompt,), generator=g).tolist()} for _ in range(n_prompts)]

    def low_share(prompts, completions, completion_ids, **kw):
        return [sum(t < V // 2 for t in c) / max(len(c), 1) for c in completion_ids]

    args = GRPOConfig(output_dir=a.out_dir, per_device_train_batch_size=a.micro, gradient_accumulation_steps=ga,
                      num_generations=a.generations, max_prompt_length=a.prompt, max_completion_length=a.new,
                      temperature=a.temperature, learning_rate=1e-6, max_grad_norm=1.0, gradient_checkpointing=False,
                      jsonl_log=False, logging_steps=0, save_strategy="no", gemm_tuning=False)
    trainer = GRPOTrainer(model=model, reward_funcs=low_share, args=args, train_dataset=ds)
    trainer._eos = None  # full-length completions: a fixed token count per step
    it = iter(trainer.get_train_dataloader())

    def sync():
        trainer.optimizer.synchronize()
        torch.cuda.synchronize()

    def step():
        sync()
        t0 = time.perf_counter()
        micro = [next(it) for _ in range(ga)]
        sync()
        t1 = time.perf_counter()
        r = trainer.optimizer_step(micro, lr=args.learning_rate)
        sync()
        return t1 - t0, time.perf_counter() - t1, r

    for _ in range(a.warmup):
        step()
    roll = upd = 0.0
    for _ in range(a.steps):
        dr, du, r = step()
        roll += dr
        upd += du
    loss = float(r["acc"][0])
    tokens = total * (a.prompt + a.new)
    rec = {"bench": "grpo", "model": a.model, "prompts_per_step": a.prompts, "generations": a.generations,
           "micro_batches": ga, "prompt_tokens": a.prompt, "new_tokens": a.new, "tokens_per_step": tokens,
           "steps": a.steps, "warmup": a.warmup, "rollout_ms_per_step": round(roll / a.steps * 1e3, 2),
           "update_ms_per_step": round(upd / a.steps * 1e3, 2),
           "rollout_new_tokens_per_sec": round(total * a.new * a.steps / roll, 1),
           "update_tokens_per_sec": round(tokens * a.steps / upd, 1), "final_loss": round(loss, 6),
           "loss_finite": math.isfinite(loss), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    if a.host_rollouts > 0:
        def one(kw):
            trainer.rollout_kwargs = kw
            sync()
            t0 = time.perf_counter()
            next(it)
            sync()
            return time.perf_counter() - t0
        dev = [one({}) for _ in range(a.host_rollouts)]
        host = [one({"device_sampling": False}) for _ in range(a.host_rollouts)]
        rec.update(micro_rollout_device_ms=round(sum(dev) / len(dev) * 1e3, 2),
                   micro_rollout_host_loop_ms=round(sum(host) / len(host) * 1e3, 2),
                   host_rollouts=a.host_rollouts)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
