#!/usr/bin/env python3
"""Reward-model step throughput on one GPU: SmolLM3-3B's trunk with random weights plus a score head, full
fine-tuning, 8 synthetic pairs x (2 x 512 tokens) per optimizer step — the 16 x 512 tokens of ``bench.py --gpus 1``,
so the two step times compare directly (this step has no LM-head GEMMs and no cross-entropy).

Prints one JSON line: pairs/s, tokens/s (both sequences of a pair count), ms per step.

    python tools/bench_reward.py --steps 10 --warmup 3
"""
import argparse
import dataclasses
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
    ap.add_argument("--pairs", type=int, default=8, help="pairs per optimizer step")
    ap.add_argument("--seq", type=int, default=512, help="tokens per sequence")
    ap.add_argument("--prompt", type=int, default=128, help="tokens the two sequences of a pair share")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--center", type=float, default=0.0, help="center_rewards_coefficient")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "outputs", "bench_reward"))
    a = ap.parse_args()

    import torch
    from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
    from llm_fine_tune_distributed_amd.models import build_model, get_config
    from llm_fine_tune_distributed_amd.ops import _ext
    from llm_fine_tune_distributed_amd.train import RewardConfig, RewardTrainer

    assert torch.cuda.is_available(), "bench_reward needs a GPU"
    assert _ext.load(), _ext.load_error()
    cfg = dataclasses.replace(get_config(a.model), num_labels=1)
    model = build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=0)
    n_pairs = a.pairs * (a.steps + a.warmup + 2)
    g = torch.Generator().manual_seed(1)
    seqs, starts = [], []
    for _ in range(n_pairs):
        prompt = torch.randint(0, cfg.vocab_size, (a.prompt,), generator=g).tolist()
        for _ in range(2):
            seqs.append(prompt + torch.randint(0, cfg.vocab_size, (a.seq - a.prompt,), generator=g).tolist())
            starts.append(a.prompt)
    ds = TokenizedDataset.from_token_lists(seqs, starts)
    args = RewardConfig(output_dir=a.out_dir, per_device_train_batch_size=a.pairs, per_device_eval_batch_size=a.pairs,
                        learning_rate=1e-6, center_rewards_coefficient=a.center, max_grad_norm=1.0,
                        gradient_checkpointing=False, max_length=a.seq, dataloader_drop_last=True, jsonl_log=False,
                        logging_steps=0, save_strategy="no", gemm_tuning=False)
    trainer = RewardTrainer(model=model, args=args, train_dataset=ds)
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
    rec = {"bench": "reward", "model": a.model, "pairs_per_step": a.pairs, "tokens_per_step": 2 * a.pairs * a.seq,
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3),
           "pairs_per_sec": round(a.pairs * a.steps / dt, 3),
           "tokens_per_sec": round(2 * a.pairs * a.seq * a.steps / dt, 1),
           "final_loss": round(loss, 5), "loss_finite": math.isfinite(loss),
           "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
