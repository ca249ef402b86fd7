"""Reference-compatible training entrypoint (``training.py`` equivalent).

Same env contract (EPOCHS, BATCH_SIZE, LEARNING_RATE, DATA_DIR, OUTPUT_DIR, AIM_REPO; WORLD_SIZE/RANK/...),
same SFTConfig values (GA 4, eval every 10 steps, logging every 2, clip 1.0, LR x world size,
best-by-eval_loss, save every 500 / keep 3), same callbacks (history, perplexity, Aim) and the same
rank-0 artifacts: ``best_model/`` (HF safetensors + tokenizer), ``training_history.json``,
``training_summary.json``. Runs on CPU/gloo too (the reference hard-fails without CUDA).

    python -m llm_fine_tune_distributed_amd.launch --nproc-per-node 8 -m llm_fine_tune_distributed_amd.cli.train
"""
from __future__ import annotations

import argparse
import json
import os

import torch


def main(argv=None):
    from ..data.dataset import load_jsonl, load_qa_parquet, train_test_split
    from ..data.prompts import format_prompt
    from ..data.synthetic import generate_qa, synthetic_preferences
    from ..data.tokenizer import load_tokenizer
    from ..parallel.process_group import cleanup_distributed, setup_distributed
    from ..train import (AimCallback, DPOConfig, DPOTrainer, GKDConfig, GKDTrainer, GRPOConfig, GRPOTrainer,
                         PerplexityCallback, RewardConfig, RewardTrainer, SFTConfig, SFTTrainer, TrainingHistoryCallback,
                         config_from_env)
    from ..train.config import apply_overrides

    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=os.getenv("MODEL_NAME", "HuggingFaceTB/SmolLM3-3B"),
                    help="preset name or local HF directory (config.json + safetensors)")
    ap.add_argument("--trainer", default="sft", choices=["sft", "dpo", "gkd", "grpo", "reward"],
                    help="sft: supervised fine-tuning; dpo: preference training on {prompt, chosen, rejected} rows "
                         "(a preference JSONL / parquet through --dataset; --set beta=...); gkd: knowledge "
                         "distillation of --model from --teacher on the SFT data (--set beta=... temperature=...); "
                         "grpo: reinforcement learning from --reward functions and / or --reward-model directories on "
                         "the questions of the Q&A data (--set num_generations=... max_completion_length=...); "
                         "reward: a reward model (score head in place of the LM head) on {chosen, rejected} rows "
                         "with an optional prompt and margin (a preference JSONL / parquet through --dataset; "
                         "--set center_rewards_coefficient=...)")
    ap.add_argument("--reward", dest="rewards", action="append", default=[], metavar="PKG.MODULE:FUNCTION",
                    help="--trainer grpo: a reward function f(prompts=, completions=, completion_ids=, **columns) -> "
                         "list[float] (repeatable; built in: llm_fine_tune_distributed_amd.train.rewards:answer_match "
                         "and :length_band)")
    ap.add_argument("--reward-model", dest="reward_models", action="append", default=[], metavar="DIR",
                    help="--trainer grpo: a reward model saved by --trainer reward (a one-label "
                         "...ForSequenceClassification directory with the policy's vocabulary; repeatable; models "
                         "come after the --reward functions in reward_weights' order)")
    ap.add_argument("--teacher", default=os.getenv("TEACHER_MODEL_NAME"),
                    help="--trainer gkd: the teacher, a preset name or local HF directory with the student's vocabulary")
    ap.add_argument("--dataset", default=os.getenv("DATASET_PATH", "data/qa_dataset.parquet"),
                    help="parquet/jsonl Q&A file; 'synthetic' (or a missing file) generates the synthetic set")
    ap.add_argument("--freeze-policy", default=os.getenv("FREEZE_POLICY", "last_n_layers"),
                    choices=["last_n_layers", "full", "lora"])
    ap.add_argument("--grad-accum", type=int, default=int(os.getenv("GRAD_ACCUM", "4")))
    ap.add_argument("--max-steps", type=int, default=-1)
    ap.add_argument("--max-length", type=int, default=1024)
    ap.add_argument("--packing", action="store_true")
    ap.add_argument("--lr-scheduler", default="linear")
    ap.add_argument("--no-gradient-checkpointing", action="store_true")
    ap.add_argument("--resume", default=None, help="checkpoint dir or 'auto'")
    ap.add_argument("--max-train-samples", type=int, default=None)
    ap.add_argument("--log-step-phases", action="store_true",
                    help="log data/fwd/bwd/comm_wait/optim *_ms per step (roctx ranges around each phase)")
    ap.add_argument("--log-system-metrics-every", type=int, default=int(os.getenv("LOG_SYSTEM_METRICS_EVERY", "0")),
                    help="GPU telemetry (amdsmi) into the trackers every N log steps (0 = off)")
    ap.add_argument("--config", default=os.getenv("SFT_CONFIG"),
                    help="YAML/JSON file of SFTConfig field overrides (applied over the reference defaults)")
    ap.add_argument("--set", dest="sets", action="append", default=[], metavar="FIELD=VALUE",
                    help="override one SFTConfig field (repeatable; highest precedence), e.g. "
                         "neftune_noise_alpha=5, label_smoothing_factor=0.1 or loss_type=dft")
    ap.add_argument("--precompute-only", action="store_true",
                    help="--trainer gkd with teacher_topk=K: write the teacher's top-k cache "
                         "(checkpoints/teacher_topk-<fingerprint>.pt) and stop; later runs need no --teacher")
    ap.add_argument("--merge-lora", action="store_true",
                    help="LoRA runs: write best_model/ with the adapters merged into the weights")
    a = ap.parse_args(argv)

    st = setup_distributed()
    env = config_from_env(world_size=st.world_size)
    out = env["output_dir"]
    if st.is_main:
        os.makedirs(f"{out}/best_model", exist_ok=True)
        print("Configuration:")
        for k in ("epochs", "batch_size", "learning_rate", "data_dir", "output_dir"):
            print(f"- {k}: {env[k]}")
        print(f"- model: {a.model}\n- dataset: {a.dataset}\n- device: {st.device}")

    # dataset (training.py:155-212)
    if a.dataset != "synthetic" and os.path.exists(a.dataset):
        rows = load_qa_parquet(a.dataset) if a.dataset.endswith(".parquet") else load_jsonl(a.dataset)
    elif a.trainer in ("dpo", "reward"):
        rows = synthetic_preferences(2845, seed=42)
    else:
        rows = generate_qa(2845, seed=42)
        rows = [{"full-question": r["full-question"], "answer": r["answer"]} for r in rows]
    train_rows, val_rows = train_test_split(rows, test_size=0.1, seed=42)
    if st.is_main:
        print(f"Total dataset size: {len(rows):,} | train {len(train_rows):,} | val {len(val_rows):,}")
    if a.trainer == "grpo":  # the question is the prompt; the answer column travels to the reward functions
        from ..data.prompts import WILDERNESS_EXPERT_SYSTEM_PROMPT as SYS
        as_prompt = lambda r: {"prompt": [{"role": "system", "content": SYS},  # noqa: E731
                                          {"role": "user", "content": r["full-question"]}], "answer": r["answer"]}
        train_rows = [as_prompt(r) for r in train_rows]
        val_rows = [as_prompt(r) for r in val_rows]
    elif a.trainer not in ("dpo", "reward"):
        train_rows = [format_prompt(r) for r in train_rows]
        val_rows = [format_prompt(r) for r in val_rows]
    tok_dir = a.model if os.path.isdir(a.model) else None
    tokenizer = load_tokenizer(tok_dir)

    history, ppl = TrainingHistoryCallback(), PerplexityCallback()
    aim = AimCallback(repo=env["aim_repo"], experiment="smollm3-wilderness-finetuning-distributed")
    dist_args = {}
    if st.world_size > 1:
        # the reference's ddp_bucket_cap_mb=50 (training.py:253) was sized for one TCP ring; on the xGMI
        # full mesh the cap grows with N (parallel/ddp.py plan_bucket_mb). DDP_BUCKET_CAP_MB pins it.
        cap = float(os.environ["DDP_BUCKET_CAP_MB"]) if os.environ.get("DDP_BUCKET_CAP_MB") else None
        dist_args = dict(ddp_find_unused_parameters=False, ddp_bucket_cap_mb=cap, local_rank=st.local_rank)
    config_cls, trainer_cls = {"sft": (SFTConfig, SFTTrainer), "dpo": (DPOConfig, DPOTrainer),
                               "gkd": (GKDConfig, GKDTrainer), "grpo": (GRPOConfig, GRPOTrainer),
                               "reward": (RewardConfig, RewardTrainer)}[a.trainer]
    extra = {}
    if a.trainer == "grpo":
        from ..train.rewards import resolve
        if not a.rewards and not a.reward_models:
            ap.error("--trainer grpo needs at least one --reward pkg.module:function or --reward-model DIR")
        extra["reward_funcs"] = [resolve(r) for r in a.rewards] + list(a.reward_models)
        # batches count completions (whole groups of num_generations); the best model is the best eval_reward
        dist_args = dict(dist_args, metric_for_best_model="eval_reward", greater_is_better=True)
    elif a.rewards or a.reward_models:
        ap.error("--reward and --reward-model belong to --trainer grpo")
    if a.trainer == "gkd":
        if a.teacher:
            dist_args = dict(dist_args, teacher_model_name_or_path=a.teacher)
    elif a.teacher:
        ap.error("--teacher belongs to --trainer gkd")
    if a.precompute_only and a.trainer != "gkd":
        ap.error("--precompute-only belongs to --trainer gkd with --set teacher_topk=K")
    args = config_cls(
        output_dir=f"{out}/checkpoints", per_device_train_batch_size=env["batch_size"],
        per_device_eval_batch_size=env["batch_size"], gradient_accumulation_steps=a.grad_accum,
        learning_rate=env["scaled_learning_rate"], max_grad_norm=1.0, num_train_epochs=env["epochs"],
        max_steps=a.max_steps, logging_steps=2, logging_first_step=True, save_steps=500, bf16=True,
        eval_strategy="steps", eval_steps=10, save_strategy="steps", load_best_model_at_end=True,
        save_total_limit=3, dataloader_pin_memory=True,
        dataloader_num_workers=0, remove_unused_columns=False,
        gradient_checkpointing=not a.no_gradient_checkpointing, dataloader_drop_last=True,
        max_seq_length=a.max_length, packing=a.packing, ddp_backend="nccl" if st.device.type == "cuda" else "gloo",
        freeze_policy=a.freeze_policy, lr_scheduler_type=a.lr_scheduler, max_train_samples=a.max_train_samples,
        log_step_phases=a.log_step_phases, log_system_metrics_every=a.log_system_metrics_every,
        **{"metric_for_best_model": "eval_loss", "greater_is_better": False, **dist_args})
    args = apply_overrides(args, a.config, a.sets)
    if a.trainer == "gkd":
        # with teacher_topk a cache file written earlier stands in for the teacher (GKDTrainer checks that it is there)
        if not a.teacher and args.teacher_topk is None:
            ap.error("--trainer gkd needs --teacher (a preset name or local HF directory)")
        if a.precompute_only and args.teacher_topk is None:
            ap.error("--precompute-only needs --set teacher_topk=K")
    if st.is_main:  # the resolved configuration of this run, next to its artifacts
        args.to_json(f"{out}/sft_config.json")
    trainer = trainer_cls(model=a.model, args=args, train_dataset=train_rows, eval_dataset=val_rows,
                         processing_class=tokenizer, callbacks=[history, ppl, aim], **extra)
    if st.device.type == "cuda" and st.is_main:
        print(f"VRAM after model load: {torch.cuda.memory_allocated() / 2**30:.2f} GB allocated")
    if a.precompute_only:
        trainer.precompute_teacher_topk()
        if st.is_main:
            print(f"teacher top-k cache: {trainer.teacher_topk_path()}")
        cleanup_distributed()
        return
    result = trainer.train(resume_from_checkpoint=a.resume)

    trainer.save_model(f"{out}/best_model", merge_lora=a.merge_lora)  # rank 0 writes, all ranks barrier
    if st.is_main:
        with open(f"{out}/training_history.json", "w") as f:
            json.dump(history.history, f, indent=2)
        summary = {
            "model_name": a.model, "dataset_path": a.dataset, "epochs": env["epochs"], "batch_size": env["batch_size"],
            "learning_rate": env["learning_rate"], "trainable_params": trainer.trainable_params,
            "total_params": trainer.total_params, "training_samples": len(train_rows),
            "validation_samples": len(val_rows), "final_train_loss": result.training_loss,
            "world_size": st.world_size, "distributed_training": st.world_size > 1,
            # MI355X-native additions
            "train_samples_per_second": result.metrics["train_samples_per_second"],
            "train_pure_samples_per_second": result.metrics["train_pure_samples_per_second"],
            "train_tokens_per_second": result.metrics["train_tokens_per_second"],
            "train_mfu": result.metrics["train_mfu"],
        }
        with open(f"{out}/training_summary.json", "w") as f:
            json.dump(summary, f, indent=2)
        print(f"\nDistributed Q&A fine-tuning completed successfully!\nArtifacts saved to {out}/\n"
              f"World size: {st.world_size}")
    cleanup_distributed()


if __name__ == "__main__":
    main()
