"""What ``load_best_model_at_end`` leaves in the model (CPU, fp32, PyTorch path): the best checkpoint's weights, bit for
bit — base AND adapters, in the model's own dtype — and a master copy that agrees with them. tests/test_resume_gpu.py
runs the same checks on the HIP path.

Four steps at a constant learning rate large enough that the loss goes up again, an evaluation and a checkpoint after
every step: the best checkpoint is then not the last one (asserted, so the test cannot pass on the weights train() ended
with), and the restore has something to do."""
import math
import os

import pytest
import torch

from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
from llm_fine_tune_distributed_amd.models import build_model, tiny
from llm_fine_tune_distributed_amd.models.lora import lora_state_dict
from llm_fine_tune_distributed_amd.train import SFTConfig, SFTTrainer
from llm_fine_tune_distributed_amd.train import checkpoint as ckpt

VOCAB = 1024
# learning rates at which the eval loss has its minimum before step 4: at step 3 (6.9383 against 6.9496 at step 4) for
# "full", at step 1 (6.9460 against 6.9685) for "lora" (the adapters' B starts at zero and Adam's update is ~lr per
# element whatever the gradient: a LoRA run needs a far larger rate than a full one to overshoot within four steps)
LR = {"full": 3e-3, "lora": 3.0}


def best_model_trainer(out, model, device_kw=None, **kw):
    """Shared with tests/test_resume_gpu.py."""
    a = SFTConfig(output_dir=str(out), per_device_train_batch_size=4, max_steps=4, logging_steps=1, jsonl_log=False,
                  eval_strategy="steps", eval_steps=1, save_strategy="steps", save_steps=1, save_total_limit=10,
                  load_best_model_at_end=True, metric_for_best_model="eval_loss", greater_is_better=False,
                  lr_scheduler_type="constant", dataloader_drop_last=True, **kw)
    return SFTTrainer(model=model, args=a, train_dataset=TokenizedDataset.synthetic(64, VOCAB, 30, 90, seed=2),
                      eval_dataset=TokenizedDataset.synthetic(8, VOCAB, 30, 90, seed=3))


def eval_losses(t):
    return {h["step"]: h["eval_loss"] for h in t.state.log_history if "eval_loss" in h}


def check_best_restored(t, out):
    """The assertions both files make after ``train()``; returns the best step."""
    ev = eval_losses(t)
    print("eval losses by step:", ev, "best:", t.state.best_model_checkpoint)
    best = t.state.best_model_checkpoint
    assert best is not None and os.path.isdir(best)
    step = int(best.rsplit("-", 1)[1])
    assert step != 4 and best != os.path.join(str(out), "checkpoint-4"), "best is last: the restore would be a no-op"
    assert sorted(ev) == [1, 2, 3, 4] and all(math.isfinite(v) for v in ev.values()), ev
    assert ev[step] == min(ev.values()) == t.state.best_metric
    bad = []  # every way the restore is wrong, not only the first
    disk = ckpt.load_state_dict(best)
    live = t.model.hf_state_dict()
    assert set(disk) == set(live)
    wrong = [k for k in sorted(live) if live[k].dtype != disk[k].dtype or not torch.equal(live[k].cpu(), disk[k])]
    if wrong:
        worst = max((live[k].cpu().float() - disk[k].float()).abs().max().item() for k in wrong)
        bad.append(f"base weights differ from {os.path.basename(best)}: {len(wrong)} of {len(live)} tensors, e.g. "
                   f"{wrong[0]}, largest difference {worst:.3e}")
    if t.args.freeze_policy == "lora":
        from safetensors.torch import load_file
        disk_ad = load_file(os.path.join(best, "adapter_model.safetensors"))
        live_ad = lora_state_dict(t.model)
        assert set(disk_ad) == set(live_ad) and live_ad
        wrong = [k for k in sorted(live_ad) if not torch.equal(live_ad[k].cpu(), disk_ad[k])]
        if wrong:
            bad.append(f"adapters differ from {os.path.basename(best)}: {len(wrong)} of {len(live_ad)} tensors, e.g. "
                       f"{wrong[0]}")
    if t.optimizer.master is not None:
        wrong = [t.engine.param_names[id(p)] for p, o, n, _ in t.engine.layout
                 if not torch.equal(t.optimizer.master[o:o + n], t.engine.param_flat[o:o + n].float())]
        if wrong:
            bad.append(f"master copy is not the restored parameters: {len(wrong)} of {len(t.engine.layout)} ranges, "
                       f"e.g. {wrong[0]}")
    again = t.evaluate()["eval_loss"]
    if again != ev[step]:
        bad.append(f"evaluate() after train() gives {again!r}, step {step} logged {ev[step]!r} (last step: {ev[4]!r})")
    assert not bad, "; ".join(bad)
    return step


@pytest.mark.parametrize("policy", ["full", "lora"])
def test_best_model_is_restored(tmp_path, policy):
    kw = dict(freeze_policy="lora", lora_r=4) if policy == "lora" else {}
    m = build_model(tiny(vocab_size=VOCAB), dtype=torch.float32, seed=0)
    t = best_model_trainer(tmp_path, m, learning_rate=LR[policy], **kw)
    t.train()
    check_best_restored(t, tmp_path)


def check_master_follows_restore(t, fresh_model, out, **kw):
    """Two further steps of ``train()`` on ``t`` (max_steps 4 -> 6) against a fresh trainer that starts at step 4 with
    the best checkpoint's weights, a master copy made from them, and the fourth step's moments and step count. A second
    ``train()`` without a resume draws its batches from the start of the epoch: so does the reference. (The master
    path rounds to nearest and ``full`` has no dropout: no generator is involved.)"""
    best, last = t.state.best_model_checkpoint, os.path.join(str(out), "checkpoint-4")
    ref = best_model_trainer(str(out) + "_ref", fresh_model, learning_rate=t.args.learning_rate, master_weights=True, **kw)

    class StartFromBest:
        def on_train_begin(self, args, state, control, **kw):
            ref.optimizer.load_state_dict(torch.load(os.path.join(last, "optimizer.pt"), weights_only=True))
            ref.model.load_hf_state_dict(ckpt.load_state_dict(best), strict=False)
            ref.optimizer.master.copy_(ref.engine.param_flat.float())
            state.global_step = 4

    ref.callback_handler.callbacks.insert(0, StartFromBest())
    for tr in (t, ref):
        a = tr.args
        a.max_steps, a.eval_strategy, a.save_strategy, a.load_best_model_at_end = 6, "no", "no", False
        tr.train()
    loss = {h["step"]: h["loss"] for h in t.state.log_history if "loss" in h}
    loss_ref = {h["step"]: h["loss"] for h in ref.state.log_history if "loss" in h}
    print("steps 5, 6:", [loss[s] for s in (5, 6)], "reference:", [loss_ref[s] for s in (5, 6)])
    assert loss[5] == loss_ref[5], "step 5 did not see the restored weights"
    assert loss[6] == loss_ref[6], "step 5's update did not start from the restored weights (stale master copy)"
    assert torch.equal(t.engine.param_flat, ref.engine.param_flat)
    assert torch.equal(t.optimizer.master, ref.optimizer.master)


def test_best_model_restore_reseeds_master(tmp_path):
    """With an fp32 master copy the next update starts from the master: it has to follow the restore. On a bf16 model:
    an fp32 model's ``param_flat.float()`` IS ``param_flat``, a master copy that cannot go stale."""
    def model():
        return build_model(tiny(vocab_size=VOCAB), dtype=torch.bfloat16, seed=0)

    t = best_model_trainer(tmp_path / "a", model(), learning_rate=LR["full"], master_weights=True)
    assert t.optimizer.master.data_ptr() != t.engine.param_flat.data_ptr()
    t.train()
    check_best_restored(t, tmp_path / "a")
    check_master_follows_restore(t, model(), tmp_path / "a")


def test_refresh_master_covers_the_sharded_state():
    """ZeRO-1 keeps the master copy for the owned slice of every bucket only (local offsets): ``refresh_master`` has to
    follow that mapping, not the flat one."""
    from llm_fine_tune_distributed_amd.parallel.ddp import DDPEngine
    from llm_fine_tune_distributed_amd.train.optim import ShardedAdamW
    eng = DDPEngine(build_model(tiny(vocab_size=VOCAB), dtype=torch.bfloat16, seed=0), 1, 0, shard=True)
    opt = ShardedAdamW(eng, lr=1e-3, master_weights=True)
    assert len(opt.slices) > 1
    with torch.no_grad():
        eng.param_flat.mul_(1.5)
    opt.exp_avg.fill_(0.25)
    opt.step_count = 7
    opt.refresh_master()
    for _, s, t, lo, _ in opt.slices:
        assert torch.equal(opt.master[lo:lo + t - s], eng.param_flat[s:t].float())
    assert opt.step_count == 7 and bool((opt.exp_avg == 0.25).all())  # a weight restore: the rest stays
