"""Stop a run on the HIP path and start it again: the state that exists only there, through a checkpoint, bit for bit.

The CPU resume tests run fp32 models on the PyTorch path. Here a bf16 model trains on the GPU, where the checkpoint has to
carry what feeds the kernels: the optimizer's ``step_count`` (the seed of adamw_flat's stochastic rounding), bf16 moments
and the fp32 master copy (keyed by parameter name in ``optimizer.pt``), the host generator (the seeds of ``lora_fwd``'s
dropout and of ``embedding_noise_fwd``), the LoRA wide weights (refreshed from the adapters by ``copy2d_batch``), and the
update that may still be running on a side stream when a save or a load begins.

Per recipe, on tiny-gpu widths (hidden 256, 2 q / 1 kv heads x 128, intermediate 512, vocabulary 1024, 3 layers), 64
samples of 30..90 tokens, batch 4, cosine schedule with one warm-up step:
  straight    4 steps in one run (twice: the control — two runs of the same thing are equal bit for bit, so equality is
              the bar for the resumed run and not a tolerance);
  first half  the same arguments, ``max_steps`` lowered to 2 after construction, a checkpoint at step 2;
  resumed     a fresh model and trainer, ``train(resume_from_checkpoint="auto")`` to step 4, after the host and device
              generators were disturbed.
Checked: what ``load_checkpoint`` put into the resumed trainer (before its first step) is the first half's state; after
step 4 parameters, moments, master copy, losses and gradient norms are the straight run's; and the dispatch trace of the
resumed run names the HIP kernels the recipe is about. (The hand-written weight-gradient kernels are not asked for: at
these token counts they fall back to addmm_, and tests/test_train_recipes_gpu.py owns them.)

``zero1`` asks for ``shard_optimizer_state`` at world size 1, where the trainer builds the replicated FlatAdamW (there is
nothing to shard): the recipe covers that the flag changes nothing there, not ShardedAdamW.

The best-model tests of tests/test_resume_cpu.py run here on the HIP path, too.
"""
import os

import pytest
import torch

from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
from llm_fine_tune_distributed_amd.models import build_model, tiny
from llm_fine_tune_distributed_amd.models.lora import lora_state_dict
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.train import SFTConfig, SFTTrainer
from llm_fine_tune_distributed_amd.train import checkpoint as ckpt
from llm_fine_tune_distributed_amd.train.optim import LRScheduler, get_schedule
from test_resume_cpu import best_model_trainer, check_best_restored, check_master_follows_restore

pytestmark = pytest.mark.gpu

DEV = "cuda"
LORA = dict(freeze_policy="lora", lora_r=16, lora_alpha=32.0, lora_dropout=0.1)
# id: (model, trainer arguments beyond the base, the optimizer launch the trace must show)
RECIPES = {
    "sr": ("tiny-gpu", {}, "optim.adamw.sr.bf16m"),
    "master": ("tiny-gpu", dict(master_weights=True), "optim.adamw.master.fp32m"),
    "sr_fp32_state": ("tiny-gpu", dict(optim_state_dtype="fp32"), "optim.adamw.sr.fp32m"),
    "overlap_off": ("tiny-gpu", dict(optimizer_overlap=False), "optim.adamw.sr.bf16m"),
    "zero1": ("tiny-gpu", dict(shard_optimizer_state=True), "optim.adamw.sr.bf16m"),
    "lora_dropout": ("tiny-gpu", LORA, "optim.adamw.sr.bf16m"),
    "last2_ga_ckpt_noise": ("tiny-gpu", dict(freeze_policy="last_n_layers", freeze_last_n_layers=2,
                                             gradient_accumulation_steps=2, gradient_checkpointing=True,
                                             neftune_noise_alpha=5.0, label_smoothing_factor=0.1),
                            "optim.adamw.sr.bf16m"),
    "qwen3": ("tiny-gpu-qwen3", {}, "optim.adamw.sr.bf16m"),
    "qwen2": ("tiny-gpu-qwen2", {}, "optim.adamw.sr.bf16m"),
    "mistral": ("tiny-gpu-mistral", {}, "optim.adamw.sr.bf16m"),  # window 40 < the longer samples
}


WIDTHS = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=512,
              vocab_size=1024, num_hidden_layers=3)
# the family names of tests/test_qwen3_gpu.py, test_qwen2_gpu.py and test_sliding_window_gpu.py (tiny-gpu-qwen3,
# tiny-gpu-qwen2; Mistral = Llama with a window, tiny-gpu-mistral's 40 tokens: shorter than most of the samples)
FAMILY = {"tiny-gpu": ("smollm3", {}), "tiny-gpu-qwen3": ("qwen3", {}), "tiny-gpu-qwen2": ("qwen2", {}),
          "tiny-gpu-mistral": ("llama", dict(sliding_window=40))}


def _model(name="tiny-gpu"):
    model_type, extra = FAMILY[name]
    return build_model(tiny(model_type, **WIDTHS, **extra), device=DEV, dtype=torch.bfloat16, seed=0)


class _Recorder:
    """The learning rate of every step, and a hook after the checkpoint load (``on_train_begin`` is the first callback
    after it, before any step)."""

    def __init__(self, trainer, at_begin=None):
        self.t, self.lr, self.at_begin = trainer, {}, at_begin

    def on_train_begin(self, args, state, control, **kw):
        if self.at_begin is not None:
            self.at_begin(self.t)

    def on_step_begin(self, args, state, control, **kw):
        self.lr[state.global_step + 1] = self.t.scheduler.get_lr()


def _trainer(out, model_name, kw, save_steps=0, at_begin=None, steps=4):
    kw = {"optimizer_overlap": True, **kw}
    a = SFTConfig(output_dir=str(out), per_device_train_batch_size=4, max_steps=steps, learning_rate=1e-3,
                  lr_scheduler_type="cosine", warmup_steps=1, logging_steps=1, jsonl_log=False,
                  save_strategy="steps" if save_steps else "no", save_steps=save_steps or 500,
                  dataloader_drop_last=True, **kw)
    t = SFTTrainer(model=_model(model_name), args=a, train_dataset=TokenizedDataset.synthetic(64, 1024, 30, 90, seed=2))
    t.rec = _Recorder(t, at_begin)
    t.callback_handler.callbacks.insert(0, t.rec)
    return t


def _snap(t):
    """Clones of everything a checkpoint has to carry (the side stream's update ordered first)."""
    t.optimizer.synchronize()
    torch.cuda.synchronize()
    o = t.optimizer
    s = {"param_flat": t.engine.param_flat.clone(), "exp_avg": o.exp_avg.clone(), "exp_avg_sq": o.exp_avg_sq.clone(),
         "step_count": o.step_count}
    if o.master is not None:
        s["master"] = o.master.clone()
    if t.args.freeze_policy == "lora":
        s["adapters"] = {k: v.clone() for k, v in lora_state_dict(t.model).items()}
        s["base"] = {k: v.clone() for k, v in t.model.hf_state_dict().items()}
    return s


def _logged(t, key):
    return {h["step"]: h[key] for h in t.state.log_history if key in h}


def _differences(a, b):
    """Names of what differs between two snapshots, with the largest difference (empty: equal bit for bit)."""
    out = []
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            bad = [n for n in a[k] if not torch.equal(a[k][n], b[k][n])]
            if bad:
                out.append(f"{k}: {len(bad)} of {len(a[k])} tensors, e.g. {bad[0]}")
        elif torch.is_tensor(a[k]):
            if a[k].dtype != b[k].dtype or not torch.equal(a[k], b[k]):
                d = (a[k].float() - b[k].float()).abs()
                out.append(f"{k} ({a[k].dtype}): {int((d > 0).sum())} of {d.numel()} elements, largest {d.max():.3e}")
        elif a[k] != b[k]:
            out.append(f"{k}: {a[k]} != {b[k]}")
    return out


def _read_trace():
    out = {}
    for item in _ext.ops().dispatch_trace_read().split(";"):
        if item:
            k, v = item.split("=")
            out[k] = int(v)
    return out


def _traced_train(t, **kw):
    _ext.ops().dispatch_trace(True)
    try:
        t.train(**kw)
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
    return _read_trace()


def _first_half(out, model_name, kw):
    """Steps 1 and 2 of the four-step schedule, and ``checkpoint-2`` under ``out``."""
    first = _trainer(out, model_name, kw, save_steps=2)
    first.args.max_steps = 2
    first.train()
    return first, _snap(first)


def _resume(out, model_name, kw, tamper=None):
    """A fresh model and trainer resumed from the latest checkpoint under ``out``, the host and device generators
    disturbed before and after it is built. Returns the trainer after step 4, what ``load_checkpoint`` left in it
    (taken at ``on_train_begin``, before ``tamper(trainer)`` seeds a fault) and the dispatch trace of the run."""
    loaded = {}

    def after_load(t):
        loaded.update(_snap(t), lr=t.scheduler.get_lr(), global_step=t.state.global_step)
        if tamper is not None:
            tamper(t)

    torch.manual_seed(999)
    torch.rand(3, device=DEV)
    resumed = _trainer(out, model_name, kw, at_begin=after_load)
    torch.manual_seed(998)
    torch.rand(5, device=DEV)
    torch.rand(5)
    trace = _traced_train(resumed, resume_from_checkpoint="auto")
    return resumed, loaded, trace


@pytest.mark.parametrize("name", list(RECIPES))
def test_resume_is_bit_exact(tmp_path, name):
    """Control (measured on an MI355X for every recipe): straight against straight is equal bit for bit — parameters,
    moments, master copy, losses and gradient norms — so the resumed run is held to equality as well."""
    assert _ext.load(), _ext.load_error()
    model_name, kw, optim_label = RECIPES[name]

    # ---- control: two straight runs
    straight = _trainer(tmp_path / "s", model_name, kw)
    straight.train()
    end = _snap(straight)
    again = _trainer(tmp_path / "s2", model_name, kw)
    again.train()
    control = _differences(end, _snap(again))
    losses, norms = _logged(straight, "loss"), _logged(straight, "grad_norm")
    print(f"\n[{name}] straight: loss {losses} grad_norm {norms} lr {straight.rec.lr}")
    print(f"[{name}] control, straight vs straight: {control or 'equal bit for bit'}")
    assert not control, f"two straight runs differ: {control}"
    assert losses == _logged(again, "loss") and norms == _logged(again, "grad_norm")
    assert sorted(losses) == [1, 2, 3, 4] and straight.rec.lr[3] != straight.rec.lr[2] != straight.rec.lr[1]
    del again

    # ---- first half: steps 1, 2 and checkpoint-2
    first, half = _first_half(tmp_path / "r", model_name, kw)
    assert half["step_count"] == 2 and _logged(first, "loss") == {s: losses[s] for s in (1, 2)}
    path = os.path.join(str(tmp_path / "r"), "checkpoint-2")
    osd = torch.load(os.path.join(path, "optimizer.pt"), map_location="cpu", weights_only=True)
    on_disk = {k: {str(v[k].dtype) if v[k] is not None else None for v in osd["param_state"].values()}
               for k in ("exp_avg", "exp_avg_sq", "master")}
    moments = "torch.float32" if (kw.get("master_weights") or kw.get("optim_state_dtype") == "fp32") else "torch.bfloat16"
    assert on_disk == {"exp_avg": {moments}, "exp_avg_sq": {moments},
                       "master": {"torch.float32"} if kw.get("master_weights") else {None}}, on_disk
    assert osd["step"] == 2 and set(osd["param_state"]) == {n for n, _ in first.engine.named_params()}
    del first

    # ---- resumed: a fresh trainer, the generators disturbed before and after it is built
    resumed, loaded, trace = _resume(tmp_path / "r", model_name, kw)
    print(f"[{name}] trace of the resumed run: {trace}")

    # load round trip
    lr3, gs = loaded.pop("lr"), loaded.pop("global_step")
    assert gs == 2 and loaded["step_count"] == 2
    assert not _differences(half, loaded), f"load_checkpoint: {_differences(half, loaded)}"
    assert lr3 == straight.rec.lr[3] and resumed.rec.lr == {s: straight.rec.lr[s] for s in (3, 4)}
    if "master" in loaded:
        for p, o, n, _ in resumed.engine.layout:
            assert torch.equal(loaded["param_flat"][o:o + n], loaded["master"][o:o + n].to(torch.bfloat16)), \
                f"loaded {resumed.engine.param_names[id(p)]} is not its master copy rounded to bf16"

    # continuation
    diff = _differences(end, _snap(resumed))
    print(f"[{name}] resumed vs straight after step 4: {diff or 'equal bit for bit'}; resumed loss "
          f"{_logged(resumed, 'loss')} grad_norm {_logged(resumed, 'grad_norm')}")
    assert _logged(resumed, "loss") == losses  # (steps 1, 2 from trainer_state.json, 3 and 4 run here)
    assert _logged(resumed, "grad_norm") == norms
    assert not diff, f"after step 4 the resumed run differs from the straight one: {diff}"

    # the HIP path ran: one update launch per group of the overlapped update / per region, two steps
    assert trace.get(optim_label, 0) >= 2 and [k for k in trace if k.startswith("optim.adamw")] == [optim_label], trace
    assert any(k.startswith("attn.fwd") for k in trace) and any(k.startswith("attn.dq") for k in trace), trace
    if name == "lora_dropout":
        assert trace.get("lora.fwd.dropout", 0) > 0 and "lora.fwd" not in trace, trace
        # step 3: every wide weight registers at its first forward and is refreshed there, one launch each (3 layers x
        # qkv, o, gate_up, down); step 4: ONE batched refresh of all twelve after the update
        assert trace.get("lora.copy2d_batch", 0) == 12 + 1, trace
    if name == "last2_ga_ckpt_noise":
        assert trace.get("ew.embedding_noise.fwd", 0) >= 2, trace


def _fresh_loaded(out, path, kw):
    """A fresh trainer with checkpoint ``path`` loaded (``load_checkpoint`` wants the scheduler ``train()`` makes)."""
    t = _trainer(out, "tiny-gpu", kw)
    t.scheduler = LRScheduler(t.optimizer, get_schedule("cosine", 4, 1))
    ckpt.load_checkpoint(path, t.model, t.optimizer, t.scheduler, 0)
    return t


def _warm_load(tmp_path):
    """The runs of test_warm_load_refreshes_the_wide_weight: eval losses at step 4, of a fresh trainer with checkpoint-2
    loaded, of the warm trainer after loading it, and once more with the load issued under a pending update; whether
    the warm trainer's state equalled the fresh one's each time; the two traces."""
    ev = TokenizedDataset.synthetic(8, 1024, 30, 90, seed=3)
    t = _trainer(tmp_path, "tiny-gpu", LORA, save_steps=2)
    t.train()
    path = os.path.join(str(tmp_path), "checkpoint-2")
    at4 = t.evaluate(ev)["eval_loss"]  # (and the wide weights are step 4's from here on)
    fresh = _fresh_loaded(tmp_path / "f", path, LORA)
    want, want_state = fresh.evaluate(ev)["eval_loss"], _snap(fresh)

    def load_and_evaluate():
        ckpt.load_checkpoint(path, t.model, t.optimizer, t.scheduler, 0)
        _ext.ops().dispatch_trace(True)
        try:
            got = t.evaluate()["eval_loss"]
        finally:
            _ext.ops().dispatch_trace(False)
        return got, _read_trace(), _differences(want_state, _snap(t))

    warm = load_and_evaluate()
    # once more, the load called straight after an optimizer step, its update pending on the side stream
    batch = next(iter(t.get_train_dataloader()))
    t.optimizer_step([batch], 1e-3)
    assert t.optimizer.overlap and t.optimizer._pending
    pending = load_and_evaluate()
    print(f"\n[warm] step 4 {at4!r}, fresh load of checkpoint-2 {want!r}, warm load {warm[0]!r} (trace {warm[1]}), "
          f"under a pending update {pending[0]!r} (trace {pending[1]})")
    return at4, want, warm, pending


def test_warm_load_refreshes_the_wide_weight(tmp_path):
    """A checkpoint loaded into a model that has already run: the LoRA wide weight W' = [W | B] and A_cat are refreshed
    when the parameter epoch OR the adapters' version counters change, and a load moves only the latter. An evaluation
    between the last update and the load brings the wide weights up to date with step 4, so that only the version
    counters can tell the next forward that the adapters are checkpoint-2's again.

    Then the same with the update still pending on the side stream when ``load_checkpoint`` is called: the load has to
    order itself after it (``optimizer.synchronize()``), or the update overwrites what was loaded. (At this size the
    update is over long before the checkpoint is read from disk: this half shows that such a load is right, not that
    an unordered one would be caught.)"""
    assert _ext.load(), _ext.load_error()
    at4, want, warm, pending = _warm_load(tmp_path)
    assert want != at4, "steps 3 and 4 changed nothing: the test would pass without a refresh"
    for got, trace, diff in (warm, pending):
        assert trace.get("lora.copy2d_batch", 0) == 1, trace  # one batched refresh of all twelve wide weights
        assert got == want
        assert not diff, diff


@pytest.mark.parametrize("fault", ["step_count", "generator", "wide_key"])
def test_seeded_faults_are_seen(tmp_path, fault, monkeypatch):
    """The checks can fail: three faults seeded in Python, one per piece of state the CPU tests cannot see.
    step_count  ``sr``: the optimizer counts one step too many after the load — another stochastic-rounding seed (and
                bias correction): parameters and moments differ after step 4;
    generator   ``lora_dropout``: the checkpoint's generator state is not restored — steps 3 and 4 draw other dropout
                seeds for ``lora_fwd``: the loss of step 3 differs already;
    wide_key    the wide weights' key leaves out the adapters' version counters: the warm load is not seen, and the next
                forward runs on step 4's W' and A_cat."""
    assert _ext.load(), _ext.load_error()
    if fault == "wide_key":
        from llm_fine_tune_distributed_amd.ops import fused
        monkeypatch.setattr(fused._WideEntry, "state", lambda self: (fused._PARAM_EPOCH[0],))
        at4, want, warm, pending = _warm_load(tmp_path)
        assert warm[0] != want and warm[0] == at4 and "lora.copy2d_batch" not in warm[1], (at4, want, warm)
        return
    name = {"step_count": "sr", "generator": "lora_dropout"}[fault]
    model_name, kw, _ = RECIPES[name]
    straight = _trainer(tmp_path / "s", model_name, kw)
    straight.train()
    _first_half(tmp_path / "r", model_name, kw)
    tamper = None
    if fault == "step_count":
        def tamper(t):
            t.optimizer.step_count += 1
    else:
        monkeypatch.setattr(ckpt, "set_rng_state", lambda st: None)
    resumed, loaded, _ = _resume(tmp_path / "r", model_name, kw, tamper=tamper)
    diff = _differences(_snap(straight), _snap(resumed))
    print(f"\n[fault {fault}] {diff}; loss {_logged(straight, 'loss')} vs {_logged(resumed, 'loss')}")
    assert any(d.startswith("param_flat") for d in diff) and any(d.startswith("exp_avg") for d in diff), diff
    if fault == "generator":
        assert _logged(resumed, "loss")[3] != _logged(straight, "loss")[3]
    else:  # the load itself was right, and step 3's forward ran on the right weights
        assert _logged(resumed, "loss")[3] == _logged(straight, "loss")[3]


# learning rates at which the eval loss has its minimum before step 4 on this model, from a scan on an MI355X (every run
# of it gave the same bits twice): full / master 1e-3 -> 6.9881, 6.9846, 6.9867, 6.9866 (best: step 2); lora 1.5 ->
# 6.9860, 6.9871, 6.9870, 6.9943 (best: step 1; at 2.0 and above the bf16 gradients overflow by step 4)
BEST_LR = {"full": 1e-3, "lora": 1.5, "master": 1e-3}


@pytest.mark.parametrize("case", ["full", "lora", "master"])
def test_best_model_is_restored(tmp_path, case):
    """tests/test_resume_cpu.py's checks on the HIP path: bf16 weights equal to the best checkpoint's on disk (base
    through ``hf_state_dict()``, adapters), ``evaluate()`` equal to the eval loss logged at the best step, and with a
    master copy: equal to the restored parameters, and the next ``train()`` starts from them."""
    assert _ext.load(), _ext.load_error()
    kw = {"full": {}, "lora": dict(freeze_policy="lora", lora_r=16, lora_alpha=32.0),
          "master": dict(master_weights=True)}[case]
    t = best_model_trainer(tmp_path / "a", _model(), learning_rate=BEST_LR[case], optimizer_overlap=True, **kw)
    t.train()
    check_best_restored(t, tmp_path / "a")
    if case == "master":
        check_master_follows_restore(t, _model(), tmp_path / "a", optimizer_overlap=True)
