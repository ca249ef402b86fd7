"""What the trainers share (train/frozen.py) on the CPU: the cache file names of DPOTrainer and GKDTrainer against the
names recorded before the fingerprint was shared, the branches of resolve_model, hold_frozen, and the evaluation
collator of the base loaders."""
import json
import os

import pytest
import torch

from llm_fine_tune_distributed_amd.data.collator import SFTCollator
from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
from llm_fine_tune_distributed_amd.models import CausalLM, build_model, get_config
from llm_fine_tune_distributed_amd.train import (DPOConfig, DPOTrainer, GKDConfig, GKDTrainer, SFTConfig, SFTTrainer,
                                                 checkpoint as ckpt)
from llm_fine_tune_distributed_amd.train.frozen import hold_frozen, resolve_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_cache_names.json")
CPU = torch.device("cpu")

# two pairs (chosen at 2i, rejected at 2i + 1) that share their prompt, and one more pair to evaluate on
_TRAIN = [[5, 6, 7, 8], [5, 6, 9], [10, 11, 12, 13, 14], [10, 11, 15, 16]]
_EVAL = [[20, 21, 22], [20, 21, 23, 24]]


def _sets(loss_start: bool):
    ls = (lambda n: [2] * n) if loss_start else (lambda n: None)
    return (TokenizedDataset.from_token_lists(_TRAIN, ls(len(_TRAIN))),
            TokenizedDataset.from_token_lists(_EVAL, ls(len(_EVAL))))


def _quiet(out, **kw):
    return dict(output_dir=str(out), per_device_train_batch_size=2, per_device_eval_batch_size=2, jsonl_log=False,
                save_strategy="no", dataloader_pin_memory=False, **kw)


def _dpo(out, train, ev=None):
    return DPOTrainer(model="tiny", args=DPOConfig(**_quiet(out)), train_dataset=train, eval_dataset=ev)


def _gkd(out, train, ev=None, teacher="tiny"):
    return GKDTrainer(model="tiny", args=GKDConfig(**_quiet(out, teacher_topk=4, beta=0.0)), train_dataset=train,
                      eval_dataset=ev, teacher_model=teacher)


def cache_names(out):
    """The cache file names of fixed tiny sets: DPO with and without an eval set, GKD (teacher_topk=4) on sets without
    a loss_start, with one, and with one on the train set only."""
    train, ev = _sets(True)
    plain, plain_ev = _sets(False)
    ref, topk = (lambda t: os.path.basename(t.ref_logps_path())), (lambda t: os.path.basename(t.teacher_topk_path()))
    return {"dpo_train": ref(_dpo(out, train)), "dpo_train_eval": ref(_dpo(out, train, ev)),
            "gkd_plain_train": topk(_gkd(out, plain)), "gkd_train_eval": topk(_gkd(out, train, ev)),
            "gkd_train_plain_eval": topk(_gkd(out, train, plain_ev))}


def test_cache_names_are_the_recorded_ones(tmp_path):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = cache_names(tmp_path)
    assert got == want
    assert len(set(got.values())) == len(got)  # every set, and an eval set or none, is another file


# ------------------------------------------------------------------------------------------------ resolve_model
def _same_weights(a, b):
    return all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))


def test_resolve_model_branches(tmp_path):
    obj = build_model(get_config("tiny-llama"), dtype=torch.float32, seed=3)
    assert resolve_model(obj, CPU) is obj and resolve_model(None, CPU) is None
    d = str(tmp_path / "hf")
    ckpt.save_pretrained(obj, d)
    assert any(f.endswith(".safetensors") for f in os.listdir(d))
    for spec in ("tiny-llama", d):
        m = resolve_model(spec, CPU)
        assert isinstance(m, CausalLM) and m.score is None
        assert {p.device for p in m.parameters()} == {CPU} and {p.dtype for p in m.parameters()} == {torch.bfloat16}
        assert m.inv_freq.device == CPU
    # the seed draws a preset's weights; a directory's are the saved ones whatever the seed
    assert _same_weights(resolve_model("tiny-llama", CPU), build_model(get_config("tiny-llama"), seed=0))
    assert _same_weights(resolve_model("tiny-llama", CPU, seed=7), build_model(get_config("tiny-llama"), seed=7))
    assert not _same_weights(resolve_model("tiny-llama", CPU, seed=7), resolve_model("tiny-llama", CPU))
    from_dir = resolve_model(d, CPU, seed=7)
    assert _same_weights(from_dir, resolve_model(d, CPU)) and _same_weights(from_dir, ckpt.from_pretrained(d))
    # num_labels=1 gives a score head on both string branches: a config override / a from_pretrained keyword (which
    # draws the head the directory does not hold from the seed, and leaves the trunk as saved)
    for spec in ("tiny-llama", d):
        rm = resolve_model(spec, CPU, seed=7, num_labels=1)
        assert rm.score is not None and rm.config.num_labels == 1
    assert _same_weights(rm, ckpt.from_pretrained(d, num_labels=1, seed=7))
    assert not torch.equal(rm.score, resolve_model(d, CPU, seed=8, num_labels=1).score)
    assert torch.equal(rm.model.embed_tokens, from_dir.model.embed_tokens)
    with pytest.raises(ValueError, match="unknown model"):
        resolve_model("no-such-preset", CPU)


# ------------------------------------------------------------------------------------------------ hold_frozen
_REFUSALS = {"teacher": ("teacher_model must be a preset name, a local HF directory or a CausalLM",
                         "the teacher must not be the student object: it is frozen and never updated"),
             "reference": ("ref_model must be a preset name, a local HF directory or a CausalLM",
                           "the reference must not be the policy object: it is frozen and never updated"),
             "reward model": (None, "a reward model must not be the policy object: it is frozen and never updated")}


@pytest.mark.parametrize("what", sorted(_REFUSALS))
def test_hold_frozen_refusals(what):
    type_msg, same_msg = _REFUSALS[what]
    m = build_model(get_config("tiny-llama"), dtype=torch.float32)
    with pytest.raises(ValueError) as e:
        hold_frozen(m, CPU, trained=m, what=what)
    assert str(e.value) == same_msg
    assert m.training and all(p.requires_grad for p in m.parameters())  # refused before anything was touched
    with pytest.raises(TypeError) as e:
        hold_frozen(torch.nn.Linear(2, 2), CPU, trained=m, what=what)
    assert type_msg is None or str(e.value) == type_msg


@pytest.mark.parametrize("cast", [False, True])
def test_hold_frozen_freezes(cast):
    student = build_model(get_config("tiny-llama"), dtype=torch.float32)
    m = build_model(get_config("tiny-llama"), dtype=torch.float32, seed=1)
    assert m.training and m.inv_freq.dtype == torch.float32
    held = hold_frozen(m, CPU, trained=student, what="teacher", cast_bf16=cast)
    assert held is m and not m.training and not any(mod.training for mod in m.modules())
    assert not any(p.requires_grad for p in m.parameters())
    assert {p.dtype for p in m.parameters()} == {torch.bfloat16 if cast else torch.float32}
    assert m.inv_freq.dtype == torch.float32 and m.inv_freq.device == CPU


def test_callers_refuse_the_trained_object(tmp_path):
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer
    train, _ = _sets(False)
    m = build_model(get_config("tiny"), dtype=torch.float32)
    with pytest.raises(ValueError, match="the teacher must not be the student object"):
        GKDTrainer(model=m, args=GKDConfig(**_quiet(tmp_path)), train_dataset=train, teacher_model=m)
    rows = [{"prompt_ids": [5, 6, 7]}, {"prompt_ids": [8, 9]}]
    t = GRPOTrainer(model=m, reward_funcs=lambda completions, **kw: [0.0] * len(completions),
                    args=GRPOConfig(**_quiet(tmp_path, num_generations=2, beta=0.04)), train_dataset=rows, ref_model=m)
    with pytest.raises(ValueError, match="the reference must not be the policy object"):
        t._reference()


# ------------------------------------------------------------------------------------------------ eval collator
def test_user_collator_serves_both_base_loaders(tmp_path):
    train, ev = _sets(False)
    mine = SFTCollator(0, None, None, False, None)
    t = SFTTrainer(model="tiny", args=SFTConfig(**_quiet(tmp_path)), train_dataset=train, eval_dataset=ev,
                   data_collator=mine)
    assert t.eval_collator is None
    assert t.get_train_dataloader().collator is mine and t.get_eval_dataloader().collator is mine
    assert t.collator is mine


def test_gkd_eval_loader_yields_the_eval_sets_cached_rows(tmp_path):
    train, ev = _sets(True)
    t = _gkd(tmp_path, train, ev)
    t.precompute_teacher_topk()
    d = torch.load(t.teacher_topk_path(), weights_only=True)
    train_collator = t.collator
    loader = t.get_eval_dataloader()
    assert t.collator is train_collator and loader.collator is t.eval_collator is not train_collator
    assert t.get_train_dataloader().collator is train_collator
    batches = list(loader)
    assert len(batches) == 1 and batches[0]["input_ids"].dim() == 2  # both eval samples, in order, one padded row each
    b = batches[0]
    for s in range(len(ev)):
        o, n = int(ev.offsets[s]), len(ev[s])
        assert b["input_ids"][s, :n].tolist() == ev[s]
        assert torch.equal(b["teacher_ids"][s, :n], d["eval_ids"][o:o + n])
        assert torch.equal(b["teacher_logps"][s, :n], d["eval_logps"][o:o + n])
    n = int(ev.offsets[-1])
    assert not torch.equal(d["eval_logps"], d["train_logps"][:n])  # (the train set's rows would not have passed)
