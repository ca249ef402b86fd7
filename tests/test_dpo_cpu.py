"""DPO on the CPU reference path (fp32 ``tiny-llama`` passed as a ``CausalLM``): the torch twins of the three
preference ops against fp64, tokenisation and collation of preference rows, and DPOTrainer — learning, gradient
accumulation, two gloo ranks, resume, refusals, the CLI switch."""
import glob
import json
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
from llm_fine_tune_distributed_amd.data.preference import (PreferenceCollator, cached_tokenize_preferences,
                                                           tokenize_preference_rows)
from llm_fine_tune_distributed_amd.data.synthetic import synthetic_preferences
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import reference as ref

LN2 = math.log(2.0)


def token_pairs(n, vocab, seed=0):
    """n pairs of random tokens: a prompt of 3-8 tokens shared by two completions of 2-11 tokens."""
    g = torch.Generator().manual_seed(seed)
    seqs, starts = [], []
    for _ in range(n):
        p = torch.randint(3, vocab, (int(torch.randint(3, 9, (1,), generator=g)),), generator=g).tolist()
        for _ in range(2):
            seqs.append(p + torch.randint(3, vocab, (int(torch.randint(2, 12, (1,), generator=g)),), generator=g).tolist())
            starts.append(len(p))
    return TokenizedDataset.from_token_lists(seqs, starts)


def tiny_model(seed=0):
    return build_model(get_config("tiny-llama"), device="cpu", dtype=torch.float32, seed=seed)


def dpo_trainer(out, model, ds, eval_ds=None, ref_model=None, **kw):
    from llm_fine_tune_distributed_amd.train import DPOConfig, DPOTrainer
    base = dict(output_dir=str(out), per_device_train_batch_size=4, learning_rate=5e-4, lr_scheduler_type="constant",
                beta=0.1, logging_steps=1, jsonl_log=False, save_strategy="no", dataloader_drop_last=True)
    base.update(kw)
    return DPOTrainer(model=model, args=DPOConfig(**base), train_dataset=ds, eval_dataset=eval_ds, ref_model=ref_model)


def train_logs(t):
    return [h for h in t.state.log_history if "loss" in h]


# ------------------------------------------------------------------------------------------------ twins
def test_seq_logp_sum_twin():
    g = torch.Generator().manual_seed(0)
    lens = [1, 63, 64, 65, 129, 0, 1000]
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist() + [sum(lens) + 7], dtype=torch.int32)
    nll = torch.rand(sum(lens) + 7, generator=g) * 4
    got = ops.seq_logp_sum(nll, cu, len(lens))
    c = cu.tolist()
    want = torch.stack([-nll[c[s]:c[s + 1]].double().sum() for s in range(len(lens))])
    assert got.dtype == torch.float32 and got[5].item() == 0.0
    assert torch.allclose(got.double(), want, rtol=1e-5, atol=0)
    assert torch.equal(ref.seq_logp_sum(nll.double(), cu, 3), ref.seq_logp_sum(nll.double(), cu, len(lens))[:3])


def test_scale_rows_by_seq_twin():
    g = torch.Generator().manual_seed(1)
    lens, tail = [1, 63, 0, 65], 5
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist() + [sum(lens) + tail], dtype=torch.int32)
    x = torch.randn(sum(lens) + tail, 24, generator=g)
    coef, gs = torch.tensor([0.0, -1.5, 9.0, 0.37]), torch.tensor([1.0 / 7.0])
    c = cu.tolist()
    want = torch.zeros_like(x, dtype=torch.float64)
    for s in range(4):
        want[c[s]:c[s + 1]] = x[c[s]:c[s + 1]].double() * (coef[s].double() * gs.double())
    got = ops.scale_rows_by_seq(x, coef, cu, 4, gs)
    assert torch.allclose(got.double(), want, rtol=1e-6, atol=0)
    assert not got[c[4]:].view(torch.int32).any()  # tail rows: +0
    xb = x.to(torch.bfloat16)
    gb = ops.scale_rows_by_seq(xb, coef, cu, 4, gs)  # bf16: one fp32 product of the two scalars, one per element, one RNE
    assert torch.equal(gb, (xb.float() * (coef * gs)[torch.repeat_interleave(torch.arange(5), torch.tensor(lens + [tail]))
                                                     .clamp(max=3)][:, None]).to(torch.bfloat16)
                       .masked_fill(torch.arange(x.shape[0])[:, None] >= c[4], 0.0))
    y = x.clone()
    assert ops.scale_rows_by_seq(y, coef, cu, 4, gs, inplace=True) is y and torch.equal(y, got)


def test_dpo_pair_twin_and_gradcheck():
    beta, P = 0.1, 9
    g = torch.Generator().manual_seed(2)
    rl = -40 * torch.rand(2 * P, generator=g, dtype=torch.float64)
    delta = torch.tensor([0.0, 1e-3, -1e-3, 5.0, -5.0, 1e5, -1e5, 2.0, -0.7], dtype=torch.float64)
    lp = rl.clone()
    lp[0::2] += delta
    inv = torch.tensor([1.0 / P], dtype=torch.float64)
    st = ref.dpo_pair(lp, rl, inv, beta)
    assert torch.isfinite(st).all()
    d = (lp[0::2] - lp[1::2]) - (rl[0::2] - rl[1::2])
    want_loss = torch.nn.functional.softplus(-beta * d)
    want_coef = -beta * torch.sigmoid(-beta * d) / P
    assert torch.allclose(st[0], want_loss, rtol=1e-12, atol=1e-300)
    assert torch.allclose(st[1], want_coef, rtol=1e-12, atol=1e-300)
    assert abs(st[0][0].item() - LN2) < 1e-15 and st[1][0].item() == -beta / 2 / P
    st32 = ref.dpo_pair(lp.float(), rl.float(), inv.float(), beta)
    assert torch.isfinite(st32).all()
    live = delta.abs() < 100
    assert torch.allclose(st32[0][live].double(), want_loss[live], rtol=1e-4, atol=0)
    loss, _ = ops.dpo_loss(lp.float(), rl.float(), inv.float(), beta)
    assert abs(loss.item() - want_loss.sum().item() / P) < 1e-3 * want_loss.sum().item() / P
    x = (rl + torch.randn(2 * P, generator=g, dtype=torch.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: ops.dpo_loss(v, rl, inv, 0.3)[0], (x,))
    with pytest.raises(ValueError):
        ops.dpo_loss(lp[:-1], rl[:-1], inv, beta)


def test_lm_head_seq_logps_matches_autograd():
    g = torch.Generator().manual_seed(3)
    h = torch.randn(24, 16, generator=g, requires_grad=True)
    w = torch.randn(40, 16, generator=g, requires_grad=True)
    cu = torch.tensor([0, 5, 12, 12, 21, 24], dtype=torch.int32)
    labels = torch.randint(0, 40, (24,), generator=g)
    labels[:2] = -100
    labels[21:] = -100
    c = torch.tensor([0.7, -1.3, 2.0, 0.0])
    logps, _ = ops.lm_head_seq_logps(h, w, labels, cu, 4)
    gh, gw = torch.autograd.grad((logps * c).sum(), (h, w))
    h64, w64 = h.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    lp = torch.log_softmax(h64 @ w64.t(), -1)
    tok = torch.where(labels != -100, lp.gather(1, labels.clamp(min=0)[:, None])[:, 0], torch.zeros((), dtype=torch.float64))
    cl = cu.tolist()
    want = torch.stack([tok[cl[s]:cl[s + 1]].sum() for s in range(4)])
    rh, rw = torch.autograd.grad((want * c.double()).sum(), (h64, w64))
    assert torch.allclose(logps.double(), want, rtol=1e-5) and logps[2].item() == 0.0
    assert torch.allclose(gh.double(), rh, rtol=1e-4, atol=1e-5) and torch.allclose(gw.double(), rw, rtol=1e-4, atol=1e-5)
    assert not gh[21:].any() and not gh[cl[3]:cl[4]].any()  # pad rows; the sequence with dlogps == 0
    assert torch.equal(h, h.detach().clone())


# ------------------------------------------------------------------------------------------------ tokenisation, collation
@pytest.fixture(scope="module")
def tokenizer():
    from llm_fine_tune_distributed_amd.data.tokenizer import load_tokenizer
    return load_tokenizer()


def test_preference_tokenisation(tokenizer, tmp_path):
    rows = synthetic_preferences(6, seed=1)
    assert all(set(r) == {"prompt", "chosen", "rejected"} and r["chosen"] != r["rejected"] for r in rows)
    eos = tokenizer.eos_token_id
    rows[1]["chosen"] += tokenizer.eos_token  # already ends with EOS: not appended twice
    rows[2] = {"prompt": [{"role": "user", "content": rows[2]["prompt"]}],  # TRL's conversational format
               "chosen": [{"role": "assistant", "content": rows[2]["chosen"]}],
               "rejected": [{"role": "assistant", "content": rows[2]["rejected"]}]}
    ds = tokenize_preference_rows(rows, tokenizer)
    assert len(ds) == 12
    for i, r in enumerate(rows):
        msgs = [{"role": "user", "content": r["prompt"]}] if isinstance(r["prompt"], str) else r["prompt"]
        pids = tokenizer.encode(tokenizer.apply_chat_template(msgs, tokenize=False, add_generation_prompt=True))
        c, rj = ds[2 * i], ds[2 * i + 1]
        ls = int(ds.loss_start[2 * i])
        assert ls == int(ds.loss_start[2 * i + 1]) == len(pids)      # loss_start: the prompt length
        assert c[:ls] == rj[:ls] == pids                              # both sequences share the prompt ids
        for s in (c, rj):
            assert s[-1] == eos and s[-2] != eos                      # EOS once
    text = rows[0]["chosen"]
    assert ds[0][int(ds.loss_start[0]):] == tokenizer.encode(text) + [eos]  # completion tokenised on its own
    # truncation: max_prompt_length keeps the prompt's tail, max_length cuts the completion's tail
    full_p = int(ds.loss_start[0])
    tr = tokenize_preference_rows(rows, tokenizer, max_length=full_p + 2, max_prompt_length=full_p - 3)
    assert int(tr.loss_start[0]) == full_p - 3 and tr[0][:full_p - 3] == ds[0][3:full_p]
    assert len(tr[0]) == full_p + 2 and tr[0][full_p - 3:] == ds[0][full_p:full_p + 5]
    # the main-process-first cache, under its own fingerprint
    cache = str(tmp_path / "cache")
    a = cached_tokenize_preferences(rows, tokenizer, cache, max_length=64)
    files = sorted(os.listdir(cache))
    assert len(files) == 1 and files[0].startswith("tokenized-")
    import llm_fine_tune_distributed_amd.data.preference as pref
    orig = pref.tokenize_preference_rows
    pref.tokenize_preference_rows = lambda *a, **k: (_ for _ in ()).throw(AssertionError("cache missed"))
    try:
        b = cached_tokenize_preferences(rows, tokenizer, cache, max_length=64)
    finally:
        pref.tokenize_preference_rows = orig
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.offsets, b.offsets) and torch.equal(a.loss_start, b.loss_start)
    cached_tokenize_preferences(rows, tokenizer, cache, max_length=32)
    assert len(os.listdir(cache)) == 2  # other options: another fingerprint


def test_preference_collator_matches_hand_built_batch():
    seqs = [[11, 12, 13, 21, 22], [11, 12, 13, 31], [14, 15, 41, 42, 43], [14, 15, 51, 52]]
    ds = TokenizedDataset.from_token_lists(seqs, [3, 3, 2, 2])
    refs = torch.tensor([-1.0, -2.0, -3.0, -4.0])
    b = PreferenceCollator(0, 8, ref_logps=refs)(ds, torch.tensor([1, 0]))
    order = [2, 3, 0, 1]  # pair 1 (chosen, rejected), then pair 0
    ids = sum((seqs[i] for i in order), [])
    assert b["input_ids"].tolist() == ids + [0] * (24 - len(ids))
    assert b["cu_seqlens"].tolist() == [0, 5, 9, 14, 18, 24] and b["cu_seqlens"].dtype == torch.int32
    assert b["position_ids"].tolist()[:18] == [0, 1, 2, 3, 4, 0, 1, 2, 3, 0, 1, 2, 3, 4, 0, 1, 2, 3]
    i = -100
    assert b["labels"].tolist() == [i, 41, 42, 43, i, i, 51, 52, i, i, i, 21, 22, i, i, i, 31, i] + [i] * 6
    assert b["shifted"] and b["n_seqs"] == 4 and b["num_items"] == 2 and b["num_samples"] == 2
    assert b["num_tokens"] == 18 and b["max_seqlen"] == 6
    assert b["ref_logps"].tolist() == [-3.0, -4.0, -1.0, -2.0]


# ------------------------------------------------------------------------------------------------ trainer
def test_dpo_learns(tmp_path):
    m = tiny_model()
    ds = token_pairs(16, m.config.vocab_size)
    t = dpo_trainer(tmp_path, m, ds, eval_ds=ds, max_steps=24)
    t.train()
    logs = train_logs(t)
    assert len(logs) == 24
    print("losses:", [round(h["loss"], 5) for h in logs])
    assert abs(logs[0]["loss"] - LN2) < 1e-5
    tail = logs[16:]
    assert sum(h["loss"] for h in tail) / 8 < 0.45
    assert all(h["rewards/accuracies"] >= 0.9 for h in tail)
    for k in ("rewards/chosen", "rewards/rejected", "rewards/margins", "logps/chosen", "logps/rejected", "grad_norm",
              "learning_rate", "epoch", "num_tokens"):
        assert k in logs[0], k
    assert len(glob.glob(os.path.join(str(tmp_path), "ref_logps-*.pt"))) == 1
    ev = t.evaluate()
    for k in ("eval_loss", "eval_rewards/chosen", "eval_rewards/rejected", "eval_rewards/accuracies",
              "eval_rewards/margins", "eval_logps/chosen", "eval_logps/rejected"):
        assert k in ev and math.isfinite(ev[k]), k
    assert ev["eval_loss"] < 0.45 and ev["eval_rewards/accuracies"] >= 0.9
    out = t.state.log_history[-2]
    assert out["train_samples_per_second"] > 0  # samples are pairs: 24 steps x 4
    assert t.state.samples_seen == 96 and t.state.tokens_seen == sum(h["num_tokens"] - p["num_tokens"]
                                                                     for h, p in zip(logs[1:], logs[:-1])) + logs[0]["num_tokens"]


def test_dpo_ref_model_and_lora(tmp_path):
    """A fresh LoRA run scores the reference with B = 0, i.e. the base model: the same reference log-probabilities as
    an explicit ``ref_model=`` with the base weights, and a first loss of ln 2."""
    ds = token_pairs(8, 1024)
    t = dpo_trainer(tmp_path / "a", tiny_model(), ds, max_steps=2, freeze_policy="lora", lora_r=4, lora_dropout=0.0)
    t.train()
    assert abs(train_logs(t)[0]["loss"] - LN2) < 1e-5
    t2 = dpo_trainer(tmp_path / "b", tiny_model(seed=5), ds, ref_model=tiny_model(), max_steps=1)
    t2.train()
    assert t2._ref_model is None  # released
    assert torch.allclose(t.collator.ref_logps, t2.collator.ref_logps, rtol=1e-5)
    assert abs(train_logs(t2)[0]["loss"] - LN2) > 1e-4  # the policy (seed 5) is not the reference


def _grads_of_step(tmp, per_dev, ga, merge):
    m = tiny_model()
    ds = token_pairs(4, m.config.vocab_size, seed=4)
    t = dpo_trainer(tmp, m, ds, per_device_train_batch_size=per_dev, gradient_accumulation_steps=ga, max_steps=1,
                    ga_merge_max_tokens=merge)
    grads = {}
    step = t.optimizer.step

    def capture(*a, **k):  # the step's accumulated gradients, as the optimizer receives them
        grads["flat"] = t.engine.grad_flat.clone()
        return step(*a, **k)

    t.optimizer.step = capture
    t.train()
    return grads["flat"], train_logs(t)[0]


@pytest.mark.parametrize("merge", [0, 32768])
def test_dpo_grad_accumulation_equals_big_batch(tmp_path, merge):
    big, lb = _grads_of_step(tmp_path / "big", 4, 1, merge)
    ga, lg = _grads_of_step(tmp_path / "ga", 2, 2, merge)
    e = ((ga - big).norm() / big.norm()).item()
    print("GA 2 x 2 against 1 x 4, merge", merge, ": relative gradient difference", e)
    assert big.norm() > 0 and e < 1e-5
    assert abs(lb["loss"] - lg["loss"]) < 1e-6 and abs(lb["rewards/margins"] - lg["rewards/margins"]) < 1e-6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out_dir, per_dev):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import llm_fine_tune_distributed_amd.parallel.process_group as pgm
    pgm._STATE = None
    torch.manual_seed(0)
    m = tiny_model(seed=3)
    ds = token_pairs(8, m.config.vocab_size, seed=7)
    t = dpo_trainer(out_dir, m, ds, per_device_train_batch_size=per_dev, learning_rate=1e-3, max_steps=2,
                    ddp_check_sync_every=1, ddp_bucket_cap_mb=0.05, ddp_first_bucket_mb=0.01)
    t.train()
    torch.save({"params": t.engine.params_by_name().clone(), "log": train_logs(t), "ref": t.collator.ref_logps},
               os.path.join(out_dir, f"r{world}_{rank}.pt"))
    pgm.cleanup_distributed()


def test_dpo_two_ranks_match_single_process():
    d = tempfile.mkdtemp()
    _rank(0, 1, _free_port(), d, 4)
    mp.spawn(_rank, args=(2, _free_port(), d, 2), nprocs=2, join=True)
    single = torch.load(os.path.join(d, "r1_0.pt"))
    r0, r1 = (torch.load(os.path.join(d, f"r2_{r}.pt")) for r in range(2))
    assert torch.equal(r0["params"], r1["params"])  # ranks bit-identical
    assert torch.allclose(r0["ref"], single["ref"], rtol=1e-5) and torch.equal(r0["ref"], r1["ref"])
    assert torch.allclose(r0["params"], single["params"], atol=1e-5, rtol=1e-4)
    for a, b in zip(single["log"], r0["log"]):
        assert abs(a["loss"] - b["loss"]) < 1e-4
        assert abs(a["grad_norm"] - b["grad_norm"]) < 1e-3


def test_dpo_resume(tmp_path):
    ds = token_pairs(16, 1024, seed=2)
    kw = dict(max_steps=4, save_strategy="steps", save_steps=2, save_total_limit=5)
    full = dpo_trainer(tmp_path / "full", tiny_model(), ds, **kw)
    full.train()
    want = {h["step"]: h["loss"] for h in train_logs(full)}
    first = dpo_trainer(tmp_path / "run", tiny_model(), ds, **kw)
    first.args.max_steps = 2
    first.train()
    ck = os.path.join(str(tmp_path / "run"), "checkpoint-2")
    assert os.path.isdir(ck)
    second = dpo_trainer(tmp_path / "run", tiny_model(seed=9), ds, **kw)
    second.train(resume_from_checkpoint=ck)
    got = {h["step"]: h["loss"] for h in train_logs(second)}
    assert sorted(got) == [1, 2, 3, 4]  # (steps 1-2: the checkpoint's log history)
    assert got[3] == want[3] and got[4] == want[4], (got, want)
    assert torch.equal(second.engine.params_by_name(), full.engine.params_by_name())
    for f in glob.glob(os.path.join(str(tmp_path / "run"), "ref_logps-*.pt")):
        os.remove(f)
    third = dpo_trainer(tmp_path / "run", tiny_model(seed=9), ds, **kw)
    with pytest.raises(FileNotFoundError, match="ref"):
        third.train(resume_from_checkpoint=ck)


def test_dpo_config_refusals(tmp_path):
    from llm_fine_tune_distributed_amd.train import DPOConfig, DPOTrainer, SFTConfig
    a = DPOConfig()
    assert a.beta == 0.1 and a.learning_rate == 1e-6 and a.loss_type == "sigmoid" and a.max_prompt_length is None
    assert isinstance(a, SFTConfig) and DPOConfig(neftune_noise_alpha=5.0).neftune_noise_alpha == 5.0
    for bad in (dict(context_parallel_size=2), dict(packing=True), dict(label_smoothing_factor=0.1),
                dict(loss_type="ipo"), dict(loss_type="nll"), dict(beta=0.0)):
        with pytest.raises(ValueError):
            DPOConfig(**bad)
    assert isinstance(a.replace(beta=0.5), DPOConfig) and a.replace(beta=0.5).beta == 0.5
    with pytest.raises(TypeError):
        DPOTrainer(model=tiny_model(), args=SFTConfig(output_dir=str(tmp_path)), train_dataset=token_pairs(4, 1024))
    a.context_parallel_size = 2  # set after construction: the trainer refuses it too
    with pytest.raises(NotImplementedError, match="context parallel"):
        DPOTrainer(model=tiny_model(), args=a, train_dataset=token_pairs(4, 1024))
    m = tiny_model()
    m.model.layers[0].self_attn.cp_group = object()
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.sequence_logps(torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long))


def test_sft_logs_unchanged(tmp_path):
    """The hooks DPOTrainer overrides leave SFTTrainer's log entries as they were: keys and their order."""
    from llm_fine_tune_distributed_amd.train import SFTConfig, SFTTrainer
    ds = TokenizedDataset.synthetic(16, 1024, 5, 20, seed=7)
    a = SFTConfig(output_dir=str(tmp_path), per_device_train_batch_size=4, max_steps=1, logging_steps=1, jsonl_log=False,
                  save_strategy="no")
    t = SFTTrainer(model=tiny_model(), args=a, train_dataset=ds, eval_dataset=ds)
    t.train()
    assert list(train_logs(t)[0]) == ["loss", "grad_norm", "learning_rate", "epoch", "mean_token_accuracy", "entropy",
                                      "num_tokens", "step"]
    assert list(t.evaluate()) == ["eval_loss", "eval_runtime", "eval_samples_per_second", "eval_steps_per_second",
                                  "eval_mean_token_accuracy", "eval_entropy", "eval_num_tokens", "epoch"]


def test_train_cli_dpo(tmp_path, monkeypatch):
    from llm_fine_tune_distributed_amd.cli import train as cli
    out = tmp_path / "out"
    monkeypatch.setenv("OUTPUT_DIR", str(out))
    monkeypatch.setenv("EPOCHS", "1")
    monkeypatch.setenv("BATCH_SIZE", "2")
    monkeypatch.setenv("LEARNING_RATE", "1e-4")
    monkeypatch.setenv("AIM_REPO", str(tmp_path / "aim"))
    data = tmp_path / "prefs.jsonl"
    with open(data, "w") as f:
        for r in synthetic_preferences(24, seed=3):
            f.write(json.dumps(r) + "\n")
    cli.main(["--trainer", "dpo", "--model", "tiny", "--dataset", str(data), "--max-steps", "2", "--grad-accum", "1",
              "--no-gradient-checkpointing", "--max-length", "128", "--set", "beta=0.25", "--set", "logging_steps=1"])
    resolved = json.load(open(out / "sft_config.json"))
    assert resolved["beta"] == 0.25 and resolved["loss_type"] == "sigmoid"
    logs = [json.loads(l) for l in open(out / "checkpoints" / "metrics.jsonl")]
    steps = [h for h in logs if "loss" in h]
    assert len(steps) == 2
    for k in ("rewards/chosen", "rewards/rejected", "rewards/accuracies", "rewards/margins"):
        assert all(k in h for h in steps), k
    assert glob.glob(str(out / "checkpoints" / "ref_logps-*.pt"))
