"""Reward modelling on the CPU reference path: the twins of the three reward ops against plain autograd in fp64, the
score head through the model, HF ``...ForSequenceClassification`` directories, the freeze policies, ``RewardTrainer``
(learning, margins, implicit-prompt rows, gradient accumulation, resume, two gloo ranks), reward models as GRPO reward
functions, the CLI switch and the refusals."""
import contextlib
import dataclasses
import hashlib
import io
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
from llm_fine_tune_distributed_amd.data.preference import (PreferenceCollator, preference_margins,
                                                           tokenize_preference_rows)
from llm_fine_tune_distributed_amd.data.synthetic import synthetic_preferences
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.models.config import PRESETS, tiny
from llm_fine_tune_distributed_amd.ops import reference as ref
from llm_fine_tune_distributed_amd.train import checkpoint as ckpt

LN2 = math.log(2.0)
V = 1024
GOOD, BAD = 5, 6  # the last token of a chosen / a rejected sequence of the separable pairs


def reward_model(preset="tiny-llama", seed=0, dtype=torch.float32):
    return build_model(dataclasses.replace(get_config(preset), num_labels=1), device="cpu", dtype=dtype, seed=seed)


def separable_pairs(n, seed=0):
    """n pairs over a shared random prefix of 3-10 tokens; the chosen sequence ends in GOOD, the rejected in BAD."""
    g = torch.Generator().manual_seed(seed)
    seqs, starts = [], []
    for _ in range(n):
        p = torch.randint(8, V, (int(torch.randint(3, 11, (1,), generator=g)),), generator=g).tolist()
        seqs += [p + [GOOD], p + [BAD]]
        starts += [len(p), len(p)]
    return TokenizedDataset.from_token_lists(seqs, starts)


def reward_trainer(out, model, ds, eval_ds=None, **kw):
    from llm_fine_tune_distributed_amd.train import RewardConfig, RewardTrainer
    base = dict(output_dir=str(out), per_device_train_batch_size=4, learning_rate=1e-3, lr_scheduler_type="constant",
                logging_steps=1, jsonl_log=False, save_strategy="no", dataloader_drop_last=True)
    base.update(kw)
    return RewardTrainer(model=model, args=RewardConfig(**base), train_dataset=ds, eval_dataset=eval_ds)


def train_logs(t):
    return [h for h in t.state.log_history if "loss" in h]


def quiet_train(t, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return t.train(**kw)


# ------------------------------------------------------------------------------------------------ twins
SEG = [1, 5, 0, 3, 2]  # an empty segment in the middle; a 4-row pad segment follows


def _score_case(H=24, dtype=torch.float64):
    g = torch.Generator().manual_seed(0)
    cu = torch.tensor([0] + torch.tensor(SEG).cumsum(0).tolist() + [sum(SEG) + 4], dtype=torch.int32)
    h = torch.randn(sum(SEG) + 4, H, generator=g, dtype=torch.float64).to(dtype)
    w = torch.randn(1, H, generator=g, dtype=torch.float64).to(dtype)
    return h, w, cu


@pytest.mark.parametrize("H", [8, 24, 520])
def test_seq_score_against_autograd_fp64(H):
    h, w, cu = _score_case(H)
    c = cu.tolist()
    last = [c[s + 1] - 1 for s in range(len(SEG)) if SEG[s]]
    coef = torch.tensor([0.5, -2.0, 1e30, 3.0, -1.0], dtype=torch.float64)  # the empty segment's weight must not matter
    for n_seqs in (len(SEG), 2):
        hh, ww = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
        got = ops.seq_score(hh, ww, cu, n_seqs)
        assert got.dtype == torch.float64 and got.shape == (n_seqs,)
        (got * coef[:n_seqs]).sum().backward()
        h2, w2 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
        rows = [s for s in range(n_seqs) if SEG[s]]
        want = torch.zeros(n_seqs, dtype=torch.float64)
        plain = torch.stack([(h2[c[s + 1] - 1] * w2[0]).sum() for s in rows])
        (plain * coef[rows]).sum().backward()
        want[rows] = plain.detach()
        assert torch.allclose(got.detach(), want, rtol=1e-12, atol=1e-13)
        if n_seqs > 2:
            assert got[2].item() == 0.0 and not math.copysign(1.0, got[2].item()) < 0  # the empty segment: +0
        assert torch.allclose(hh.grad, h2.grad, rtol=1e-12, atol=0) and torch.allclose(ww.grad, w2.grad, rtol=1e-12)
        keep = torch.zeros(h.shape[0], dtype=torch.bool)
        keep[[r for r in last if r < c[n_seqs]]] = True
        assert not hh.grad[~keep].any()  # empty segment, pad segment, segments past n_seqs, inner rows: zero rows
        assert hh.grad[keep].abs().sum(1).min() > 0


def test_seq_score_twin_details():
    h, w, cu = _score_case(24, torch.float32)
    hb, wb = h.to(torch.bfloat16), w.to(torch.bfloat16)
    s = ref.seq_score(hb, wb, cu, len(SEG))
    assert s.dtype == torch.float32
    assert torch.equal(ref.seq_score(hb, wb, cu, 2), s[:2])
    g = torch.tensor([1.0, -0.5, 1e30, 2.0, 0.25])
    dh, dw = ref.seq_score_bwd(g, hb, wb, cu, len(SEG))
    assert dh.dtype == torch.bfloat16 and dw.dtype == torch.float32 and torch.isfinite(dh.float()).all()
    c = cu.tolist()
    assert torch.equal(dh[c[2] - 1], (g[1] * wb[0].float()).to(torch.bfloat16))  # untouched by the empty segment 2
    assert not dh[c[5]:].view(torch.int16).any()  # pad rows: +0
    assert ref.seq_score_bwd(g, hb, wb, cu, len(SEG), need_dh=False)[0] is None
    assert ref.seq_score_bwd(g, hb, wb, cu, len(SEG), need_dw=False)[1] is None
    with pytest.raises(ValueError):
        ops.seq_score(h, w, cu, len(SEG) + 2)  # more sequences than segments
    with pytest.raises(ValueError):
        ops.seq_score(h, w[:, :8], cu, 2)
    with pytest.raises(ValueError):
        ref.seq_score(h[:, :12], w[:, :12], cu, 2)  # H % 8


def test_seq_score_frozen_halves():
    h, w, cu = _score_case()
    hh = h.clone().requires_grad_(True)
    ops.seq_score(hh, w, cu, 3).sum().backward()  # frozen head
    assert hh.grad is not None
    ww = w.clone().requires_grad_(True)
    ops.seq_score(h, ww, cu, 3).sum().backward()  # frozen trunk
    assert ww.grad is not None
    p = torch.nn.Parameter(w.clone())
    p.main_grad, p._sftamd_fresh, p._sftamd_remaining = torch.zeros_like(p), True, 1
    ops.seq_score(h, p, cu, 3).sum().backward()
    assert p.grad is None and torch.allclose(p.main_grad, ww.grad) and p._sftamd_remaining == 0


@pytest.mark.parametrize("c", [0.0, 0.01])
@pytest.mark.parametrize("with_margin", [False, True])
def test_reward_pair_against_autograd_fp64(c, with_margin):
    P = 9
    g = torch.Generator().manual_seed(2)
    z = torch.tensor([0.0, 1e-3, -1e-3, 5.0, -5.0, 1e4, -1e4, 2.0, -0.7], dtype=torch.float64)
    rr = torch.randn(P, generator=g, dtype=torch.float64)
    scores = torch.stack([rr + z, rr], dim=1).reshape(-1)
    m = torch.rand(P, generator=g, dtype=torch.float64) if with_margin else None
    inv = torch.tensor([1.0 / P], dtype=torch.float64)
    st = ref.reward_pair(scores, m, inv, c)
    assert st.shape == (4, P) and torch.isfinite(st).all()
    x = scores.clone().requires_grad_(True)
    zz = x[0::2] - x[1::2] - (m if with_margin else 0.0)
    cc = float(torch.tensor(c, dtype=torch.float32))  # the kernel's coefficient is a float
    per = -torch.nn.functional.logsigmoid(zz) + cc * (x[0::2] + x[1::2]) ** 2
    (per.sum() / P).backward()
    assert torch.allclose(st[0], per.detach(), rtol=1e-12, atol=1e-300)
    assert torch.allclose(st[1], x.grad[0::2], rtol=1e-11, atol=1e-300)
    assert torch.allclose(st[2], x.grad[1::2], rtol=1e-11, atol=1e-300)
    assert torch.equal(st[3], zz.detach())
    if c == 0.0:
        assert torch.equal(st[2].view(torch.int64), (-st[1]).view(torch.int64))
        if not with_margin:
            assert abs(st[0][0].item() - LN2) < 1e-15 and st[1][0].item() == -0.5 / P
    y = scores.clone().requires_grad_(True)
    loss, st2 = ops.reward_pair_loss(y, m, inv, c)
    loss.backward()
    assert torch.allclose(loss, per.detach().sum() / P, rtol=1e-12) and torch.equal(st2, st)
    assert torch.allclose(y.grad, x.grad, rtol=1e-11, atol=1e-300)
    st32 = ref.reward_pair(scores.float(), None if m is None else m.float(), inv.float(), c)
    assert st32.dtype == torch.float32 and torch.isfinite(st32).all()
    with pytest.raises(ValueError):
        ops.reward_pair_loss(scores[:-1], None, inv)
    with pytest.raises(ValueError):
        ops.reward_pair_loss(scores, torch.zeros(P + 1, dtype=torch.float64), inv)
    with pytest.raises(ValueError):
        ops.reward_pair_loss(scores, None, inv, -1.0)


# ------------------------------------------------------------------------------------------------ model + HF layout
LENS = [10, 7, 1]


def _packed(seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (sum(LENS),), generator=g)
    cu = torch.tensor([0, 10, 17, 18], dtype=torch.int32)
    return ids, cu


@pytest.mark.parametrize("mt", ["smollm3", "llama", "qwen3", "qwen2"])
def test_hf_sequence_classification_parity(mt, tmp_path):
    from transformers import AutoModelForSequenceClassification
    m = build_model(tiny(mt, num_labels=1), dtype=torch.float32, seed=3)
    assert m.lm_head is None and tuple(m.score.shape) == (1, m.config.hidden_size) and m.score.dtype == torch.float32
    assert all(p._sftamd_uses == 1 for p in m.parameters())
    ids, cu = _packed()
    with torch.no_grad():
        s = m.sequence_scores(ids, cu_seqlens=cu)
    d = str(tmp_path / "rm")
    ckpt.save_pretrained(m, d)
    cfg = json.load(open(os.path.join(d, "config.json")))
    assert cfg["architectures"][0].endswith("ForSequenceClassification") and cfg["num_labels"] == 1
    assert cfg["pad_token_id"] is not None
    sd = ckpt.load_state_dict(d)
    assert "lm_head.weight" not in sd and tuple(sd["score.weight"].shape) == (1, m.config.hidden_size)
    hf = AutoModelForSequenceClassification.from_pretrained(d, dtype=torch.float32).eval()
    got, o = [], 0
    for L in LENS:  # one sequence per call
        with torch.no_grad():
            got.append(hf(input_ids=ids[o:o + L][None]).logits[0, 0])
        o += L
    err = (torch.stack(got) - s).abs().max().item()
    print(mt, "max |hf - sequence_scores|", err)
    assert err < 1e-4
    m2 = ckpt.from_pretrained(d, dtype=torch.float32)
    assert m2.is_reward_model
    with torch.no_grad():
        assert torch.equal(m2.sequence_scores(ids, cu_seqlens=cu), s)  # round trip: bit-equal
    # a padded [B, T] batch scores column lengths[b] - 1, column T - 1 by default
    pad = torch.full((2, 10), int(m.config.pad_token_id))
    pad[0], pad[1, :7] = ids[:10], ids[10:17]
    with torch.no_grad():
        sp = m.sequence_scores(pad, lengths=torch.tensor([10, 7]))
        assert torch.allclose(sp, s[:2], atol=1e-5)
        assert torch.equal(m.sequence_scores(pad)[0], sp[0])


def test_causal_directory_loads_as_reward_model(tmp_path):
    lm = build_model(get_config("tiny-llama"), dtype=torch.float32, seed=1)
    d = str(tmp_path / "lm")
    ckpt.save_pretrained(lm, d)
    assert "lm_head.weight" in ckpt.load_state_dict(d)
    a = ckpt.from_pretrained(d, dtype=torch.float32, num_labels=1, seed=4)
    b = ckpt.from_pretrained(d, dtype=torch.float32, num_labels=1, seed=4)
    c = ckpt.from_pretrained(d, dtype=torch.float32, num_labels=1, seed=5)
    assert a.is_reward_model and a.lm_head is None
    assert torch.equal(a.score, b.score) and not torch.equal(a.score, c.score)  # a fresh head, equal for equal seeds
    assert 0.2 * a.config.initializer_range < a.score.std().item() < 3 * a.config.initializer_range
    assert torch.equal(a.model.embed_tokens, lm.model.embed_tokens)
    assert torch.equal(a.model.layers[1].mlp.down_proj, lm.model.layers[1].mlp.down_proj)
    out = str(tmp_path / "rm")
    ckpt.save_pretrained(a, out)
    sd = ckpt.load_state_dict(out)
    assert "lm_head.weight" not in sd and "score.weight" in sd
    assert not ckpt.from_pretrained(d, dtype=torch.float32).is_reward_model  # the directory itself is a causal LM


def test_presets_unchanged_without_num_labels():
    """With num_labels None nothing changes: every preset's config.json is byte-identical to what it was before the
    field existed (golden digests), and a causal model has no score parameter."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "preset_config_sha256.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(PRESETS)
    for name, make in PRESETS.items():
        cfg = make()
        assert cfg.num_labels is None
        text = json.dumps(cfg.to_hf_dict(), indent=2)
        assert "num_labels" not in text and "ForSequenceClassification" not in text
        assert hashlib.sha256(text.encode()).hexdigest() == want[name], name
    lm = build_model(get_config("tiny"), dtype=torch.float32)
    assert lm.score is None and not any("score" in n for n, _ in lm.named_parameters())
    assert lm.model.embed_tokens._sftamd_uses == 2
    for bad in (0, 2, 3):
        with pytest.raises(ValueError, match="num_labels"):
            tiny(num_labels=bad)


def test_refused_methods():
    rm, lm = reward_model(), build_model(get_config("tiny-llama"), dtype=torch.float32)
    ids, cu = _packed()
    with pytest.raises(RuntimeError, match="reward model"):
        lm.sequence_scores(ids, cu_seqlens=cu)
    for call in (lambda: rm(ids[None], labels=ids[None]), lambda: rm(ids[None]), lambda: rm.logits_rows(ids),
                 lambda: rm.token_logps(ids, ids), lambda: rm.sequence_logps(ids, ids),
                 lambda: rm.policy_loss(ids, ids, torch.zeros(1)), lambda: rm.lm_head_weight,
                 lambda: rm.distill_loss(ids, ids, torch.zeros(1))):
        with pytest.raises(RuntimeError, match="reward model"):
            call()
    from llm_fine_tune_distributed_amd.inference.generation import generate
    with pytest.raises(RuntimeError, match="reward model"):
        generate(rm, ids[:4].tolist(), max_new_tokens=2)
    rm.model.layers[0].self_attn.cp_group = object()
    with pytest.raises(NotImplementedError, match="context parallel"):
        rm.sequence_scores(ids, cu_seqlens=cu)


def test_freeze_policies_keep_the_head(tmp_path):
    from llm_fine_tune_distributed_amd.models.freeze import apply_freeze_policy
    rm = reward_model()
    apply_freeze_policy(rm, "last_n_layers", n_last=1)
    on = {n for n, p in rm.named_parameters() if p.requires_grad}
    assert "score" in on and "model.embed_tokens" not in on and not any(n.startswith("model.layers.0.") for n in on)
    assert any(n.startswith("model.layers.3.") for n in on)
    rm = reward_model(seed=2)
    ds = separable_pairs(8)
    t = reward_trainer(tmp_path, rm, ds, max_steps=3, freeze_policy="lora", lora_r=4, lora_dropout=0.0)
    on = {n for n, p in rm.named_parameters() if p.requires_grad}
    assert "score" in on and all(n == "score" or ".lora." in n for n in on)
    before = rm.score.detach().clone()
    quiet_train(t)
    assert not torch.equal(rm.score, before)
    ids, cu = _packed()
    rm.eval()
    with torch.no_grad():
        live = rm.sequence_scores(ids, cu_seqlens=cu)
    t.save_model(str(tmp_path / "adapters"))
    ac = json.load(open(tmp_path / "adapters" / "adapter_config.json"))
    assert ac["task_type"] == "SEQ_CLS" and "score.weight" in ckpt.load_state_dict(str(tmp_path / "adapters"))
    t.save_model(str(tmp_path / "merged"), merge_lora=True)
    assert not os.path.exists(tmp_path / "merged" / "adapter_model.safetensors")
    merged = ckpt.from_pretrained(str(tmp_path / "merged"), dtype=torch.float32).eval()
    with torch.no_grad():
        got = merged.sequence_scores(ids, cu_seqlens=cu)
    assert torch.allclose(got, live, atol=1e-5), (got, live)


# ------------------------------------------------------------------------------------------------ data
def test_implicit_prompt_rows_and_margins():
    from llm_fine_tune_distributed_amd.data.tokenizer import load_tokenizer
    tk = load_tokenizer()
    rows = [{"chosen": "the river is north", "rejected": "no idea", "margin": 1.5},
            {"chosen": [{"role": "user", "content": "where?"}, {"role": "assistant", "content": "north"}],
             "rejected": [{"role": "user", "content": "where?"}, {"role": "assistant", "content": "dunno"}]}]
    ds = tokenize_preference_rows(rows, tk, max_length=64)
    assert len(ds) == 4 and ds.loss_start.tolist() == [0, 0, 0, 0]
    seq = lambda i: ds.tokens[ds.offsets[i]:ds.offsets[i + 1]].tolist()  # noqa: E731
    assert seq(0) == tk.encode("the river is north") + [tk.eos_token_id]
    whole = tk.encode(tk.apply_chat_template(rows[1]["chosen"], tokenize=False))  # no generation prompt, no extra EOS
    assert len(whole) > 64 and seq(2) == whole[:64]  # max_length cuts the tail
    assert len(tokenize_preference_rows(rows[1:], tk, max_length=None).tokens) > 2 * 64
    m = preference_margins(rows)
    assert m.tolist() == [1.5, 0.0] and preference_margins(rows[1:]) is None
    b = PreferenceCollator(0, None, margins=m)(ds, torch.tensor([1, 0]))
    assert b["margins"].tolist() == [0.0, 1.5] and b["n_seqs"] == 4 and b["num_items"] == 2
    with_prompt = [{"prompt": "where?", "chosen": "north", "rejected": "dunno"}]
    assert tokenize_preference_rows(with_prompt, tk).loss_start.tolist()[0] > 0  # DPO's tokenisation, unchanged


# ------------------------------------------------------------------------------------------------ trainer
TRAIN_KEYS = ("loss", "accuracy", "margin", "mean_reward", "min_reward", "max_reward", "num_tokens", "grad_norm",
              "learning_rate", "epoch")
EVAL_KEYS = ("eval_loss", "eval_accuracy", "eval_margin", "eval_mean_reward", "eval_min_reward", "eval_max_reward")


def test_reward_trainer_learns(tmp_path):
    rm = reward_model()
    ds = separable_pairs(16)
    b0 = PreferenceCollator(0, None)(ds, torch.arange(16))
    with torch.no_grad():
        s0 = rm.sequence_scores(b0["input_ids"], cu_seqlens=b0["cu_seqlens"], n_seqs=32).double()
    t = reward_trainer(tmp_path, rm, ds, eval_ds=ds, max_steps=30)
    quiet_train(t)
    logs = train_logs(t)
    assert len(logs) == 30
    print("losses:", [round(h["loss"], 4) for h in logs])
    for k in TRAIN_KEYS:
        assert k in logs[0] and math.isfinite(logs[0][k]), k
    z0 = s0[0::2] - s0[1::2]
    per_pair = torch.nn.functional.softplus(-z0)
    # the first logged loss is the mean softplus(-(r_c - r_r)) of the four pairs of the first batch, at the initial model
    want0 = per_pair[list(_batches_of(t)[0])].mean().item()
    assert abs(logs[0]["loss"] - want0) < 1e-5, (logs[0]["loss"], want0)
    assert sum(h["loss"] for h in logs[-5:]) / 5 < 0.5 * logs[0]["loss"]
    assert logs[-1]["accuracy"] == 1.0 and logs[-1]["margin"] > 0
    assert logs[-1]["min_reward"] <= logs[-1]["mean_reward"] <= logs[-1]["max_reward"]
    ev = t.evaluate()
    for k in EVAL_KEYS:
        assert k in ev and math.isfinite(ev[k]), k
    assert ev["eval_accuracy"] == 1.0 and ev["eval_loss"] < 0.5 * LN2
    out = str(tmp_path / "saved")
    t.save_model(out)
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["architectures"] == ["LlamaForSequenceClassification"] and cfg["num_labels"] == 1
    again = ckpt.from_pretrained(out, dtype=torch.float32).eval()
    rm.eval()
    with torch.no_grad():
        assert torch.equal(again.sequence_scores(b0["input_ids"], cu_seqlens=b0["cu_seqlens"], n_seqs=32),
                           rm.sequence_scores(b0["input_ids"], cu_seqlens=b0["cu_seqlens"], n_seqs=32))


def _batches_of(t):
    """The pair indices of every batch of epoch 0 of the trainer's sampler."""
    loader = t.get_train_dataloader()
    loader.set_epoch(0)
    return [tuple(int(i) for i in idx) for idx in loader.sampler]


def test_margin_and_centering_change_the_loss(tmp_path):
    ds = separable_pairs(4, seed=3)
    b0 = PreferenceCollator(0, None)(ds, torch.arange(4))
    rm = reward_model(seed=1)
    with torch.no_grad():
        s = rm.sequence_scores(b0["input_ids"], cu_seqlens=b0["cu_seqlens"], n_seqs=8).double()
    z, tot = s[0::2] - s[1::2], s[0::2] + s[1::2]
    margins = torch.tensor([0.5, 1.0, 2.0, 0.0])
    plain = reward_trainer(tmp_path / "a", reward_model(seed=1), ds, max_steps=1)
    quiet_train(plain)
    assert abs(train_logs(plain)[0]["loss"] - torch.nn.functional.softplus(-z).mean().item()) < 1e-5
    with_m = reward_trainer(tmp_path / "b", reward_model(seed=1), ds, max_steps=1)
    with_m.collator.margins = margins
    quiet_train(with_m)
    want = torch.nn.functional.softplus(-(z - margins.double())).mean().item()
    assert abs(train_logs(with_m)[0]["loss"] - want) < 1e-5 and want > train_logs(plain)[0]["loss"]
    cen = reward_trainer(tmp_path / "c", reward_model(seed=1), ds, max_steps=1, center_rewards_coefficient=0.01)
    quiet_train(cen)
    want = (torch.nn.functional.softplus(-z) + float(torch.tensor(0.01)) * tot ** 2).mean().item()
    assert abs(train_logs(cen)[0]["loss"] - want) < 1e-5


def test_text_rows_with_margin_column_train(tmp_path):
    rows = [dict(r, margin=0.25 * (i % 3)) for i, r in enumerate(synthetic_preferences(8, seed=1))]
    implicit = [{"chosen": r["prompt"] + " " + r["chosen"], "rejected": r["prompt"] + " " + r["rejected"]}
                for r in rows[:4]]
    implicit += [{"chosen": [{"role": "user", "content": r["prompt"]}, {"role": "assistant", "content": r["chosen"]}],
                  "rejected": [{"role": "user", "content": r["prompt"]}, {"role": "assistant", "content": r["rejected"]}]}
                 for r in rows[4:]]
    for name, data, has_m in (("explicit", rows, True), ("implicit", implicit, False)):
        t = reward_trainer(tmp_path / name, reward_model("tiny"), data, eval_ds=data[:4], max_steps=2, max_length=256,
                           dataset_cache=False)
        assert (t.collator.margins is not None) == has_m and len(t.train_dataset) == 16
        if has_m:
            assert t.collator.margins.tolist() == [0.25 * (i % 3) for i in range(8)]
            assert t.eval_collator.margins.tolist() == [0.0, 0.25, 0.5, 0.0]
        quiet_train(t)
        assert len(train_logs(t)) == 2 and all(math.isfinite(h["loss"]) for h in train_logs(t))
        assert math.isfinite(t.evaluate()["eval_loss"])


def _params_after_one_step(tmp, per_dev, ga):
    t = reward_trainer(tmp, reward_model(seed=2), separable_pairs(8, seed=4), per_device_train_batch_size=per_dev,
                       gradient_accumulation_steps=ga, max_steps=1)
    grads = {}
    step = t.optimizer.step

    def capture(*a, **k):  # the step's accumulated gradients, as the optimizer receives them
        grads["flat"] = t.engine.grad_flat.clone()
        return step(*a, **k)

    t.optimizer.step = capture
    quiet_train(t)
    return t.engine.params_by_name().clone(), grads["flat"], train_logs(t)[0]


def test_grad_accumulation_equals_big_batch(tmp_path):
    """GA 2 x 4 pairs against 1 x 8: the same gradients (fp32 summation order apart) and the same parameters after the
    step. Adam's first update is lr g / (|g| + 1e-8): where |g| is itself of the size of the rounding difference the
    update may differ by up to 2 lr, so the parameters are compared everywhere at 1e-6 but for a 1e-4 share."""
    big, gb, lb = _params_after_one_step(tmp_path / "big", 8, 1)
    ga, gg, lg = _params_after_one_step(tmp_path / "ga", 4, 2)
    e = ((gg - gb).norm() / gb.norm()).item()
    off = ((big - ga).abs() > 1e-6).float().mean().item()
    print("GA 2 x 4 against 1 x 8: relative gradient difference", e, "share of parameters off by > 1e-6:", off)
    assert gb.norm() > 0 and e < 1e-5
    assert off < 1e-4 and (big - ga).abs().max().item() <= 2.0e-3 + 1e-9
    assert abs(lb["loss"] - lg["loss"]) < 1e-6 and abs(lb["margin"] - lg["margin"]) < 1e-6
    assert lb["min_reward"] == pytest.approx(lg["min_reward"], abs=1e-6)


def test_reward_resume(tmp_path):
    ds = separable_pairs(16, seed=2)
    kw = dict(max_steps=4, save_strategy="steps", save_steps=2, save_total_limit=5)
    full = reward_trainer(tmp_path / "full", reward_model(), ds, **kw)
    quiet_train(full)
    want = {h["step"]: h["loss"] for h in train_logs(full)}
    first = reward_trainer(tmp_path / "run", reward_model(), ds, **kw)
    first.args.max_steps = 2
    quiet_train(first)
    ck = os.path.join(str(tmp_path / "run"), "checkpoint-2")
    assert "score.weight" in ckpt.load_state_dict(ck)
    second = reward_trainer(tmp_path / "run", reward_model(seed=9), ds, **kw)
    quiet_train(second, resume_from_checkpoint=ck)
    got = {h["step"]: h["loss"] for h in train_logs(second)}
    assert got[3] == want[3] and got[4] == want[4], (got, want)
    assert torch.equal(second.engine.params_by_name(), full.engine.params_by_name())


def test_model_given_by_name_or_causal_directory(tmp_path):
    from llm_fine_tune_distributed_amd.train import RewardConfig, RewardTrainer, SFTConfig
    ds = separable_pairs(4)
    t = reward_trainer(tmp_path / "a", "tiny-llama", ds, max_steps=1)
    assert t.model.is_reward_model and t.model.lm_head is None
    lm = build_model(get_config("tiny-llama"), dtype=torch.float32, seed=1)
    ckpt.save_pretrained(lm, str(tmp_path / "lm"))
    t = reward_trainer(tmp_path / "b", str(tmp_path / "lm"), ds, max_steps=1)
    assert t.model.is_reward_model and torch.equal(t.model.model.norm.weight.float(), lm.model.norm.weight)
    with pytest.raises(TypeError, match="score head"):
        reward_trainer(tmp_path / "c", lm, ds)
    with pytest.raises(TypeError, match="RewardConfig"):
        RewardTrainer(model=reward_model(), args=SFTConfig(output_dir=str(tmp_path)), train_dataset=ds)
    a = RewardConfig()
    assert a.max_length == 1024 and a.center_rewards_coefficient is None and isinstance(a, SFTConfig)
    for bad in (dict(context_parallel_size=2), dict(packing=True), dict(label_smoothing_factor=0.1),
                dict(loss_type="dft"), dict(loss_type="sigmoid"), dict(center_rewards_coefficient=-1.0)):
        with pytest.raises(ValueError, match="RewardConfig"):
            RewardConfig(**bad)
    a.context_parallel_size = 2  # set after construction: the trainer refuses it too
    with pytest.raises((NotImplementedError, ValueError), match="context"):
        RewardTrainer(model=reward_model(), args=a, train_dataset=ds)
    odd = TokenizedDataset.from_token_lists([[3, 4], [5, 6], [7, 8]], [1, 1, 1])
    with pytest.raises(ValueError, match="2N"):
        reward_trainer(tmp_path / "d", reward_model(), odd)
    import llm_fine_tune_distributed_amd as top
    assert top.RewardTrainer is RewardTrainer and top.RewardConfig is RewardConfig


# ------------------------------------------------------------------------------------------------ two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out_dir, per_dev, preset, shard):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import llm_fine_tune_distributed_amd.parallel.process_group as pgm
    pgm._STATE = None
    torch.manual_seed(0)
    t = reward_trainer(out_dir, reward_model(preset, seed=3), separable_pairs(8, seed=7),
                       per_device_train_batch_size=per_dev, max_steps=2, ddp_check_sync_every=1, ddp_bucket_cap_mb=0.05,
                       ddp_first_bucket_mb=0.01, shard_optimizer_state=shard)
    quiet_train(t)
    torch.save({"params": t.engine.params_by_name().clone(), "log": train_logs(t)},
               os.path.join(out_dir, f"r{world}_{rank}_{int(shard)}.pt"))
    pgm.cleanup_distributed()


@pytest.mark.parametrize("preset", ["tiny-llama", "tiny"])  # "tiny" ties its embedding: one use on a reward model
def test_two_ranks_match_single_process(preset):
    d = tempfile.mkdtemp()
    _rank(0, 1, _free_port(), d, 4, preset, False)
    single = torch.load(os.path.join(d, "r1_0_0.pt"))
    for shard in (False, True):
        mp.spawn(_rank, args=(2, _free_port(), d, 2, preset, shard), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r2_{r}_{int(shard)}.pt")) for r in range(2))
        assert torch.equal(r0["params"], r1["params"])  # ranks bit-identical
        # against one process the fp32 summation order differs, and Adam's lr g / (sqrt(v) + 1e-8) turns a rounding
        # difference into up to 2 lr per step where |g| is of that size itself: DPO's 1e-5 for all but a 1e-4 share
        diff = (r0["params"] - single["params"]).abs()
        print(preset, "ZeRO-1" if shard else "DDP", "max parameter difference", diff.max().item(), "share over 1e-5",
              (diff > 1e-5).float().mean().item())
        assert (diff > 1e-5).float().mean().item() < 1e-4 and diff.max().item() <= 2 * 2 * 1e-3 + 1e-9
        for a, b in zip(single["log"], r0["log"]):
            assert abs(a["loss"] - b["loss"]) < 1e-4 and abs(a["grad_norm"] - b["grad_norm"]) < 1e-3
            assert abs(a["min_reward"] - b["min_reward"]) < 1e-4 and abs(a["max_reward"] - b["max_reward"]) < 1e-4
            assert a["accuracy"] == b["accuracy"]


# ------------------------------------------------------------------------------------------------ GRPO
def low_share(prompts, completions, completion_ids, **kw):
    return [sum(t < V // 2 for t in c) / max(len(c), 1) for c in completion_ids]


def prompt_rows(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"prompt_ids": torch.randint(3, V, (int(k),), generator=g).tolist()}
            for k in torch.randint(3, 9, (n,), generator=g)]


def grpo_trainer(out, model, ds, rewards, **kw):
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer
    base = dict(output_dir=str(out), per_device_train_batch_size=8, num_generations=4, max_completion_length=6,
                learning_rate=1e-3, lr_scheduler_type="constant", logging_steps=1, jsonl_log=False, save_strategy="no")
    base.update(kw)
    return GRPOTrainer(model=model, reward_funcs=rewards, args=GRPOConfig(**base), train_dataset=ds)


def test_grpo_with_reward_models(tmp_path):
    policy = build_model(get_config("tiny-llama"), dtype=torch.float32, seed=0)
    rm = reward_model(seed=6)
    ds = prompt_rows(4)
    t = grpo_trainer(tmp_path / "a", policy, ds, [rm, low_share], reward_weights=[2.0, 0.5], max_steps=2,
                     save_strategy="steps", save_steps=2)
    assert t.reward_names == ["CausalLM", "low_share"] and t.reward_funcs[0] is rm
    assert not rm.training and not any(p.requires_grad for p in rm.parameters())
    rm_ids = {id(p) for p in rm.parameters()}
    assert not rm_ids & set(t.engine.param_names)  # in no optimizer group
    b = t._make_batch(0, 0, torch.tensor([0, 1]))
    rows = [ds[i] for i in (0, 1) for _ in range(4)]
    toks = b["completion_ids"]
    per_fn = t._rewards(rows, toks)
    assert per_fn.dtype == torch.float64 and per_fn.shape == (2, 8)
    ids = torch.tensor([x for r, c in zip(rows, toks) for x in r["prompt_ids"] + c])
    lens = torch.tensor([len(r["prompt_ids"]) + len(c) for r, c in zip(rows, toks)])
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32)
    with torch.no_grad():
        want = rm.sequence_scores(ids, cu_seqlens=cu, n_seqs=8)
    assert torch.equal(per_fn[0], want.double())  # bit for bit
    assert torch.allclose(b["rewards"].double(), 2.0 * per_fn[0] + 0.5 * per_fn[1], atol=1e-6)
    quiet_train(t)
    logs = train_logs(t)
    assert all("rewards/CausalLM/mean" in h and "rewards/low_share/mean" in h for h in logs)
    ck = os.path.join(str(tmp_path / "a"), "checkpoint-2")
    assert "score.weight" not in ckpt.load_state_dict(ck)
    assert json.load(open(os.path.join(ck, "config.json")))["architectures"] == ["LlamaForCausalLM"]
    names = torch.load(os.path.join(ck, "optimizer.pt"), weights_only=True)
    assert "score" not in json.dumps(sorted(str(k) for k in _keys(names)))
    t.save_model(str(tmp_path / "policy"))
    assert "score.weight" not in ckpt.load_state_dict(str(tmp_path / "policy"))
    # a directory, named by its basename; two entries of one name are numbered
    d = str(tmp_path / "my-rm")
    ckpt.save_pretrained(rm, d)
    t2 = grpo_trainer(tmp_path / "b", build_model(get_config("tiny-llama"), dtype=torch.float32), ds, [d], max_steps=1)
    assert t2.reward_names == ["my-rm"] and t2.reward_funcs[0].is_reward_model
    assert t2.reward_funcs[0].score.dtype == torch.bfloat16
    quiet_train(t2)
    assert "rewards/my-rm/mean" in train_logs(t2)[0]
    t3 = grpo_trainer(tmp_path / "c", build_model(get_config("tiny-llama"), dtype=torch.float32), ds, [d, d],
                      max_steps=1)
    assert t3.reward_names == ["my-rm_0", "my-rm_1"]


def _keys(obj):
    if isinstance(obj, dict):
        for k, v in obj.items():
            yield k
            yield from _keys(v)


def test_grpo_reward_model_refusals(tmp_path):
    policy = build_model(get_config("tiny-llama"), dtype=torch.float32)
    ds = prompt_rows(4)
    small = build_model(dataclasses.replace(get_config("tiny-llama"), vocab_size=512, num_labels=1), dtype=torch.float32)
    with pytest.raises(ValueError, match="vocab_size"):
        grpo_trainer(tmp_path, policy, ds, [small])
    with pytest.raises(TypeError, match="reward models"):
        grpo_trainer(tmp_path, policy, ds, [build_model(get_config("tiny-llama"), dtype=torch.float32)])  # no head
    lm_dir = str(tmp_path / "lm")
    ckpt.save_pretrained(policy, lm_dir)
    for bad in (lm_dir, str(tmp_path / "missing"), str(tmp_path)):
        with pytest.raises(TypeError, match="reward models"):
            grpo_trainer(tmp_path, policy, ds, [low_share, bad])


# ------------------------------------------------------------------------------------------------ CLI
def _cli_env(tmp_path, monkeypatch):
    monkeypatch.setenv("OUTPUT_DIR", str(tmp_path / "out"))
    monkeypatch.setenv("EPOCHS", "1")
    monkeypatch.setenv("BATCH_SIZE", "2")
    monkeypatch.setenv("LEARNING_RATE", "1e-4")
    monkeypatch.setenv("AIM_REPO", str(tmp_path / "aim"))
    data = tmp_path / "prefs.jsonl"
    with open(data, "w") as f:
        for i, r in enumerate(synthetic_preferences(24, seed=3)):
            f.write(json.dumps(dict(r, margin=0.1 * (i % 2))) + "\n")
    return data, tmp_path / "out"


def test_train_cli_reward(tmp_path, monkeypatch):
    from llm_fine_tune_distributed_amd.cli import train as cli
    data, out = _cli_env(tmp_path, monkeypatch)
    cli.main(["--trainer", "reward", "--model", "tiny", "--dataset", str(data), "--max-steps", "2", "--grad-accum", "1",
              "--no-gradient-checkpointing", "--max-length", "128", "--set", "center_rewards_coefficient=0.01",
              "--set", "logging_steps=1", "--freeze-policy", "full"])
    resolved = json.load(open(out / "sft_config.json"))
    assert resolved["center_rewards_coefficient"] == 0.01
    steps = [h for h in (json.loads(l) for l in open(out / "checkpoints" / "metrics.jsonl")) if "loss" in h]
    assert len(steps) == 2 and all(k in h for h in steps for k in ("accuracy", "margin", "mean_reward"))
    cfg = json.load(open(out / "best_model" / "config.json"))
    assert cfg["architectures"] == ["SmolLM3ForSequenceClassification"]


def test_train_cli_reward_model_flag_is_grpo_only(tmp_path, monkeypatch):
    from llm_fine_tune_distributed_amd.cli import train as cli
    data, _ = _cli_env(tmp_path, monkeypatch)
    with pytest.raises(SystemExit):
        cli.main(["--trainer", "reward", "--model", "tiny", "--dataset", str(data), "--reward-model", str(tmp_path)])
    with pytest.raises(SystemExit):
        cli.main(["--trainer", "grpo", "--model", "tiny", "--dataset", "synthetic"])  # neither --reward nor a model
