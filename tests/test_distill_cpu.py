"""Knowledge distillation on the CPU (the reference path): ref.generalized_jsd and its gradient, GKDConfig, and
GKDTrainer on tiny models."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.data.synthetic import generate_qa
from llm_fine_tune_distributed_amd.data.tokenizer import load_tokenizer
from llm_fine_tune_distributed_amd.models import build_model, get_config, tiny
from llm_fine_tune_distributed_amd.ops import reference as ref
from llm_fine_tune_distributed_amd.train import GKDConfig, GKDTrainer, TrainingHistoryCallback

BETAS = [0.0, 0.3, 0.5, 1.0]
TAUS = [0.9, 1.0, 2.0]


def _case(M=7, V=40, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    s = (3 * torch.randn(M, V, generator=g, dtype=torch.float64)).to(dtype)
    t = (3 * torch.randn(M, V, generator=g, dtype=torch.float64)).to(dtype)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[2] = -100
    labels[M - 1] = -100
    return s, t, labels


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("beta", BETAS)
def test_grad_is_autograd_of_the_loss_fp64(beta, tau):
    s, t, labels = _case()
    scale = torch.tensor([1.0 / 7.0], dtype=torch.float64)
    x = s.clone().requires_grad_(True)
    loss = ref.generalized_jsd(x, t, labels, beta, tau)[0]
    (loss.sum() * scale).sum().backward()
    got = ref.generalized_jsd_grad(s, t, labels, scale, beta, tau)
    assert got.dtype == torch.float64
    assert (got - x.grad).abs().max().item() < 1e-14
    assert not got[2].any() and not got[-1].any()


@pytest.mark.parametrize("tau", TAUS)
def test_beta_0_and_1_are_the_two_kl_directions(tau):
    s, t, labels = _case(seed=1)
    lp, lq = F.log_softmax(s / tau, -1), F.log_softmax(t / tau, -1)
    valid = (labels != -100).double()
    fwd = F.kl_div(lp, lq, reduction="none", log_target=True).sum(-1) * valid  # KL(teacher || student)
    rev = F.kl_div(lq, lp, reduction="none", log_target=True).sum(-1) * valid  # KL(student || teacher)
    assert torch.allclose(ref.generalized_jsd(s, t, labels, 0.0, tau)[0], fwd, rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref.generalized_jsd(s, t, labels, 1.0, tau)[0], rev, rtol=1e-12, atol=1e-14)
    # and the mixture is TRL's expression: beta KL(teacher || m) + (1 - beta) KL(student || m)
    beta = 0.3
    lm = torch.logsumexp(torch.stack([lp + torch.log1p(torch.tensor(-beta, dtype=torch.float64)),
                                      lq + torch.log(torch.tensor(beta, dtype=torch.float64))]), 0)
    mix = (beta * F.kl_div(lm, lq, reduction="none", log_target=True).sum(-1)
           + (1 - beta) * F.kl_div(lm, lp, reduction="none", log_target=True).sum(-1)) * valid
    assert torch.allclose(ref.generalized_jsd(s, t, labels, beta, tau)[0], mix, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("beta", BETAS)
def test_teacher_equal_to_student_costs_nothing(beta):
    s, _, labels = _case(seed=2)
    loss = ref.generalized_jsd(s, s.clone(), labels, beta, 0.9)[0]
    grad = ref.generalized_jsd_grad(s, s.clone(), labels, torch.ones(1, dtype=torch.float64), beta, 0.9)
    assert loss.abs().max().item() < 1e-14 and grad.abs().max().item() < 1e-14


@pytest.mark.parametrize("beta", BETAS)
def test_masked_rows_contribute_nothing_and_do_not_enter_the_normalisation(beta):
    """The op's loss over all rows with two of them masked equals the loss over the unmasked rows alone, with the
    same count of valid rows; so do the gradients of the unmasked rows, and the masked rows get none."""
    s, t, labels = _case(seed=3)
    keep = labels != -100
    n = int(keep.sum())
    assert 0 < n < len(labels)
    W = torch.eye(s.shape[1], dtype=torch.float64)  # an LM head that hands h through: logits = h
    inv = torch.tensor([1.0 / n], dtype=torch.float64)
    h_all = s.clone().requires_grad_(True)
    loss_all, stats = ops.lm_head_distill_loss(h_all, W, t, labels, inv, beta, 0.9)
    loss_all.backward()
    h_kept = s[keep].clone().requires_grad_(True)
    loss_kept, _ = ops.lm_head_distill_loss(h_kept, W, t[keep], labels[keep], inv, beta, 0.9)
    loss_kept.backward()
    assert stats.shape == (5, len(labels)) and not stats[0][~keep].any()
    assert abs(loss_all.item() - loss_kept.item()) < 1e-6 * max(1.0, abs(loss_kept.item()))
    assert torch.allclose(h_all.grad[keep], h_kept.grad, rtol=1e-5, atol=1e-7)
    assert not h_all.grad[~keep].any()
    # the mean over valid rows, not over all rows
    per_row = ref.generalized_jsd(s, t, labels, beta, 0.9)[0]
    assert abs(loss_all.item() - per_row[keep].mean().item()) < 1e-6 * max(1.0, per_row[keep].mean().item())


def test_fp32_inputs_far_apart_stay_finite():
    """Logit gaps past 100: fp32 probabilities underflow, the log-domain loss and gradient do not."""
    s, t, labels = _case(M=4, V=32, seed=4, dtype=torch.float32)
    s[0, :8] += 150.0
    t[0, 8:16] += 150.0
    labels[:] = 1
    for beta in BETAS:
        loss = ref.generalized_jsd(s, t, labels, beta, 1.0)[0]
        grad = ref.generalized_jsd_grad(s, t, labels, torch.ones(1), beta, 1.0)
        want = ref.generalized_jsd(s.double(), t.double(), labels, beta, 1.0)[0]
        assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
        assert torch.allclose(loss.double(), want, rtol=1e-5, atol=1e-6)


def test_op_refusals():
    s, t, labels = _case()
    W = torch.eye(s.shape[1], dtype=torch.float64)
    inv = torch.ones(1, dtype=torch.float64)
    for kw in (dict(beta=1.5), dict(beta=-0.1), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            ops.lm_head_distill_loss(s, W, t, labels, inv, **kw)
    with pytest.raises(ValueError, match="teacher_logits"):
        ops.lm_head_distill_loss(s, W, t[:, :-8], labels, inv)


# ------------------------------------------------------------------------------------------------ config
def test_gkd_config_accepts_and_rejects():
    c = GKDConfig()
    assert (c.beta, c.temperature, c.lmbda, c.seq_kd, c.teacher_model_name_or_path) == (0.5, 0.9, 0.0, False, None)
    GKDConfig(beta=0.0, temperature=2.0, teacher_model_name_or_path="tiny-llama", packing=True,
              gradient_accumulation_steps=2, freeze_policy="lora", assistant_only_loss=True)
    GKDConfig(beta=1.0)
    with pytest.raises(ValueError, match="TRL's default is lmbda=0.5"):
        GKDConfig(lmbda=0.5)
    for kw, why in ((dict(seq_kd=True), "seq_kd"), (dict(label_smoothing_factor=0.1), "label_smoothing_factor"),
                    (dict(loss_type="dft"), "loss_type"), (dict(context_parallel_size=2), "context_parallel_size"),
                    (dict(beta=1.5), "beta"), (dict(beta=-0.1), "beta"), (dict(temperature=0.0), "temperature"),
                    (dict(temperature=-1.0), "temperature")):
        with pytest.raises(ValueError, match=why):
            GKDConfig(**kw)
    # a field set after construction is caught when the trainer is built
    c = GKDConfig(output_dir="unused")
    c.lmbda = 1.0
    with pytest.raises(ValueError, match="lmbda"):
        GKDTrainer(model="tiny", args=c, teacher_model="tiny-llama")


# ------------------------------------------------------------------------------------------------ trainer
@pytest.fixture(scope="module")
def tk():
    return load_tokenizer()


def _student(seed=0):
    return build_model(tiny(vocab_size=1024), dtype=torch.float32, seed=seed)


def _teacher(seed=5):
    return build_model(get_config("tiny-llama"), dtype=torch.bfloat16, seed=seed)


def _args(out, **kw):
    base = dict(output_dir=str(out), per_device_train_batch_size=4, learning_rate=2e-3, max_steps=5, logging_steps=1,
                lr_scheduler_type="constant", save_strategy="no", jsonl_log=False, seed=1)
    base.update(kw)
    return GKDConfig(**base)


def test_gkd_trainer_steps(tmp_path, tk):
    rows = generate_qa(8, seed=0)
    teacher = _teacher()
    before = {n: p.detach().clone() for n, p in teacher.named_parameters()}
    h = TrainingHistoryCallback()
    t = GKDTrainer(model=_student(), args=_args(tmp_path / "run", per_device_train_batch_size=8),
                   train_dataset=rows, eval_dataset=rows[:4], processing_class=tk, teacher_model=teacher, callbacks=[h])
    assert t.teacher is teacher and not teacher.training
    assert not any(p.requires_grad for p in teacher.parameters())
    assert all(p.dtype == torch.bfloat16 for p in teacher.parameters())
    ids = {id(p) for p in teacher.parameters()}
    assert not ids & {id(p) for p in t.model.parameters()}
    t.train()
    logs = [x for x in h.history if "loss" in x]
    assert len(logs) == 5
    for k in ("loss", "grad_norm", "learning_rate", "epoch", "mean_token_accuracy", "teacher_agreement", "num_tokens"):
        assert all(k in x for x in logs), k
    assert all(0.0 <= x["teacher_agreement"] <= 1.0 for x in logs)
    # the same 8 rows every step: the distillation loss falls
    assert logs[-1]["loss"] < logs[0]["loss"], [x["loss"] for x in logs]
    ev = t.evaluate()
    for k in ("eval_loss", "eval_mean_token_accuracy", "eval_teacher_agreement", "eval_num_tokens"):
        assert k in ev, k
    assert ev["eval_loss"] > 0
    # the teacher: bit-identical, still frozen and in eval mode, absent from what save_model writes
    for n, p in teacher.named_parameters():
        assert torch.equal(p, before[n]), n
    assert not teacher.training
    t.save_model(str(tmp_path / "saved"))
    from safetensors.torch import load_file
    sd = load_file(str(tmp_path / "saved" / "model.safetensors"))
    want = t.model.hf_state_dict()
    assert set(sd) == set(want)
    for k in sd:
        assert torch.equal(sd[k], want[k].to(sd[k].dtype)), k
    assert json.load(open(tmp_path / "saved" / "config.json"))["model_type"] == t.model.config.model_type != \
        teacher.config.model_type


def test_gkd_trainer_teacher_by_name_and_vocab_mismatch(tmp_path, tk):
    a = _args(tmp_path / "byname", teacher_model_name_or_path="tiny-llama")
    t = GKDTrainer(model=_student(), args=a, train_dataset=generate_qa(4), processing_class=tk)
    assert t.teacher.config.model_type == "llama" and t.args.to_dict()["teacher_model_name_or_path"] == "tiny-llama"
    small = build_model(tiny("llama", vocab_size=512), dtype=torch.bfloat16, seed=1)
    with pytest.raises(ValueError, match="vocab_size"):
        GKDTrainer(model=_student(), args=_args(tmp_path / "mismatch"), train_dataset=generate_qa(4),
                   processing_class=tk, teacher_model=small)
    with pytest.raises(ValueError, match="teacher"):
        GKDTrainer(model=_student(), args=_args(tmp_path / "none"), train_dataset=generate_qa(4), processing_class=tk)


@pytest.mark.parametrize("packing", [False, True])
def test_gkd_ga_merge_matches_separate_passes(tmp_path, tk, packing):
    """A step with GA 2 merged into one pass equals the same step as two passes (the tolerances of
    tests/test_trainer_cpu.py::test_ga_merge_matches_separate_passes)."""
    rows = generate_qa(16, seed=4)
    res = {}
    for merge in (0, 1 << 16):
        h = TrainingHistoryCallback()
        a = _args(tmp_path / str(merge), gradient_accumulation_steps=2, learning_rate=1e-3, max_steps=2,
                  packing=packing, ga_merge_max_tokens=merge, lr_scheduler_type="linear")
        t = GKDTrainer(model=_student(seed=7), args=a, train_dataset=rows, processing_class=tk,
                       teacher_model=_teacher(), callbacks=[h])
        # the teacher's bf16 weights, computed with in fp32: a merged padded batch is re-padded to another length,
        # which moves the roundings of a bf16 forward on the CPU (2.6e-4 on 237 of 722,944 parameters), and that is
        # the teacher's arithmetic, not the merging this test is about
        for p in t.teacher.parameters():
            p.data = p.data.float()
        t.train()
        res[merge] = ([x for x in h.history if "loss" in x], t.engine.param_flat.clone())
    (l0, p0), (l1, p1) = res[0], res[1 << 16]
    assert torch.allclose(p0, p1, atol=1e-5, rtol=1e-4)
    for a, b in zip(l0, l1):
        for k in ("loss", "grad_norm", "mean_token_accuracy", "teacher_agreement", "num_tokens"):
            assert abs(a[k] - b[k]) <= 1e-5 * max(1.0, abs(a[k])), (k, a[k], b[k])


def test_train_cli_gkd(tmp_path, monkeypatch):
    from llm_fine_tune_distributed_amd.cli import train as cli
    out = tmp_path / "out"
    monkeypatch.setenv("OUTPUT_DIR", str(out))
    monkeypatch.setenv("EPOCHS", "1")
    monkeypatch.setenv("BATCH_SIZE", "2")
    monkeypatch.setenv("LEARNING_RATE", "1e-4")
    monkeypatch.setenv("AIM_REPO", str(tmp_path / "aim"))
    cli.main(["--trainer", "gkd", "--model", "tiny", "--teacher", "tiny-llama", "--dataset", "synthetic",
              "--max-steps", "1", "--grad-accum", "1", "--no-gradient-checkpointing", "--max-length", "128",
              "--max-train-samples", "8", "--freeze-policy", "full", "--set", "beta=0.25", "--set", "logging_steps=1",
              "--set", "eval_strategy=no", "--set", "max_eval_samples=4"])
    resolved = json.load(open(out / "sft_config.json"))
    assert resolved["beta"] == 0.25 and resolved["temperature"] == 0.9
    assert resolved["teacher_model_name_or_path"] == "tiny-llama"
    logs = [json.loads(l) for l in open(out / "checkpoints" / "metrics.jsonl")]
    steps = [x for x in logs if "loss" in x]
    assert len(steps) == 1 and "teacher_agreement" in steps[0]
    assert os.path.exists(out / "best_model" / "model.safetensors")
