"""GRPO off the GPU: GRPOConfig and its rejections, the advantage arithmetic, the fp32 twins of csrc/policy.hip and of
ce_fwd's temperature objective against fp64, the rollout loader's contract, GRPOTrainer on the reference path (resume,
two gloo ranks, a learning run) and the CLI with --reward."""
import contextlib
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
from llm_fine_tune_distributed_amd.inference.generation import generate_batch, rollout_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import reference as ref
from llm_fine_tune_distributed_amd.train.grpo import RolloutLoader, compute_advantages, rollout_seed

V = 1024


def tiny_model(seed=0):
    return build_model(get_config("tiny-llama"), device="cpu", dtype=torch.float32, seed=seed)


def low_share(prompts, completions, completion_ids, **kw):
    """The share of completion tokens below vocab / 2: a function of the token ids, so no tokenizer is needed."""
    return [sum(t < V // 2 for t in c) / max(len(c), 1) for c in completion_ids]


def prompt_rows(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"prompt_ids": torch.randint(3, V, (int(k),), generator=g).tolist()}
            for k in torch.randint(3, 9, (n,), generator=g)]


def grpo_trainer(out, model, ds, rewards=low_share, eval_ds=None, ref_model=None, **kw):
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer
    base = dict(output_dir=str(out), per_device_train_batch_size=8, num_generations=4, max_completion_length=6,
                learning_rate=1e-3, lr_scheduler_type="constant", logging_steps=1, jsonl_log=False, save_strategy="no")
    base.update(kw)
    return GRPOTrainer(model=model, reward_funcs=rewards, args=GRPOConfig(**base), train_dataset=ds,
                       eval_dataset=eval_ds, ref_model=ref_model)


def train_logs(t):
    return [h for h in t.state.log_history if "loss" in h]


def quiet_train(t, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return t.train(**kw)


# ------------------------------------------------------------------------------------------------ config
def test_grpo_config_defaults_and_refusals(tmp_path):
    from llm_fine_tune_distributed_amd import GRPOConfig as Top
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer, SFTConfig
    a = GRPOConfig()
    assert Top is GRPOConfig and isinstance(a, SFTConfig)
    assert (a.num_generations, a.max_completion_length, a.temperature, a.top_k, a.repetition_penalty) == (8, 256, 1.0, 0, 1.0)
    assert (a.beta, a.epsilon, a.epsilon_high, a.num_iterations, a.loss_type, a.scale_rewards) == \
        (0.0, 0.2, None, 1, "dapo", "group")
    assert a.reward_weights is None and a.mask_truncated_completions is False
    assert a.metric_for_best_model == "eval_reward" and a.greater_is_better is True
    assert hasattr(a, "max_prompt_length")
    for bad, why in ((dict(loss_type="bnpo"), "LOCAL"), (dict(loss_type="nll"), "supervised"),
                     (dict(loss_type="dft"), "supervised"), (dict(loss_type="gspo"), "loss_type"),
                     (dict(top_p=0.9), "top_p"), (dict(importance_sampling_level="sequence"), "sequence"),
                     (dict(packing=True), "packing"), (dict(label_smoothing_factor=0.1), "label_smoothing"),
                     (dict(context_parallel_size=2), "context"), (dict(scale_rewards="std"), "scale_rewards"),
                     (dict(num_generations=1), "num_generations"), (dict(temperature=0.0), "temperature"),
                     (dict(top_k=65), "top_k"), (dict(beta=-0.1), "beta"), (dict(epsilon=1.0), "epsilon"),
                     (dict(num_iterations=0), "num_iterations"), (dict(max_completion_length=0), "max_completion")):
        with pytest.raises(ValueError, match=why):
            GRPOConfig(**bad)
    assert GRPOConfig(scale_rewards=False).scale_rewards == "none" and GRPOConfig(scale_rewards=True).scale_rewards == "group"
    assert isinstance(a.replace(beta=0.04), GRPOConfig) and a.replace(beta=0.04).beta == 0.04
    m, ds = tiny_model(), prompt_rows(4)
    with pytest.raises(ValueError, match="multiple of num_generations"):
        grpo_trainer(tmp_path, m, ds, per_device_train_batch_size=6)
    with pytest.raises(TypeError, match="GRPOConfig"):
        GRPOTrainer(model=m, reward_funcs=low_share, args=SFTConfig(output_dir=str(tmp_path)), train_dataset=ds)
    with pytest.raises(TypeError, match="reward models"):
        grpo_trainer(tmp_path, m, ds, rewards=tiny_model(1))
    with pytest.raises(TypeError, match="reward models"):
        grpo_trainer(tmp_path, m, ds, rewards=[low_share, "some/reward-model"])
    with pytest.raises(ValueError, match="reward_funcs"):
        grpo_trainer(tmp_path, m, ds, rewards=None)
    with pytest.raises(ValueError, match="reward_weights"):
        grpo_trainer(tmp_path, m, ds, reward_weights=[1.0, 2.0])
    late = GRPOConfig(output_dir=str(tmp_path))
    late.context_parallel_size = 2  # set after construction: the trainer refuses it too
    with pytest.raises((NotImplementedError, ValueError), match="context"):
        GRPOTrainer(model=m, reward_funcs=low_share, args=late, train_dataset=ds)
    m.model.layers[0].self_attn.cp_group = object()
    z = torch.zeros(4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.policy_loss(z, z, torch.zeros(1))
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.token_logps(z, z)


# ------------------------------------------------------------------------------------------------ advantages
def test_advantages_by_hand():
    r = torch.tensor([[1.0, 0.0, 0.0, 1.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 2.0, 3.0]])
    # unbiased stds: sqrt(1/3), 0, sqrt(5/3); over all 12 rewards: sum 16, sum of squares 32, so the squared
    # deviations add up to 32 - 16^2 / 12 = 32 / 3 and the unbiased variance is 32 / 33
    s0, s2 = math.sqrt(1.0 / 3.0), math.sqrt(5.0 / 3.0)
    adv, std = compute_advantages(r, "group")
    assert torch.allclose(std, torch.tensor([s0, 0.0, s2]), atol=1e-6)
    want = torch.tensor([[0.5, -0.5, -0.5, 0.5], [0, 0, 0, 0], [-1.5, -0.5, 0.5, 1.5]])
    assert torch.allclose(adv, want / (torch.tensor([s0, 0.0, s2])[:, None] + 1e-4), atol=1e-6)
    assert not adv[1].any()                                   # a group of equal rewards teaches nothing
    adv_b, _ = compute_advantages(r, "batch")
    sb = math.sqrt(32.0 / 33.0)
    assert torch.allclose(adv_b, want / (sb + 1e-4), atol=1e-6)
    adv_n, _ = compute_advantages(r, "none")
    assert torch.equal(adv_n, want)
    with pytest.raises(ValueError):
        compute_advantages(r, "rank")


# ------------------------------------------------------------------------------------------------ twins
def rel_err(got, want64):
    d = (got.double() - want64).abs()
    return torch.where(want64 != 0, d / want64.abs().clamp_min(1e-300),
                       torch.where(d > 0, torch.full_like(d, math.inf), d))


def _tok_case():
    g = torch.Generator().manual_seed(17)
    lens, pad = [1, 63, 64, 65, 200, 5], 7
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    c.append(c[-1] + pad)
    M = c[-1]
    nll = (2.0 * torch.randn(M, generator=g)).abs() + 0.01
    labels = torch.randint(0, 1000, (M,), generator=g)
    labels[torch.rand(M, generator=g) < 0.3] = -100
    labels[0] = 5
    labels[c[5]:] = -100
    r = torch.tensor([0.6, 0.95, 1.05, 1.5])[torch.randint(0, 4, (M,), generator=g)]
    old = (-nll.double() - r.double().log()).float()
    d = (0.05 + 0.55 * torch.rand(M, generator=g)) * (2 * torch.randint(0, 2, (M,), generator=g) - 1)
    adv = torch.tensor([0.7, -1.3, 0.0, 0.4, -0.9, 0.5])
    return nll, old, (-nll + d).float(), labels, adv, torch.tensor(c, dtype=torch.int32), len(lens)


@pytest.mark.parametrize("per_seq_mean", [False, True])
@pytest.mark.parametrize("has_ref", [False, True])
@pytest.mark.parametrize("has_old", [False, True])
def test_grpo_token_twin_against_fp64_autograd(has_old, has_ref, per_seq_mean):
    nll, old, rlp, labels, adv, cu, S = _tok_case()
    old, rlp = (old if has_old else None), (rlp if has_ref else None)
    lo, hi, beta = 0.2, 0.28, 0.04
    inv = torch.tensor([1.0 / 37.0])
    rows, seq = ref.grpo_token(nll, old, rlp, labels, adv, cu, S, inv, lo, hi, beta, per_seq_mean)
    assert rows.dtype == torch.float32 and rows.shape == (2, nll.numel()) and seq.shape == (6, S)
    # fp64 autograd of the formula
    c = cu.tolist()
    lp = (-nll.double()).requires_grad_(True)
    comp = torch.zeros(nll.numel(), dtype=torch.bool)
    A, w = torch.zeros(nll.numel(), dtype=torch.float64), torch.zeros(nll.numel(), dtype=torch.float64)
    for s in range(S):
        comp[c[s]:c[s + 1]] = labels[c[s]:c[s + 1]] >= 0
        A[c[s]:c[s + 1]] = adv[s].double()
        w[c[s]:c[s + 1]] = inv.double() / (max(int(comp[c[s]:c[s + 1]].sum()), 1) if per_seq_mean else 1)
    r = torch.exp(lp - (old.double() if has_old else lp.detach()))
    l = -torch.min(r * A, r.clamp(1 - lo, 1 + hi) * A)
    kl = torch.zeros_like(l)
    if has_ref:
        d = rlp.double() - lp
        kl = torch.exp(d) - d - 1
        l = l + beta * kl
    want0 = torch.where(comp, w * l, torch.zeros_like(l))
    (g,) = torch.autograd.grad(want0.sum(), lp)
    want1 = torch.where(comp, g, torch.zeros_like(g))
    assert rel_err(rows[0], want0.detach()).max().item() < 5e-6
    assert rel_err(rows[1], want1).max().item() < 5e-6
    rd = r.detach()
    for i, v in enumerate((want0.detach(), comp.double(), (comp & (rd < 1 - lo) & (A < 0)).double(),
                           (comp & (rd > 1 + hi) & (A > 0)).double(), torch.where(comp, kl.detach(), kl.detach() * 0),
                           torch.where(comp, rd, rd * 0))):
        want = torch.stack([v[c[s]:c[s + 1]].sum() for s in range(S)])
        if i in (1, 2, 3):
            assert torch.equal(seq[i].double(), want)
        else:
            assert rel_err(seq[i], want).max().item() < 2e-5
    assert not rows[:, ~comp].any() and seq[1, 5] == 0
    # the fp64 form of the twin is the same function
    r64, _ = ref.grpo_token(nll.double(), None if old is None else old.double(), None if rlp is None else rlp.double(),
                            labels, adv.double(), cu, S, inv.double(), lo, hi, beta, per_seq_mean)
    assert r64.dtype == torch.float64 and torch.allclose(r64[0], want0.detach(), rtol=1e-12, atol=0)
    # poison off the completion rows changes nothing
    nan = torch.full_like(nll, math.nan)
    p = ref.grpo_token(torch.where(comp, nll, nan), None if old is None else torch.where(comp, old, nan),
                       None if rlp is None else torch.where(comp, rlp, nan), labels, adv, cu, S, inv, lo, hi, beta,
                       per_seq_mean)
    assert torch.equal(p[0], rows) and torch.equal(p[1], seq)
    assert ops.grpo_token_stats(nll, old, rlp, labels, adv, cu, S, inv, lo, hi, beta, per_seq_mean)[0].equal(rows)


def test_scale_rows_twin():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(37, 24, generator=g).to(torch.bfloat16)
    coef, gs = torch.randn(37, generator=g), torch.tensor([-1.0 / 0.7])
    out = ref.scale_rows(x, coef, gs)
    want = (x.float() * (coef * gs)[:, None]).to(torch.bfloat16)
    assert out.dtype == torch.bfloat16 and torch.equal(out, want)
    assert torch.allclose(ref.scale_rows(x.double(), coef.double(), gs.double()),
                          x.double() * (coef.double() * gs.double())[:, None], rtol=1e-15)
    y = x.clone()
    assert ops.scale_rows(y, coef, gs, inplace=True) is y and torch.equal(y, want)


@pytest.mark.parametrize("tau", [0.7, 1.5])
def test_cross_entropy_twin_at_a_temperature(tau):
    g = torch.Generator().manual_seed(2)
    x = (3 * torch.randn(6, 264, generator=g)).to(torch.bfloat16)
    labels = torch.tensor([0, 263, -100, 17, 100, 5])
    loss, lse, correct, ent = ref.cross_entropy(x, labels, temperature=tau)
    lp = torch.log_softmax(x.double() / tau, -1)
    valid = labels != -100
    want = torch.where(valid, -lp.gather(-1, labels.clamp(min=0)[:, None]).squeeze(-1), torch.zeros(6, dtype=torch.float64))
    assert torch.allclose(loss.double(), want, atol=1e-5) and loss[2] == 0
    assert torch.allclose(lse.double(), torch.logsumexp(x.double() / tau, -1), atol=1e-5)
    assert torch.allclose(ent.double(), -(lp.exp() * lp).sum(-1), atol=1e-4)
    grad = ref.cross_entropy_grad(x, labels, torch.tensor([0.5]), temperature=tau)
    xs = x.double().requires_grad_(True)
    nll = -torch.log_softmax(xs / tau, -1).gather(-1, labels.clamp(min=0)[:, None]).squeeze(-1)
    (gw,) = torch.autograd.grad((nll * valid).sum() * 0.5, xs)
    assert torch.allclose(grad.double(), gw * tau, atol=1e-6)       # the twin leaves the chain rule's 1 / tau out
    same = ref.cross_entropy(x, labels, temperature=1.0)
    assert all(torch.equal(a, b) for a, b in zip(same, ref.cross_entropy(x, labels)))
    for bad in (dict(temperature=0.0), dict(temperature=0.7, label_smoothing=0.1), dict(temperature=0.7, loss_mode=1)):
        with pytest.raises(ValueError):
            ref.cross_entropy(x, labels, **bad)


def test_lm_head_policy_loss_matches_autograd():
    g = torch.Generator().manual_seed(3)
    M, H, Vv, tau = 40, 16, 64, 0.8
    h = torch.randn(M, H, generator=g).requires_grad_(True)       # fp32: the reference path computes the loss in fp32
    w = (0.3 * torch.randn(Vv, H, generator=g)).requires_grad_(True)
    cu = torch.tensor([0, 12, 30, 40], dtype=torch.int32)
    labels = torch.randint(0, Vv, (M,), generator=g)
    labels[:4] = -100
    labels[30:] = -100
    adv = torch.tensor([0.9, -0.6])
    inv = torch.tensor([1.0 / 24.0])
    with torch.no_grad():
        lp0 = ops.lm_head_token_logps(h, w, labels, tau).double()
    old = lp0 - torch.tensor([0.6, 0.95, 1.05, 1.5], dtype=torch.float64)[torch.randint(0, 4, (M,), generator=g)].log()
    rlp = lp0 + 0.2 * torch.randn(M, generator=g, dtype=torch.float64)
    loss, stats, rows, seq = ops.lm_head_policy_loss(h, w, labels, adv, cu, 2, inv, old, rlp, 0.2, 0.28, 0.04, tau, False)
    loss.backward()
    h2, w2 = h.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    adv, inv = adv.double(), inv.double()
    lp = torch.log_softmax((h2 @ w2.t()) / tau, -1)[torch.arange(M), labels.clamp(min=0)]
    A = torch.cat([adv[:1].expand(12), adv[1:].expand(18), torch.zeros(10, dtype=torch.float64)])
    r = torch.exp(lp - old)
    d = rlp - lp
    l = -torch.min(r * A, r.clamp(0.8, 1.28) * A) + 0.04 * (torch.exp(d) - d - 1)
    comp = (labels >= 0) & (torch.arange(M) < 30)
    want = (torch.where(comp, l, torch.zeros_like(l)) * inv).sum()
    want.backward()
    assert torch.allclose(loss.double(), want, rtol=1e-5)
    assert torch.allclose(h.grad.double(), h2.grad, rtol=1e-4, atol=1e-7)
    assert torch.allclose(w.grad.double(), w2.grad, rtol=1e-4, atol=1e-7)
    assert not h.grad[30:].any() and seq[1].tolist() == [8.0, 18.0] and lp0[:4].abs().sum() == 0


# ------------------------------------------------------------------------------------------------ rollouts
def test_rollout_batch_host_path():
    m = tiny_model()
    m.train()
    prompts = [r["prompt_ids"] for r in prompt_rows(3, seed=5)]
    toks, lps = rollout_batch(m, prompts, 6, None, temperature=0.9, seed=11)
    assert m.training                                            # restored
    assert [len(t) for t in toks] == [6, 6, 6] and [len(x) for x in lps] == [6, 6, 6]
    assert (toks, lps) == rollout_batch(m, prompts, 6, None, temperature=0.9, seed=11)
    # the log-probabilities are token_logps of the same sequences
    m.eval()
    for p, t, lp in zip(prompts, toks, lps):
        ids = torch.tensor(p + t)
        labels = torch.tensor([-100] * (len(p) - 1) + t + [-100])
        with torch.no_grad():
            got = m.token_logps(ids, labels, shift_labels=False, temperature=0.9)
        assert torch.allclose(got[len(p) - 1:-1], torch.tensor(lp), atol=1e-4)
    # an EOS ends its row; top_k > 0 gives no log-probabilities; generate_batch is what it was
    eos = toks[0][2]
    te, le = rollout_batch(m, prompts, 6, eos, temperature=0.9, seed=11)
    assert te[0] == toks[0][:toks[0].index(eos) + 1] and len(le[0]) == len(te[0])
    tk, lk = rollout_batch(m, prompts, 4, None, top_k=5, seed=11)
    assert lk is None and [len(t) for t in tk] == [4, 4, 4]
    assert rollout_batch(m, [], 4, None) == ([], []) and rollout_batch(m, prompts, 0, None)[0] == [[], [], []]
    assert generate_batch(m, prompts, 4, seed=3) == generate_batch(m, prompts, 4, seed=3)


# ------------------------------------------------------------------------------------------------ loader
class _Sampler:
    def __init__(self, n):
        self.n, self.epoch = n, 0

    def set_epoch(self, e):
        self.epoch = e

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter([torch.tensor([10 * self.epoch + i]) for i in range(self.n)])


def test_rollout_loader_schedule_replay_and_skip():
    made = []

    def make(epoch, f, idx):
        made.append((epoch, f, int(idx)))
        return {"f": f, "serial": len(made)}

    ld = RolloutLoader(_Sampler(5), make, ga=2, mu=3)
    assert len(ld) == 12                                        # 4 of the 5 fresh batches (whole steps) x 3 iterations
    out = [(b["f"], b["iteration"], b["serial"]) for b in ld.iter()]
    assert [(f, it) for f, it, _ in out] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2),
                                             (2, 0), (3, 0), (2, 1), (3, 1), (2, 2), (3, 2)]
    assert made == [(0, 0, 0), (0, 1, 1), (0, 2, 2), (0, 3, 3)]  # each fresh batch generated once, replays reuse it
    assert [s for _, _, s in out] == [1, 2, 1, 2, 1, 2, 3, 4, 3, 4, 3, 4]
    made.clear()
    ld.set_epoch(1)
    rest = [(b["f"], b["iteration"]) for b in ld.iter(skip=6)]
    assert rest == [(2, 0), (3, 0), (2, 1), (3, 1), (2, 2), (3, 2)]
    assert made == [(1, 2, 12), (1, 3, 13)]                     # nothing generated for the skipped positions
    with pytest.raises(ValueError, match="gradient_accumulation"):
        RolloutLoader(_Sampler(1), make, ga=2, mu=1)
    assert len({rollout_seed(42, e, i, r) for e in range(3) for i in range(4) for r in range(2)}) == 24
    assert rollout_seed(42, 1, 2, 0) == rollout_seed(42, 1, 2, 0) and 0 <= rollout_seed(7, 0, 0, 0) < 2 ** 30


def test_trainer_batches_groups_seeds_and_masks(tmp_path):
    ds = prompt_rows(8, seed=1)
    for i, r in enumerate(ds):
        r["tag"] = f"row{i}"
    seen = []

    def spy(prompts, completions, completion_ids, tag, **kw):
        seen.append(list(tag))
        assert prompts == [r["prompt_ids"] for t in tag for r in ds if r["tag"] == t]
        assert completions == completion_ids                      # no tokenizer: the ids themselves
        return [float(len(c)) for c in completion_ids]

    t = grpo_trainer(tmp_path, tiny_model(), ds, rewards=[low_share, spy], reward_weights=[1.0, 0.0],
                     mask_truncated_completions=False, num_iterations=2, beta=0.04)
    assert t.reward_names == ["low_share", "spy"]
    ld = t.get_train_dataloader()
    it = ld.iter()
    b0, b0r = next(it), next(it)
    assert len(seen) == 1 and seen[0][:4] == [seen[0][0]] * 4 and seen[0][4:] == [seen[0][4]] * 4  # whole groups
    assert b0["iteration"] == 0 and b0r["iteration"] == 1 and b0r["input_ids"] is b0["input_ids"]
    assert b0["n_seqs"] == 8 and b0["advantages"].shape == (8,) and b0["cu_seqlens"].numel() >= 9
    comp = b0["labels"] >= 0
    assert int(comp.sum()) == sum(len(c) for c in b0["completion_ids"]) == b0["num_items"]
    assert torch.allclose(b0["old_logps"][comp], b0["sampler_logps"][comp], atol=1e-4)  # one policy, two paths
    assert not b0["old_logps"][~comp].any() and "ref_logps" in b0
    # the reference is a bf16 copy of this fp32 starting policy: the same log-probabilities up to the weights' rounding
    assert torch.allclose(b0["ref_logps"], b0["old_logps"], atol=2e-2) and t._ref.lm_head_weight.dtype == torch.bfloat16
    adv = b0["advantages"].view(2, 4)
    assert torch.allclose(adv.sum(1), torch.zeros(2), atol=1e-4)
    # a second trainer with the same seed regenerates the same batch; another rank or step draws differently
    t2 = grpo_trainer(tmp_path, tiny_model(), ds, rewards=low_share, num_iterations=2, beta=0.04)
    c0 = next(t2.get_train_dataloader().iter())
    assert c0["completion_ids"] == b0["completion_ids"] and torch.equal(c0["input_ids"], b0["input_ids"])
    t2.dp_rank = 1
    assert next(t2.get_train_dataloader().iter())["completion_ids"] != b0["completion_ids"]
    nxt = next(it)
    assert nxt["iteration"] == 0 and nxt["completion_ids"] != b0["completion_ids"] and len(seen) == 2
    # loss types: what num_items counts; truncated completions masked
    for lt, want in (("grpo", 8.0), ("dr_grpo", 48.0)):
        b = next(grpo_trainer(tmp_path, tiny_model(), ds, loss_type=lt).get_train_dataloader().iter())
        assert b["num_items"] == want
    tm = grpo_trainer(tmp_path, tiny_model(), ds, mask_truncated_completions=True)
    tm._eos = None                                               # nothing ends in EOS: everything is truncated
    bm = next(tm.get_train_dataloader().iter())
    assert not (bm["labels"] >= 0).any() and bm["num_items"] == 0.0


# ------------------------------------------------------------------------------------------------ training
def test_grpo_logs_evaluate_and_save(tmp_path):
    ds = prompt_rows(8, seed=2)
    t = grpo_trainer(tmp_path / "a", tiny_model(), ds, eval_ds=ds[:3], max_steps=2, num_iterations=2, beta=0.04,
                     epsilon_high=0.28, save_strategy="steps", save_steps=2)
    before = t.engine.params_by_name().clone()
    quiet_train(t)
    logs = train_logs(t)
    assert len(logs) == 2 and not torch.equal(before, t.engine.params_by_name())
    for k in ("loss", "reward", "reward_std", "rewards/low_share/mean", "frac_reward_zero_std",
              "completions/mean_length", "completions/clipped_ratio", "clip_ratio/low_mean", "clip_ratio/high_mean",
              "clip_ratio/region_mean", "kl", "entropy"):
        assert all(k in h and math.isfinite(h[k]) for h in logs), k
    assert "sampling/logp_difference" in logs[0] and logs[0]["sampling/logp_difference"] < 1e-4
    assert "sampling/logp_difference" not in logs[1] and logs[0]["reward"] == logs[1]["reward"]
    assert t.rollouts_generated == 1 and t._ref is not None
    with contextlib.redirect_stdout(io.StringIO()):
        ev = t.evaluate()
    assert set(ev) >= {"eval_reward", "eval_reward_std", "eval_completions/mean_length"} and 0 <= ev["eval_reward"] <= 1
    ck = os.path.join(str(tmp_path / "a"), "checkpoint-2")
    from safetensors import safe_open
    with safe_open(os.path.join(ck, "model.safetensors"), "pt") as f:
        names = list(f.keys())
    assert len(names) == len(t.model.hf_state_dict())           # one copy of the weights: the policy's
    assert not any(n.startswith("_ref") for n, _ in t.model.named_parameters())
    one = grpo_trainer(tmp_path / "b", tiny_model(), ds, max_steps=2)
    quiet_train(one)
    assert all(h[f"clip_ratio/{k}_mean"] == 0.0 for h in train_logs(one) for k in ("low", "high", "region"))
    assert all("kl" not in h for h in train_logs(one)) and one._ref is None and one.rollouts_generated == 2
    with pytest.raises(ValueError, match="ref_model"):
        grpo_trainer(tmp_path / "a", tiny_model(), ds, max_steps=3, beta=0.04).train(resume_from_checkpoint=ck)


def test_grpo_resume_bit_for_bit(tmp_path):
    ds = prompt_rows(8, seed=3)
    kw = dict(max_steps=4, save_strategy="steps", save_steps=2, save_total_limit=5)
    full = grpo_trainer(tmp_path / "full", tiny_model(), ds, **kw)
    quiet_train(full)
    want = {h["step"]: (h["loss"], h["reward"]) for h in train_logs(full)}
    first = grpo_trainer(tmp_path / "run", tiny_model(), ds, **kw)
    first.args.max_steps = 2
    quiet_train(first)
    ck = os.path.join(str(tmp_path / "run"), "checkpoint-2")
    second = grpo_trainer(tmp_path / "run", tiny_model(seed=9), ds, **kw)
    quiet_train(second, resume_from_checkpoint=ck)
    got = {h["step"]: (h["loss"], h["reward"]) for h in train_logs(second)}
    assert sorted(got) == [1, 2, 3, 4] and got[3] == want[3] and got[4] == want[4], (got, want)
    assert second.rollouts_generated == 2                        # steps 3 and 4 only
    assert torch.equal(second.engine.params_by_name(), full.engine.params_by_name())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import llm_fine_tune_distributed_amd.parallel.process_group as pgm
    pgm._STATE = None
    torch.manual_seed(0)
    t = grpo_trainer(out_dir, tiny_model(seed=3), prompt_rows(8, seed=7), max_steps=2, ddp_check_sync_every=1,
                     ddp_bucket_cap_mb=0.05, ddp_first_bucket_mb=0.01)
    first = next(t.get_train_dataloader().iter())["completion_ids"]
    quiet_train(t)
    torch.save({"params": t.engine.params_by_name().clone(), "log": train_logs(t), "first": first},
               os.path.join(out_dir, f"r{world}_{rank}.pt"))
    pgm.cleanup_distributed()


def test_grpo_two_gloo_ranks():
    d = tempfile.mkdtemp()
    mp.spawn(_rank, args=(2, _free_port(), d), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(d, f"r2_{r}.pt")) for r in range(2))
    assert torch.equal(r0["params"], r1["params"])               # the ranks stay bit-identical
    assert r0["first"] != r1["first"]                            # each rank rolls out its own prompts, its own seed
    assert len(r0["log"]) == 2 and all(math.isfinite(h["loss"]) for h in r0["log"])
    for a, b in zip(r0["log"], r1["log"]):                       # logs are all-reduced: the same on both ranks
        assert a["reward"] == b["reward"] and a["loss"] == b["loss"]
    again = tempfile.mkdtemp()
    mp.spawn(_rank, args=(2, _free_port(), again), nprocs=2, join=True)
    s0 = torch.load(os.path.join(again, "r2_0.pt"))
    assert torch.equal(s0["params"], r0["params"]) and s0["first"] == r0["first"]  # the same seeds: the same run


def test_grpo_learns(tmp_path):
    """tiny, seed 42, 16 prompts, 2 prompts x 8 generations of 8 tokens per step, lr 3e-3 constant, 40 steps, reward =
    share of completion tokens below vocab / 2. Observed on the CPU: mean reward 0.497 over steps 1-10, 0.855 over
    steps 31-40 (lr 1e-3: 0.494 -> 0.544; lr 1e-2: 0.605 -> 1.000)."""
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer
    m = build_model(get_config("tiny"), device="cpu", dtype=torch.float32, seed=0)
    g = torch.Generator().manual_seed(0)
    ds = [{"prompt_ids": torch.randint(3, V, (int(n),), generator=g).tolist()}
          for n in torch.randint(3, 9, (16,), generator=g)]
    a = GRPOConfig(output_dir=str(tmp_path), per_device_train_batch_size=16, num_generations=8, max_completion_length=8,
                   max_steps=40, learning_rate=3e-3, lr_scheduler_type="constant", logging_steps=1, jsonl_log=False,
                   save_strategy="no")
    t = GRPOTrainer(model=m, reward_funcs=low_share, args=a, train_dataset=ds)
    quiet_train(t)
    r = [h["reward"] for h in train_logs(t)]
    first, last = sum(r[:10]) / 10, sum(r[-10:]) / 10
    print(f"\n[grpo] learning run: mean reward {first:.3f} (steps 1-10) -> {last:.3f} (steps 31-40)")
    assert len(r) == 40 and last > first + 0.15, (first, last)


# ------------------------------------------------------------------------------------------------ CLI and rewards
def test_builtin_rewards():
    from llm_fine_tune_distributed_amd.train import rewards
    ids = [[1] * 4, [1] * 16, [1] * 192, [1] * 288, [1] * 400, []]
    assert rewards.length_band(completion_ids=ids) == [0.25, 1.0, 1.0, 0.5, 0.0, 0.0]
    got = rewards.answer_match(completions=["  Boil it ", "first, boil IT for a minute", "filter it", "x"],
                               answer=["boil it", "Boil  it", "boil it", None])
    assert got == [1.0, 0.5, 0.0, 0.0]
    with pytest.raises(ValueError, match="answer"):
        rewards.answer_match(completions=["a"])
    assert rewards.resolve("llm_fine_tune_distributed_amd.train.rewards:length_band") is rewards.length_band
    for bad in ("no_colon", "llm_fine_tune_distributed_amd.train.rewards:missing"):
        with pytest.raises(ValueError):
            rewards.resolve(bad)


def test_train_cli_grpo(tmp_path, monkeypatch):
    from llm_fine_tune_distributed_amd.cli import train as cli
    from llm_fine_tune_distributed_amd.data.synthetic import generate_qa
    out = tmp_path / "out"
    monkeypatch.setenv("OUTPUT_DIR", str(out))
    monkeypatch.setenv("EPOCHS", "1")
    monkeypatch.setenv("BATCH_SIZE", "8")
    monkeypatch.setenv("LEARNING_RATE", "1e-4")
    monkeypatch.setenv("AIM_REPO", str(tmp_path / "aim"))
    data = tmp_path / "qa.jsonl"
    with open(data, "w") as f:
        for r in generate_qa(24, seed=3):
            f.write(json.dumps({"full-question": r["full-question"], "answer": r["answer"]}) + "\n")
    common = ["--model", "tiny", "--dataset", str(data), "--max-steps", "2", "--grad-accum", "1",
              "--no-gradient-checkpointing"]
    with pytest.raises(SystemExit):
        cli.main(common + ["--reward", "llm_fine_tune_distributed_amd.train.rewards:length_band"])  # not --trainer grpo
    with pytest.raises(SystemExit):
        cli.main(common + ["--trainer", "grpo"])                                                    # no --reward
    cli.main(common + ["--trainer", "grpo", "--reward", "llm_fine_tune_distributed_amd.train.rewards:answer_match",
                       "--reward", "llm_fine_tune_distributed_amd.train.rewards:length_band",
                       "--set", "num_generations=4", "--set", "max_completion_length=4", "--set", "max_prompt_length=24",
                       "--set", "logging_steps=1", "--set", "reward_weights=[1.0, 0.5]"])
    resolved = json.load(open(out / "sft_config.json"))
    assert resolved["num_generations"] == 4 and resolved["loss_type"] == "dapo"
    assert resolved["metric_for_best_model"] == "eval_reward"
    logs = [json.loads(l) for l in open(out / "checkpoints" / "metrics.jsonl")]
    steps = [h for h in logs if "loss" in h]
    assert len(steps) == 2
    for k in ("reward", "rewards/answer_match/mean", "rewards/length_band/mean", "completions/mean_length"):
        assert all(k in h for h in steps), k
    assert all(h["rewards/length_band/mean"] == 0.25 or h["completions/mean_length"] < 4 for h in steps)
