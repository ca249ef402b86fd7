"""The SFT objectives on CPU: the three SFTConfig fields (neftune_noise_alpha, label_smoothing_factor, loss_type)
through every way a field is set, the statistics of the NEFTune noise twin, the per-token noise magnitude for each batch layout,
parity of the smoothed and dft losses with HF's LabelSmoother / TRL's dft_loss definition, and the trainer's handling of
all three (noise only while train() runs, resume reproduces it, eval_loss is the objective)."""
import json
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
from llm_fine_tune_distributed_amd.models import build_model, tiny
from llm_fine_tune_distributed_amd.ops import reference as ref
from llm_fine_tune_distributed_amd.train import SFTConfig, SFTTrainer
from llm_fine_tune_distributed_amd.train.config import apply_overrides

SEEDS = (1, 12345, 2 ** 31 - 2)


# ------------------------------------------------------------------------------------------------ configuration
def test_fields_default_off():
    c = SFTConfig()
    assert c.neftune_noise_alpha is None and c.label_smoothing_factor == 0.0 and c.loss_type == "nll"
    c.validate_objective()


def test_fields_through_kwargs_and_to_dict(recwarn):
    c = SFTConfig(neftune_noise_alpha=5, label_smoothing_factor=0.1, loss_type="nll")
    assert not [w for w in recwarn.list if "unsupported" in str(w.message)]  # no longer dropped with a warning
    d = c.to_dict()
    assert (d["neftune_noise_alpha"], d["label_smoothing_factor"], d["loss_type"]) == (5, 0.1, "nll")
    c2 = SFTConfig(**d)
    assert (c2.neftune_noise_alpha, c2.label_smoothing_factor, c2.loss_type) == (5, 0.1, "nll")
    assert c.replace(loss_type="dft", label_smoothing_factor=0.0).loss_type == "dft"


def test_fields_through_yaml_json_and_set(tmp_path):
    y = tmp_path / "c.yaml"
    y.write_text("sft_config:\n  neftune_noise_alpha: 5\n  label_smoothing_factor: 0.1\n")
    c = apply_overrides(SFTConfig(), str(y))
    assert c.neftune_noise_alpha == 5 and c.label_smoothing_factor == 0.1 and c.loss_type == "nll"
    j = tmp_path / "c.json"
    j.write_text(json.dumps({"loss_type": "dft", "neftune_noise_alpha": 2.5}))
    c = apply_overrides(SFTConfig(), str(j))
    assert c.loss_type == "dft" and c.neftune_noise_alpha == 2.5
    c = apply_overrides(SFTConfig(), None, ["neftune_noise_alpha=5", "label_smoothing_factor=0.05", "loss_type=dft"])
    assert c.neftune_noise_alpha == 5.0 and c.label_smoothing_factor == 0.05 and c.loss_type == "dft"
    assert apply_overrides(c, None, ["neftune_noise_alpha=none"]).neftune_noise_alpha is None
    # what the trainer writes next to a checkpoint (sft_config.json: to_json) reads back as a config file
    p = tmp_path / "sft_config.json"
    SFTConfig(neftune_noise_alpha=5, label_smoothing_factor=0.1).to_json(str(p))
    c = apply_overrides(SFTConfig(), str(p))
    assert c.neftune_noise_alpha == 5 and c.label_smoothing_factor == 0.1


def test_shipped_example_config_loads():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "configs", "smollm3_lora_1gpu.yaml")
    assert "neftune_noise_alpha" in open(path).read()
    apply_overrides(SFTConfig(), path).validate_objective()


@pytest.mark.parametrize("kw", [{"neftune_noise_alpha": -1.0}, {"label_smoothing_factor": 1.0},
                                {"label_smoothing_factor": -0.1}, {"loss_type": "focal"},
                                {"loss_type": "dft", "label_smoothing_factor": 0.1}])
def test_validation_errors_when_the_trainer_is_built(tmp_path, kw):
    m = build_model(tiny(), dtype=torch.float32, seed=0)
    ds = TokenizedDataset.synthetic(4, m.config.vocab_size, 5, 9, seed=1)
    with pytest.raises(ValueError):
        SFTTrainer(model=m, args=SFTConfig(output_dir=str(tmp_path), jsonl_log=False, **kw), train_dataset=ds)


def test_zero_alpha_and_dft_alone_are_valid():
    SFTConfig(neftune_noise_alpha=0).validate_objective()
    SFTConfig(loss_type="dft").validate_objective()
    SFTConfig(label_smoothing_factor=0.999).validate_objective()


# ------------------------------------------------------------------------------------------------ the noise twin
@pytest.mark.parametrize("seed", SEEDS)
def test_noise_twin_statistics(seed):
    n = 2 ** 20
    u = ref.embedding_noise_u(torch.arange(n, dtype=torch.int64), seed)
    assert u.dtype == torch.float32
    assert bool((u.abs() < 1).all()) and bool((u != 0).all())
    k = u.double() * 2 ** 23  # odd integers: exact in fp32
    assert bool((k == k.round()).all()) and bool((k.abs() % 2 == 1).all())
    ud = u.double()
    mean, var = ud.mean().item(), ud.var(unbiased=False).item()
    print(f"\n[objectives] noise twin seed {seed}: mean {mean:.3e} 3 var {3 * var:.5f}")
    assert abs(mean) < 4 / math.sqrt(3 * n)   # four standard errors of the mean of a uniform on (-1, 1): 2.26e-3
    assert abs(3 * var - 1) < 3.5e-3          # four standard errors of the variance


def test_noise_twin_values():
    """embedding_noise == the gather plus mag * u in two fp32 roundings and one rounding to the weight's dtype; a zero
    magnitude returns the gathered row bit for bit; 64-bit element indices reach the high word of the hash."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(50, 24, generator=g).to(torch.bfloat16)
    ids = torch.tensor([[0, 49, 7], [7, 7, 3]])
    mag = torch.tensor([0.5, 0.0, 0.25, 1.0, 0.125, 3.0])
    out = ref.embedding_noise(ids, w, mag, 77)
    assert out.shape == (2, 3, 24) and out.dtype == torch.bfloat16
    flat = out.view(6, 24)
    assert torch.equal(flat[1], w[49])
    u = ref.embedding_noise_u(torch.arange(6 * 24).view(6, 24), 77)
    want = (w[ids.reshape(-1)].float() + mag[:, None] * u).to(torch.bfloat16)
    assert torch.equal(flat, want)
    assert not torch.equal(flat[2], flat[3])  # the same id at two positions: different noise
    assert not torch.equal(out, ref.embedding_noise(ids, w, mag, 78))
    assert torch.equal(out, ref.embedding_noise(ids, w, mag, 77))
    big = torch.tensor([5, 5 + 2 ** 32, 5 + 2 ** 33])
    assert len(set(ref.embedding_noise_u(big, 1).tolist())) == 3


# ------------------------------------------------------------------------------------------------ the magnitude
def _tiny_model(seed=3, **kw):
    return build_model(tiny(**kw), dtype=torch.float32, seed=seed)


def test_mag_padded_batch():
    m = _tiny_model()
    m.neftune_noise_alpha = 5.0
    H, B, T = m.config.hidden_size, 3, 11
    cu = torch.arange(0, (B + 1) * T, T, dtype=torch.int32)
    mag = m._neftune_mag(cu, B * T, (B, T))
    assert mag.dtype == torch.float32 and mag.shape == (B * T,)
    assert torch.equal(mag, torch.full((B * T,), 5.0 / math.sqrt(T * H)))  # pad rows included: HF's alpha / sqrt(T H)
    assert m._neftune_mag(cu, B * T, (B, T)) is mag                        # the cached constant
    m.neftune_noise_alpha = 2.0
    assert torch.equal(m._neftune_mag(cu, B * T, (B, T)), torch.full((B * T,), 2.0 / math.sqrt(T * H)))


def test_mag_packed_batch():
    m = _tiny_model()
    m.neftune_noise_alpha = 5.0
    H = m.config.hidden_size
    lens = [4, 9, 1, 6]
    cu = torch.tensor([0, 4, 13, 14, 20], dtype=torch.int32)
    mag = m._neftune_mag(cu, 20, None)
    want = torch.cat([torch.full((n,), 5.0 / math.sqrt(n * H), dtype=torch.float64) for n in lens])
    assert mag.dtype == torch.float32 and mag.shape == (20,)
    assert torch.allclose(mag.double(), want, rtol=2e-7, atol=0)
    # rows past the last boundary (not produced by the collator) count as one more segment
    mag = m._neftune_mag(cu, 23, None)
    assert torch.allclose(mag[20:].double(), torch.full((3,), 5.0 / math.sqrt(3 * H), dtype=torch.float64), rtol=2e-7)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cp_mag_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _tiny_model()
    m.enable_context_parallel(dist.group.WORLD, "zigzag")
    m.neftune_noise_alpha = 5.0
    B, L = 2, 6  # this rank's chunk of sequences of global length L * world
    cu = torch.arange(0, (B + 1) * L, L, dtype=torch.int32)
    torch.save(m._neftune_mag(cu, B * L, (B, L)), os.path.join(out_dir, f"mag{rank}.pt"))
    dist.destroy_process_group()


def test_mag_context_parallel_uses_the_global_length():
    d = tempfile.mkdtemp()
    mp.spawn(_cp_mag_worker, args=(2, _free_port(), d), nprocs=2, join=True)
    H = tiny().hidden_size
    mag = torch.load(os.path.join(d, "mag0.pt"))
    assert torch.equal(mag, torch.full((12,), 5.0 / math.sqrt(12 * H)))  # L_m = 6 local x 2 ranks


# ------------------------------------------------------------------------------------------------ model: noise gating
def _batch(cfg, B=2, T=13, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.vocab_size, (B, T), generator=g)
    labels = ids.clone()
    labels[1, 9:] = -100
    return ids, labels


def test_noise_only_in_training_forwards_with_grad():
    m = _tiny_model()
    ids, labels = _batch(m.config)
    m.train()
    clean = m(ids, labels=labels).loss.item()
    m.neftune_noise_alpha = 5.0
    torch.manual_seed(4)
    noisy = m(ids, labels=labels).loss.item()
    torch.manual_seed(4)
    again = m(ids, labels=labels).loss.item()
    other = m(ids, labels=labels).loss.item()  # the next draw of the generator: another noise field
    assert noisy != clean and noisy == again and other != noisy
    with torch.no_grad():
        assert m(ids, labels=labels).loss.item() == clean
    m.eval()
    assert m(ids, labels=labels).loss.item() == clean
    m.train()
    m.neftune_rank = 1  # the rank is mixed into the seed
    torch.manual_seed(4)
    assert m(ids, labels=labels).loss.item() != noisy


def test_noise_leaves_the_embedding_backward_as_it_is():
    """The noise is additive: d out / d weight is the plain gather's, so with the same upstream gradient the embedding
    gradient equals EmbeddingFn's bit for bit."""
    import llm_fine_tune_distributed_amd.ops as ops
    g = torch.Generator().manual_seed(1)
    w1 = torch.randn(40, 16, generator=g).requires_grad_(True)
    w2 = w1.detach().clone().requires_grad_(True)
    ids = torch.tensor([3, 3, 39, 0, 7])
    dy = torch.randn(5, 16, generator=g)
    ops.embedding(ids, w1).backward(dy)
    ops.noisy_embedding(ids, w2, torch.full((5,), 0.3), 9).backward(dy)
    assert torch.equal(w1.grad, w2.grad)


# ------------------------------------------------------------------------------------------------ loss parity
def _loss_and_grads(m, ids, labels, **kw):
    for p in m.parameters():
        p.grad = None
    m.reset_grad_use_counters()
    out = m(ids, labels=labels, **kw)
    out.loss.backward()
    return out, {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _autograd_reference(m, ids, labels, loss_of_logits):
    for p in m.parameters():
        p.grad = None
    m.reset_grad_use_counters()
    logits = m(ids, return_logits=True).logits.view(*ids.shape, -1)
    loss = loss_of_logits(logits)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _assert_same(loss, grads, want_loss, want_grads):
    assert abs(loss.item() - want_loss.item()) < 1e-5 * max(1.0, abs(want_loss.item())), (loss, want_loss)
    for n, g in want_grads.items():
        e = (grads[n] - g).abs().max().item()
        assert e < 1e-5 * max(1.0, g.abs().max().item()), (n, e)


@pytest.mark.parametrize("eps", [0.1, 0.3])
def test_label_smoothing_equals_hf_label_smoother(eps):
    from transformers.trainer_pt_utils import LabelSmoother
    m = _tiny_model()
    m.train()
    ids, labels = _batch(m.config)
    out, grads = _loss_and_grads(m, ids, labels, label_smoothing=eps)
    want, want_grads = _autograd_reference(
        m, ids, labels, lambda lg: LabelSmoother(epsilon=eps)({"logits": lg}, labels, shift_labels=True))
    _assert_same(out.loss, grads, want, want_grads)
    plain = m(ids, labels=labels)
    assert abs(plain.loss.item() - out.loss.item()) > 1e-3  # it is another objective
    assert torch.equal(plain.stats[1:], out.stats[1:])       # lse, entropy, correct: the TRL metrics do not move
    shifted = torch.cat([labels[:, 1:], torch.full_like(labels[:, :1], -100)], 1).reshape(-1)
    assert bool((out.stats[0][shifted == -100] == 0).all())


def test_dft_equals_its_definition_under_autograd():
    """TRL dft_loss: -stopgrad(p_y) log p_y per token, summed over the valid tokens / their count."""
    m = _tiny_model()
    m.train()
    ids, labels = _batch(m.config)

    def dft(lg):
        lp = torch.log_softmax(lg[:, :-1].float(), -1)
        y = labels[:, 1:]
        valid = y != -100
        lpy = lp.gather(-1, y.clamp(min=0)[..., None]).squeeze(-1)
        return (-(lpy.exp().detach() * lpy) * valid).sum() / valid.sum()

    out, grads = _loss_and_grads(m, ids, labels, loss_type="dft")
    want, want_grads = _autograd_reference(m, ids, labels, dft)
    _assert_same(out.loss, grads, want, want_grads)
    plain = m(ids, labels=labels)
    assert torch.equal(plain.stats[1:], out.stats[1:])


def test_default_arguments_take_the_plain_path():
    m = _tiny_model()
    m.train()
    ids, labels = _batch(m.config)
    a, ga = _loss_and_grads(m, ids, labels)
    b, gb = _loss_and_grads(m, ids, labels, label_smoothing=0.0, loss_type="nll")
    assert torch.equal(a.loss, b.loss) and all(torch.equal(ga[n], gb[n]) for n in ga)
    with pytest.raises(ValueError):
        m(ids, labels=labels, label_smoothing=0.1, loss_type="dft")
    with pytest.raises(ValueError):
        m(ids, labels=labels, loss_type="focal")


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(out_dir, max_steps=3, save_steps=0, seed=3, **kw):
    m = _tiny_model(seed)
    ds = TokenizedDataset.synthetic(32, m.config.vocab_size, 6, 14, seed=7)
    a = SFTConfig(output_dir=str(out_dir), per_device_train_batch_size=4, learning_rate=1e-3, max_steps=max_steps,
                  logging_steps=1, logging_first_step=True, save_steps=save_steps,
                  save_strategy="steps" if save_steps else "no", dataloader_drop_last=True, jsonl_log=False,
                  lr_scheduler_type="constant", **kw)
    return SFTTrainer(model=m, args=a, train_dataset=ds,
                      eval_dataset=TokenizedDataset.synthetic(8, m.config.vocab_size, 6, 14, seed=9))


def _losses(t):
    return [h["loss"] for h in t.state.log_history if "loss" in h]


def test_trainer_neftune(tmp_path):
    t0 = _trainer(tmp_path / "a0")
    t0.train()
    t5 = _trainer(tmp_path / "a5", neftune_noise_alpha=5)
    assert t5.model.neftune_noise_alpha == 0.0  # only while train() runs
    t5.train()
    assert t5.model.neftune_noise_alpha == 0.0
    l0, l5 = _losses(t0), _losses(t5)
    assert len(l0) == len(l5) == 3 and all(a != b for a, b in zip(l0, l5))
    # one seed, two runs: bit-equal
    t5b = _trainer(tmp_path / "b5", neftune_noise_alpha=5)
    t5b.train()
    assert _losses(t5b) == l5 and torch.equal(t5b.engine.param_flat, t5.engine.param_flat)
    # checkpoint after step 2 + resume: step 3 bit for bit (the noise seed comes from the checkpointed CPU generator)
    t2 = _trainer(tmp_path / "c5", save_steps=2, neftune_noise_alpha=5)
    t2.args.max_steps = 2
    t2.train()
    t3 = _trainer(tmp_path / "c5", neftune_noise_alpha=5)
    torch.manual_seed(999)  # whatever the process drew before: the resume restores the generator
    t3.train(resume_from_checkpoint="auto")
    assert t3.state.global_step == 3 and _losses(t3)[-1] == l5[2]
    assert torch.equal(t3.engine.param_flat, t5.engine.param_flat)


def test_evaluate_never_sees_noise(tmp_path):
    t0 = _trainer(tmp_path / "e0")
    t5 = _trainer(tmp_path / "e5", neftune_noise_alpha=5)
    t5.model.neftune_noise_alpha = 5.0  # even when left on: evaluate() runs model.eval() under no_grad
    assert t0.evaluate()["eval_loss"] == t5.evaluate()["eval_loss"]


def test_noise_is_off_after_train_raises(tmp_path):
    t = _trainer(tmp_path / "r", neftune_noise_alpha=5)
    seen = {}

    def boom(resume=None):
        seen["alpha"], seen["rank"] = t.model.neftune_noise_alpha, t.model.neftune_rank
        raise RuntimeError("stop")

    t._train = boom
    with pytest.raises(RuntimeError):
        t.train()
    assert seen == {"alpha": 5.0, "rank": 0} and t.model.neftune_noise_alpha == 0.0


@pytest.mark.parametrize("kw", [{"label_smoothing_factor": 0.1}, {"loss_type": "dft"}])
def test_trainer_objective_is_logged_and_evaluated(tmp_path, kw):
    """The first logged loss is the formula on the first batch (initial weights), and eval_loss is the same objective
    over the eval set."""
    t = _trainer(tmp_path / "o", max_steps=1, **kw)
    probe = _tiny_model(3)  # the trainer's initial weights
    probe.eval()
    eps = kw.get("label_smoothing_factor", 0.0)

    def objective(batches):
        tot, cnt = 0.0, 0
        with torch.no_grad():
            for b in batches:
                inp = t._model_inputs(b)
                out = probe(**inp, return_logits=True)  # the plain per-token nll and lse, whatever the batch layout
                lg = out.logits.double().reshape(out.stats.shape[1], -1)
                nll, lse = out.stats[0].double(), out.stats[1].double()
                valid = nll != 0  # ignored tokens have loss exactly 0 (a random model's valid tokens never do)
                if eps:
                    per = (1 - eps) * nll + eps * (lse - lg.mean(-1))
                else:
                    per = torch.exp(-nll) * nll
                tot += (per * valid).sum().item()
                cnt += int(valid.sum())
        return tot / cnt

    want_train = objective([next(iter(t.get_train_dataloader()))])
    want_eval = objective(list(t.get_eval_dataloader()))
    ev = t.evaluate()["eval_loss"]
    assert abs(ev - want_eval) < 1e-5 * want_eval, (ev, want_eval)
    t.train()
    got = _losses(t)[0]
    assert abs(got - want_train) < 1e-5 * want_train, (got, want_train)
    plain = _trainer(tmp_path / "p", max_steps=1)
    assert abs(plain.evaluate()["eval_loss"] - ev) > 1e-4  # and not the plain cross-entropy
