"""Offline distillation on the CPU (the reference path): GKDConfig.teacher_topk, ref.teacher_topk / distill_topk and
its gradient, the teacher's top-k cache file of GKDTrainer, and the alignment of the cached rows with the tokens of
every batch form."""
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.data.collator import DistillTopKCollator
from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
from llm_fine_tune_distributed_amd.models import build_model, get_config, tiny
from llm_fine_tune_distributed_amd.ops import reference as ref
from llm_fine_tune_distributed_amd.train import GKDConfig, GKDTrainer

K, TAU, VOCAB = 16, 0.9, 1024


# ------------------------------------------------------------------------------------------------ config
def test_config_validation():
    with pytest.raises(ValueError, match="beta=0"):
        GKDConfig(teacher_topk=64)  # beta defaults to 0.5
    with pytest.raises(ValueError, match="beta=0"):
        GKDConfig(teacher_topk=64, beta=1.0)
    for k in (0, 257, -1, 1.5, True):
        with pytest.raises(ValueError, match="teacher_topk"):
            GKDConfig(teacher_topk=k, beta=0.0)
    for k in (1, 64, 256):
        assert GKDConfig(teacher_topk=k, beta=0.0).teacher_topk == k
    # a field set after construction is caught when the trainer is built
    c = GKDConfig(output_dir="unused")
    c.teacher_topk = 8
    with pytest.raises(ValueError, match="beta=0"):
        GKDTrainer(model="tiny", args=c, teacher_model="tiny-llama")


def test_config_default_leaves_every_existing_default_unchanged():
    import dataclasses
    c = GKDConfig()
    assert c.teacher_topk is None and c.beta == 0.5 and c.temperature == 0.9 and c.lmbda == 0.0 and c.seq_kd is False
    assert c.teacher_model_name_or_path is None
    from llm_fine_tune_distributed_amd.train import SFTConfig
    s = SFTConfig()
    own = {"beta", "temperature", "lmbda", "seq_kd", "teacher_model_name_or_path", "teacher_topk"}
    assert {f.name for f in dataclasses.fields(GKDConfig)} - {f.name for f in dataclasses.fields(SFTConfig)} == own
    for f in dataclasses.fields(SFTConfig):
        assert getattr(c, f.name) == getattr(s, f.name), f.name


# ------------------------------------------------------------------------------------------------ the definition
def _case(M=7, V=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = 3 * torch.randn(M, V, generator=g, dtype=torch.float64)
    t = 3 * torch.randn(M, V, generator=g, dtype=torch.float64)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[2] = -100
    labels[M - 1] = -100
    return s, t, labels


def test_ref_teacher_topk_tie_rule():
    x = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0, 2.0, 0.5],
                      [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0],
                      [0.0, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0, 9.0]])
    for dt in (torch.bfloat16, torch.float32, torch.float64):
        ids, lps = ref.teacher_topk(x.to(dt), 5, 2.0)
        assert ids.dtype == torch.int32 and ids.tolist() == [[1, 2, 5, 6, 0], [0, 1, 2, 3, 4], [7, 0, 1, 2, 3]]
        want = torch.log_softmax(x.double() / 2.0, -1).gather(1, ids.long())
        assert lps.dtype == (torch.float64 if dt == torch.float64 else torch.float32)
        assert torch.allclose(lps.double(), want, atol=1e-6)
    ids, _ = ref.teacher_topk(x, 8, 1.0)
    assert ids[0].tolist() == [1, 2, 5, 6, 0, 7, 3, 4]  # -0 and +0 are equal: by column
    for bad in (0, 9, 257):
        with pytest.raises(ValueError):
            ref.teacher_topk(x, bad, 1.0)
    with pytest.raises(ValueError):
        ref.teacher_topk(x, 2, 0.0)


@pytest.mark.parametrize("tau", [0.9, 1.0, 2.0])
def test_full_support_is_the_forward_kl_and_gradients_sum_to_zero(tau):
    s, t, labels = _case(V=256, seed=1)
    scale = torch.tensor([1.0 / 7.0], dtype=torch.float64)
    ids, lps = ref.teacher_topk(t, 256, tau)
    loss, lse, mass, correct, agree = ref.distill_topk(s, ids, lps, labels, tau)
    fkl = ref.generalized_jsd(s, t, labels, 0.0, tau)
    assert (loss - fkl[0]).abs().max().item() < 1e-13 and (lse - fkl[1]).abs().max().item() < 1e-13
    assert (mass - 1).abs().max().item() < 1e-13
    assert torch.equal(correct, fkl[3]) and torch.equal(agree, fkl[4])
    g = ref.distill_topk_grad(s, ids, lps, labels, scale, tau)
    assert (g - ref.generalized_jsd_grad(s, t, labels, scale, 0.0, tau)).abs().max().item() < 1e-15
    for k in (1, 7, 64):
        ids, lps = ref.teacher_topk(t, k, tau)
        x = s.clone().requires_grad_(True)
        (ref.distill_topk(x, ids, lps, labels, tau)[0].sum() * scale).sum().backward()
        g = ref.distill_topk_grad(s, ids, lps, labels, scale, tau)
        assert (g - x.grad).abs().max().item() < 1e-15
        assert g.sum(-1).abs().max().item() < 1e-15       # the gradient sums to zero for every k
        assert not g[2].any() and not g[-1].any()          # label -100
        m = ref.distill_topk(s, ids, lps, labels, tau)[2]
        assert bool((m > 0).all()) and bool((m < 1).all())


def test_op_on_the_reference_path_and_its_refusals():
    s, t, labels = _case(V=64, seed=2)
    W = torch.eye(64, dtype=torch.float64)  # an LM head that hands h through: logits = h
    ids, lps = ref.teacher_topk(t, 7, TAU)
    inv = torch.tensor([1.0 / 5.0], dtype=torch.float64)
    h = s.clone().requires_grad_(True)
    loss, stats = ops.lm_head_distill_topk_loss(h, W, ids, lps.float(), labels, inv, TAU)
    loss.backward()
    want = ref.distill_topk_grad(s, ids, lps.float(), labels, inv, TAU)
    assert stats.shape == (5, 7) and (h.grad - want).abs().max().item() < 1e-12
    assert abs(loss.item() - ref.distill_topk(s, ids, lps.float(), labels, TAU)[0].sum().item() / 5.0) < 1e-6
    tid, tlp = ops.lm_head_topk_logps(t, W, 7, TAU)
    assert torch.equal(tid, ids) and tlp.dtype == torch.float32 and not tlp.requires_grad
    for bad in (lambda: ops.lm_head_distill_topk_loss(h, W, ids.long(), lps.float(), labels, inv, TAU),
                lambda: ops.lm_head_distill_topk_loss(h, W, ids, lps, labels, inv, TAU),          # fp64 logps
                lambda: ops.lm_head_distill_topk_loss(h, W, ids[:5], lps[:5].float(), labels, inv, TAU),
                lambda: ops.lm_head_distill_topk_loss(h, W, ids, lps[:, :6].float(), labels, inv, TAU),
                lambda: ops.lm_head_distill_topk_loss(h, W, ids, lps.float(), labels, inv, 0.0)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ trainer
def _student(seed=0):
    return build_model(tiny(vocab_size=VOCAB), dtype=torch.float32, seed=seed)


def _f64(m):
    """The model's weights (bf16 values once a trainer has loaded it as a teacher) computed with in fp64: a bf16 or
    fp32 forward on the CPU moves in its last bits with the shape of the batch a row sits in, which reorders near-ties
    of a random teacher; in fp64 the caching pass and a training batch give the same top-k of a row, so the tests below
    can ask for equality."""
    for p in m.parameters():
        p.data = p.data.double()
    return m


def _teacher(seed=5):
    m = build_model(get_config("tiny-llama"), dtype=torch.bfloat16, seed=seed)
    return _f64(m.eval().requires_grad_(False))


def _data(n=12, seed=3, lo=9, hi=40, loss_start=False):
    ds = TokenizedDataset.synthetic(n, VOCAB, lo, hi, seed=seed)
    if loss_start:  # assistant_only_loss: the loss starts inside every sample
        ds.loss_start = (ds.lengths() // 3).to(torch.int32)
    return ds


def _args(out, **kw):
    base = dict(output_dir=str(out), per_device_train_batch_size=4, per_device_eval_batch_size=3, learning_rate=2e-3,
                max_steps=3, logging_steps=1, lr_scheduler_type="constant", save_strategy="no", jsonl_log=False,
                seed=1, beta=0.0, temperature=TAU, teacher_topk=K, dataloader_pin_memory=False)
    base.update(kw)
    return GKDConfig(**base)


def _trainer(out, teacher=None, train=None, evalset=None, **kw):
    t = GKDTrainer(model=_student(), args=_args(out, **kw), train_dataset=train if train is not None else _data(),
                   eval_dataset=evalset, teacher_model=teacher)
    if t.teacher is not None:
        _f64(t.teacher)  # (the trainer made it bf16)
    return t


def test_cache_round_trip_and_refusals(tmp_path):
    out = tmp_path / "run"
    with pytest.raises(ValueError, match="needs a teacher"):  # no file, no teacher: the existing error
        _trainer(out)
    train, ev = _data(), _data(5, seed=9)
    t = _trainer(out, _teacher(), train, ev)
    path = t.teacher_topk_path()
    assert os.path.basename(path).startswith("teacher_topk-") and not os.path.exists(path)
    t.precompute_teacher_topk()
    assert t.teacher is None and os.path.exists(path) and not [f for f in os.listdir(out) if ".tmp" in f]
    d = torch.load(path, weights_only=True)
    n_train, n_eval = int(train.offsets[-1]), int(ev.offsets[-1])
    assert d["meta"] == {"k": K, "temperature": TAU, "vocab_size": VOCAB}
    assert d["train_ids"].shape == (n_train, K) and d["train_ids"].dtype == torch.int32
    assert d["train_logps"].shape == (n_train, K) and d["train_logps"].dtype == torch.float32
    assert d["eval_ids"].shape == (n_eval, K) and d["eval_logps"].shape == (n_eval, K)
    assert torch.equal(t.collator.teacher_ids, d["train_ids"]) and torch.equal(t.eval_collator.teacher_logps,
                                                                               d["eval_logps"])
    # every row is a descending, distinct top-k of a distribution
    assert bool((d["train_logps"][:, :-1] >= d["train_logps"][:, 1:]).all()) and bool((d["train_logps"] < 0).all())
    assert all(len(set(r)) == K for r in d["train_ids"][:50].tolist())
    # the row of sample i at position j is offsets[i] + j: the teacher on sample 3 alone
    te = _teacher()
    ids3 = torch.tensor(train[3])
    want = ref.teacher_topk(te.logits_rows(ids3[None]), K, TAU)
    o = int(train.offsets[3])
    assert torch.equal(d["train_ids"][o:o + len(ids3)], want[0])
    assert torch.equal(d["train_logps"][o:o + len(ids3)], want[1].float())
    # a second trainer without a teacher: the file stands in for it, and gives the same steps
    t.train()
    t2 = _trainer(out, None, train, ev)
    assert t2.teacher is None
    t2.train()
    la, lb = ([h["loss"] for h in x.state.log_history if "loss" in h] for x in (t, t2))
    assert len(la) == 3 and la == lb and torch.equal(t.engine.param_flat, t2.engine.param_flat)
    assert all("teacher_mass" in h and 0 < h["teacher_mass"] < 1 for h in t.state.log_history if "loss" in h)
    ev_m = t2.evaluate()
    assert ev_m["eval_loss"] > 0 and 0 < ev_m["eval_teacher_mass"] < 1
    # the fingerprint covers the data, k, the temperature: any change is another file, and without a teacher an error
    for kw in (dict(teacher_topk=8), dict(temperature=1.0)):
        with pytest.raises(ValueError, match="needs a teacher"):
            _trainer(out, None, train, ev, **kw)
    with pytest.raises(ValueError, match="needs a teacher"):
        _trainer(out, None, _data(seed=4), ev)
    with pytest.raises(ValueError, match="needs a teacher"):
        _trainer(out, None, train, None)
    # a file put under another run's name is refused by what it records
    other = _trainer(tmp_path / "other", _teacher(), train, ev, teacher_topk=8)
    os.makedirs(tmp_path / "other", exist_ok=True)
    import shutil
    shutil.copy(path, other.teacher_topk_path())
    with pytest.raises(ValueError, match="was written for"):
        other.train()
    # a resume needs the file
    fresh = _trainer(tmp_path / "fresh", _teacher(), train, ev)
    with pytest.raises(FileNotFoundError, match="top-k cache"):
        fresh.train(resume_from_checkpoint=str(tmp_path / "nowhere" / "checkpoint-2"))
    # a caller's collator cannot carry the cache
    from llm_fine_tune_distributed_amd.data.collator import SFTCollator
    with pytest.raises(ValueError, match="DistillTopKCollator"):
        GKDTrainer(model=_student(), args=_args(out), train_dataset=train, teacher_model=_teacher(),
                   data_collator=SFTCollator(0))


FORMS = {"padded": dict(padding_free=False), "packing": dict(packing=True, max_length=48),
         "padding_free": dict(padding_free=True), "max_length": dict(padding_free=False, max_length=20),
         "max_length padding_free": dict(padding_free=True, max_length=20),
         "ga2 merged": dict(padding_free=False, gradient_accumulation_steps=2, ga_merge_max_tokens=1 << 16),
         "ga2 merged padding_free": dict(padding_free=True, gradient_accumulation_steps=2, ga_merge_max_tokens=1 << 16),
         "ga2 unmerged": dict(padding_free=False, gradient_accumulation_steps=2, ga_merge_max_tokens=0)}


def _online_loss(trainer, teacher, b):
    """The loss of batch b with the teacher run on that batch: ref.teacher_topk of its logits in place of the cache."""
    kw = trainer._model_inputs(b)
    labels = kw.pop("labels")
    shift = kw.pop("shift_labels", True)
    with torch.no_grad():
        t_logits = teacher.logits_rows(**kw)
    ids, lps = ref.teacher_topk(t_logits, K, TAU)
    out = trainer.model.distill_topk_loss(labels=labels, teacher_ids=ids, teacher_logps=lps.float(),
                                          shift_labels=shift, num_items_in_batch=float(b["num_items"]),
                                          temperature=TAU, **kw)
    return out, ids


@pytest.mark.parametrize("loss_start", [False, True])
@pytest.mark.parametrize("form", list(FORMS))
def test_cached_rows_follow_the_tokens_of_every_batch_form(form, loss_start, tmp_path):
    """For every batch form, the loss through the cache equals, exactly, the loss with the teacher run on that batch:
    a cache row attached to the wrong token cannot do that. Train and eval set alike. (A pad row's cached values are id
    0 / log-probability 0 and its label -100; only rows with a label are compared.)"""
    train, ev = _data(16, loss_start=loss_start), _data(7, seed=11, loss_start=loss_start)
    teacher = _teacher()
    kw = FORMS[form]
    t = _trainer(tmp_path / "run", teacher, train, ev, **kw)
    t.precompute_teacher_topk()
    assert t.teacher is None
    t.model.eval()
    ga = int(kw.get("gradient_accumulation_steps", 1))
    seen = 0
    for name, loader in (("train", t.get_train_dataloader()), ("eval", t.get_eval_dataloader())):
        assert isinstance(loader.collator, DistillTopKCollator)
        batches = list(loader)
        groups = [batches[i:i + ga] for i in range(0, len(batches), ga)] if name == "train" else [[b] for b in batches]
        for micro in groups:
            merged = t._merge_micro(list(micro)) if name == "train" else micro
            if form.startswith("ga2 merged") and name == "train" and len(micro) == 2:
                assert len(merged) == 1 and merged[0]["num_items"] == sum(b["num_items"] for b in micro)
            elif name == "train":
                assert len(merged) == len(micro)
            for b in merged:
                packed = "cu_seqlens" in b
                k_shape = tuple(b["input_ids"].shape) + (K,)
                assert tuple(b["teacher_ids"].shape) == k_shape and b["teacher_ids"].dtype == torch.int32
                assert tuple(b["teacher_logps"].shape) == k_shape and b["teacher_logps"].dtype == torch.float32
                assert packed == ("padding_free" in form or form == "packing")
                n = float(b["num_items"])
                with torch.no_grad():
                    loss, _ = t._distill(b, n)
                    want, ids = _online_loss(t, teacher, b)
                assert loss.item() == want.loss.item() and loss.item() > 0, (name, loss.item(), want.loss.item())
                valid = (want.stats[0] != 0)
                assert torch.equal(b["teacher_ids"].reshape(-1, K)[valid], ids[valid])
                seen += int(valid.sum())
    assert seen > 100


def test_packing_that_stops_early_at_max_tokens(tmp_path):
    """packing=True with a token budget two samples overflow: the pack holds fewer samples than the batch asked for,
    and the cached rows are those of the samples it holds."""
    train = _data(8, lo=30, hi=40)
    t = _trainer(tmp_path / "run", _teacher(), train, None, packing=True, max_length=25, per_device_train_batch_size=4)
    t.precompute_teacher_topk()
    b = next(iter(t.get_train_dataloader()))
    assert b["num_samples"] < 4
    teacher = _teacher()
    with torch.no_grad():
        loss, _ = t._distill(b, float(b["num_items"]))
        want, _ = _online_loss(t, teacher, b)
    assert loss.item() == want.loss.item() > 0


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
    t = _trainer(os.path.join(out_dir, f"w{world}"), _teacher(), _data(11), _data(5, seed=9),
                 per_device_train_batch_size=2, per_device_eval_batch_size=1)
    t.precompute_teacher_topk()
    assert t.teacher is None and t.collator.teacher_ids is not None
    pgm.cleanup_distributed()


def test_two_ranks_write_the_file_one_rank_writes():
    d = tempfile.mkdtemp()
    _rank(0, 1, _free_port(), d)
    mp.spawn(_rank, args=(2, _free_port(), d), nprocs=2, join=True)
    files = {w: [f for f in os.listdir(os.path.join(d, f"w{w}")) if f.startswith("teacher_topk-")] for w in (1, 2)}
    assert len(files[1]) == 1 and files[1] == files[2]  # one file each, one fingerprint
    a, b = (torch.load(os.path.join(d, f"w{w}", files[w][0]), weights_only=True) for w in (1, 2))
    assert a["meta"] == b["meta"] and set(a) == set(b)
    for k in ("train_ids", "train_logps", "eval_ids", "eval_logps"):
        assert torch.equal(a[k], b[k]), k
