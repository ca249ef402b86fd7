"""Qwen3 family on the CPU (fp32 / fp64 reference path): parity with transformers' Qwen3ForCausalLM through a saved
directory, the save round trip, the gradients of the per-head QK RMSNorm + RoPE node, rejected configs, generation,
trainer / LoRA plumbing and a world-2 DDP step."""
import json
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import test_distributed_cpu as dist_harness
from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.data.synthetic import generate_qa
from llm_fine_tune_distributed_amd.data.tokenizer import load_tokenizer
from llm_fine_tune_distributed_amd.inference.generation import generate, generate_batch
from llm_fine_tune_distributed_amd.models import ModelConfig, apply_freeze_policy, build_model, get_config
from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora
from llm_fine_tune_distributed_amd.ops import reference as ref
from llm_fine_tune_distributed_amd.train import SFTConfig, SFTTrainer
from llm_fine_tune_distributed_amd.train import checkpoint as ckpt

VOCAB = 512


def _randomise_qk_norms(named_params, seed=11):
    """q_norm / k_norm weights random around 1: with ones the norm's weight path would go unchecked."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in named_params:
            if "q_norm" in n or "k_norm" in n:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))


@pytest.fixture(scope="module")
def hf_dir():
    """A tiny fp32 Qwen3ForCausalLM saved by transformers, and the model itself."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    torch.manual_seed(0)
    hc = Qwen3Config(vocab_size=VOCAB, hidden_size=96, intermediate_size=160, num_hidden_layers=3,
                     num_attention_heads=4, num_key_value_heads=2, head_dim=32, max_position_embeddings=256,
                     tie_word_embeddings=False)
    hm = Qwen3ForCausalLM(hc).float()
    _randomise_qk_norms(hm.named_parameters())
    d = tempfile.mkdtemp()
    hm.save_pretrained(d)
    return d, hm


def _load_ours(d):
    cfg = get_config(d)
    m = build_model(cfg, dtype=torch.float32)
    m.load_hf_state_dict(ckpt.load_state_dict(d))  # strict: no unexpected keys
    return m


def _tiny_qwen3(seed=2):
    m = build_model(get_config("tiny-qwen3"), dtype=torch.float32, seed=seed)
    _randomise_qk_norms(m.named_parameters())
    return m


# ------------------------------------------------------------------------------------------------ HF parity
def test_hf_parity_padded_and_packed(hf_dir):
    d, hm = hf_dir
    hm.eval()
    m = _load_ours(d)
    assert m.config.model_type == "qwen3" and m.config.qk_norm
    torch.manual_seed(1)
    a = torch.randint(0, VOCAB, (24,))
    b = torch.randint(0, VOCAB, (17,))
    ids = torch.zeros(2, 24, dtype=torch.long)
    ids[0], ids[1, :17] = a, b
    labels = ids.clone()
    labels[1, 17:] = -100
    with torch.no_grad():
        ho = hm(input_ids=ids, labels=labels)
        mo = m(ids, labels=labels, return_logits=True)
        pk = m(torch.cat([a, b]), cu_seqlens=torch.tensor([0, 24, 41], dtype=torch.int32), max_seqlen=24,
               return_logits=True)
    # (the tolerances of test_model_cpu.test_parity_with_transformers)
    assert abs(ho.loss.item() - mo.loss.item()) < 1e-5
    assert (ho.logits.reshape(-1, VOCAB) - mo.logits).abs().max() < 1e-4
    valid = torch.cat([ho.logits[0], ho.logits[1, :17]])
    assert (valid - pk.logits).abs().max() < 1e-4


def test_save_round_trip_loads_in_transformers(hf_dir, tmp_path):
    from transformers import Qwen3ForCausalLM
    d, hm = hf_dir
    hm.eval()
    m = _load_ours(d)
    out = str(tmp_path / "out")
    ckpt.save_pretrained(m, out)
    with open(os.path.join(out, "config.json")) as f:
        cj = json.load(f)
    assert cj["architectures"] == ["Qwen3ForCausalLM"] and cj["model_type"] == "qwen3"
    assert "no_rope_layers" not in cj and "no_rope_layer_interval" not in cj
    hm2, info = Qwen3ForCausalLM.from_pretrained(out, torch_dtype=torch.float32, output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"]
    ids = torch.randint(0, VOCAB, (2, 16))
    with torch.no_grad():
        assert (hm2.eval()(input_ids=ids).logits - hm(input_ids=ids).logits).abs().max() < 1e-4
        assert (hm2(input_ids=ids).logits.reshape(-1, VOCAB) - m(ids, return_logits=True).logits).abs().max() < 1e-4


def test_presets_and_param_counts():
    from llm_fine_tune_distributed_amd.models import qwen3_4b, qwen3_8b
    c4, c8 = qwen3_4b(), qwen3_8b()
    assert (c4.hidden_size, c4.intermediate_size, c4.num_hidden_layers, c4.tie_word_embeddings) == (2560, 9728, 36, True)
    assert (c8.hidden_size, c8.intermediate_size, c8.num_hidden_layers, c8.tie_word_embeddings) == (4096, 12288, 36, False)
    for c in (c4, c8):
        assert (c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.vocab_size) == (32, 8, 128, 151936)
        assert c.rope_theta == 1e6 and c.rms_norm_eps == 1e-6 and c.qk_norm and all(c.no_rope_layers)
    assert get_config("Qwen/Qwen3-4B") == c4 and get_config("qwen3-8b") == c8
    assert get_config("tiny-gpu-qwen3").head_dim == 128
    m = build_model(get_config("tiny-qwen3"), dtype=torch.float32)
    assert m.num_parameters() == m.config.num_parameters()  # the two norms count
    at = m.model.layers[0].self_attn
    assert torch.equal(at.q_norm.weight, torch.ones(32)) and torch.equal(at.k_norm.weight, torch.ones(32))
    # other families: no new parameters, other unknown model types still become llama
    assert not hasattr(build_model(get_config("tiny-llama"), dtype=torch.float32).model.layers[0].self_attn, "q_norm")
    assert ModelConfig.from_hf_dict({"model_type": "mistral", "hidden_size": 64, "num_attention_heads": 4,
                                     "num_hidden_layers": 1}).model_type == "llama"


@pytest.mark.parametrize("key,val", [("attention_bias", True), ("use_sliding_window", True),
                                     ("layer_types", ["full_attention", "sliding_attention"])])
def test_unsupported_qwen3_configs_raise(key, val):
    d = get_config("tiny-qwen3").to_hf_dict()
    if key == "layer_types":
        d["num_hidden_layers"] = 2
    ModelConfig.from_hf_dict(d)  # the plain config loads
    d[key] = val
    with pytest.raises(NotImplementedError, match=key):
        ModelConfig.from_hf_dict(d)


# ------------------------------------------------------------------------------------------------ gradients
def test_qk_norm_rope_reference_gradients_fp64():
    """QKNormRopeFn (reference path, closed-form backward) against autograd through an independent composition."""
    torch.manual_seed(0)
    M, nq, nkv, D, eps = 13, 4, 2, 32, 1e-6
    nh = nq + nkv
    qkv = torch.randn(M, (nq + 2 * nkv) * D, dtype=torch.float64)
    qw = 1 + 0.3 * torch.randn(D, dtype=torch.float64)
    kw = 1 + 0.3 * torch.randn(D, dtype=torch.float64)
    pos = torch.randint(0, 4000, (M,))
    fr = pos.double()[:, None] * ref.rope_inv_freq(D, 1e6, None).double()[None]
    cos, sin = fr.cos(), fr.sin()
    G = torch.randn_like(qkv)

    def grads(fn):
        x, a, b = (t.clone().requires_grad_(True) for t in (qkv, qw, kw))
        y = fn(x, a, b)
        return (y,) + torch.autograd.grad((y * G).sum(), (x, a, b))

    def independent(x, a, b):
        heads = x[:, : nh * D].view(M, nh, D)
        w = torch.cat([a.expand(nq, D), b.expand(nkv, D)], 0)
        n = F.rms_norm(heads, (D,), eps=eps) * w
        return torch.cat([ref.apply_rope(n, cos, sin).reshape(M, nh * D), x[:, nh * D:]], -1)

    got = grads(lambda x, a, b: ops.qk_norm_rope_(x.clone(), a, b, cos, sin, nq, nkv, D, eps))
    want = grads(independent)
    for g, w, name in zip(got, want, ("y", "dqkv", "dq_weight", "dk_weight")):
        assert torch.allclose(g, w, atol=1e-10, rtol=0), (name, (g - w).abs().max().item())
    # the differentiable reference itself, and the no-grad form (in place, no autograd node)
    assert torch.allclose(ref.qk_norm_rope(qkv, qw, kw, cos, sin, nq, nkv, D, eps), want[0], atol=1e-12, rtol=0)
    with torch.no_grad():
        x = qkv.clone()
        assert ops.qk_norm_rope_(x, qw, kw, cos, sin, nq, nkv, D, eps) is x
    assert torch.allclose(x, want[0], atol=1e-12, rtol=0)


def test_model_gradients_match_hf(hf_dir):
    """main_grad path of q_norm, k_norm and qkv_proj == plain autograd of the HF model (the bounds of
    test_model_cpu.test_gradients_match_autograd_reference)."""
    d, hm = hf_dir
    m = _load_ours(d)
    for p in m.parameters():
        p.main_grad = torch.zeros_like(p)
    torch.manual_seed(3)
    ids = torch.randint(0, VOCAB, (2, 20))
    m.reset_grad_use_counters()
    m(ids, labels=ids).loss.backward()
    hm.zero_grad()
    hm(input_ids=ids, labels=ids).loss.backward()
    hsd = dict(hm.named_parameters())
    for i in (0, 2):
        at = m.model.layers[i].self_attn
        pre = f"model.layers.{i}.self_attn."
        qkv_ref = torch.cat([hsd[pre + f"{n}_proj.weight"].grad for n in "qkv"], 0)
        assert torch.allclose(at.qkv_proj.main_grad, qkv_ref, atol=1e-5, rtol=1e-3)
        assert hsd[pre + "q_norm.weight"].grad.abs().max() > 1e-4  # (not a comparison of zeros)
        assert torch.allclose(at.q_norm.weight.main_grad, hsd[pre + "q_norm.weight"].grad, atol=1e-5, rtol=1e-3)
        assert torch.allclose(at.k_norm.weight.main_grad, hsd[pre + "k_norm.weight"].grad, atol=1e-5, rtol=1e-3)
    assert torch.allclose(m.model.norm.weight.main_grad, hsd["model.norm.weight"].grad, atol=1e-5, rtol=1e-3)
    hm.zero_grad()


# ------------------------------------------------------------------------------------------------ generation
def test_greedy_cache_matches_full_forward():
    torch.manual_seed(0)
    m = _tiny_qwen3()
    prompt = torch.randint(0, 512, (9,)).tolist()
    out = generate(m, prompt, max_new_tokens=6, do_sample=False, repetition_penalty=1.0)
    seq = list(prompt)
    for _ in range(6):
        with torch.no_grad():
            lg = m(torch.tensor(seq)[None], return_logits=True).logits
        seq.append(int(lg[-1].argmax()))
    assert out == seq[len(prompt):]


def test_generate_batch_rows_equal_generate():
    torch.manual_seed(0)
    m = _tiny_qwen3()
    prompts = [torch.randint(0, 512, (n,)).tolist() for n in (5, 11, 8)]
    kw = dict(max_new_tokens=8, temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.1, do_sample=True)
    got = generate_batch(m, prompts, seed=7, **kw)
    for b, p in enumerate(prompts):
        assert got[b] == generate(m, p, seed=7 + b, **kw), b
    greedy = generate_batch(m, prompts, max_new_tokens=8, do_sample=False, repetition_penalty=1.0)
    for b, p in enumerate(prompts):
        assert greedy[b] == generate(m, p, max_new_tokens=8, do_sample=False, repetition_penalty=1.0), b


# ------------------------------------------------------------------------------------------------ trainer / LoRA
@pytest.fixture(scope="module")
def tk():
    return load_tokenizer()


def _norms(m):
    return torch.cat([torch.cat([l.self_attn.q_norm.weight.detach(), l.self_attn.k_norm.weight.detach()])
                      for l in m.model.layers])


def test_trainer_lowers_loss_and_resume_restores_norms(tmp_path, tk):
    rows = generate_qa(8, seed=0)

    def mk(seed):
        a = SFTConfig(output_dir=str(tmp_path / "run"), per_device_train_batch_size=8, learning_rate=3e-3, max_steps=3,
                      logging_steps=1, save_steps=3, dataloader_drop_last=True, jsonl_log=False)
        return SFTTrainer(model=build_model(get_config("tiny-qwen3"), dtype=torch.float32, seed=seed), args=a,
                          train_dataset=rows, processing_class=tk)

    t1 = mk(1)
    t1.train()
    losses = [h["loss"] for h in t1.state.log_history if "loss" in h]
    assert len(losses) == 3 and losses[-1] < losses[0], losses
    trained = _norms(t1.model)
    assert (trained - 1).abs().max() > 1e-4  # the norms trained (they sit in the optimizer)
    t2 = mk(9)  # other weights; the checkpoint at step 3 puts the trained ones back, no step runs
    assert torch.equal(_norms(t2.model), torch.ones_like(trained))
    out = t2.train(resume_from_checkpoint="auto")
    assert out.global_step == 3
    assert torch.equal(_norms(t2.model), trained)


def test_qk_norms_have_no_weight_decay():
    from llm_fine_tune_distributed_amd.parallel.ddp import _no_decay
    m = build_model(get_config("tiny-qwen3"), dtype=torch.float32)
    qk = [(n, p) for n, p in m.named_parameters() if "q_norm" in n or "k_norm" in n]
    assert len(qk) == 2 * m.config.num_hidden_layers and all(_no_decay(n, p) for n, p in qk)


def test_freeze_policies_cover_the_norms():
    m = build_model(get_config("tiny-qwen3"), dtype=torch.float32)
    apply_freeze_policy(m, "last_n_layers", n_last=1)
    flags = [l.self_attn.q_norm.weight.requires_grad and l.self_attn.k_norm.weight.requires_grad
             for l in m.model.layers]
    assert flags == [False] * (len(flags) - 1) + [True]
    apply_freeze_policy(m, "lora", lora_config=LoRAConfig(r=4))
    assert not any(p.requires_grad for n, p in m.named_parameters() if "q_norm" in n or "k_norm" in n)
    ids = torch.randint(0, m.config.vocab_size, (2, 12))
    m(ids, labels=ids).loss.backward()  # the LoRA route of a qk-norm layer trains the adapters only
    at = m.model.layers[0].self_attn
    assert at.q_norm.weight.grad is None and at.lora["qkv"].B[0].grad is not None


def test_merged_lora_export_matches_live_model(tmp_path):
    from transformers import AutoModelForCausalLM
    torch.manual_seed(0)
    m = _tiny_qwen3(seed=5)
    apply_lora(m, LoRAConfig(r=4, lora_alpha=8, lora_dropout=0.0,
                             target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "up_proj", "down_proj"]))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".lora." in n and p.numel() > 0:
                p.normal_(0.0, 0.05)
    m.eval()
    ids = torch.randint(0, m.config.vocab_size, (2, 16))
    with torch.no_grad():
        mo = m(ids, return_logits=True).logits
    ckpt.save_pretrained(m, str(tmp_path / "merged"), merge_lora=True)
    hm = AutoModelForCausalLM.from_pretrained(str(tmp_path / "merged"), torch_dtype=torch.float32).eval()
    assert type(hm).__name__ == "Qwen3ForCausalLM"
    with torch.no_grad():
        ho = hm(input_ids=ids).logits
    assert (ho.reshape(mo.shape) - mo).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------ distributed
def _run_qwen3(rank, world, port, out_dir, per_dev, ga, steps):
    """test_distributed_cpu._run with its model swapped for tiny-qwen3 (the harness builds `tiny()`)."""
    _as_qwen3(dist_harness._run, rank, world, port, out_dir, per_dev, ga, steps)


def _as_qwen3(fn, *args):
    """Run a worker of another test module that builds `tiny(...)` with the model type swapped for qwen3."""
    import llm_fine_tune_distributed_amd.models as models
    orig = models.tiny
    models.tiny = lambda *a, **k: orig("qwen3", **k)
    try:
        fn(*args)
    finally:
        models.tiny = orig


def _cp_worker_qwen3(rank, world, port, out_dir, layout):
    import test_context_parallel_cpu as cp_harness
    _as_qwen3(cp_harness._model_worker, rank, world, port, out_dir, layout)


def test_context_parallel_matches_single_process():
    """The qk-norm route into ring_attention (world 2, zig-zag): loss and every gradient, the norms included, equal
    one process on the whole batch (test_context_parallel_cpu's worker and bounds)."""
    import torch.multiprocessing as mp
    from llm_fine_tune_distributed_amd.models import tiny
    d = tempfile.mkdtemp()
    mp.spawn(_cp_worker_qwen3, args=(2, dist_harness._free_port(), d, "zigzag"), nprocs=2, join=True)
    torch.manual_seed(0)
    cfg = tiny("qwen3", num_hidden_layers=4)
    ids = torch.randint(0, cfg.vocab_size, (2, 21))
    labels = ids.clone()
    labels[1, 15:] = -100
    m = build_model(cfg, dtype=torch.float32, seed=7)
    n = float((labels[:, 1:] != -100).sum())
    m.reset_grad_use_counters()
    out = m(ids, labels=labels, num_items_in_batch=torch.tensor([n]))
    out.loss.backward()
    r0 = torch.load(os.path.join(d, "m0.pt"))
    assert abs(r0["loss"] - out.loss.item()) < 1e-5
    assert any("q_norm" in k for k in r0["grads"])
    for name, p in m.named_parameters():
        e = (r0["grads"][name] - p.grad).abs().max().item()
        assert e < 1e-5 * max(1.0, p.grad.abs().max().item()), (name, e)


def test_ddp2_one_step_matches_single_process():
    import torch.multiprocessing as mp
    d = tempfile.mkdtemp()
    _run_qwen3(0, 1, dist_harness._free_port(), d, 4, 1, 1)
    mp.spawn(_run_qwen3, args=(2, dist_harness._free_port(), d, 2, 1, 1), nprocs=2, join=True)
    single = torch.load(os.path.join(d, "r1_0.pt"))
    r0 = torch.load(os.path.join(d, "r2_0.pt"))
    r1 = torch.load(os.path.join(d, "r2_1.pt"))
    n = build_model(get_config("tiny-qwen3"), dtype=torch.float32).num_parameters()
    assert single["params"].numel() == n  # the qwen3 model ran: the norms are in the flat parameters
    assert torch.equal(r0["params"], r1["params"])
    assert torch.allclose(r0["params"], single["params"], atol=1e-5, rtol=1e-4)
    assert abs(single["log"][0]["loss"] - r0["log"][0]["loss"]) < 1e-4
    assert abs(single["log"][0]["grad_norm"] - r0["log"][0]["grad_norm"]) < 1e-3
