"""Qwen2 / Qwen2.5 family on the CPU (fp32 / fp64 reference path): parity with transformers' Qwen2ForCausalLM through a
saved directory, the save round trip, the gradients of the qkv bias + RoPE node, rejected configs, generation, trainer /
LoRA / gradient-checkpointing plumbing, context parallelism and a world-2 DDP step. The biases are random everywhere
(HF initialises them to zero, which would leave the path unchecked)."""
import json
import os
import tempfile

import pytest
import torch

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


def _is_bias(name):
    return name.endswith("qkv_bias") or name.endswith("_proj.bias")


def _randomise_biases(named_params, seed=11):
    """q / k / v biases N(0, 0.5): with HF's zeros the bias path would go unchecked."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in named_params:
            if _is_bias(n):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))


@pytest.fixture(scope="module")
def hf_dir():
    """A tiny fp32 Qwen2ForCausalLM saved by transformers, and the model itself."""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(0)
    hc = Qwen2Config(vocab_size=VOCAB, hidden_size=96, intermediate_size=160, num_hidden_layers=3,
                     num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256,
                     tie_word_embeddings=False)
    hm = Qwen2ForCausalLM(hc).float()
    _randomise_biases(hm.named_parameters())
    d = tempfile.mkdtemp()
    hm.save_pretrained(d)
    return d, hm


def _load_ours(d):
    cfg = get_config(d)
    m = build_model(cfg, dtype=torch.float32)
    m.load_hf_state_dict(ckpt.load_state_dict(d))  # strict: no unexpected keys
    return m


def _tiny_qwen2(seed=2):
    m = build_model(get_config("tiny-qwen2"), dtype=torch.float32, seed=seed)
    _randomise_biases(m.named_parameters())
    return m


# ------------------------------------------------------------------------------------------------ HF parity
def test_hf_saved_directory_loads(hf_dir):
    """get_config + load_hf_state_dict(strict) on a directory transformers saved: the config is a qwen2 one (its
    rope_parameters and inert sliding-window keys read), every bias lands, the strict checks hold both ways."""
    d, hm = hf_dir
    cfg = get_config(d)
    assert cfg.model_type == "qwen2" and cfg.qkv_bias and not cfg.qk_norm
    assert cfg.head_dim == 24 and cfg.rope_theta == 10000.0 and "max_window_layers" in cfg.extra
    m = _load_ours(d)
    hsd = hm.state_dict()
    for i, l in enumerate(m.model.layers):
        want = torch.cat([hsd[f"model.layers.{i}.self_attn.{n}_proj.bias"] for n in "qkv"])
        assert want.abs().max() > 0.1 and torch.equal(l.self_attn.qkv_bias, want)
    sd = ckpt.load_state_dict(d)
    no_bias = {k: v for k, v in sd.items() if not k.endswith("k_proj.bias")}
    with pytest.raises(KeyError, match="k_proj.bias"):
        build_model(cfg, dtype=torch.float32).load_hf_state_dict(no_bias)
    llama = ModelConfig.from_hf_dict({**cfg.to_hf_dict(), "model_type": "llama"})
    assert not llama.qkv_bias
    with pytest.raises(KeyError, match="unexpected keys.*proj.bias"):
        build_model(llama, dtype=torch.float32).load_hf_state_dict(sd)


def test_hf_parity_padded_and_packed(hf_dir):
    d, hm = hf_dir
    hm.eval()
    m = _load_ours(d)
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
    # (the tolerances of test_qwen3_cpu.test_hf_parity_padded_and_packed)
    assert abs(ho.loss.item() - mo.loss.item()) < 1e-5
    assert (ho.logits.reshape(-1, VOCAB) - mo.logits).abs().max() < 1e-4
    valid = torch.cat([ho.logits[0], ho.logits[1, :17]])
    assert (valid - pk.logits).abs().max() < 1e-4


def test_save_round_trip_loads_in_transformers(hf_dir, tmp_path):
    from transformers import Qwen2ForCausalLM
    d, hm = hf_dir
    hm.eval()
    m = _load_ours(d)
    out = str(tmp_path / "out")
    ckpt.save_pretrained(m, out)
    with open(os.path.join(out, "config.json")) as f:
        cj = json.load(f)
    assert cj["architectures"] == ["Qwen2ForCausalLM"] and cj["model_type"] == "qwen2"
    assert cj["use_sliding_window"] is False and "max_window_layers" in cj
    for k in ("no_rope_layers", "no_rope_layer_interval", "mlp_bias", "attention_bias"):
        assert k not in cj, k
    hm2, info = Qwen2ForCausalLM.from_pretrained(out, torch_dtype=torch.float32, output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"]
    ids = torch.randint(0, VOCAB, (2, 16))
    with torch.no_grad():
        assert (hm2.eval()(input_ids=ids).logits - hm(input_ids=ids).logits).abs().max() < 1e-4
        assert (hm2(input_ids=ids).logits.reshape(-1, VOCAB) - m(ids, return_logits=True).logits).abs().max() < 1e-4
    m2 = _load_ours(out)  # and our own directory reads back
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))


def test_presets_and_param_counts():
    from llm_fine_tune_distributed_amd.models import qwen2_5_1_5b, qwen2_5_3b, qwen2_5_7b
    shapes = {"qwen2.5-1.5b": (qwen2_5_1_5b, 1536, 8960, 28, 12, 2, True),
              "qwen2.5-3b": (qwen2_5_3b, 2048, 11008, 36, 16, 2, True),
              "qwen2.5-7b": (qwen2_5_7b, 3584, 18944, 28, 28, 4, False)}
    for name, (fn, h, i, L, nq, nkv, tied) in shapes.items():
        c = fn()
        assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads,
                c.num_key_value_heads, c.tie_word_embeddings) == (h, i, L, nq, nkv, tied)
        assert c.model_type == "qwen2" and c.qkv_bias and not c.qk_norm and c.head_dim == 128
        assert c.rope_theta == 1e6 and c.rms_norm_eps == 1e-6 and all(c.no_rope_layers)
        assert get_config(name) == c and get_config("Qwen/Qwen2.5-" + name.split("-")[1].upper()) == c
        # the count formula at the real widths, against a two-layer model's own parameters
        c.num_hidden_layers, c.no_rope_layers, c.vocab_size = 2, [1, 1], 1024
        with torch.device("meta"):
            from llm_fine_tune_distributed_amd.models import CausalLM
            assert sum(p.numel() for p in CausalLM(c).parameters()) == c.num_parameters()
    assert get_config("tiny-gpu-qwen2").head_dim == 128
    for name in ("tiny-qwen2", "tiny-gpu-qwen2"):
        m = build_model(get_config(name), dtype=torch.float32)
        assert m.num_parameters() == m.config.num_parameters() == sum(p.numel() for p in m.parameters())
    at = m.model.layers[0].self_attn
    assert at.qkv_bias.shape == (m.config.qkv_size,) and not at.qkv_bias.any()  # zero-initialised, as in HF
    for other in ("tiny-llama", "tiny-qwen3", "tiny"):
        assert not hasattr(build_model(get_config(other), dtype=torch.float32).model.layers[0].self_attn, "qkv_bias")


@pytest.mark.parametrize("key,val", [("use_sliding_window", True),
                                     ("layer_types", ["full_attention", "sliding_attention"])])
def test_unsupported_qwen2_configs_raise(key, val):
    d = get_config("tiny-qwen2").to_hf_dict()
    if key == "layer_types":
        d["num_hidden_layers"] = 2
    d["sliding_window"] = 4096
    c = ModelConfig.from_hf_dict(d)  # the plain config loads, the inert window keys kept
    assert c.extra == {"sliding_window": 4096} and c.to_hf_dict()["sliding_window"] == 4096
    d[key] = val
    with pytest.raises(NotImplementedError, match=key):
        ModelConfig.from_hf_dict(d)


def test_qwen3_still_rejects_attention_bias():
    d = get_config("tiny-qwen3").to_hf_dict()
    d["attention_bias"] = True
    with pytest.raises(NotImplementedError, match="attention_bias"):
        ModelConfig.from_hf_dict(d)


# ------------------------------------------------------------------------------------------------ gradients
def test_qkv_bias_rope_reference_gradients_fp64():
    """QKVBiasRopeFn (reference path, closed-form backward) against fp64 autograd of the reference and of an
    independent composition."""
    torch.manual_seed(0)
    M, nq, nkv, D = 13, 4, 2, 32
    nh = nq + nkv
    qkv = torch.randn(M, (nq + 2 * nkv) * D, dtype=torch.float64)
    bias = 0.5 * torch.randn((nq + 2 * nkv) * D, dtype=torch.float64)
    pos = torch.randint(0, 4000, (M,))
    fr = pos.double()[:, None] * ref.rope_inv_freq(D, 1e6, None).double()[None]
    cos, sin = fr.cos(), fr.sin()
    G = torch.randn_like(qkv)

    def grads(fn, need_bias=True):
        x, b = qkv.clone().requires_grad_(True), bias.clone().requires_grad_(need_bias)
        y = fn(x, b)
        return (y,) + torch.autograd.grad((y * G).sum(), (x, b) if need_bias else (x,))

    def independent(x, b):
        t = (x + b).view(M, nq + 2 * nkv, D)
        h1, h2 = t[:, :nh, : D // 2], t[:, :nh, D // 2:]
        c, s = cos[:, None], sin[:, None]
        rot = torch.cat([h1 * c - h2 * s, h2 * c + h1 * s], -1)
        return torch.cat([rot.reshape(M, nh * D), t[:, nh:].reshape(M, nkv * D)], -1)

    got = grads(lambda x, b: ops.qkv_bias_rope_(x.clone(), b, cos, sin, nq, nkv, D))
    want = grads(lambda x, b: ref.qkv_bias_rope(x, b, cos, sin, nq, nkv, D))
    indep = grads(independent)
    for g, w, i, name in zip(got, want, indep, ("y", "dqkv", "dbias")):
        assert torch.allclose(g, w, atol=1e-12, rtol=0), (name, (g - w).abs().max().item())
        assert torch.allclose(w, i, atol=1e-12, rtol=0), (name, (w - i).abs().max().item())
    assert got[2].abs().max() > 1  # (not a comparison of zeros)
    # a frozen bias: the same dqkv through the plain inverse rotation
    frozen = grads(lambda x, b: ops.qkv_bias_rope_(x.clone(), b, cos, sin, nq, nkv, D), need_bias=False)
    assert torch.allclose(frozen[1], want[1], atol=1e-12, rtol=0)
    # it returns its input object; under no_grad it makes no node
    x = qkv.clone().requires_grad_(True)
    xc = x.clone()
    assert ops.qkv_bias_rope_(xc, bias, cos, sin, nq, nkv, D) is xc and xc.grad_fn is not None
    with torch.no_grad():
        x = qkv.clone()
        y = ops.qkv_bias_rope_(x, bias.clone().requires_grad_(True), cos, sin, nq, nkv, D)
    assert y is x and y.grad_fn is None and not y.requires_grad
    assert torch.allclose(x, want[0], atol=1e-12, rtol=0)


def test_model_gradients_match_hf(hf_dir):
    """main_grad path of qkv_bias and qkv_proj == plain autograd of the HF model (the bounds of
    test_qwen3_cpu.test_model_gradients_match_hf)."""
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
        bias_ref = torch.cat([hsd[pre + f"{n}_proj.bias"].grad for n in "qkv"], 0)
        assert bias_ref.abs().max() > 1e-4  # (not a comparison of zeros)
        assert torch.allclose(at.qkv_bias.main_grad, bias_ref, atol=1e-5, rtol=1e-3)
        # the q and k bias gradients are a few 1e-5 at this size, under that atol: each group also to 1e-3 of its own
        # largest entry (both sides are fp32, whose round-off is ~1e-6 of the largest)
        for got, want in zip(at.qkv_bias.main_grad.split([96, 48, 48]), bias_ref.split([96, 48, 48])):
            assert want.abs().max() > 1e-6 and (got - want).abs().max() < 1e-3 * want.abs().max()
    assert torch.allclose(m.model.norm.weight.main_grad, hsd["model.norm.weight"].grad, atol=1e-5, rtol=1e-3)
    hm.zero_grad()


def test_gradient_checkpointing_gives_the_same_gradients():
    """Recomputing a layer re-runs the in-place node on a fresh GEMM output: same loss, same gradients."""
    torch.manual_seed(0)
    m = _tiny_qwen2()
    m.train()
    ids = torch.randint(0, 512, (2, 14))

    def run(ckpt_on):
        m.gradient_checkpointing = ckpt_on
        for p in m.parameters():
            p.grad = None
        m.reset_grad_use_counters()
        loss = m(ids, labels=ids).loss
        loss.backward()
        return loss.item(), {n: p.grad.clone() for n, p in m.named_parameters()}

    l0, g0 = run(False)
    l1, g1 = run(True)
    assert l0 == l1
    assert sum(_is_bias(n) for n in g0) == m.config.num_hidden_layers
    for n in g0:
        assert torch.allclose(g0[n], g1[n], atol=1e-7, rtol=1e-6), n
        assert g0[n].abs().max() > 0, n


# ------------------------------------------------------------------------------------------------ generation
def test_greedy_cache_matches_full_forward():
    torch.manual_seed(0)
    m = _tiny_qwen2()
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
    m = _tiny_qwen2()
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


def _biases(m):
    return torch.cat([l.self_attn.qkv_bias.detach() for l in m.model.layers])


def test_trainer_lowers_loss_and_resume_restores_biases(tmp_path, tk):
    rows = generate_qa(8, seed=0)

    def mk(seed):
        a = SFTConfig(output_dir=str(tmp_path / "run"), per_device_train_batch_size=8, learning_rate=3e-3, max_steps=3,
                      logging_steps=1, save_steps=3, dataloader_drop_last=True, jsonl_log=False)
        return SFTTrainer(model=build_model(get_config("tiny-qwen2"), dtype=torch.float32, seed=seed), args=a,
                          train_dataset=rows, processing_class=tk)

    t1 = mk(1)
    t1.train()
    losses = [h["loss"] for h in t1.state.log_history if "loss" in h]
    assert len(losses) == 3 and losses[-1] < losses[0], losses
    trained = _biases(t1.model)
    assert trained.abs().max() > 1e-4  # the biases trained (they sit in the optimizer)
    t2 = mk(9)  # other weights; the checkpoint at step 3 puts the trained ones back, no step runs
    assert not _biases(t2.model).any()
    out = t2.train(resume_from_checkpoint="auto")
    assert out.global_step == 3
    assert torch.equal(_biases(t2.model), trained)


def test_biases_have_no_weight_decay():
    from llm_fine_tune_distributed_amd.parallel.ddp import _no_decay
    m = build_model(get_config("tiny-qwen2"), dtype=torch.float32)
    bs = [(n, p) for n, p in m.named_parameters() if _is_bias(n)]
    assert len(bs) == m.config.num_hidden_layers and all(_no_decay(n, p) for n, p in bs)


def test_freeze_policies_cover_the_biases():
    m = build_model(get_config("tiny-qwen2"), dtype=torch.float32)
    apply_freeze_policy(m, "last_n_layers", n_last=1)
    flags = [l.self_attn.qkv_bias.requires_grad for l in m.model.layers]
    assert flags == [False] * (len(flags) - 1) + [True]
    ids = torch.randint(0, m.config.vocab_size, (2, 12))
    m.reset_grad_use_counters()
    m(ids, labels=ids).loss.backward()  # frozen layers take the plain inverse rotation, the last one trains its bias
    assert m.model.layers[0].self_attn.qkv_bias.grad is None and m.model.layers[-1].self_attn.qkv_bias.grad is not None
    apply_freeze_policy(m, "lora", lora_config=LoRAConfig(r=4))
    assert not any(p.requires_grad for n, p in m.named_parameters() if _is_bias(n))
    for p in m.parameters():
        p.grad = None
    m(ids, labels=ids).loss.backward()  # the LoRA route of a bias layer trains the adapters only
    at = m.model.layers[0].self_attn
    assert at.qkv_bias.grad is None and at.lora["qkv"].B[0].grad is not None


def test_merged_lora_export_matches_live_model(tmp_path):
    from transformers import AutoModelForCausalLM
    torch.manual_seed(0)
    m = _tiny_qwen2(seed=5)
    biases = _biases(m).clone()
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
    assert type(hm).__name__ == "Qwen2ForCausalLM"
    got = torch.cat([torch.cat([getattr(l.self_attn, n + "_proj").bias for n in "qkv"]) for l in hm.model.layers])
    assert torch.equal(got, biases)  # carried unchanged
    with torch.no_grad():
        ho = hm(input_ids=ids).logits
    assert (ho.reshape(mo.shape) - mo).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------ distributed
def _as_qwen2(fn, *args):
    """Run a worker of another test module that builds `tiny(...)` with the model type swapped for qwen2 and the
    biases randomised (the workers build from a seed, so every process gets the same ones)."""
    import llm_fine_tune_distributed_amd.models as models
    orig_tiny, orig_build = models.tiny, models.build_model

    def build(*a, **k):
        m = orig_build(*a, **k)
        _randomise_biases(m.named_parameters())
        return m

    models.tiny = lambda *a, **k: orig_tiny("qwen2", **k)
    models.build_model = build
    try:
        fn(*args)
    finally:
        models.tiny, models.build_model = orig_tiny, orig_build


def _run_qwen2(rank, world, port, out_dir, per_dev, ga, steps):
    _as_qwen2(dist_harness._run, rank, world, port, out_dir, per_dev, ga, steps)


def _cp_worker_qwen2(rank, world, port, out_dir, layout):
    import test_context_parallel_cpu as cp_harness
    _as_qwen2(cp_harness._model_worker, rank, world, port, out_dir, layout)


def test_context_parallel_matches_single_process():
    """The bias route into ring_attention (world 2, zig-zag): loss and every gradient, the biases included, equal
    one process on the whole batch (test_context_parallel_cpu's worker and bounds)."""
    import torch.multiprocessing as mp
    from llm_fine_tune_distributed_amd.models import tiny
    d = tempfile.mkdtemp()
    mp.spawn(_cp_worker_qwen2, args=(2, dist_harness._free_port(), d, "zigzag"), nprocs=2, join=True)
    torch.manual_seed(0)
    cfg = tiny("qwen2", num_hidden_layers=4)
    ids = torch.randint(0, cfg.vocab_size, (2, 21))
    labels = ids.clone()
    labels[1, 15:] = -100
    m = build_model(cfg, dtype=torch.float32, seed=7)
    _randomise_biases(m.named_parameters())
    n = float((labels[:, 1:] != -100).sum())
    m.reset_grad_use_counters()
    out = m(ids, labels=labels, num_items_in_batch=torch.tensor([n]))
    out.loss.backward()
    r0 = torch.load(os.path.join(d, "m0.pt"))
    assert abs(r0["loss"] - out.loss.item()) < 1e-5
    assert any(_is_bias(k) for k in r0["grads"])
    for name, p in m.named_parameters():
        e = (r0["grads"][name] - p.grad).abs().max().item()
        assert e < 1e-5 * max(1.0, p.grad.abs().max().item()), (name, e)


def test_ddp2_one_step_matches_single_process():
    import torch.multiprocessing as mp
    d = tempfile.mkdtemp()
    _run_qwen2(0, 1, dist_harness._free_port(), d, 4, 1, 1)
    mp.spawn(_run_qwen2, args=(2, dist_harness._free_port(), d, 2, 1, 1), nprocs=2, join=True)
    single = torch.load(os.path.join(d, "r1_0.pt"))
    r0 = torch.load(os.path.join(d, "r2_0.pt"))
    r1 = torch.load(os.path.join(d, "r2_1.pt"))
    n = build_model(get_config("tiny-qwen2"), dtype=torch.float32).num_parameters()
    assert single["params"].numel() == n  # the qwen2 model ran: the biases are in the flat parameters
    assert torch.equal(r0["params"], r1["params"])
    assert torch.allclose(r0["params"], single["params"], atol=1e-5, rtol=1e-4)
    assert abs(single["log"][0]["loss"] - r0["log"][0]["loss"]) < 1e-4
    assert abs(single["log"][0]["grad_norm"] - r0["log"][0]["grad_norm"]) < 1e-3
