"""Sliding-window attention and the Mistral family on the CPU (fp32 / fp64 reference path): the reference mask against
a brute-force loop, parity with transformers' MistralForCausalLM through a saved directory (logits past the window,
padded batches, gradients), the save round trip, generation past the window, rejected configs and the FLOP model.

One definition everywhere: window W > 0 lets the query at position i of its sequence see the keys j with
i - W < j <= i (W keys, itself included: transformers' sliding_window_overlay); 0 / None is no window."""
import json
import math
import os
import tempfile

import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import generate, generate_batch
from llm_fine_tune_distributed_amd.models import ModelConfig, build_model, get_config
from llm_fine_tune_distributed_amd.ops import reference as ref
from llm_fine_tune_distributed_amd.train import checkpoint as ckpt

VOCAB = 512
WINDOW = 8


# ------------------------------------------------------------------------------------------------ reference mask
def _brute_force(qkv, nq, nkv, D, lens, scale, window):
    """Attention one query at a time over an explicit key list (fp64)."""
    M = qkv.shape[0]
    q = qkv[:, :nq * D].view(M, nq, D)
    k = qkv[:, nq * D:(nq + nkv) * D].view(M, nkv, D)
    v = qkv[:, (nq + nkv) * D:].view(M, nkv, D)
    out = torch.zeros(M, nq, D, dtype=qkv.dtype)
    s = 0
    for L in lens:
        for i in range(L):
            keys = [j for j in range(L) if j <= i and (window == 0 or j > i - window)]
            for h in range(nq):
                g = h // (nq // nkv)
                sc = torch.stack([(q[s + i, h] * k[s + j, g]).sum() * scale for j in keys])
                p = torch.softmax(sc, 0)
                out[s + i, h] = sum(p[n] * v[s + j, g] for n, j in enumerate(keys))
        s += L
    return out.view(M, nq * D)


@pytest.mark.parametrize("window", [1, 3, 8, 64])
def test_reference_window_mask_against_brute_force(window):
    lens, nq, nkv, D = [1, 5, 40], 4, 2, 8
    torch.manual_seed(window)
    qkv = torch.randn(sum(lens), (nq + 2 * nkv) * D, dtype=torch.float64)
    cu = torch.tensor([0, 1, 6, 46], dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    got = ref.attention(qkv, nq, nkv, D, cu, scale, True, window)
    want = _brute_force(qkv, nq, nkv, D, lens, scale, window)
    assert (got - want).abs().max() < 1e-12
    full = ref.attention(qkv, nq, nkv, D, cu, scale, True)
    assert torch.equal(ref.attention(qkv, nq, nkv, D, cu, scale, True, 0), full)
    if window >= max(lens):
        assert torch.equal(got, full)  # W >= len is the plain causal result, exactly
    else:
        assert (got - full).abs().max() > 1e-3  # (and a smaller one is not)
        # sequences no longer than the window are untouched
        for s, e in zip(cu[:-1].tolist(), cu[1:].tolist()):
            if e - s <= window:
                assert torch.equal(got[s:e], full[s:e])


def test_window_requires_causal():
    qkv = torch.randn(6, 4 * 8, dtype=torch.float64)
    cu = torch.tensor([0, 6], dtype=torch.int32)
    with pytest.raises(ValueError, match="causal"):
        ref.attention(qkv, 2, 1, 8, cu, None, False, 3)
    from llm_fine_tune_distributed_amd import ops
    with pytest.raises(ValueError, match="causal"):
        ops.flash_attention(qkv.float(), cu, 6, 2, 1, 8, causal=False, window=3)
    ops.flash_attention(qkv.float(), cu, 6, 2, 1, 8, causal=False, window=0)


def test_every_row_sees_itself():
    """No degenerate (all-masked) row exists under the window: the mask's diagonal is always set, so the GPU tests'
    block metric needs no case beyond the length-1 / W = 1 ones (out = V, dq = dk = 0)."""
    for T in (1, 2, 33, 65):
        for W in (1, 16, 64, 65, 4096):
            mask = torch.ones(T, T, dtype=torch.bool).tril() & ~torch.ones(T, T, dtype=torch.bool).tril(-W)
            assert mask.diagonal().all() and (mask.sum(-1) == torch.arange(1, T + 1).clamp(max=W)).all()
    # W = 1: the softmax of the one score is 1: out is the V row, the gradient of q and k is zero
    nq, nkv, D = 4, 2, 8
    qkv = torch.randn(9, (nq + 2 * nkv) * D, dtype=torch.float64, requires_grad=True)
    cu = torch.tensor([0, 9], dtype=torch.int32)
    o = ref.attention(qkv, nq, nkv, D, cu, None, True, 1)
    v = qkv[:, (nq + nkv) * D:].view(9, nkv, D).repeat_interleave(nq // nkv, 1).reshape(9, nq * D)
    assert torch.equal(o, v.detach())
    (g,) = torch.autograd.grad(o, qkv, torch.randn_like(o))
    assert g[:, :(nq + nkv) * D].abs().max() == 0


# ------------------------------------------------------------------------------------------------ HF parity
@pytest.fixture(scope="module")
def hf_dir():
    """A tiny fp32 MistralForCausalLM (window 8, GQA, 2 layers, eager attention) saved by transformers."""
    from transformers import MistralConfig, MistralForCausalLM
    torch.manual_seed(0)
    hc = MistralConfig(vocab_size=VOCAB, hidden_size=96, intermediate_size=160, num_hidden_layers=2,
                       num_attention_heads=4, num_key_value_heads=2, head_dim=24, max_position_embeddings=256,
                       sliding_window=WINDOW, tie_word_embeddings=False, attn_implementation="eager")
    hm = MistralForCausalLM(hc).float().eval()
    d = tempfile.mkdtemp()
    hm.save_pretrained(d)
    return d, hm


def _load_ours(d):
    cfg = get_config(d)
    m = build_model(cfg, dtype=torch.float32)
    m.load_hf_state_dict(ckpt.load_state_dict(d))  # strict: no unexpected keys
    return m


def test_hf_saved_directory_reads_the_window(hf_dir):
    d, _ = hf_dir
    cfg = get_config(d)
    assert cfg.model_type == "llama" and cfg.sliding_window == WINDOW and cfg.head_dim == 24
    m = _load_ours(d)
    assert [l.self_attn.window for l in m.model.layers] == [WINDOW, WINDOW]


@pytest.mark.parametrize("T", [40, 8])
def test_hf_logit_parity(hf_dir, T):
    """T = 40: past the window (the parent commit ignored it: this case fails there). T = 8: the window is inert.
    Tolerances: tests/test_model_cpu.py::test_parity_with_transformers."""
    d, hm = hf_dir
    m = _load_ours(d)
    torch.manual_seed(1)
    ids = torch.randint(0, VOCAB, (1, T))
    with torch.no_grad():
        ho = hm(input_ids=ids, labels=ids)
        mo = m(ids, labels=ids, return_logits=True)
        full = build_model(dataclasses_replace(m.config, sliding_window=None), dtype=torch.float32)
        full.load_state_dict(m.state_dict())
        fo = full(ids, return_logits=True)
    assert abs(ho.loss.item() - mo.loss.item()) < 1e-5
    assert (ho.logits.reshape(-1, VOCAB) - mo.logits).abs().max() < 1e-4
    if T > WINDOW:  # (the comparison can tell: the same weights without the window give other logits)
        assert (fo.logits - mo.logits).abs().max() > 1e-2
        assert torch.equal(fo.logits[:WINDOW], mo.logits[:WINDOW])
    else:
        assert torch.equal(fo.logits, mo.logits)


def dataclasses_replace(cfg, **kw):
    import dataclasses
    return dataclasses.replace(cfg, **kw)


def test_hf_parity_padded_and_packed(hf_dir):
    d, hm = hf_dir
    m = _load_ours(d)
    torch.manual_seed(2)
    a = torch.randint(0, VOCAB, (40,))
    b = torch.randint(0, VOCAB, (23,))
    ids = torch.zeros(2, 40, dtype=torch.long)
    ids[0], ids[1, :23] = a, b
    labels = ids.clone()
    labels[1, 23:] = -100
    am = (torch.arange(40)[None] < torch.tensor([40, 23])[:, None]).long()
    with torch.no_grad():
        ho = hm(input_ids=ids, attention_mask=am, labels=labels)
        mo = m(ids, labels=labels, return_logits=True)
        pk = m(torch.cat([a, b]), cu_seqlens=torch.tensor([0, 40, 63], dtype=torch.int32), max_seqlen=40,
               return_logits=True)
    assert abs(ho.loss.item() - mo.loss.item()) < 1e-5
    valid = torch.cat([ho.logits[0], ho.logits[1, :23]])
    ours = torch.cat([mo.logits[:40], mo.logits[40:63]])
    assert (valid - ours).abs().max() < 1e-4
    assert (valid - pk.logits).abs().max() < 1e-4


def test_model_gradients_match_hf(hf_dir):
    """One training step's gradients (main_grad path) == plain autograd of the HF model on the same weights and batch,
    at the bounds of tests/test_model_cpu.py::test_gradients_match_autograd_reference; 30 tokens: past the window."""
    d, hm = hf_dir
    m = _load_ours(d)
    for p in m.parameters():
        p.main_grad = torch.zeros_like(p)
    torch.manual_seed(3)
    ids = torch.randint(0, VOCAB, (2, 30))
    m.reset_grad_use_counters()
    m(ids, labels=ids).loss.backward()
    hm.zero_grad()
    hm.train()
    hm(input_ids=ids, labels=ids).loss.backward()
    hm.eval()
    hsd = dict(hm.named_parameters())
    for i in (0, 1):
        at = m.model.layers[i].self_attn
        pre = f"model.layers.{i}.self_attn."
        qkv_ref = torch.cat([hsd[pre + f"{n}_proj.weight"].grad for n in "qkv"], 0)
        assert torch.allclose(at.qkv_proj.main_grad, qkv_ref, atol=1e-5, rtol=1e-3)
        assert torch.allclose(at.o_proj.main_grad, hsd[pre + "o_proj.weight"].grad, atol=1e-5, rtol=1e-3)
    assert torch.allclose(m.model.embed_tokens.main_grad, hsd["model.embed_tokens.weight"].grad, atol=1e-5, rtol=1e-3)
    assert torch.allclose(m.model.norm.weight.main_grad, hsd["model.norm.weight"].grad, atol=1e-5, rtol=1e-3)
    hm.zero_grad()


def test_tiny_mistral_training_step_matches_hf(tmp_path):
    """The ``tiny-mistral`` preset itself: saved, loaded by transformers, one step's gradients on both sides."""
    from transformers import MistralForCausalLM
    m = build_model(get_config("tiny-mistral"), dtype=torch.float32, seed=5)
    ckpt.save_pretrained(m, str(tmp_path / "m"))
    hm = MistralForCausalLM.from_pretrained(str(tmp_path / "m"), torch_dtype=torch.float32,
                                            attn_implementation="eager")
    assert hm.config.sliding_window == 8
    for p in m.parameters():
        p.main_grad = torch.zeros_like(p)
    torch.manual_seed(4)
    ids = torch.randint(0, m.config.vocab_size, (2, 28))
    m.reset_grad_use_counters()
    lo = m(ids, labels=ids).loss
    lo.backward()
    lh = hm(input_ids=ids, labels=ids).loss
    lh.backward()
    assert abs(lo.item() - lh.item()) < 1e-5
    hsd = dict(hm.named_parameters())
    for i in range(m.config.num_hidden_layers):
        pre = f"model.layers.{i}.self_attn."
        qkv_ref = torch.cat([hsd[pre + f"{n}_proj.weight"].grad for n in "qkv"], 0)
        assert torch.allclose(m.model.layers[i].self_attn.qkv_proj.main_grad, qkv_ref, atol=1e-5, rtol=1e-3), i
    assert torch.allclose(m.model.norm.weight.main_grad, hsd["model.norm.weight"].grad, atol=1e-5, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ round trip
def test_save_round_trip_loads_in_transformers(hf_dir, tmp_path):
    from transformers import MistralForCausalLM
    d, hm = hf_dir
    m = _load_ours(d)
    out = str(tmp_path / "out")
    ckpt.save_pretrained(m, out)
    with open(os.path.join(out, "config.json")) as f:
        cj = json.load(f)
    assert cj["architectures"] == ["MistralForCausalLM"] and cj["model_type"] == "mistral"
    assert cj["sliding_window"] == WINDOW
    hm2, info = MistralForCausalLM.from_pretrained(out, torch_dtype=torch.float32, output_loading_info=True,
                                                   attn_implementation="eager")
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"]
    assert hm2.config.sliding_window == WINDOW
    torch.manual_seed(5)
    ids = torch.randint(0, VOCAB, (2, 32))
    with torch.no_grad():
        assert (hm2.eval()(input_ids=ids).logits - hm(input_ids=ids).logits).abs().max() < 1e-4
        assert (hm2(input_ids=ids).logits.reshape(-1, VOCAB) - m(ids, return_logits=True).logits).abs().max() < 1e-4
    m2 = _load_ours(out)  # and our own directory reads back, window included
    assert m2.config.sliding_window == WINDOW
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))


def test_mistral_without_window_saves_as_llama(tmp_path):
    d = get_config("tiny-mistral").to_hf_dict()
    assert d["model_type"] == "mistral" and d["sliding_window"] == 8
    for missing in ({**d, "sliding_window": None}, {k: v for k, v in d.items() if k != "sliding_window"}):
        cfg = ModelConfig.from_hf_dict(missing)
        assert cfg.model_type == "llama" and cfg.sliding_window is None
        out = cfg.to_hf_dict()
        assert out["architectures"] == ["LlamaForCausalLM"] and out["model_type"] == "llama"
        assert "sliding_window" not in out
    # a llama-type config with no window is what it was
    assert get_config("tiny-llama").sliding_window is None
    assert get_config("tiny-llama").to_hf_dict()["model_type"] == "llama"
    # a qwen2 config's inert sliding_window key stays inert
    q = ModelConfig.from_hf_dict({**get_config("tiny-qwen2").to_hf_dict(), "sliding_window": 4096})
    assert q.sliding_window is None and q.extra["sliding_window"] == 4096


# ------------------------------------------------------------------------------------------------ generation
def test_greedy_generation_matches_full_windowed_forward():
    """24 new tokens from a 5-token prompt: the cache outgrows the window of 8 three times over."""
    m = build_model(get_config("tiny-mistral"), dtype=torch.float32, seed=2)
    torch.manual_seed(0)
    prompt = torch.randint(0, m.config.vocab_size, (5,)).tolist()
    out = generate(m, prompt, max_new_tokens=24, do_sample=False, repetition_penalty=1.0)
    seq = list(prompt)
    for _ in range(24):
        with torch.no_grad():
            lg = m(torch.tensor(seq)[None], return_logits=True).logits
        seq.append(int(lg[-1].argmax()))
    assert out == seq[len(prompt):]
    # (the window matters for these tokens: the same weights without it generate something else)
    import dataclasses
    full = build_model(dataclasses.replace(m.config, sliding_window=None), dtype=torch.float32)
    full.load_state_dict(m.state_dict())
    assert generate(full, prompt, max_new_tokens=24, do_sample=False, repetition_penalty=1.0) != out


def test_generate_batch_rows_equal_generate():
    m = build_model(get_config("tiny-mistral"), dtype=torch.float32, seed=2)
    torch.manual_seed(0)
    prompts = [torch.randint(0, m.config.vocab_size, (n,)).tolist() for n in (5, 13, 9)]
    greedy = generate_batch(m, prompts, max_new_tokens=24, do_sample=False, repetition_penalty=1.0)
    for b, p in enumerate(prompts):
        assert greedy[b] == generate(m, p, max_new_tokens=24, do_sample=False, repetition_penalty=1.0), b
    kw = dict(max_new_tokens=12, temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.1, do_sample=True)
    got = generate_batch(m, prompts, seed=7, **kw)
    for b, p in enumerate(prompts):
        assert got[b] == generate(m, p, seed=7 + b, **kw), b


# ------------------------------------------------------------------------------------------------ config errors
def test_mixed_layer_types_raise():
    d = get_config("tiny-mistral").to_hf_dict()
    with pytest.raises(NotImplementedError, match="layer_types"):
        ModelConfig.from_hf_dict({**d, "layer_types": ["sliding_attention", "full_attention"] * 2})
    assert ModelConfig.from_hf_dict({**d, "layer_types": ["sliding_attention"] * 4}).sliding_window == 8
    assert ModelConfig.from_hf_dict({**d, "layer_types": ["full_attention"] * 4}).sliding_window is None
    with pytest.raises(ValueError, match="sliding_window"):
        ModelConfig(model_type="llama", sliding_window=0)


def test_window_with_context_parallel_raises():
    from llm_fine_tune_distributed_amd.train import SFTConfig, SFTTrainer
    m = build_model(get_config("tiny-mistral"), dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.enable_context_parallel(object())
    assert all(l.self_attn.cp_group is None for l in m.model.layers)
    build_model(get_config("tiny-llama"), dtype=torch.float32).enable_context_parallel(None)  # no window: as before
    assert SFTConfig(context_parallel_size=2).context_parallel_size == 2 and SFTTrainer is not None


def test_presets():
    c = get_config("mistral-7b")
    assert c == get_config("mistralai/Mistral-7B-v0.1")
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers) == (4096, 14336, 32)
    assert (c.num_attention_heads, c.num_key_value_heads, c.head_dim) == (32, 8, 128)
    assert (c.vocab_size, c.rope_theta, c.rms_norm_eps, c.tie_word_embeddings) == (32000, 10000.0, 1e-5, False)
    assert (c.bos_token_id, c.eos_token_id, c.max_position_embeddings, c.sliding_window) == (1, 2, 32768, 4096)
    assert c.num_parameters() == 7_241_732_096
    assert get_config("tiny-mistral").sliding_window == 8
    g = get_config("tiny-gpu-mistral")
    assert (g.head_dim, g.num_attention_heads // g.num_key_value_heads, g.num_hidden_layers, g.sliding_window) == \
        (128, 4, 2, 40)


# ------------------------------------------------------------------------------------------------ FLOP model
def test_flop_model_counts_the_window():
    import dataclasses
    w = get_config("mistral-7b")
    full = dataclasses.replace(w, sliding_window=None)
    for T in (1, 512, 4096):
        assert w.flops_per_token(T) == full.flops_per_token(T)
    for T in (4097, 8192, 32768):
        assert w.flops_per_token(T) < full.flops_per_token(T)
    # exact form: row i sees min(i + 1, W) keys instead of i + 1, and the difference is what the count loses
    c = get_config("tiny-mistral")
    T, W = 40, 8
    lost = sum(i + 1 - min(i + 1, W) for i in range(T))
    per_pair = c.num_hidden_layers * 4.0 * c.num_attention_heads * c.head_dim / T
    unwindowed = dataclasses.replace(c, sliding_window=None).flops_per_token(T, training=False)
    assert abs(unwindowed - c.flops_per_token(T, training=False) - per_pair * lost) < 1e-9 * unwindowed
    assert c.flops_per_token(W + 1) < dataclasses.replace(c, sliding_window=None).flops_per_token(W + 1)
