"""Sliding-window attention on MI355X: the windowed instantiations of fwd32 / bwd_dkdv32 / bwd_dq32 / bwd_dq3 and the
windowed decode kernels against the fp64 reference, tiny-gpu-mistral on the HIP path against the PyTorch path (full SFT
and LoRA), generation past the window, and the time the skipped tiles save.

Conventions of tests/test_attention_blocks_gpu.py: the fp64 reference with autograd, every (sequence, head) block on
its own (tests/_blockwise.py) at the project's bounds, 2e-2 for out and 3e-2 for dq / dk / dv, both dQ paths
(SFTAMD_ATTN_DS_MB "" = materialised dS^T + dq32, "0" = the recomputing dq3), flash_bwd and flash_bwd_rope.

Window W: the query at position i sees the keys j with i - W < j <= i. Every row sees itself, so the reference has no
degenerate block beyond the length-1 / W = 1 ones (out = V, dq = dk = 0), which _blockwise judges against the rms of
the whole gradient (checked on the CPU: tests/test_sliding_window_cpu.py::test_every_row_sees_itself)."""
import math
import statistics

import pytest
import torch

import _rowwise as rw
from _blockwise import assert_blocks_close, block_rel_err
from llm_fine_tune_distributed_amd.inference.generation import generate, generate_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 128
OUT_BOUND, GRAD_BOUND = 2e-2, 3e-2

EDGES = [1, 2, 31, 33, 64, 65, 129, 1]
RAGGED = [300, 17, 129, 66]
CASES = {"edges_8_2": (EDGES, 8, 2), "edges_4_4": (EDGES, 4, 4), "edges_12_3": (EDGES, 12, 3),
         "ragged_8_2": (RAGGED, 8, 2), "ragged_4_4": (RAGGED, 4, 4), "ragged_12_3": (RAGGED, 12, 3),
         "long_ends": ([1, 511, 512, 1], 16, 4)}
# 1: out = V; 16, 33: rows with no visible key in their wave's first tile, both mask edges in one tile; 64 / 65: the
# tile-boundary off-by-one; 100: the window edge and the diagonal in different tiles of a workgroup; 4096 > len: window=0
WINDOWS = [1, 16, 33, 64, 65, 100, 4096]


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()


def _rope_tables(lens):
    pos = torch.cat([torch.arange(l) for l in lens]).to(DEV).double()
    ang = pos[:, None] / (10000 ** (torch.arange(0, 64, device=DEV).double() / 64))[None]
    return ang.cos(), ang.sin()


def _inverse_rope64(g, cos, sin, nq, nkv):
    M = g.shape[0]
    qk = g[:, :(nq + nkv) * D].reshape(M, nq + nkv, D)
    x1, x2 = qk[..., :64], qk[..., 64:]
    c, s = cos[:, None, :], sin[:, None, :]
    rot = torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], dim=-1).reshape(M, -1)
    return torch.cat([rot, g[:, (nq + nkv) * D:]], dim=1)


@pytest.fixture(scope="module")
def attn_ref():
    """Inputs and the fp64 reference (out, dqkv, inverse-RoPE dqkv) per (case, window): computed once, shared by the two
    dQ paths, never modified."""
    cache = {}

    def get(name, window):
        key = (name, window)
        if key not in cache:
            lens, nq, nkv = CASES[name]
            g = torch.Generator(device=DEV).manual_seed(100 * list(CASES).index(name) + WINDOWS.index(window) + 1)
            cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
            M = int(cu[-1])
            qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, generator=g).to(torch.bfloat16)
            dout = torch.randn(M, nq * D, device=DEV, generator=g).to(torch.bfloat16)
            q64 = qkv.double().requires_grad_(True)
            o64 = ref.attention(q64, nq, nkv, D, cu, 1 / math.sqrt(D), True, window)
            (g64,) = torch.autograd.grad(o64, q64, dout.double())
            cos, sin = _rope_tables(lens)
            cache[key] = dict(lens=lens, nq=nq, nkv=nkv, cu=cu, qkv=qkv, dout=dout, o64=o64.detach(), g64=g64,
                              g64_rope=_inverse_rope64(g64, cos, sin, nq, nkv),
                              cos=cos.float().contiguous(), sin=sin.float().contiguous())
        return cache[key]
    yield get
    cache.clear()


def _grad_blocks(dqkv, want, r, what):
    """dq / dk / dv per (sequence, head) at GRAD_BOUND. Where the reference of dq (dk) is zero everywhere — W = 1: every
    row sees one key — no block has a magnitude of its own and the rms of dq (dk) is zero too, so those blocks are
    judged against the rms of the whole gradient dqkv, which is what _blockwise does for the zero blocks of a length-1
    sequence among others."""
    nq, nkv, cu = r["nq"], r["nkv"], r["cu"].tolist()
    worst = {}
    for name, lo, hi in (("dq", 0, nq * D), ("dk", nq * D, (nq + nkv) * D), ("dv", (nq + nkv) * D, (nq + 2 * nkv) * D)):
        w = want[:, lo:hi]
        if w.abs().max() == 0:
            rms = want.pow(2).mean().sqrt()
            e = torch.cat([block_rel_err(dqkv[s:t, lo:hi], w[s:t], t - s, D, rms) for s, t in zip(cu[:-1], cu[1:])])
            worst[name] = e.max().item()
            assert worst[name] <= GRAD_BOUND, (what, name, worst[name])
            continue
        worst[name] = assert_blocks_close(dqkv[:, lo:hi], w, 0, D, GRAD_BOUND, f"{what} {name}", row_splits=cu)
    return worst


def _poison_ds(lens, nq):
    """A NaN-filled bf16 block of the dS^T size, allocated and freed: the caching allocator hands it to the backward's
    at::empty, so a dS^T tile that bwd_dq32 reads and bwd_dkdv32 did not write shows as NaN instead of passing by the
    luck of what the memory held."""
    lp = (max(lens) + 127) // 128 * 128
    t = torch.full((len(lens) * nq * lp * lp,), float("nan"), dtype=torch.bfloat16, device=DEV)
    del t


@pytest.mark.parametrize("ds_mb", ["", "0"])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", list(CASES))
def test_windowed_attention_per_sequence_and_head(name, window, ds_mb, attn_ref, monkeypatch):
    monkeypatch.setenv("SFTAMD_ATTN_DS_MB", ds_mb)
    r = attn_ref(name, window)
    lens, nq, nkv, cu, qkv, dout = r["lens"], r["nq"], r["nkv"], r["cu"], r["qkv"], r["dout"]
    scale, rep, ms = 1 / math.sqrt(D), r["nq"] // r["nkv"], max(r["lens"])
    ops = _ext.ops()
    what = f"{name} window={window} ds_mb={ds_mb!r}"
    out, lse = ops.flash_fwd(qkv, cu, ms, nq, nkv, D, scale, True, window)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), what
    w_out = assert_blocks_close(out, r["o64"], 0, D, OUT_BOUND, f"{what} out", row_splits=cu.tolist())
    if ds_mb == "":
        _poison_ds(lens, nq)
    dqkv = ops.flash_bwd(dout, qkv, out, lse, cu, ms, nq, nkv, D, scale, True, None, window)
    assert torch.isfinite(dqkv.float()).all(), what
    w = _grad_blocks(dqkv, r["g64"], r, what)
    if ds_mb == "":
        _poison_ds(lens, nq)
    dqkv_r = ops.flash_bwd_rope(dout, qkv, out, lse, cu, ms, nq, nkv, D, scale, True, r["cos"], r["sin"], None, window)
    assert torch.isfinite(dqkv_r.float()).all(), what
    w_r = _grad_blocks(dqkv_r, r["g64_rope"], r, what + " rope")
    print(f"sliding_window {what}: worst (sequence, head) block out {w_out:.3e}, "
          + ", ".join(f"{k} {v:.3e}" for k, v in w.items()) + "; rope " + ", ".join(f"{k} {v:.3e}" for k, v in w_r.items()))
    v = qkv[:, (nq + nkv) * D:].view(-1, nkv, D).repeat_interleave(rep, 1).reshape(-1, nq * D)
    # A row that sees one key (W = 1: every row; else the first row of a sequence): the softmax of its one score is 1,
    # so out is the V row bit for bit. Where every key of a sequence is seen by that one row alone (W = 1, or a sequence
    # of one token) dq = dk = 0, held as test_attention_blocks_gpu holds the length-1 sequences: to 1e-4 of the
    # gradient's rms. (dS = p (dP - delta) there is the difference of two fp32 sums of the same 128 products in two
    # orders, not a literal zero.) With W = 1 the reference dq / dk are zero everywhere, so the rms is dqkv's.
    cul = cu.tolist()
    rows = torch.cat([torch.arange(cul[b], cul[b + 1] if window == 1 else cul[b] + 1) for b in range(len(lens))]).to(DEV)
    assert torch.equal(out[rows], v[rows]), (what, "one-key rows", (out[rows] != v[rows]).any(-1).nonzero().flatten()[:8])
    whole = window == 1
    rms = {k: r["g64"][:, slice(None) if whole else sl].pow(2).mean().sqrt().item()
           for k, sl in (("dq", slice(0, nq * D)), ("dk", slice(nq * D, (nq + nkv) * D)))}
    zero_rows = torch.cat([torch.arange(0)] + [torch.arange(cul[b], cul[b + 1]) for b, l in enumerate(lens)
                                               if whole or l == 1]).to(DEV)
    for g in (dqkv, dqkv_r) if zero_rows.numel() else ():
        assert g[zero_rows, :nq * D].abs().max().item() <= 1e-4 * rms["dq"], (what, g[zero_rows, :nq * D].abs().max())
        assert g[zero_rows, nq * D:(nq + nkv) * D].abs().max().item() <= 1e-4 * rms["dk"], what
    if window >= ms:  # W >= len: the window=0 result bit for bit
        out0, lse0 = ops.flash_fwd(qkv, cu, ms, nq, nkv, D, scale, True)
        assert torch.equal(out.view(torch.int16), out0.view(torch.int16)) and torch.equal(lse, lse0), what
        d0 = ops.flash_bwd(dout, qkv, out0, lse0, cu, ms, nq, nkv, D, scale, True)
        d0r = ops.flash_bwd_rope(dout, qkv, out0, lse0, cu, ms, nq, nkv, D, scale, True, r["cos"], r["sin"])
        assert torch.equal(dqkv.view(torch.int16), d0.view(torch.int16)), what
        assert torch.equal(dqkv_r.view(torch.int16), d0r.view(torch.int16)), what


def test_window_needs_causal_and_defaults_to_none():
    nq, nkv = 4, 2
    cu = torch.tensor([0, 70], dtype=torch.int32, device=DEV)
    qkv = torch.randn(70, (nq + 2 * nkv) * D, device=DEV).to(torch.bfloat16)
    ops = _ext.ops()
    with pytest.raises(RuntimeError, match="causal"):
        ops.flash_fwd(qkv, cu, 70, nq, nkv, D, 0.1, False, 16)
    a, la = ops.flash_fwd(qkv, cu, 70, nq, nkv, D, 0.1, True)
    b, lb = ops.flash_fwd(qkv, cu, 70, nq, nkv, D, 0.1, True, 0)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(la, lb)


# ------------------------------------------------------------------------------------------------ decode
DECODE = [(40, L) for L in (1, 39, 40, 41, 255, 256, 257, 600)] + [(256, L) for L in (256, 257, 513)]


def _decode_inputs(L, nq, nkv, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(nq * D, generator=g, device=DEV).bfloat16()
    kc = torch.randn(S, nkv, D, generator=g, device=DEV).bfloat16()
    vc = torch.randn(S, nkv, D, generator=g, device=DEV).bfloat16()
    kc[L:], vc[L:] = float("nan"), float("nan")  # rows past the live length are never read
    return q, kc, vc


@pytest.mark.parametrize("window,L", DECODE)
def test_decode_attention_window(window, L):
    """decode_attention over cache[max(0, L - W):L] against fp64, per head, with the bound of test_decode_edges_gpu
    (2 x the fp32 emulation's error). 256-key chunks: L - W at, before and after a chunk edge."""
    nq, nkv, S = 8, 2, 640
    q, kc, vc = _decode_inputs(L, nq, nkv, S, 1000 * window + L)
    ln = torch.tensor([L], dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(D)
    out = _ext.ops().decode_attention(q, kc, vc, ln, nq, nkv, scale, window)
    lo = max(0, L - window)
    want, em = rw.decode_refs(q.view(nq, D), kc[lo:L], vc[lo:L], scale)
    assert_blocks_close(out.view(nq, D), want, 1, D, rw.row_bound(em, want), f"decode W={window} L={L}")
    if window >= L:  # W >= len: bit-identical to window=0
        out0 = _ext.ops().decode_attention(q, kc, vc, ln, nq, nkv, scale)
        assert torch.equal(out.view(torch.int16), out0.view(torch.int16))
    elif L - window >= 8:  # (the window matters: the full-cache result is something else)
        full, _ = rw.decode_refs(q.view(nq, D), kc[:L], vc[:L], scale)
        assert (full - want).abs().max() > 1e-2


@pytest.mark.parametrize("window", [40, 256])
def test_decode_attention_batched_window_mixed_lengths(window):
    nq, nkv, S = 8, 2, 640
    lens = [L for w, L in DECODE if w == window] + [window - 1, 1]
    B = len(lens)
    g = torch.Generator(device=DEV).manual_seed(window)
    qkv = torch.randn(B, (nq + 2 * nkv) * D, generator=g, device=DEV).bfloat16()
    kc = torch.randn(B, S, nkv, D, generator=g, device=DEV).bfloat16()
    vc = torch.randn(B, S, nkv, D, generator=g, device=DEV).bfloat16()
    for b, L in enumerate(lens):
        kc[b, L - 1:], vc[b, L - 1:] = float("nan"), float("nan")
    k0, v0 = kc.clone(), vc.clone()
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(D)
    out = _ext.ops().decode_attention_batched(qkv, kc, vc, ln, nq, nkv, scale, window)
    knew = qkv[:, nq * D:(nq + nkv) * D].view(B, nkv, D)
    vnew = qkv[:, (nq + nkv) * D:].view(B, nkv, D)
    for b, L in enumerate(lens):
        k0[b, L - 1], v0[b, L - 1] = knew[b], vnew[b]
        lo = max(0, L - window)
        want, em = rw.decode_refs(qkv[b, :nq * D].view(nq, D), k0[b, lo:L], v0[b, lo:L], scale)
        assert_blocks_close(out[b].view(nq, D), want, 1, D, rw.row_bound(em, want), f"batched decode W={window} L={L}")
    assert torch.equal(kc.view(torch.int16), k0.view(torch.int16)) and torch.equal(vc.view(torch.int16), v0.view(torch.int16))
    # W >= every length: bit-identical to window=0
    short = [min(L, window) for L in lens]
    ls = torch.tensor(short, dtype=torch.int32, device=DEV)
    for b, L in enumerate(short):  # (finite rows up to the shorter lengths)
        kc[b, :L], vc[b, :L] = torch.randn_like(kc[b, :L]), torch.randn_like(vc[b, :L])
    k1, v1 = kc.clone(), vc.clone()
    a = _ext.ops().decode_attention_batched(qkv, kc, vc, ls, nq, nkv, scale, window)
    b_ = _ext.ops().decode_attention_batched(qkv, k1, v1, ls, nq, nkv, scale)
    assert torch.equal(a.view(torch.int16), b_.view(torch.int16))


# ------------------------------------------------------------------------------------------------ model
def _step(model, ids, labels, cu, ms, hip: bool, monkeypatch):
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    out = model(ids, labels=labels, cu_seqlens=cu, max_seqlen=ms, shift_labels=False)
    out.loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
    return out.loss.detach().float(), grads


@pytest.mark.parametrize("policy", ["full", "lora"])
def test_tiny_gpu_mistral_step_hip_vs_reference(policy, monkeypatch):
    """tiny-gpu-mistral (window 40) on a padding-free batch of ragged lengths, the HIP path against
    SFTAMD_DISABLE_HIP=1 on the same bf16 weights, at the bounds of
    test_qwen2_gpu.test_tiny_gpu_qwen2_step_hip_vs_reference (loss 2e-2, every gradient 5e-2)."""
    torch.manual_seed(0)
    cfg = get_config("tiny-gpu-mistral")
    assert cfg.sliding_window == 40
    m = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=1)
    if policy == "lora":
        apply_lora(m, LoRAConfig(r=8, lora_alpha=16, lora_dropout=0.0))
        with torch.no_grad():
            for n, p in m.named_parameters():
                if ".lora." in n and p.numel() > 0:
                    p.normal_(0.0, 0.05)
    lens = [130, 47, 79]
    cu = torch.tensor([0, 130, 177, 256], dtype=torch.int32, device=DEV)
    ids = torch.randint(0, cfg.vocab_size, (sum(lens),), device=DEV)
    labels = torch.cat([torch.cat([ids[s + 1:e], ids.new_tensor([-100])]) for s, e in zip(cu[:-1].tolist(), cu[1:].tolist())])
    l_hip, g_hip = _step(m, ids, labels, cu, max(lens), True, monkeypatch)
    l_ref, g_ref = _step(m, ids, labels, cu, max(lens), False, monkeypatch)
    assert abs(l_hip.item() - l_ref.item()) < 2e-2 * abs(l_ref.item())
    assert set(g_hip) == set(g_ref) and len(g_ref) == sum(p.requires_grad for p in m.parameters())
    for n in g_ref:
        e = (g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)
        print(f"tiny-gpu-mistral {policy} {n}: {e.item():.3e}")
        assert e < 5e-2, (n, e.item())


EMBED_GAIN = 3.0


@pytest.fixture(scope="module")
def gen_model():
    """tiny-gpu-mistral with random bf16 weights and a greedy decode that has one answer.

    Two greedy decodes in bf16 can only be asked for the same 48 tokens where the reference itself is decided: with
    plain random weights it is not (the top two logits of such a model are often closer than one bf16 step, 2^-8 of a
    logit near 1: its fp32 margins fall to 2e-4 within 48 steps and its bf16 and fp32 greedy outputs already differ),
    so the result would be a matter of rounding, not of the window. Here the token embeddings are 3 x larger and
    lm_head row perm[t] is token t's (unscaled) embedding, so the residual stream's own token speaks loudest: the next
    token is perm[current] with fp32 margins of 1 to 3 at logits of 3 to 4, 60 bf16 steps and more (measured on the
    reference path in fp32 on the CPU, on weights of the same construction, with no kernel involved). The layers still
    move every logit: taking the window away shifts the logits by 0.3 to 0.9, which
    test_decode_step_logits_feel_the_window holds against the paths' own difference."""
    m = build_model(get_config("tiny-gpu-mistral"), device=DEV, dtype=torch.bfloat16, seed=3)
    perm = torch.randperm(m.config.vocab_size, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        m.lm_head[perm] = m.model.embed_tokens
        m.model.embed_tokens.mul_(EMBED_GAIN)
    return m


def test_generate_past_the_window_equals_reference_path(gen_model, monkeypatch):
    """48 new tokens from a 21-token prompt: past the window of 40. Graph and no-graph decode equal the reference
    path's tokens."""
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(0, 1024, (21,), generator=g).tolist()
    kw = dict(max_new_tokens=48, do_sample=False, repetition_penalty=1.0)
    a = generate(gen_model, prompt, use_graph=True, **kw)
    b = generate(gen_model, prompt, use_graph=False, **kw)
    assert a == b and len(a) == 48 and len(set(a)) > 24  # (not one token over and over)
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "1")
    want = generate(gen_model, prompt, use_graph=False, **kw)
    assert a == want


def test_generate_batch_past_the_window_equals_reference_path(gen_model, monkeypatch):
    """generate_batch, graph and no-graph, equals generate row for row, and the reference path's tokens."""
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 1024, (n,), generator=g).tolist() for n in (37, 5, 66)]
    kw = dict(max_new_tokens=48, do_sample=False, repetition_penalty=1.0)
    a = generate_batch(gen_model, prompts, use_graph=True, **kw)
    b = generate_batch(gen_model, prompts, use_graph=False, **kw)
    assert a == b
    for i, p in enumerate(prompts):
        assert a[i] == generate(gen_model, p, **kw), i
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "1")
    for i, p in enumerate(prompts):
        assert a[i] == generate(gen_model, p, use_graph=False, **kw), i


def test_decode_step_logits_feel_the_window(gen_model, monkeypatch):
    """The tokens above are decided by wide margins, so they alone would not notice a decode path that dropped the
    window. One decode step at cache length 71 (70 tokens prefilled, window 40) on every path, as logits: the
    hipGraph decoder, the eager HIP decoder and the batched decoder (two rows, 70 and 55 tokens) against the
    reference path's eager step, and the reference path once more with the window taken away.

    Bound: the logits here are below 8 in magnitude, where bf16 values are 2^-5 apart; each path rounds its logits once
    (half a step each, one step between two paths) on top of what the bf16 hidden states carry, so two right paths
    agree to 4 steps = 0.125. The window's own effect has to exceed twice that, or the comparison could not tell."""
    from llm_fine_tune_distributed_amd.inference.generation import (BatchGraphDecoder, BatchKVCache, GraphDecoder,
                                                                    KVCache, forward_cached, prefill_batch)
    m = gen_model
    g = torch.Generator().manual_seed(2)
    seq = torch.randint(0, 1024, (71,), generator=g).tolist()
    short = torch.randint(0, 1024, (56,), generator=g).tolist()
    bound = 4 * 2.0 ** -5

    def single(hip, use_graph=False):
        monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
        cache = KVCache(m.config, 80, DEV)
        forward_cached(m, torch.tensor(seq[:70], device=DEV), cache, prefill=True)
        if not hip:
            return forward_cached(m, torch.tensor(seq[70:], device=DEV), cache, prefill=False).clone()
        return GraphDecoder(m, cache).step(seq[70], 70, use_graph=use_graph).clone()

    def batched(use_graph):
        monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0")
        cache = BatchKVCache(m.config, 2, 80, DEV)
        prefill_batch(m, [seq[:70], short[:55]], cache)
        return BatchGraphDecoder(m, cache).step([seq[70], short[55]], use_graph=use_graph).clone()

    want = single(False)
    assert want.abs().max() < 8
    windows = [l.self_attn.window for l in m.model.layers]
    try:
        for l in m.model.layers:
            l.self_attn.window = 0
        full = single(False)
    finally:
        for l, w in zip(m.model.layers, windows):
            l.self_attn.window = w
    effect = (full - want).abs().max().item()
    errs = {"eager": (single(True) - want).abs().max().item(),
            "graph": (single(True, True) - want).abs().max().item(),
            "batched": (batched(False)[0] - want).abs().max().item(),
            "batched graph": (batched(True)[0] - want).abs().max().item()}
    print(f"decode step logits: window effect {effect:.3f}, paths against the reference path {errs}, bound {bound:.3f}")
    assert effect > 2 * bound, effect
    for k, e in errs.items():
        assert e <= bound, (k, e)


# ------------------------------------------------------------------------------------------------ tile skipping
def test_window_skips_tiles():
    """One sequence of 8192 tokens, 16 q / 4 kv heads, forward + backward: window=512 takes less than half the time of
    window=0 (the unchanged kernels) in the same process. Per 128-query block the windowed kernels visit at most
    (512 + 128) / 64 + 1 = 11 key tiles against a causal mean of 64, about 6 x less tile work; one half leaves a factor
    3 for launch overhead and the delta / epilogue passes, which do not shrink. Median of 5 after a warm-up.

    Measured once on one MI355X: profiles/sliding_window.md."""
    nq, nkv, T = 16, 4, 8192
    cu = torch.tensor([0, T], dtype=torch.int32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn(T, (nq + 2 * nkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(T, nq * D, device=DEV, generator=g).to(torch.bfloat16)
    ops, scale = _ext.ops(), 1 / math.sqrt(D)

    def once(window):
        out, lse = ops.flash_fwd(qkv, cu, T, nq, nkv, D, scale, True, window)
        return ops.flash_bwd(dout, qkv, out, lse, cu, T, nq, nkv, D, scale, True, None, window)

    def timed(window):
        once(window)
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            once(window)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    t0, tw = timed(0), timed(512)
    print(f"sliding_window timing T={T} {nq}/{nkv} fwd+bwd: window=0 {t0:.3f} ms, window=512 {tw:.3f} ms, "
          f"ratio {tw / t0:.3f}")
    assert tw < 0.5 * t0, (tw, t0)
