"""Decode attention at head_dim 64 (csrc/decode_attention_d64.hip): the kernel per (sequence, head) against fp64 with
the bound of tests/test_decode_edges_gpu.py (2 x the fp32 emulation's own error), lengths on both sides of the MFMA
tile (16 / 32), the wave (64) and the chunk (256), NaN at and past the live length; bad lengths and rejections;
generate / generate_batch / rollout_batch of tiny-gpu-d64 on the graph decoder, its logits against an fp32 forward."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import (BatchGraphDecoder, BatchKVCache, KVCache,
                                                                forward_cached, generate, generate_batch,
                                                                prefill_batch, rollout_batch)
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext

import _rowwise as rw
from _blockwise import assert_blocks_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
D = 64
ALL_LENS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513, 600]
NEW = 16


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(B, S, nq, nkv, seed, d=D):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(B, (nq + 2 * nkv) * d, generator=g, device=DEV).to(BF16)
    kc = torch.randn(B, S, nkv, d, generator=g, device=DEV).to(BF16)
    vc = torch.randn(B, S, nkv, d, generator=g, device=DEV).to(BF16)
    return qkv, kc, vc


@pytest.mark.parametrize("S", [600, 512])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (14, 2), (8, 1), (32, 8)])  # rep = 1, 7, 8, 4
def test_decode_attention_d64_heads_and_lengths(nq, nkv, S):
    lens = [L for L in ALL_LENS if L <= S]
    B = len(lens)
    qkv, kc, vc = _inputs(B, S, nq, nkv, nq * 1000 + S)
    for b, L in enumerate(lens):  # the append overwrites row L - 1; nothing else at or past it may be read
        kc[b, L - 1:] = float("nan")
        vc[b, L - 1:] = float("nan")
    k0, v0 = kc.clone(), vc.clone()
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(D)
    out = _ext.ops().decode_attention_batched(qkv, kc, vc, ln, nq, nkv, scale)
    assert out.shape == (B, nq * D) and out.dtype == BF16
    knew = qkv[:, nq * D:(nq + nkv) * D].view(B, nkv, D)
    vnew = qkv[:, (nq + nkv) * D:].view(B, nkv, D)
    figs = []
    for b, L in enumerate(lens):
        k0[b, L - 1], v0[b, L - 1] = knew[b], vnew[b]
        q = qkv[b, :nq * D].view(nq, D)
        want, em = rw.decode_refs(q, k0[b, :L], v0[b, :L], scale)
        bound = rw.row_bound(em, want)  # per head, against this sequence's own magnitude
        worst = assert_blocks_close(out[b].view(nq, D), want, 1, D, bound, f"decode d64 nq={nq} nkv={nkv} L={L}")
        figs.append((L, f"{worst:.2e}", f"{bound:.2e}"))
        one = _ext.ops().decode_attention(qkv[b, :nq * D].contiguous(), kc[b], vc[b], ln[b:b + 1], nq, nkv, scale)
        assert torch.equal(bits(one), bits(out[b])), (L, "single != batched")
    assert torch.equal(bits(kc), bits(k0)) and torch.equal(bits(vc), bits(v0))  # one row appended, nothing else
    print(f"\n[decode d64] nq={nq} nkv={nkv} S={S} (L, worst, bound): {figs}")


def test_decode_attention_d64_bad_lengths_and_rejections():
    S, nq, nkv = 40, 4, 2
    scale = 1 / math.sqrt(D)
    qkv, kc, vc = _inputs(4, S, nq, nkv, 3)
    k0, v0 = kc.clone(), vc.clone()
    ln = torch.tensor([0, S + 1, -3, 5], dtype=torch.int32, device=DEV)
    out = _ext.ops().decode_attention_batched(qkv, kc, vc, ln, nq, nkv, scale)
    k0[3, 4], v0[3, 4] = qkv[3, nq * D:(nq + nkv) * D].view(nkv, D), qkv[3, (nq + nkv) * D:].view(nkv, D)
    assert torch.equal(bits(kc), bits(k0)) and torch.equal(bits(vc), bits(v0))  # the bad rows wrote nothing
    assert not out[:3].float().any()
    want, em = rw.decode_refs(qkv[3, :nq * D].view(nq, D), k0[3, :5], v0[3, :5], scale)
    assert_blocks_close(out[3].view(nq, D), want, 1, D, rw.row_bound(em, want), "decode d64 beside bad rows")
    with pytest.raises(RuntimeError, match="window"):
        _ext.ops().decode_attention_batched(qkv, kc, vc, ln, nq, nkv, scale, 8)
    q32, k32, v32 = _inputs(4, S, nq, nkv, 3, d=32)
    with pytest.raises(RuntimeError, match="64 and 128"):
        _ext.ops().decode_attention_batched(q32, k32, v32, ln, nq, nkv, scale)


# ----------------------------------------------------------------------------- end to end on tiny-gpu-d64
@pytest.fixture(scope="module")
def model():
    return build_model(get_config("tiny-gpu-d64"), device="cuda", dtype=BF16, seed=5)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(0, 1024, (n,), generator=g).tolist() for n in (37, 5, 250)]  # 250 + 16 crosses a chunk


def test_d64_generate_batch_equals_generate_and_graph_equals_eager(model, prompts):
    kw = dict(max_new_tokens=NEW, do_sample=False)
    for p in prompts:
        assert generate_batch(model, [p], **kw) == [generate(model, p, **kw)]
    ps = prompts + [prompts[0]]
    a = generate_batch(model, ps, use_graph=True, **kw)
    assert a == generate_batch(model, ps, use_graph=False, **kw)
    assert a[0] == a[-1] and all(len(o) == NEW for o in a)


def test_d64_batched_logits_teacher_forced(model, prompts):
    """8 forced tokens per sequence through BatchGraphDecoder.step and through the eager decode of forward_cached, both
    against an fp32 CPU forward: they round at the same bf16 points outside attention, so 2 x the eager error holds."""
    cfg = model.config
    n = 8
    g = torch.Generator().manual_seed(1)
    forced = torch.randint(0, 1024, (len(prompts), n), generator=g)
    ref_m = build_model(cfg, device="cpu", dtype=torch.float32, seed=5)
    ref_m.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    ref_m.eval()
    cache = BatchKVCache(cfg, len(prompts), max(len(p) for p in prompts) + n + 1, DEV)
    prefill_batch(model, prompts, cache)
    dec = BatchGraphDecoder(model, cache)
    got = torch.stack([dec.step(forced[:, t].tolist()).clone() for t in range(n)], 1).cpu()  # [B, n, V]
    assert cache.lens == [len(p) + n for p in prompts]
    for b, p in enumerate(prompts):
        c1 = KVCache(cfg, len(p) + n + 1, DEV)
        forward_cached(model, torch.tensor(p, device=DEV), c1, prefill=True)
        eager = torch.stack([forward_cached(model, forced[b, t:t + 1].to(DEV), c1, prefill=False)
                             for t in range(n)]).cpu()
        with torch.no_grad():
            full = ref_m(torch.tensor(p + forced[b].tolist())[None], return_logits=True).logits.float()
        want = full.reshape(-1, full.shape[-1])[len(p):len(p) + n]
        e_eager = (eager - want).abs().max().item()
        e_hip = (got[b] - want).abs().max().item()
        print(f"seq {b} (prompt {len(p)}): max |logit err| eager {e_eager:.5f} graph decoder {e_hip:.5f}")
        assert e_hip <= 2 * e_eager, (b, e_hip, e_eager)


def test_d64_rollouts_take_the_device_path(model, prompts):
    _ext.ops().dispatch_trace(True)
    try:
        toks, lps = rollout_batch(model, prompts, NEW, None, temperature=0.9, top_k=0, seed=21)
    finally:
        _ext.ops().dispatch_trace(False)
    assert "decode.d64=" in _ext.ops().dispatch_trace_read()
    assert [len(t) for t in toks] == [NEW] * 3 and [len(x) for x in lps] == [NEW] * 3
    assert all(math.isfinite(x) and x <= 0 for row in lps for x in row)
    assert (toks, lps) == rollout_batch(model, prompts, NEW, None, temperature=0.9, top_k=0, seed=21, use_graph=False)
