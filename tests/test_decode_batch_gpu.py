"""Batched decode on MI355X: the batched split-K decode attention (append + per-sequence lengths), the batched
fused sampler (row b == the single-row sampler with seed + b, finished rows frozen), generate_batch against
generate, and the batched decoder's logits against the single-sequence decoder under teacher forcing."""
import math

import numpy as np
import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import (BatchGraphDecoder, BatchKVCache, GraphDecoder,
                                                                KVCache, forward_cached, generate, generate_batch,
                                                                prefill_batch)
from llm_fine_tune_distributed_amd.models import build_model, tiny
from llm_fine_tune_distributed_amd.ops import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------- attention op
@pytest.mark.parametrize("nq,nkv", [(4, 2), (16, 4)])
def test_decode_attention_batched(nq, nkv):
    torch.manual_seed(0)
    D, B, S = 128, 4, 600  # three 256-key chunks, the last one partial
    lens = [1, 256, 257, 600]
    qkv = torch.randn(B, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    kc = torch.randn(B, S, nkv, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn(B, S, nkv, D, device=DEV, dtype=torch.bfloat16)
    for b, L in enumerate(lens):  # the append must overwrite row L - 1, nothing may read at or past it otherwise
        kc[b, L - 1:] = float("nan")
        vc[b, L - 1:] = float("nan")
    k0, v0 = kc.clone(), vc.clone()
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out = _ext.ops().decode_attention_batched(qkv, kc, vc, ln, nq, nkv, 1 / math.sqrt(D))
    assert out.shape == (B, nq * D) and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    knew = qkv[:, nq * D:(nq + nkv) * D].view(B, nkv, D)
    vnew = qkv[:, (nq + nkv) * D:].view(B, nkv, D)
    for b, L in enumerate(lens):
        K = torch.cat([k0[b, :L - 1], knew[b][None]]).float()
        V = torch.cat([v0[b, :L - 1], vnew[b][None]]).float()
        qf = qkv[b, :nq * D].float().view(nkv, nq // nkv, D)
        att = torch.einsum("grd,sgd->grs", qf, K) / math.sqrt(D)
        ref_o = torch.einsum("grs,sgd->grd", att.softmax(-1), V).reshape(-1)
        assert rel_err(out[b], ref_o) < 1e-2, (b, L)  # per sequence: one wrong sequence must not hide in the batch
        assert torch.equal(bits(kc[b, L - 1]), bits(knew[b])) and torch.equal(bits(vc[b, L - 1]), bits(vnew[b]))
        k0[b, L - 1], v0[b, L - 1] = knew[b], vnew[b]
    # every other cache element bitwise unchanged (NaN compared as bit patterns)
    assert torch.equal(bits(kc), bits(k0)) and torch.equal(bits(vc), bits(v0))


def test_decode_attention_batched_skips_bad_lengths():
    """A length outside (0, S_max] must not become a write: the row is skipped and the caches stay as they are."""
    torch.manual_seed(0)
    D, B, S, nq, nkv = 128, 3, 40, 4, 2
    qkv = torch.randn(B, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    kc = torch.randn(B, S, nkv, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    k0, v0 = kc.clone(), vc.clone()
    ln = torch.tensor([0, S + 1, -3], dtype=torch.int32, device=DEV)
    out = _ext.ops().decode_attention_batched(qkv, kc, vc, ln, nq, nkv, 1 / math.sqrt(D))
    assert torch.equal(bits(kc), bits(k0)) and torch.equal(bits(vc), bits(v0))
    assert torch.isfinite(out.float()).all()


# ----------------------------------------------------------------------------- sampler
V, B, K, T, P, RP = 5000, 3, 12, 0.7, 0.9, 1.2  # three 2048-logit tiles, the last one partial
HIST = [[3, 17, 400], [1, 2, 3, 4, 4999], [2048, 2049, 4095, 4096]]


def _presence():
    words = np.zeros((B, (V + 31) // 32), dtype=np.uint32)
    for b, h in enumerate(HIST):
        for t in h:
            words[b, t >> 5] |= np.uint32(1 << (t & 31))
    return torch.from_numpy(words.view(np.int32).copy()).cuda()


def _batch_state(cap):
    return dict(presence=_presence(), state=torch.zeros(B, 4, dtype=torch.long, device=DEV),
                tok=torch.zeros(B, dtype=torch.long, device=DEV), pos=torch.zeros(B, dtype=torch.long, device=DEV),
                len=torch.ones(B, dtype=torch.int32, device=DEV),
                log=torch.full((B, cap), -1, dtype=torch.long, device=DEV),
                done=torch.zeros(B, dtype=torch.int32, device=DEV))


def _sample_batch(logits, s, eos=-1, do_sample=True, seed=1234):
    _ext.ops().sample_tokens(logits, s["presence"], s["state"], s["tok"], s["pos"], s["len"], s["log"], s["done"], eos,
                             T, K, P, RP, do_sample, seed)


def _penalised(logits):
    lg = logits.float().clone()
    for b, h in enumerate(HIST):
        idx = torch.tensor(h, device=DEV)
        sc = lg[b, idx]
        lg[b, idx] = torch.where(sc < 0, sc * RP, sc / RP)
    return lg


def test_sample_tokens_rows_match_single_sampler():
    torch.manual_seed(0)
    steps, seed = 50, 1234
    logits = torch.randn(steps, B, V, device=DEV) * 2
    for b, h in enumerate(HIST):
        logits[:, b, h] += 3.0  # make the penalised tokens competitive
    s = _batch_state(steps)
    for t in range(steps):
        _sample_batch(logits[t], s, seed=seed)
    pres = _presence()
    for b in range(B):
        p1 = pres[b].clone()
        st = torch.zeros(4, dtype=torch.long, device=DEV)
        tok, pos = torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV)
        ln = torch.ones(1, dtype=torch.int32, device=DEV)
        log = torch.full((steps,), -1, dtype=torch.long, device=DEV)
        for t in range(steps):
            _ext.ops().sample_token(logits[t, b].contiguous(), p1, st, tok, pos, ln, log, T, K, P, RP, True, seed + b)
        assert torch.equal(s["log"][b], log), b
        assert torch.equal(s["state"][b], st) and torch.equal(s["presence"][b], p1)
        assert int(s["tok"][b]) == int(tok) and int(s["pos"][b]) == int(pos) and int(s["len"][b]) == int(ln)
    assert len({tuple(r) for r in s["log"].tolist()}) == B  # the rows are different streams
    assert int(s["done"].sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sample_tokens_greedy_is_penalised_argmax(dtype):
    torch.manual_seed(1)
    logits = (torch.randn(B, V, device=DEV) * 2).to(dtype)
    for b, h in enumerate(HIST):
        logits[b, h] += 6.0
    s = _batch_state(4)
    _sample_batch(logits, s, do_sample=False)
    assert s["tok"].tolist() == _penalised(logits).argmax(-1).tolist()
    assert s["log"][:, 0].tolist() == s["tok"].tolist() and s["state"][:, 0].tolist() == [1] * B


def test_sample_tokens_done_row_is_frozen_and_eos_sets_done():
    torch.manual_seed(2)
    logits = torch.randn(B, V, device=DEV) * 2
    want = _penalised(logits).argmax(-1).tolist()
    assert len(set(want)) == B
    s = _batch_state(4)
    s["done"][1] = 1
    s["tok"][1], s["pos"][1], s["len"][1] = 77, 5, 6
    s["state"][1] = torch.tensor([2, 77, 5, 6], device=DEV)
    s["log"][1, :2] = torch.tensor([9, 77], device=DEV)
    before = {k: v.clone() for k, v in s.items()}
    _sample_batch(logits, s, eos=want[0], do_sample=False)
    for k in ("tok", "pos", "len", "state", "presence", "log", "done"):  # the finished row writes nothing
        assert torch.equal(s[k][1], before[k][1]), k
    # row 0 drew the EOS: logged, flagged, and it stops advancing; row 2 goes on
    assert s["done"].tolist() == [1, 1, 0]
    assert int(s["log"][0, 0]) == want[0] and int(s["tok"][0]) == want[0] and int(s["state"][0, 0]) == 1
    assert int(s["pos"][0]) == int(before["pos"][0]) and int(s["len"][0]) == int(before["len"][0])
    assert int(s["tok"][2]) == want[2] and int(s["pos"][2]) == 1 and int(s["len"][2]) == 2
    # the next step leaves the row that drew EOS untouched as well
    mid = {k: v.clone() for k, v in s.items()}
    _sample_batch(torch.randn(B, V, device=DEV), s, eos=want[0], do_sample=False)
    for k in ("tok", "pos", "len", "state", "presence", "log", "done"):
        assert torch.equal(s[k][:2], mid[k][:2]), k
    assert int(s["state"][2, 0]) == 2


# ----------------------------------------------------------------------------- end to end
NEW = 16


@pytest.fixture(scope="module")
def model():
    cfg = tiny(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=1024,
               vocab_size=1024, num_hidden_layers=2)
    return build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=5)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(0, 1024, (n,), generator=g).tolist() for n in (37, 5, 250)]  # 250 + 16 crosses a chunk


@pytest.mark.parametrize("rp", [1.0, 1.3])
def test_batch_of_one_equals_generate_greedy(model, prompts, rp):
    for p in prompts:
        kw = dict(max_new_tokens=NEW, do_sample=False, repetition_penalty=rp)
        assert generate_batch(model, [p], **kw) == [generate(model, p, **kw)]


def test_batch_of_one_equals_generate_sampled(model, prompts):
    for p in prompts:
        kw = dict(max_new_tokens=NEW, seed=7)
        assert generate_batch(model, [p], **kw) == [generate(model, p, **kw)]


def test_duplicate_prompt_and_graph_vs_eager(model, prompts):
    ps = prompts + [prompts[0]]
    kw = dict(max_new_tokens=NEW, do_sample=False, repetition_penalty=1.3)
    a = generate_batch(model, ps, use_graph=True, **kw)
    b = generate_batch(model, ps, use_graph=False, **kw)
    assert a[0] == a[-1]  # cross-sequence indexing errors break this
    assert a == b
    assert all(len(o) == NEW for o in a)
    host = generate_batch(model, ps, device_sampling=False, **kw)  # host sampling over the same decoder
    assert host == a


def test_eos_stops_one_sequence_only(model, prompts):
    kw = dict(max_new_tokens=NEW, do_sample=False, repetition_penalty=1.3)
    free = generate_batch(model, prompts, **kw)
    eos = free[0][5]
    out = generate_batch(model, prompts, eos_token_id=eos, **kw)
    assert len(out[0]) < NEW and out[0][-1] == eos
    for o, f in zip(out, free):
        assert o == (f[:f.index(eos) + 1] if eos in f else f)


def test_batched_logits_teacher_forced(model, prompts):
    """8 forced tokens per sequence through BatchGraphDecoder.step and through one GraphDecoder per sequence, both
    against an fp32 CPU full forward of the same weights. The batched path may use another GEMM kernel (M = 3
    instead of M = 1) at the same bf16 rounding points: its error per sequence is held to 2x the single decoder's."""
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
        d1 = GraphDecoder(model, c1)
        single = []
        for t in range(n):
            single.append(d1.step(int(forced[b, t]), c1.len).clone())
            c1.len += 1
        single = torch.stack(single).cpu()
        with torch.no_grad():
            full = ref_m(torch.tensor(p + forced[b].tolist())[None], return_logits=True).logits.float()
        want = full.reshape(-1, full.shape[-1])[len(p):len(p) + n]
        e_single = (single - want).abs().max().item()
        e_batch = (got[b] - want).abs().max().item()
        print(f"seq {b} (prompt {len(p)}): max |logit err| single {e_single:.5f} batched {e_batch:.5f}")
        assert e_batch <= 2 * e_single, (b, e_batch, e_single)
