"""The decode-time kernels at their edges (csrc/decode_attention.hip, csrc/sampler.hip).

Decode attention, single and batched: GQA ratios 1, 4 and 8 (MAXREP), lengths on both sides of every 256-key chunk
edge, NaN beyond the live length, each (sequence, head) on its own against fp64 with a bound of 2 x the fp32
emulation's error (tests/_rowwise.py), and bitwise agreement of the two entry points, which share split_body.

Sampler: the draw is a pure function of (seed, step), so the kernel's token log is compared with an exact torch twin
(_rowwise.sampler_twin) at every step; only steps where u lies within 1e-4 * kept of a cumulative boundary, or a rank's
mass-above within 1e-4 of top_p, are left out (native fp32 exp against fp64 may decide them otherwise), and their share
is asserted from the reference alone. Greedy decoding must return argmax, the LOWEST index, on exact ties."""
import math

import numpy as np
import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext

import _rowwise as rw
from _blockwise import assert_blocks_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
D = 128


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ decode attention
ALL_LENS = [1, 2, 255, 256, 257, 511, 512, 513, 600]


@pytest.mark.parametrize("S", [600, 512])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 1), (16, 2), (32, 8)])  # rep = 1, 8, 8, 4
def test_decode_attention_heads_and_lengths(nq, nkv, S):
    lens = [L for L in ALL_LENS if L <= S]
    B = len(lens)
    g = torch.Generator(device=DEV).manual_seed(nq * 1000 + S)
    qkv = torch.randn(B, (nq + 2 * nkv) * D, generator=g, device=DEV).to(BF16)
    kc = torch.randn(B, S, nkv, D, generator=g, device=DEV).to(BF16)
    vc = torch.randn(B, S, nkv, D, generator=g, device=DEV).to(BF16)
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
        worst = assert_blocks_close(out[b].view(nq, D), want, 1, D, bound, f"decode batched nq={nq} nkv={nkv} L={L}")
        figs.append((L, f"{worst:.2e}", f"{bound:.2e}"))
        # the single-sequence entry point on the same (appended) cache: the same split_body, the same bits
        one = _ext.ops().decode_attention(qkv[b, :nq * D].contiguous(), kc[b], vc[b], ln[b:b + 1], nq, nkv, scale)
        assert torch.equal(bits(one), bits(out[b])), (L, "single != batched")
    assert torch.equal(bits(kc), bits(k0)) and torch.equal(bits(vc), bits(v0))  # one row appended, nothing else
    print(f"\n[decode] attention nq={nq} nkv={nkv} S={S} (L, worst, bound): {figs}")


# ------------------------------------------------------------------------------------------------ sampler
K, T, RP, SEED, STEPS = 12, 0.7, 1.2, 1234, 400
HIST = [3, 17, 400]
HIST_B = [[3, 17, 400], [1, 2, 3, 4, 1999], [2047, 2048, 5, 6]]
MAX_SKIPPED = 0.03


def _presence(V, hists):
    words = np.zeros((len(hists), (V + 31) // 32), dtype=np.uint32)
    for b, h in enumerate(hists):
        for t in h:
            words[b, t >> 5] |= np.uint32(1 << (t & 31))
    return torch.from_numpy(words.view(np.int32).copy()).to(DEV)


def _compare(log, logits_cpu, hist, seed, P, what, k=K):
    toks, amb = rw.twin_run(logits_cpu, hist, seed, T, k, P, RP, forced=log)
    # the share of close calls, from the reference alone (the twin on its own history)
    _, amb_own = rw.twin_run(logits_cpu, hist, seed, T, k, P, RP)
    share = sum(amb_own) / len(amb_own)
    assert share <= MAX_SKIPPED and sum(amb) / len(amb) <= MAX_SKIPPED, (what, share)
    bad = [(t, log[t], toks[t]) for t in range(len(log)) if not amb[t] and log[t] != toks[t]]
    print(f"\n[decode] sampler {what}: {sum(amb)} of {len(amb)} steps too close to call ({sum(amb_own)} on the twin's "
          f"own history), {len(bad)} mismatches")
    assert not bad, (what, bad[:5])


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("P", [0.9, 1.0])
@pytest.mark.parametrize("V", [5000, 2048, 2049])
def test_sample_token_equals_the_twin(V, P, dtype):
    logits_cpu = rw.sampler_logits(STEPS, V, HIST, SEED).to(dtype)
    logits = logits_cpu.to(DEV)
    pres = _presence(V, [HIST])[0].contiguous()
    state = torch.zeros(4, dtype=torch.long, device=DEV)
    log = torch.full((STEPS,), -1, dtype=torch.long, device=DEV)
    for t in range(STEPS):
        _ext.ops().sample_token(logits[t], pres, state, None, None, None, log, T, K, P, RP, True, SEED)
    assert int(state[0]) == STEPS
    _compare(log.tolist(), logits_cpu, HIST, SEED, P, f"single V={V} P={P} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("V,k", [(50000, 12), (151936, 40)])
def test_sample_token_equals_the_twin_many_candidates(V, k, dtype):
    """25 tiles x 12 and 75 tiles x 40 candidates: more than the 256 threads of the merge block, so every thread of
    final_body holds several (the qwen3 vocabulary with the default top_k is the second case)."""
    assert -(-V // 2048) * k > 256
    steps = 300
    logits_cpu = rw.sampler_logits(steps, V, HIST, SEED).to(dtype)
    logits = logits_cpu.to(DEV)
    pres = _presence(V, [HIST])[0].contiguous()
    state = torch.zeros(4, dtype=torch.long, device=DEV)
    log = torch.full((steps,), -1, dtype=torch.long, device=DEV)
    for t in range(steps):
        _ext.ops().sample_token(logits[t], pres, state, None, None, None, log, T, k, 0.9, RP, True, SEED)
    _compare(log.tolist(), logits_cpu, HIST, SEED, 0.9, f"single V={V} K={k} {dtype}", k)


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("V,P", [(5000, 0.9), (2049, 1.0)])
def test_sample_tokens_rows_equal_the_twin(V, P, dtype):
    B = len(HIST_B)
    logits_cpu = rw.sampler_logits(STEPS, V, HIST_B, SEED, rows=B).to(dtype)
    logits = logits_cpu.to(DEV)
    pres = _presence(V, HIST_B)
    state = torch.zeros(B, 4, dtype=torch.long, device=DEV)
    log = torch.full((B, STEPS), -1, dtype=torch.long, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    for t in range(STEPS):
        _ext.ops().sample_tokens(logits[t], pres, state, None, None, None, log, done, -1, T, K, P, RP, True, SEED)
    assert int(done.sum()) == 0
    for b in range(B):  # row b draws with seed + b
        _compare(log[b].tolist(), logits_cpu[:, b], HIST_B[b], SEED + b, P, f"batched row {b} V={V} P={P} {dtype}")


# exact ties at the maximum: (index a, index b, penalised index or None). 4.0 is the maximum (everything else is
# clamped to 3); with the penalty 2.0 a history token at 8.0 becomes exactly 4.0 in fp32 and in bf16.
TIES = [(1, 256, None), (5, 2047, None), (7, 2048 + 3, None), (300, 9, 300), (9, 2048 + 300, 2048 + 300)]


def _tie_logits(V, a, b, pen_idx, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lg = (torch.randn(V, generator=g) * 1.0).clamp(max=3.0)
    lg[a] = lg[b] = 4.0
    if pen_idx is not None:
        lg[pen_idx] = 8.0
    return lg.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("a,b,pen_idx", TIES)
def test_greedy_ties_resolve_to_the_lowest_index(a, b, pen_idx, dtype):
    V, pen = 5000, 2.0
    hist = [pen_idx] if pen_idx is not None else []
    lg = _tie_logits(V, a, b, pen_idx, dtype, 7 + a)
    keys = rw.penalised_scaled(lg, rw.history_mask(V, hist) if hist else torch.zeros(V, dtype=torch.bool), 1.0, pen,
                               do_sample=False)
    assert keys[a] == keys[b] == keys.max() and int((keys == keys.max()).sum()) == 2
    want = int(keys.argmax())
    assert want == min(a, b)
    # single row
    pres = _presence(V, [hist])[0].contiguous()
    state = torch.zeros(4, dtype=torch.long, device=DEV)
    tok = torch.full((1,), -1, dtype=torch.long, device=DEV)
    _ext.ops().sample_token(lg.to(DEV), pres, state, tok, None, None, None, 1.0, 1, 1.0, pen, False, 0)
    assert int(tok) == want, ("sample_token", int(tok), want)
    # batched: the tie row between two rows without a tie
    other = _tie_logits(V, 11, 11, None, dtype, 99)
    rows = torch.stack([other, lg, other]).to(DEV)
    presb = _presence(V, [[], hist, []])
    stb = torch.zeros(3, 4, dtype=torch.long, device=DEV)
    tokb = torch.full((3,), -1, dtype=torch.long, device=DEV)
    done = torch.zeros(3, dtype=torch.int32, device=DEV)
    _ext.ops().sample_tokens(rows, presb, stb, tokb, None, None, None, done, -1, 1.0, 1, 1.0, pen, False, 0)
    assert tokb.tolist() == [11, want, 11], ("sample_tokens", tokb.tolist(), want)


def test_sample_token_refuses_top_k_above_the_vocabulary():
    V = 8
    lg = torch.zeros(V, device=DEV)
    pres = torch.zeros(1, dtype=torch.int32, device=DEV)
    state = torch.zeros(4, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match="top_k"):
        _ext.ops().sample_token(lg, pres, state, None, None, None, None, 1.0, 12, 1.0, 1.0, True, 0)
    assert state.tolist() == [0, 0, 0, 0]  # a host check: nothing ran
