"""Shared-prompt decode attention (the prefix / suffix kernels of csrc/decode_attention_d64.hip, reached through
decode_attention_batched with a prefix): every row against fp64 over its concatenated keys with the bound of
tests/test_decode_attention_d64_gpu.py, G * rep below, at and across the MFMA tile, prefix lengths on both sides of
the wave and the chunk, NaN wherever nothing may be read; rows independent of their group; the unshared path inside
the same bound; stale memory; rejections; rollout_batch(num_generations) and a GRPOTrainer step end to end."""
import functools
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import rollout_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext

import _rowwise as rw
from _blockwise import assert_blocks_close
from _stale import assert_fill_independent, bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
PLENS = [1, 63, 64, 65, 256, 257]   # one group each
PMAX, SOWN = 300, 70
OWN = (1, 17, 65)                   # row b's own length, the token being appended included
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


@functools.lru_cache(maxsize=None)
def _case(D, nq, nkv, G):
    """Inputs of one step (never modified: callers clone the caches) and per row (want64, bound) over its live keys."""
    g = torch.Generator(device=DEV).manual_seed(D + 100 * nq + G)
    n, B = len(PLENS), len(PLENS) * G

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device=DEV).to(BF16)
    qkv, pk, pv = rnd(B, (nq + 2 * nkv) * D), rnd(n, PMAX, nkv, D), rnd(n, PMAX, nkv, D)
    kc, vc = rnd(B, SOWN, nkv, D), rnd(B, SOWN, nkv, D)
    own = [OWN[b % 3] for b in range(B)]
    for i, P in enumerate(PLENS):
        pk[i, P:], pv[i, P:] = NAN, NAN
    for b in range(B):  # the append overwrites own row own - 1; nothing else at or past it may be read
        kc[b, own[b] - 1:], vc[b, own[b] - 1:] = NAN, NAN
    k1, v1 = kc.clone(), vc.clone()  # the caches after the step
    refs = []
    for b in range(B):
        k1[b, own[b] - 1] = qkv[b, nq * D:(nq + nkv) * D].view(nkv, D)
        v1[b, own[b] - 1] = qkv[b, (nq + nkv) * D:].view(nkv, D)
        P = PLENS[b // G]
        K, V = torch.cat([pk[b // G, :P], k1[b, :own[b]]]), torch.cat([pv[b // G, :P], v1[b, :own[b]]])
        want, em = rw.decode_refs(qkv[b, :nq * D].view(nq, D), K, V, 1 / math.sqrt(D))
        refs.append((want, rw.row_bound(em, want)))
    lens = torch.tensor([PLENS[b // G] + own[b] for b in range(B)], dtype=torch.int32, device=DEV)
    return qkv, kc, vc, lens, pk, pv, torch.tensor(PLENS, dtype=torch.int32, device=DEV), k1, v1, refs


def _run(qkv, kc, vc, lens, nq, nkv, D, *prefix):
    return _ext.ops().decode_attention_batched(qkv, kc, vc, lens, nq, nkv, 1 / math.sqrt(D), 0, *prefix)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nq,nkv,G", [(4, 4, 3), (8, 2, 4), (14, 2, 5), (32, 8, 8)])  # G * rep = 3, 16, 35, 32
def test_prefixed_step_against_fp64_and_the_unshared_path(D, nq, nkv, G):
    qkv, kc0, vc0, lens, pk, pv, pl, k1, v1, refs = _case(D, nq, nkv, G)
    kc, vc = kc0.clone(), vc0.clone()
    out = _run(qkv, kc, vc, lens, nq, nkv, D, pk, pv, pl, G)
    assert out.shape == (len(refs), nq * D) and out.dtype == BF16
    assert torch.equal(bits(kc), bits(k1)) and torch.equal(bits(vc), bits(v1))  # one row appended, nothing else
    # the parent's path: every row's prompt copied into its own slab
    ku = torch.full((len(refs), PMAX + SOWN, nkv, D), NAN, dtype=BF16, device=DEV)
    vu = ku.clone()
    for b in range(len(refs)):
        P, own = PLENS[b // G], OWN[b % 3]
        ku[b, :P], vu[b, :P] = pk[b // G, :P], pv[b // G, :P]
        ku[b, P:P + own - 1], vu[b, P:P + own - 1] = kc0[b, :own - 1], vc0[b, :own - 1]
    unshared = _run(qkv, ku, vu, lens, nq, nkv, D)
    figs = []
    for b, (want, bound) in enumerate(refs):
        what = f"D={D} nq={nq} nkv={nkv} G={G} row {b} (prefix {PLENS[b // G]}, own {OWN[b % 3]})"
        worst = assert_blocks_close(out[b].view(nq, D), want, 1, D, bound, "prefixed " + what)
        other = assert_blocks_close(unshared[b].view(nq, D), want, 1, D, bound, "unshared " + what)
        figs.append((worst / bound, other / bound))
    print(f"\n[decode prefix] D={D} nq={nq} nkv={nkv} G={G}: worst error / bound over the rows, prefixed "
          f"{max(f[0] for f in figs):.3f}, unshared {max(f[1] for f in figs):.3f}")


@pytest.mark.parametrize("D", [64, 128])
def test_rows_do_not_depend_on_their_group(D):
    nq, nkv, G = 14, 2, 5  # 35 columns: rows 2 and 4 straddle a column tile
    qkv, kc0, vc0, lens, pk, pv, pl, *_ = _case(D, nq, nkv, G)
    out = _run(qkv, kc0.clone(), vc0.clone(), lens, nq, nkv, D, pk, pv, pl, G)
    for b in range(qkv.shape[0]):
        i = b // G
        alone = _run(qkv[b:b + 1].clone(), kc0[b:b + 1].clone(), vc0[b:b + 1].clone(), lens[b:b + 1].clone(), nq, nkv,
                     D, pk[i:i + 1].clone(), pv[i:i + 1].clone(), pl[i:i + 1].clone(), 1)
        assert torch.equal(bits(alone[0]), bits(out[b])), (b, "G = 1 differs")
    for r in range(G):  # row r of every group among NaN neighbours
        keep = torch.arange(qkv.shape[0], device=DEV) % G == r
        q2, k2, v2 = (torch.where(keep.view(-1, *[1] * (t.dim() - 1)), t, torch.full_like(t, NAN))
                      for t in (qkv, kc0, vc0))
        got = _run(q2, k2, v2, lens, nq, nkv, D, pk, pv, pl, G)
        assert torch.equal(bits(got[keep]), bits(out[keep])), (r, "NaN neighbours differ")


def test_prefixed_step_fill_independent():
    D, nq, nkv, G = 128, 14, 2, 5
    qkv, kc0, vc0, lens, pk, pv, pl, k1, v1, refs = _case(D, nq, nkv, G)
    kc, vc = kc0.clone(), vc0.clone()
    out, _, _ = assert_fill_independent(lambda: (_run(qkv, kc, vc, lens, nq, nkv, D, pk, pv, pl, G), kc, vc),
                                        "decode_attention_batched with a prefix", col_block=D)
    assert_blocks_close(out[7].view(nq, D), refs[7][0], 1, D, refs[7][1], "prefixed under the NaN fill")


def test_rejections_and_the_unprefixed_call():
    D, nq, nkv, G = 64, 8, 2, 4
    qkv, kc0, vc0, lens, pk, pv, pl, *_ = _case(D, nq, nkv, G)
    kc, vc = kc0.clone(), vc0.clone()
    op, s = _ext.ops().decode_attention_batched, 1 / math.sqrt(D)
    for match, args in [("window", (8, pk, pv, pl, G)), ("multiple of group", (0, pk, pv, pl, 5)),
                        ("go together", (0, pk, None, pl, G)), ("go together", (0, None, None, pl, G)),
                        ("needs a prefix", (0, None, None, None, G)), ("bfloat16", (0, pk.float(), pv.float(), pl, G)),
                        ("kv heads", (0, pk[:, :, :1].contiguous(), pv[:, :, :1].contiguous(), pl, G)),
                        ("kv heads", (0, pk[..., :32].contiguous(), pv[..., :32].contiguous(), pl, G)),
                        ("contiguous", (0, pk[:, ::2], pv[:, ::2], pl, G)),
                        ("aligned", (0, pk.flatten()[4:4 + pk[:, 1:].numel()].view(6, PMAX - 1, nkv, D), pv[:, 1:]
                                     .contiguous(), pl, G))]:
        with pytest.raises(RuntimeError, match="decode_attention_batched.*" + match):
            op(qkv, kc, vc, lens, nq, nkv, s, *args)
    assert torch.equal(bits(kc), bits(kc0))  # a rejected call wrote nothing
    # without a prefix nothing changed: the old positional call, the defaults spelled out, and the single-sequence op
    own = torch.tensor([OWN[b % 3] for b in range(qkv.shape[0])], dtype=torch.int32, device=DEV)
    a = op(qkv, kc0.clone(), vc0.clone(), own, nq, nkv, s)
    b_ = op(qkv, kc, vc, own, nq, nkv, s, 0, None, None, None, 1)
    assert torch.equal(bits(a), bits(b_))
    for r in range(qkv.shape[0]):
        one = _ext.ops().decode_attention(qkv[r, :nq * D].contiguous(), kc[r], vc[r], own[r:r + 1], nq, nkv, s)
        assert torch.equal(bits(one), bits(a[r]))


# ----------------------------------------------------------------------------- end to end
def _logp_gap(m, rows, toks, lps, tau):
    """max |sampler log-probability - training-path log-probability| over the drawn tokens of ``rows[b] + toks[b]``."""
    seqs = [p + t for p, t in zip(rows, toks)]
    ids = torch.tensor([x for s in seqs for x in s], device=DEV)
    cu = torch.tensor([0] + [len(s) for s in seqs], device=DEV).cumsum(0).int()
    labels = torch.tensor([x for p, t in zip(rows, toks) for x in [-100] * (len(p) - 1) + t + [-100]], device=DEV)
    samp = torch.tensor([x for p, lp in zip(rows, lps) for x in [0.0] * (len(p) - 1) + lp + [0.0]], device=DEV)
    with torch.no_grad():
        train = m.token_logps(ids, labels, cu_seqlens=cu, max_seqlen=max(len(s) for s in seqs), shift_labels=False,
                              position_ids=torch.cat([torch.arange(len(s), device=DEV) for s in seqs]), temperature=tau)
    return (samp.double() - train.double()).abs()[labels >= 0].max().item()


@pytest.mark.parametrize("preset", ["tiny-gpu", "tiny-gpu-d64"])
def test_rollouts_share_the_prompt(preset, tmp_path):
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer
    cfg = get_config(preset)
    m = build_model(cfg, device=DEV, dtype=BF16, seed=5)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (37, 5, 250)]
    G, N, tau = 3, 16, 0.9
    rows = [p for p in prompts for _ in range(G)]
    kw = dict(max_new_tokens=N, eos_token_id=None, temperature=tau, seed=21)
    _ext.ops().dispatch_trace(True)
    try:
        toks, lps = rollout_batch(m, prompts, num_generations=G, **kw)
    finally:
        _ext.ops().dispatch_trace(False)
    assert "decode.prefix=" in _ext.ops().dispatch_trace_read()
    assert [len(t) for t in toks] == [N] * 9 and [len(x) for x in lps] == [N] * 9
    assert (toks, lps) == rollout_batch(m, prompts, num_generations=G, use_graph=False, **kw)
    t0, l0 = rollout_batch(m, rows, **kw)  # the unshared path on the same seeds: rows of a group differ, as there
    assert len({tuple(t) for t in toks[:G]}) > 1 and len({tuple(t) for t in t0[:G]}) > 1
    m.eval()
    shared, unshared = _logp_gap(m, rows, toks, lps, tau), _logp_gap(m, rows, t0, l0, tau)
    print(f"\n[shared prompt] {preset}: sampler vs training path, shared {shared:.3e}, unshared {unshared:.3e}")
    assert unshared > 0 and shared <= 2 * unshared
    diff = {}
    for on in (False, True):
        mt = build_model(cfg, device=DEV, dtype=BF16, seed=0)
        a = GRPOConfig(output_dir=str(tmp_path / str(on)), per_device_train_batch_size=2 * G, num_generations=G,
                       max_completion_length=N, temperature=tau, max_steps=1, learning_rate=1e-4, logging_steps=1,
                       lr_scheduler_type="constant", jsonl_log=False, save_strategy="no", rollout_shared_prompt=on)
        t = GRPOTrainer(model=mt, reward_funcs=lambda completion_ids, **_: [float(len(set(c))) for c in completion_ids],
                        args=a, train_dataset=[{"prompt_ids": p} for p in prompts[:2]])
        t.train()
        diff[on] = [h for h in t.state.log_history if "loss" in h][0]["sampling/logp_difference"]
    print(f"[shared prompt] {preset}: trainer sampling/logp_difference shared {diff[True]:.3e}, unshared {diff[False]:.3e}")
    assert diff[False] > 0 and diff[True] <= 2 * diff[False]
