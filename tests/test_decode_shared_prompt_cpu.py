"""The eager side of shared-prompt decoding: ops.decode_attention_batched with a prefix against the same step with
every prompt copied into its row's slab, and rollout_batch(num_generations) against the prompts repeated."""
import pytest
import torch

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.inference.generation import rollout_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config


def test_eager_prefixed_step_equals_the_copied_prompt():
    D, nq, nkv, G, P, S = 16, 4, 2, 3, 9, 6
    g = torch.Generator().manual_seed(0)
    plens, own = [4, 9], [1, 3, 5, 2, 1, 6]
    qkv = torch.randn(2 * G, (nq + 2 * nkv) * D, generator=g)
    pk, pv = torch.randn(2, P, nkv, D, generator=g), torch.randn(2, P, nkv, D, generator=g)
    kc, vc = torch.randn(2 * G, S, nkv, D, generator=g), torch.randn(2 * G, S, nkv, D, generator=g)
    ku, vu = torch.zeros(2 * G, P + S, nkv, D), torch.zeros(2 * G, P + S, nkv, D)
    for b in range(2 * G):
        p = plens[b // G]
        ku[b, :p], vu[b, :p] = pk[b // G, :p], pv[b // G, :p]
        ku[b, p:p + S], vu[b, p:p + S] = kc[b], vc[b]
    lens = torch.tensor([plens[b // G] + own[b] for b in range(2 * G)], dtype=torch.int32)
    lens[4] = plens[1]  # own = 0: no append, the prefix alone
    want = ops.decode_attention_batched(qkv, ku, vu, lens, nq, nkv)
    k0 = kc.clone()
    got = ops.decode_attention_batched(qkv, kc, vc, lens, nq, nkv, prefix_k=pk, prefix_v=pv,
                                       prefix_lens=torch.tensor(plens, dtype=torch.int32), group=G)
    assert torch.equal(kc[4], k0[4]) and torch.equal(kc[1, 2], qkv[1, nq * D:(nq + nkv) * D].view(nkv, D))
    rows = [b for b in range(2 * G) if b != 4]  # (the copied-prompt call appends row 4's K/V over its last prompt row)
    torch.testing.assert_close(got[rows], want[rows], rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="go together"):
        ops.decode_attention_batched(qkv, kc, vc, lens, nq, nkv, prefix_k=pk, group=G)
    with pytest.raises(ValueError, match="window"):
        ops.decode_attention_batched(qkv, kc, vc, lens, nq, nkv, window=4, prefix_k=pk, prefix_v=pv,
                                     prefix_lens=torch.tensor(plens, dtype=torch.int32), group=G)


def test_rollout_num_generations_repeats_the_prompts_off_the_hip_path():
    m = build_model(get_config("tiny"), device="cpu", dtype=torch.float32, seed=1)
    prompts = [[5, 9, 11], [7, 3]]
    kw = dict(max_new_tokens=5, eos_token_id=None, temperature=0.8, seed=3)
    toks, lps = rollout_batch(m, prompts, num_generations=2, **kw)
    assert (toks, lps) == rollout_batch(m, [prompts[0]] * 2 + [prompts[1]] * 2, **kw) and len(toks) == 4
