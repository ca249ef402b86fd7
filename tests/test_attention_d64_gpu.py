"""The head_dim-64 attention kernels (csrc/attention_d64.hip) per (sequence, head) against the fp64 reference with
autograd, at the bounds tests/test_attention_blocks_gpu.py holds the head_dim-128 kernels to (out 2e-2, dq / dk / dv
3e-2: fp32 accumulation with P, dS and the outputs each rounded once to bf16, at any head_dim). The kernels' tile edges
are 32 (a wave's queries or keys) and 64 (a key / query tile) and the workgroup's 128-query span at GQA rep 1: the
lengths stand at each edge - 1, the edge and the edge + 1."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close, assert_exact, traced

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 64
SCALE = 1 / math.sqrt(D)
OUT_BOUND, GRAD_BOUND = 2e-2, 3e-2

# name: (lens, nq, nkv, spare rows past cu[-1])
CASES = {"edges_gqa4": ([1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257], 8, 2, 0),
         "mha": ([300, 17, 129], 4, 4, 0),
         "rep3": ([200, 65], 12, 4, 0),
         "llama1b": ([512, 511, 7], 32, 8, 0),  # several key tiles per query: the online rescale runs
         "rep8_spare": ([96, 40], 16, 2, 8)}


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()


def _inputs(lens, nq, nkv, spare, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    M = int(cu[-1]) + spare
    qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(M, nq * D, device=DEV, generator=g).to(torch.bfloat16)
    return cu, qkv, dout


def _rope_tables(lens, M):
    pos = torch.cat([torch.arange(l) for l in lens] + [torch.zeros(M - sum(lens))]).to(DEV).double()
    ang = pos[:, None] / (10000 ** (torch.arange(0, D // 2, device=DEV).double() / (D // 2)))[None]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_fwd_bwd_per_sequence_and_head(name, causal):
    lens, nq, nkv, spare = CASES[name]
    cu, qkv, dout = _inputs(lens, nq, nkv, spare, 2 * list(CASES).index(name) + int(causal) + 1)
    T, cul, ops = int(cu[-1]), cu.tolist(), _ext.ops()
    q64 = qkv[:T].double().requires_grad_(True)
    o64 = ref.attention(q64, nq, nkv, D, cu, SCALE, causal)
    (g64,) = torch.autograd.grad(o64, q64, dout[:T].double())
    out, lse = ops.flash_fwd(qkv, cu, max(lens), nq, nkv, D, SCALE, causal)
    dqkv = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, SCALE, causal)
    what = f"{name} causal={causal}"
    worst = {"out": assert_blocks_close(out[:T], o64.detach(), 0, D, OUT_BOUND, f"{what} out", row_splits=cul)}
    for n, lo, hi in (("dq", 0, nq), ("dk", nq, nq + nkv), ("dv", nq + nkv, nq + 2 * nkv)):
        worst[n] = assert_blocks_close(dqkv[:T, lo * D:hi * D], g64[:, lo * D:hi * D], 0, D, GRAD_BOUND, f"{what} {n}",
                                       row_splits=cul)
    print(f"attention_d64 {what}: worst (sequence, head) block " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    # lse = logsumexp of the scaled, masked scores, per sequence and head
    q = qkv[:T, :nq * D].double().view(T, nq, D)
    k = qkv[:T, nq * D:(nq + nkv) * D].double().view(T, nkv, D).repeat_interleave(nq // nkv, 1)
    for s, e in zip(cul[:-1], cul[1:]):
        sc = torch.einsum("qhd,khd->hqk", q[s:e], k[s:e]) * SCALE
        if causal:
            sc = sc.masked_fill(torch.ones(e - s, e - s, device=DEV).triu(1).bool(), -math.inf)
        torch.testing.assert_close(lse[:, s:e].double(), sc.logsumexp(-1), atol=2e-3, rtol=1e-3)


def test_precomputed_delta_is_used_as_given():
    """flash_bwd given delta = sum_d dout.float() * out.float() == flash_bwd computing it, bit for bit. fp32 addition is
    not associative, so the sum is taken in the delta kernel's order: a lane's 8 elements in turn, then the xor tree
    over the row's 8 lanes (4, 2, 1); the products of two bf16 are exact in fp32."""
    lens, nq, nkv = [300, 17, 129, 1], 8, 2
    cu, qkv, dout = _inputs(lens, nq, nkv, 0, 9)
    ops = _ext.ops()
    out, lse = ops.flash_fwd(qkv, cu, max(lens), nq, nkv, D, SCALE, True)
    p = (dout.float() * out.float()).view(-1, nq, 8, 8)
    s = p[..., 0]
    for i in range(1, 8):
        s = s + p[..., i]
    s = s[..., :4] + s[..., 4:]
    s = s[..., :2] + s[..., 2:]
    delta = (s[..., 0] + s[..., 1]).t().contiguous()
    want = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, SCALE, True)
    got = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, SCALE, True, delta)
    assert_exact(got, want, "flash_bwd with delta")
    # ... and a different delta gives a different dq: the argument is read
    other = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, SCALE, True, delta + 1.0)
    assert not torch.equal(other[:, :nq * D], want[:, :nq * D])


@pytest.mark.parametrize("causal", [True, False])
def test_flash_bwd_rope_is_backward_then_inverse_rope(causal):
    lens, nq, nkv = [130, 65, 31], 6, 2
    cu, qkv, dout = _inputs(lens, nq, nkv, 0, 11)
    cos, sin = _rope_tables(lens, qkv.shape[0])
    ops = _ext.ops()
    out, lse = ops.flash_fwd(qkv, cu, max(lens), nq, nkv, D, SCALE, causal)
    want = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, SCALE, causal)
    ops.rope_(want, cos, sin, nq, nkv, D, True)
    got = ops.flash_bwd_rope(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, SCALE, causal, cos, sin)
    assert_exact(got, want, "flash_bwd_rope")


def test_deferred_rescale_row():
    """The forward rescales O / l only when a row's max grows by more than 2^8: key 200 (the fourth key tile) raises
    the score of query 300 of head 0 by ~21 in log2 (20 |q|^2 / 8 ~ 14 nats) over everything before it."""
    torch.manual_seed(1)
    nq, nkv, T = 4, 2, 384
    cu = torch.tensor([0, T], dtype=torch.int32, device=DEV)
    qkv = (0.3 * torch.randn(T, (nq + 2 * nkv) * D, device=DEV)).to(torch.bfloat16)
    qkv[200, nq * D:(nq + 1) * D] = (20.0 * qkv[300, :D].float()).to(torch.bfloat16)
    out, _ = _ext.ops().flash_fwd(qkv, cu, T, nq, nkv, D, SCALE, True)
    o64 = ref.attention(qkv.double(), nq, nkv, D, cu, SCALE, True)
    assert_blocks_close(out[300:301, :D], o64[300:301, :D], 1, D, OUT_BOUND, "the spiked query row")
    assert_blocks_close(out, o64, 64, D, OUT_BOUND, "deferred rescale")


def _step(model, ids, labels, cu, ms, hip, monkeypatch):
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    out = model(ids, labels=labels, cu_seqlens=cu, max_seqlen=ms, shift_labels=False)
    out.loss.backward()
    return out.loss.detach().float(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()
                                       if p.grad is not None}


@pytest.mark.parametrize("policy", ["full", "lora"])
def test_tiny_gpu_d64_step_hip_vs_reference(policy, monkeypatch):
    """tiny-gpu-d64 on a padding-free batch of three ragged sequences: the HIP path against SFTAMD_DISABLE_HIP=1 on the
    same bf16 weights at the bounds of tests/test_model_gpu.py (loss 2e-2, every gradient 5e-2), and the dispatch trace
    shows the head_dim-64 kernels."""
    torch.manual_seed(0)
    cfg = get_config("tiny-gpu-d64")
    assert (cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads) == (64, 4, 2)
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
    with traced() as box:
        l_hip, g_hip = _step(m, ids, labels, cu, max(lens), True, monkeypatch)
    for name in ("attn.fwd_d64", "attn.delta_d64", "attn.dkdv_d64", "attn.dq_d64"):
        assert int(box.get(name, 0)) == cfg.num_hidden_layers, (name, box)
    l_ref, g_ref = _step(m, ids, labels, cu, max(lens), False, monkeypatch)
    assert abs(l_hip.item() - l_ref.item()) < 2e-2 * abs(l_ref.item())
    assert set(g_hip) == set(g_ref) and len(g_ref) == sum(p.requires_grad for p in m.parameters())
    for n in g_ref:
        e = (g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)
        assert e < 5e-2, (policy, n, e.item())


@pytest.mark.parametrize("hd,window,msg", [(64, 8, "window"), (32, 0, "head_dim 128 and 64")])
def test_rejections(hd, window, msg):
    cu = torch.tensor([0, 40], dtype=torch.int32, device=DEV)
    qkv = torch.randn(40, 4 * hd, device=DEV).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match=msg):
        _ext.ops().flash_fwd(qkv, cu, 40, 2, 1, hd, 1 / math.sqrt(hd), True, window)
