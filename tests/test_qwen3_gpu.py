"""Qwen3 on MI355X: the per-head QK RMSNorm + RoPE kernels (csrc/qk_norm.hip) element by element against the fp32 /
fp64 reference, a model step on tiny-gpu-qwen3 against the PyTorch reference path, the default path at Qwen3-8B widths
against the fp32 reference model, and generation (hipGraph decode, batched decode)."""
import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import generate, generate_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

D = 128
EPS = 1e-6
# M: one row / less than one wave of rows / a ragged last wave / several blocks. The kernels run at most 1024 blocks of
# 32 head rows and grid-stride beyond that: (900, 32, 8) = 36000 head rows makes some blocks take a second step.
MS = [1, 5, 67, 300]
HEADS = [(2, 1), (4, 2), (32, 8)]
CASES = [(M, nq, nkv) for M in MS for nq, nkv in HEADS] + [(900, 32, 8)]


def _inputs(M, nq, nkv, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed * 1000 + M * 10 + nq)
    ld = (nq + 2 * nkv) * D
    # rows of different scale (rstd differs per head row), weights random around 1, positions up to 4000
    scale = torch.empty(M, nq + 2 * nkv, 1, device="cuda").uniform_(0.2, 4.0, generator=g)
    qkv = (torch.randn(M, nq + 2 * nkv, D, device="cuda", generator=g) * scale).reshape(M, ld).bfloat16()
    qw = (1 + 0.25 * torch.randn(D, device="cuda", generator=g)).bfloat16()
    kw = (1 + 0.25 * torch.randn(D, device="cuda", generator=g)).bfloat16()
    pos = torch.randint(0, 4001, (M,), device="cuda", generator=g)
    pos[-1] = 4000
    cos, sin = ref.rope_cos_sin(pos, D, 1e6)
    return qkv, qw, kw, cos.contiguous(), sin.contiguous()


def _assert_elements(got, want, nh, what):
    """|got - want| <= 2^-8 |want| + 1e-5 max|want over the head row|, every element (so every row and head): one
    bf16 rounding of an fp32 result plus fp32 reassociation."""
    M = got.shape[0]
    g = got.double().view(M, nh, D)
    w = want.double().view(M, nh, D)
    lim = 2.0 ** -8 * w.abs() + 1e-5 * w.abs().amax(-1, keepdim=True)
    bad = (g - w).abs() > lim
    if bad.any():
        m, h, i = [int(t[0]) for t in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound, first at token {m} head {h} col {i}: "
                             f"{g[m, h, i].item()} vs {w[m, h, i].item()}")


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("M,nq,nkv", CASES)
def test_qk_norm_rope_fwd(M, nq, nkv):
    assert _ext.load(), _ext.load_error()
    qkv, qw, kw, cos, sin = _inputs(M, nq, nkv)
    nh = nq + nkv
    want = ref.qk_norm_rope(qkv.float(), qw.float(), kw.float(), cos, sin, nq, nkv, D, EPS)  # fp32, unrounded
    out = qkv.clone()
    raw = _ext.ops().qk_norm_rope_fwd(out, qw, kw, cos, sin, nq, nkv, D, EPS, True)
    assert raw.shape == (M, nh * D) and raw.dtype == torch.bfloat16
    assert torch.equal(_bits(raw), _bits(qkv[:, : nh * D]))  # the copy for the backward
    assert torch.equal(_bits(out[:, nh * D:]), _bits(qkv[:, nh * D:]))  # V untouched
    _assert_elements(out[:, : nh * D], want[:, : nh * D], nh, "fwd")
    # the no-copy form (generation): same values, nothing returned
    out2 = qkv.clone()
    none = _ext.ops().qk_norm_rope_fwd(out2, qw, kw, cos, sin, nq, nkv, D, EPS, False)
    assert none.numel() == 0 and torch.equal(_bits(out2), _bits(out))


@pytest.mark.parametrize("M,nq,nkv", CASES)
def test_qk_norm_rope_bwd(M, nq, nkv):
    assert _ext.load(), _ext.load_error()
    qkv, qw, kw, cos, sin = _inputs(M, nq, nkv, seed=1)
    nh = nq + nkv
    g = torch.Generator(device="cuda").manual_seed(M + nq)
    dy = torch.randn(qkv.shape, device="cuda", generator=g).bfloat16()
    # fp64 autograd of the reference on the same bf16 inputs
    x, a, b = (t.double().requires_grad_(True) for t in (qkv, qw, kw))
    y = ref.qk_norm_rope(x, a, b, cos.double(), sin.double(), nq, nkv, D, EPS)
    dx_ref, dqw_ref, dkw_ref = torch.autograd.grad((y * dy.double()).sum(), (x, a, b))

    raw = qkv[:, : nh * D].contiguous()

    def run():
        d = dy.clone()
        dqw, dkw = _ext.ops().qk_norm_rope_bwd(d, raw, qw, kw, cos, sin, nq, nkv, D, EPS)
        return d, dqw, dkw

    d1, dqw, dkw = run()
    assert torch.equal(_bits(d1[:, nh * D:]), _bits(dy[:, nh * D:]))  # V columns of dqkv untouched
    _assert_elements(d1[:, : nh * D], dx_ref[:, : nh * D], nh, "dx")
    assert dqw.dtype == torch.float32 and dqw.shape == (D,) and dkw.shape == (D,)
    # fp32 partials over at most 12,000 rows (36,000 in the grid-stride case)
    for got, want, name in ((dqw, dqw_ref, "dq_weight"), (dkw, dkw_ref, "dk_weight")):
        err = (got.double() - want).abs().max().item()
        assert err <= 1e-4 * want.abs().max().item(), (name, err, want.abs().max().item())
    d2, dqw2, dkw2 = run()
    assert torch.equal(_bits(d1), _bits(d2)) and torch.equal(dqw, dqw2) and torch.equal(dkw, dkw2)  # bit-identical


def test_qk_norm_rope_empty_and_bad_shapes():
    assert _ext.load(), _ext.load_error()
    qkv, qw, kw, cos, sin = _inputs(4, 2, 1)
    e = qkv[:0]
    raw = _ext.ops().qk_norm_rope_fwd(e, qw, kw, cos[:0], sin[:0], 2, 1, D, EPS, True)
    assert raw.shape == (0, 3 * D)
    dqw, dkw = _ext.ops().qk_norm_rope_bwd(e, raw, qw, kw, cos[:0], sin[:0], 2, 1, D, EPS)
    assert not dqw.any() and not dkw.any()
    with pytest.raises(RuntimeError, match="head_dim"):
        _ext.ops().qk_norm_rope_fwd(qkv.clone(), qw, kw, cos, sin, 4, 2, 64, EPS, True)
    with pytest.raises(RuntimeError, match="cos table"):
        _ext.ops().qk_norm_rope_fwd(qkv.clone(), qw, kw, cos[:2], sin[:2], 2, 1, D, EPS, True)
    with pytest.raises(RuntimeError, match="bfloat16"):
        _ext.ops().qk_norm_rope_fwd(qkv.clone(), qw.float(), kw, cos, sin, 2, 1, D, EPS, True)


# ------------------------------------------------------------------------------------------------ model step
def _trace():
    out = {}
    for item in _ext.ops().dispatch_trace_read().split(";"):
        if item:
            k, v = item.split("=")
            out[k] = int(v)
    return out


def _step(model, ids, labels, hip: bool, monkeypatch):
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    out = model(ids, labels=labels)
    out.loss.backward()
    return out.loss.detach().float(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}


def _randomise_qk_norms(m, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.copy_((1.0 + 0.2 * torch.randn(p.shape, generator=g)).to(p))


def test_tiny_gpu_qwen3_step_hip_vs_reference(monkeypatch):
    """The default HIP path against SFTAMD_DISABLE_HIP=1 on the same bf16 weights (the bounds of
    test_model_gpu.test_model_hip_vs_reference), and what the dispatch trace shows for a qk-norm layer."""
    assert _ext.load(), _ext.load_error()
    torch.manual_seed(0)
    cfg = get_config("tiny-gpu-qwen3")
    m = build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=1)
    _randomise_qk_norms(m)
    ids = torch.randint(0, cfg.vocab_size, (4, 256), device="cuda")
    labels = ids.clone()
    labels[:, 200:] = -100
    _ext.ops().dispatch_trace(True)
    try:
        l_hip, g_hip = _step(m, ids, labels, True, monkeypatch)
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
    tr = _trace()
    L = cfg.num_hidden_layers
    assert tr.get("ew.qk_norm_rope.fwd", 0) == L and tr.get("ew.qk_norm_rope.bwd", 0) == L, tr
    assert tr.get("dgrad.c14.delta", 0) == L and "attn.delta_kernel" not in tr, tr
    assert not any(k.startswith("tn.rope") for k in tr) and "attn.bwd_rope_epi" not in tr, tr
    l_ref, g_ref = _step(m, ids, labels, False, monkeypatch)
    assert abs(l_hip.item() - l_ref.item()) < 2e-2 * abs(l_ref.item())
    assert sum("q_norm" in n or "k_norm" in n for n in g_ref) == 2 * L
    for n in g_ref:
        e = (g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)
        print(f"tiny-gpu-qwen3 {n}: {e.item():.3e}")
        assert e < 5e-2, (n, e.item())


# ------------------------------------------------------------------------------------------------ real widths
# Relative gradient error of the q_norm / k_norm weights at these widths, measured on MI355X
# (profiles/qwen3_default_path_errors.md): the bf16 PyTorch reference path (bf16 model, SFTAMD_DISABLE_HIP=1)
# against the fp32 reference model on the same weights and batch. The HIP path is allowed twice that: it rounds in
# other places (the project's usual 2x margin).
QK_NORM_BF16_REFERENCE_ERR = 2.997e-2  # the larger of q_norm (2.997e-2, layer 3) and k_norm (2.955e-2, layer 3)
QK_NORM_BOUND = 2 * QK_NORM_BF16_REFERENCE_ERR  # (the HIP path measured 3.119e-2 / 3.173e-2)


def _qwen3_8b_cut():
    from llm_fine_tune_distributed_amd.models import qwen3_8b
    cfg = qwen3_8b()
    cfg.num_hidden_layers = 4
    cfg.no_rope_layers = cfg.no_rope_layers[:4]
    cfg.vocab_size = 8192
    cfg.bos_token_id, cfg.eos_token_id = 1, 2
    return cfg


def test_default_path_qwen3_8b_widths_vs_fp32_reference(monkeypatch):
    """Qwen3-8B at its real widths (hidden 4096, intermediate 12288, 32 q / 8 kv heads x 128, untied head), 4 layers,
    8192-token vocabulary, 16 x 512 tokens: the default dispatch and every gradient against the fp32 reference model
    (the pattern of test_default_path_gpu.test_default_path_llama3_8b_widths_vs_fp32_reference)."""
    from test_default_path_gpu import LLAMA_BOUNDS, _check_errors, _report, _run_vs_reference
    cfg = _qwen3_8b_cut()
    tr, loss, loss_r, errs, norm2, total_ref = _run_vs_reference(cfg, monkeypatch)
    _report("qwen3_8b", errs, tr)
    for n, e in errs.items():
        print(f"qwen3-8b widths {n}: {e:.3e}")
    assert tr.get("ew.qk_norm_rope.fwd", 0) == 4 and tr.get("ew.qk_norm_rope.bwd", 0) == 4, tr
    assert tr.get("attn.fwd32", 0) == 4 and tr.get("attn.dkdv32", 0) == 4 and tr.get("attn.dq32", 0) == 4, tr
    # the norm sits between the GEMM and the rotation: no RoPE GEMM epilogue, no inverse RoPE in the attention backward
    assert not any(k.startswith("tn.rope") for k in tr) and "attn.bwd_rope_epi" not in tr, tr
    assert tr.get("dgrad.c14.delta", 0) == 4 and "attn.delta_kernel" not in tr, tr  # o_proj + the attention delta
    assert abs(loss - loss_r) < 2e-2 * abs(loss_r)
    assert sum("q_norm" in n or "k_norm" in n for n in errs) == 8
    _check_errors(errs, [("q_norm", QK_NORM_BOUND), ("k_norm", QK_NORM_BOUND)] + LLAMA_BOUNDS)
    assert abs(norm2 ** 0.5 - total_ref ** 0.5) < 3e-2 * total_ref ** 0.5


# ------------------------------------------------------------------------------------------------ generation
@pytest.fixture(scope="module")
def gen_model():
    m = build_model(get_config("tiny-gpu-qwen3"), device="cuda", dtype=torch.bfloat16, seed=3)
    _randomise_qk_norms(m)
    return m


def test_graph_generate_greedy_equals_reference_path(gen_model, monkeypatch):
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(0, 1024, (37,), generator=g).tolist()
    kw = dict(max_new_tokens=8, do_sample=False, repetition_penalty=1.0)
    a = generate(gen_model, prompt, use_graph=True, **kw)
    b = generate(gen_model, prompt, use_graph=False, **kw)
    assert a == b
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "1")
    want = generate(gen_model, prompt, use_graph=False, **kw)
    assert a == want


def test_generate_batch_rows_equal_generate(gen_model):
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 1024, (n,), generator=g).tolist() for n in (37, 5, 21)]
    kw = dict(max_new_tokens=8)
    got = generate_batch(gen_model, prompts, seed=7, **kw)
    for b, p in enumerate(prompts):
        assert got[b] == generate(gen_model, p, seed=7 + b, **kw), b
