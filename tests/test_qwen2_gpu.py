"""Qwen2 / Qwen2.5 on MI355X: the qkv bias + RoPE kernels (csrc/qkv_bias.hip) element by element against the fp32 /
fp64 reference, the existing attention kernels at the family's GQA ratios (7 and 8), a model step on tiny-gpu-qwen2
against the PyTorch reference path (trainable and frozen bias), the default path at Qwen2.5-7B widths against the fp32
reference model, and generation (hipGraph decode, batched decode)."""
import math

import pytest
import torch

import _rowwise as rw
from _blockwise import assert_blocks_close
from llm_fine_tune_distributed_amd.inference.generation import generate, generate_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora
from llm_fine_tune_distributed_amd.ops import _ext, fused
from llm_fine_tune_distributed_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

D = 128
# M: one row / less than one wave of rows / a ragged last step / several blocks. A launch has at most 1024 blocks over
# all heads, 32 tokens per block and step: at 28 + 2 x 4 heads that is 28 token blocks, so M = 900 (29 steps of 32) makes
# the first of them take a second grid-stride step.
MS = [1, 5, 67, 300]
HEADS = [(2, 1), (4, 2), (28, 4)]
CASES = [(M, nq, nkv) for M in MS for nq, nkv in HEADS] + [(900, 28, 4)]


def _inputs(M, nq, nkv, seed=0):
    """As test_qwen3_gpu._inputs (rows of different scale, positions up to 4000), with a bias N(0, 1) of which a few
    entries are scaled to +-50 (real Qwen2.5 key biases are large)."""
    g = torch.Generator(device="cuda").manual_seed(seed * 1000 + M * 10 + nq)
    nh3 = nq + 2 * nkv
    ld = nh3 * D
    scale = torch.empty(M, nh3, 1, device="cuda").uniform_(0.2, 4.0, generator=g)
    qkv = (torch.randn(M, nh3, D, device="cuda", generator=g) * scale).reshape(M, ld).bfloat16()
    bias = torch.randn(ld, device="cuda", generator=g)
    big = torch.randperm(ld, device="cuda", generator=g)[: 3 * nh3]  # about three per head, in q, k and v columns
    bias[big] = torch.where(bias[big] < 0, -50.0, 50.0)
    pos = torch.randint(0, 4001, (M,), device="cuda", generator=g)
    pos[-1] = 4000
    cos, sin = ref.rope_cos_sin(pos, D, 1e6)
    return qkv, bias.bfloat16(), cos.contiguous(), sin.contiguous()


def _assert_elements(got, want, nh, what):
    """|got - want| <= 2^-8 |want| + 1e-5 max|want over the head row|, every element (so every row and head): one
    bf16 rounding of an fp32 result plus fp32 reassociation (the bound of test_qwen3_gpu)."""
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


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()


@pytest.mark.parametrize("M,nq,nkv", CASES)
def test_qkv_bias_rope_fwd(M, nq, nkv):
    qkv, bias, cos, sin = _inputs(M, nq, nkv)
    nh = nq + nkv
    want = ref.qkv_bias_rope(qkv.float(), bias.float(), cos, sin, nq, nkv, D)  # fp32, unrounded
    out = qkv.clone()
    assert _ext.ops().qkv_bias_rope_fwd(out, bias, cos, sin, nq, nkv, D) is None
    _assert_elements(out[:, : nh * D], want[:, : nh * D], nh, "fwd q|k")
    v_want = (qkv[:, nh * D:].float() + bias[nh * D:].float()).bfloat16()
    assert torch.equal(_bits(out[:, nh * D:]), _bits(v_want))  # one fp32 add, one rounding: bit-identical


@pytest.mark.parametrize("M,nq,nkv", CASES)
def test_qkv_bias_rope_bwd(M, nq, nkv):
    qkv, bias, cos, sin = _inputs(M, nq, nkv, seed=1)
    nh = nq + nkv
    g = torch.Generator(device="cuda").manual_seed(M + nq)
    dy = torch.randn(qkv.shape, device="cuda", generator=g).bfloat16()
    # fp64 autograd of the reference on the same bf16 inputs
    x, b = (t.double().requires_grad_(True) for t in (qkv, bias))
    y = ref.qkv_bias_rope(x, b, cos.double(), sin.double(), nq, nkv, D)
    dx_ref, db_ref = torch.autograd.grad((y * dy.double()).sum(), (x, b))

    def run():
        d = dy.clone()
        return d, _ext.ops().qkv_bias_rope_bwd(d, cos, sin, nq, nkv, D)

    d1, db = run()
    assert torch.equal(_bits(d1[:, nh * D:]), _bits(dy[:, nh * D:]))  # V columns of dqkv untouched
    _assert_elements(d1[:, : nh * D], dx_ref[:, : nh * D], nh, "dx")
    assert db.dtype == torch.float32 and db.shape == ((nq + 2 * nkv) * D,)
    # fp32 sums over at most 900 rows, each column group against its own largest entry (test_qk_norm_rope_bwd's bound)
    for name, lo, hi in (("q", 0, nq * D), ("k", nq * D, nh * D), ("v", nh * D, (nh + nkv) * D)):
        err = (db[lo:hi].double() - db_ref[lo:hi]).abs().max().item()
        print(f"qkv_bias_rope_bwd M={M} {nq}+{nkv} dbias {name}: err {err:.3e} of max {db_ref[lo:hi].abs().max().item():.3e}")
        assert err <= 1e-4 * db_ref[lo:hi].abs().max().item(), (name, err, db_ref[lo:hi].abs().max().item())
    d2, db2 = run()
    assert torch.equal(_bits(d1), _bits(d2)) and torch.equal(db, db2)  # bit-identical


def test_qkv_bias_rope_empty_and_bad_shapes():
    qkv, bias, cos, sin = _inputs(4, 2, 1)
    e = qkv[:0]
    _ext.ops().qkv_bias_rope_fwd(e, bias, cos[:0], sin[:0], 2, 1, D)
    db = _ext.ops().qkv_bias_rope_bwd(e, cos[:0], sin[:0], 2, 1, D)
    assert db.shape == (4 * D,) and db.dtype == torch.float32 and not db.any()
    with pytest.raises(RuntimeError, match="head_dim"):
        _ext.ops().qkv_bias_rope_fwd(qkv.clone(), bias, cos, sin, 4, 2, 64)
    with pytest.raises(RuntimeError, match="head_dim"):
        _ext.ops().qkv_bias_rope_bwd(qkv.clone(), cos, sin, 4, 2, 64)
    with pytest.raises(RuntimeError, match="cos table"):
        _ext.ops().qkv_bias_rope_fwd(qkv.clone(), bias, cos[:2], sin[:2], 2, 1, D)
    with pytest.raises(RuntimeError, match="cos table"):
        _ext.ops().qkv_bias_rope_bwd(qkv.clone(), cos[:2], sin[:2], 2, 1, D)
    with pytest.raises(RuntimeError, match="bfloat16"):
        _ext.ops().qkv_bias_rope_fwd(qkv.clone(), bias.float(), cos, sin, 2, 1, D)
    with pytest.raises(RuntimeError, match="bias must be"):
        _ext.ops().qkv_bias_rope_fwd(qkv.clone(), bias[:-D], cos, sin, 2, 1, D)


# ------------------------------------------------------------------------------------------------ attention ratios
@pytest.mark.parametrize("nq,nkv", [(28, 4), (16, 2)])  # GQA ratios 7 (Qwen2.5-7B) and 8 (Qwen2.5-3B)
def test_flash_attention_at_qwen2_gqa_ratios(nq, nkv):
    """flash_fwd / flash_bwd per (sequence, head) against the fp64 reference, with the bounds of
    test_attention_blocks_gpu (2e-2 for out, 3e-2 for the gradients)."""
    lens = [1, 65, 130]
    g = torch.Generator(device="cuda").manual_seed(nq)
    cu = torch.tensor([0, 1, 66, 196], dtype=torch.int32, device="cuda")
    M, scale = 196, 1 / math.sqrt(D)
    qkv = torch.randn(M, (nq + 2 * nkv) * D, device="cuda", generator=g).bfloat16()
    dout = torch.randn(M, nq * D, device="cuda", generator=g).bfloat16()
    q64 = qkv.double().requires_grad_(True)
    o64 = ref.attention(q64, nq, nkv, D, cu, scale, True)
    (g64,) = torch.autograd.grad(o64, q64, dout.double())
    out, lse = _ext.ops().flash_fwd(qkv, cu, max(lens), nq, nkv, D, scale, True)
    assert_blocks_close(out, o64.detach(), 0, D, 2e-2, f"{nq}/{nkv} out", row_splits=cu.tolist())
    dqkv = _ext.ops().flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True)
    for name, lo, hi in (("dq", 0, nq * D), ("dk", nq * D, (nq + nkv) * D), ("dv", (nq + nkv) * D, (nq + 2 * nkv) * D)):
        assert_blocks_close(dqkv[:, lo:hi], g64[:, lo:hi], 0, D, 3e-2, f"{nq}/{nkv} {name}", row_splits=cu.tolist())


def test_decode_attention_batched_at_ratio_7():
    """decode_attention_batched at 28 q / 4 kv heads, B = 3, each (sequence, head) against fp64 with the bound of
    test_decode_edges_gpu (2 x the fp32 emulation's error)."""
    nq, nkv, S, lens = 28, 4, 300, [1, 257, 300]
    B = len(lens)
    g = torch.Generator(device="cuda").manual_seed(7)
    qkv = torch.randn(B, (nq + 2 * nkv) * D, generator=g, device="cuda").bfloat16()
    kc = torch.randn(B, S, nkv, D, generator=g, device="cuda").bfloat16()
    vc = torch.randn(B, S, nkv, D, generator=g, device="cuda").bfloat16()
    for b, L in enumerate(lens):
        kc[b, L - 1:] = float("nan")
        vc[b, L - 1:] = float("nan")
    k0, v0 = kc.clone(), vc.clone()
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    scale = 1 / math.sqrt(D)
    out = _ext.ops().decode_attention_batched(qkv, kc, vc, ln, nq, nkv, scale)
    knew = qkv[:, nq * D:(nq + nkv) * D].view(B, nkv, D)
    vnew = qkv[:, (nq + nkv) * D:].view(B, nkv, D)
    for b, L in enumerate(lens):
        k0[b, L - 1], v0[b, L - 1] = knew[b], vnew[b]
        want, em = rw.decode_refs(qkv[b, :nq * D].view(nq, D), k0[b, :L], v0[b, :L], scale)
        assert_blocks_close(out[b].view(nq, D), want, 1, D, rw.row_bound(em, want), f"decode 28/4 L={L}")
    assert torch.equal(_bits(kc), _bits(k0)) and torch.equal(_bits(vc), _bits(v0))  # one row appended, nothing else


# ------------------------------------------------------------------------------------------------ model step
def _trace():
    out = {}
    for item in _ext.ops().dispatch_trace_read().split(";"):
        if item:
            k, v = item.split("=")
            out[k] = int(v)
    return out


def _step(model, ids, labels, hip: bool, monkeypatch, trace=False):
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    tr = None
    if trace:
        _ext.ops().dispatch_trace(True)
    try:
        out = model(ids, labels=labels)
        out.loss.backward()
        torch.cuda.synchronize()
    finally:
        if trace:
            _ext.ops().dispatch_trace(False)
            tr = _trace()
    grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
    return out.loss.detach().float(), grads, tr


def _randomise_biases(m, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("qkv_bias"):
                p.copy_((0.5 * torch.randn(p.shape, generator=g)).to(p))


def _tiny_batch(cfg):
    ids = torch.randint(0, cfg.vocab_size, (4, 256), device="cuda")
    labels = ids.clone()
    labels[:, 200:] = -100
    return ids, labels


def test_tiny_gpu_qwen2_step_hip_vs_reference(monkeypatch):
    """The default HIP path against SFTAMD_DISABLE_HIP=1 on the same bf16 weights (the bounds of
    test_qwen3_gpu.test_tiny_gpu_qwen3_step_hip_vs_reference), and what the dispatch trace shows for a bias layer."""
    torch.manual_seed(0)
    cfg = get_config("tiny-gpu-qwen2")
    m = build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=1)
    _randomise_biases(m)
    ids, labels = _tiny_batch(cfg)
    l_hip, g_hip, tr = _step(m, ids, labels, True, monkeypatch, trace=True)
    L = cfg.num_hidden_layers
    assert tr.get("ew.qkv_bias_rope.fwd", 0) == L and tr.get("ew.qkv_bias_rope.bwd", 0) == L, tr
    assert tr.get("dgrad.c14.delta", 0) == L and "attn.delta_kernel" not in tr, tr
    assert not any(k.startswith("tn.rope") for k in tr) and "attn.bwd_rope_epi" not in tr, tr
    l_ref, g_ref, _ = _step(m, ids, labels, False, monkeypatch)
    assert abs(l_hip.item() - l_ref.item()) < 2e-2 * abs(l_ref.item())
    assert sum(n.endswith("qkv_bias") for n in g_ref) == L and set(g_hip) == set(g_ref)  # every bias has a gradient
    assert len(g_ref) == len(list(m.parameters()))
    for n in g_ref:
        e = (g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)
        print(f"tiny-gpu-qwen2 {n}: {e.item():.3e}")
        assert e < 5e-2, (n, e.item())


def test_frozen_bias_runs_the_plain_inverse_rope(monkeypatch):
    """With LoRA the biases are frozen: no column sums, the inverse rotation of the gradient runs on the plain RoPE
    kernel (which leaves no trace entry: its calls are counted at ops.fused._rope_inplace). What that route computes is
    checked element by element in test_qkv_bias_rope_autograd_routes; here, which kernels a LoRA step runs.

    No bound is put on the adapter gradients here. Measured once on MI355X with these shapes and biases N(0, 0.5), each
    path against an fp32 model on the reference path: the q / k adapters of the last layer are off by 1.3e-1 / 9.5e-2
    (A) and 1.4e-1 / 1.2e-1 (B) on the HIP path, 1.7e-2 .. 3.2e-2 on the bf16 PyTorch path; the v adapters agree
    (6e-3 both). With zero biases every qkv adapter agrees (HIP <= 1.7e-2, bf16 PyTorch <= 1.2e-2), as on tiny-gpu and
    tiny-gpu-qwen3. The deviation comes with a large common component in q and k, through flash_bwd (delta from the
    bf16-rounded attention output), not through the bias kernels: profiles/qwen2_default_path_errors.md."""
    torch.manual_seed(0)
    cfg = get_config("tiny-gpu-qwen2")
    m = build_model(cfg, device="cuda", dtype=torch.bfloat16, seed=1)
    _randomise_biases(m)
    apply_lora(m, LoRAConfig(r=8, lora_alpha=16, lora_dropout=0.0))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".lora." in n and p.numel() > 0:
                p.normal_(0.0, 0.05)
    ids, labels = _tiny_batch(cfg)
    calls = []
    plain = fused._rope_inplace

    def counted(qkv, cos, sin, n_q, n_kv, hd, inverse):
        calls.append((inverse, qkv.is_cuda))
        return plain(qkv, cos, sin, n_q, n_kv, hd, inverse)

    monkeypatch.setattr(fused, "_rope_inplace", counted)
    l_hip, g_hip, tr = _step(m, ids, labels, True, monkeypatch, trace=True)
    monkeypatch.setattr(fused, "_rope_inplace", plain)
    L = cfg.num_hidden_layers
    assert tr.get("ew.qkv_bias_rope.fwd", 0) == L and "ew.qkv_bias_rope.bwd" not in tr, tr
    assert calls == [(True, True)] * L, calls
    assert not any(n.endswith("qkv_bias") for n in g_hip)
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert set(g_hip) == trainable and all(".lora." in n for n in trainable)
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in g_hip.values())
    l_ref, _, _ = _step(m, ids, labels, False, monkeypatch)
    assert abs(l_hip.item() - l_ref.item()) < 2e-2 * abs(l_ref.item())


@pytest.mark.parametrize("trainable", [True, False])
def test_qkv_bias_rope_autograd_routes(trainable):
    """ops.qkv_bias_rope_ on the GPU through autograd: a trainable bias takes the bwd kernel (dbias in bias.grad), a
    frozen one the plain inverse RoPE kernel and no column sums; the input gradient is the same either way, element by
    element against fp64 autograd of the reference (the kernels' bounds)."""
    from llm_fine_tune_distributed_amd import ops
    M, nq, nkv = 67, 4, 2
    nh = nq + nkv
    qkv, bias, cos, sin = _inputs(M, nq, nkv, seed=2)
    g = torch.Generator(device="cuda").manual_seed(5)
    dy = torch.randn(qkv.shape, device="cuda", generator=g).bfloat16()
    x64, b64 = (t.double().requires_grad_(True) for t in (qkv, bias))
    y64 = ref.qkv_bias_rope(x64, b64, cos.double(), sin.double(), nq, nkv, D)
    dx_ref, db_ref = torch.autograd.grad((y64 * dy.double()).sum(), (x64, b64))
    x = qkv.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(trainable)
    _ext.ops().dispatch_trace(True)
    try:
        xc = x.clone()
        y = ops.qkv_bias_rope_(xc, b, cos, sin, nq, nkv, D)
        assert y is xc
        y.backward(dy.clone())
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
    tr = _trace()
    assert tr.get("ew.qkv_bias_rope.fwd", 0) == 1 and tr.get("ew.qkv_bias_rope.bwd", 0) == int(trainable), tr
    _assert_elements(y.detach()[:, : nh * D], y64.detach()[:, : nh * D], nh, "y")
    _assert_elements(x.grad[:, : nh * D], dx_ref[:, : nh * D], nh, "dx")
    assert torch.equal(_bits(x.grad[:, nh * D:]), _bits(dy[:, nh * D:]))
    if trainable:
        # the kernel's fp32 column sums (within 1e-4 max|want|, as in test_qkv_bias_rope_bwd) rounded once to the
        # bias's bf16: half a bf16 ulp is at most 2^-8 of the entry (8 significand bits)
        assert b.grad.dtype == torch.bfloat16
        lim = 2.0 ** -8 * db_ref.abs() + 1e-4 * db_ref.abs().max()
        assert ((b.grad.double() - db_ref).abs() <= lim).all(), ((b.grad.double() - db_ref).abs() - lim).max().item()
    else:
        assert b.grad is None


# ------------------------------------------------------------------------------------------------ real widths
# Relative gradient error of the qkv_bias vectors at these widths, measured on MI355X
# (profiles/qwen2_default_path_errors.md): the bf16 PyTorch reference path (bf16 model, SFTAMD_DISABLE_HIP=1) against
# the fp32 reference model on the same weights and batch. The HIP path is allowed twice that: it rounds in other places
# (the project's usual 2x margin).
QKV_BIAS_BF16_REFERENCE_ERR = 1.321e-2  # the largest of the four layers (layer 0)
QKV_BIAS_BOUND = 2 * QKV_BIAS_BF16_REFERENCE_ERR


def _qwen2_5_7b_cut():
    from llm_fine_tune_distributed_amd.models import qwen2_5_7b
    cfg = qwen2_5_7b()
    cfg.num_hidden_layers = 4
    cfg.no_rope_layers = cfg.no_rope_layers[:4]
    cfg.vocab_size = 8192
    cfg.bos_token_id, cfg.eos_token_id = 1, 2
    return cfg


def _build_with_random_biases(*a, **k):
    """build_model with the biases N(0, 0.5) instead of HF's zeros (seeded: the same in every model built)."""
    m = build_model(*a, **k)
    _randomise_biases(m)
    return m


def test_default_path_qwen2_5_7b_widths_vs_fp32_reference(monkeypatch):
    """Qwen2.5-7B at its real widths (hidden 3584, intermediate 18944, 28 q / 4 kv heads x 128, untied head), 4 layers,
    8192-token vocabulary, 16 x 512 tokens, random biases: the default dispatch and every gradient against the fp32
    reference model (the pattern of test_qwen3_gpu.test_default_path_qwen3_8b_widths_vs_fp32_reference)."""
    import test_default_path_gpu as dp
    monkeypatch.setattr(dp, "build_model", _build_with_random_biases)
    cfg = _qwen2_5_7b_cut()
    tr, loss, loss_r, errs, norm2, total_ref = dp._run_vs_reference(cfg, monkeypatch)
    dp._report("qwen2_5_7b", errs, tr)
    for n, e in errs.items():
        print(f"qwen2.5-7b widths {n}: {e:.3e}")
    assert tr.get("ew.qkv_bias_rope.fwd", 0) == 4 and tr.get("ew.qkv_bias_rope.bwd", 0) == 4, tr
    assert tr.get("attn.fwd32", 0) == 4 and tr.get("attn.dkdv32", 0) == 4 and tr.get("attn.dq32", 0) == 4, tr
    # the bias sits between the GEMM and the rotation: no RoPE GEMM epilogue, no inverse RoPE in the attention backward
    assert not any(k.startswith("tn.rope") for k in tr) and "attn.bwd_rope_epi" not in tr, tr
    assert tr.get("dgrad.c14.delta", 0) == 4 and "attn.delta_kernel" not in tr, tr  # o_proj + the attention delta
    assert abs(loss - loss_r) < 2e-2 * abs(loss_r)
    assert sum("qkv_bias" in n for n in errs) == 4
    dp._check_errors(errs, [("qkv_bias", QKV_BIAS_BOUND)] + dp.LLAMA_BOUNDS)
    assert abs(norm2 ** 0.5 - total_ref ** 0.5) < 3e-2 * total_ref ** 0.5


# ------------------------------------------------------------------------------------------------ generation
@pytest.fixture(scope="module")
def gen_model():
    m = build_model(get_config("tiny-gpu-qwen2"), device="cuda", dtype=torch.bfloat16, seed=3)
    _randomise_biases(m)
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
