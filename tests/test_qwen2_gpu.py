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

    The adapter gradients are judged stage by stage in test_lora_bias_layer_backward_stage_by_stage. Measured on MI355X
    with these shapes and biases N(0, 0.5), each path against an fp32 model on the reference path: the q / k adapters
    of the last layer are off by 1.3e-1 / 9.5e-2 (A) and 1.4e-1 / 1.2e-1 (B) on the HIP path, 1.7e-2 .. 3.2e-2 on the
    bf16 PyTorch path; the v adapters agree (6e-3 both); with zero biases every qkv adapter agrees (HIP <= 1.7e-2).
    Attribution, measured per stage on the captured tensors: flash_bwd alone accounts for 2.6e-1 / 1.2e-1 (A) and
    1.4e-1 / 1.1e-1 (B) of the last layer's q / k adapter gradients and for 4e-3 or less with the exact delta handed
    over; the inverse RoPE for 2e-3 and the LoRA backward for 4e-3 at most. flash_bwd is within 2 x the emulation of its
    own arithmetic: the deviation is the cost of delta = rowsum(dO . bf16 O) under a common component of v, q and k,
    not a defect of a kernel: profiles/attention_common_mode.md, profiles/qwen2_default_path_errors.md."""
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


def _capture_attention_stages(m, ids, labels, monkeypatch):
    """One HIP step of ``m`` with the tensors around every layer's attention node recorded (clones; forward order):
    per layer the qkv entering FlashAttnFn, its out, the dout and dqkv of its backward, the delta handed over, the
    gradient before / after the plain inverse RoPE with its tables, and the X / dy / adapters / returned gradients of
    the qkv projection's wide LoRA backward."""
    cfg = m.config
    wide_n = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim
    attn, deltas, ropes, loras = [], [], [], []
    apply0, take0, rope0, lora0 = fused.FlashAttnFn.apply, fused._take_delta, fused._rope_inplace, fused._lora_wide_bwd

    def attn_apply(qkv, cu, max_seqlen, n_q, n_kv, hd, scale, causal, link=None):
        rec = dict(qkv=qkv.detach().clone(), cu=cu, args=(cu, max_seqlen, n_q, n_kv, hd, scale, causal))
        qkv.register_hook(lambda g: rec.__setitem__("dqkv", g.detach().clone()))
        out = apply0(qkv, cu, max_seqlen, n_q, n_kv, hd, scale, causal, link)
        rec["out"] = out.detach().clone()
        out.register_hook(lambda g: rec.__setitem__("dout", g.detach().clone()))
        attn.append(rec)
        return out

    def take(*a):
        d = take0(*a)
        deltas.append(None if d is None else d.detach().clone())
        return d

    def rope(qkv, cos, sin, n_q, n_kv, hd, inverse):
        pre = qkv.detach().clone()
        r = rope0(qkv, cos, sin, n_q, n_kv, hd, inverse)
        ropes.append(dict(inverse=inverse, pre=pre, post=qkv.detach().clone(), cos=cos, sin=sin))
        return r

    def lora_bwd(X, acat, wide, ab, state, dy2d, need_dx, gu=None):
        res = lora0(X, acat, wide, ab, state, dy2d, need_dx, gu)
        if dy2d.shape[1] == wide_n and gu is None:
            loras.append(dict(X=X.detach().clone(), dy=dy2d.detach().clone(), state=state,
                              ab=[t.detach().clone() for t in ab], dAs=res[1], dBs=res[2]))
        return res

    monkeypatch.setattr(fused.FlashAttnFn, "apply", attn_apply)
    monkeypatch.setattr(fused, "_take_delta", take)
    monkeypatch.setattr(fused, "_rope_inplace", rope)
    monkeypatch.setattr(fused, "_lora_wide_bwd", lora_bwd)
    try:
        _, grads, _ = _step(m, ids, labels, True, monkeypatch)
    finally:
        monkeypatch.setattr(fused.FlashAttnFn, "apply", apply0)
        monkeypatch.setattr(fused, "_take_delta", take0)
        monkeypatch.setattr(fused, "_rope_inplace", rope0)
        monkeypatch.setattr(fused, "_lora_wide_bwd", lora0)
    L = cfg.num_hidden_layers
    assert len(attn) == len(deltas) == len(ropes) == len(loras) == L, (len(attn), len(deltas), len(ropes), len(loras))
    # the backward visits the layers last to first
    return [dict(attn=attn[i], delta=deltas[L - 1 - i], rope=ropes[L - 1 - i], lora=loras[L - 1 - i]) for i in range(L)], grads


def _rel(got, want):
    return ((got.double() - want).norm() / want.norm().clamp_min(1e-300)).item()


def test_lora_bias_layer_backward_stage_by_stage(monkeypatch):
    """The model, biases, LoRA init and batch of test_frozen_bias_runs_the_plain_inverse_rope, one HIP step with the
    tensors around every layer's attention node captured, and every stage of the backward between the attention
    output's gradient and the q / k / v adapter gradients judged ON ITS OWN captured bf16 inputs against fp64 of that
    stage alone:

    (a) flash_bwd: the metrics of tests/test_attention_common_mode_gpu.py (blocks, token-reduced gradients, the
        sum_j dk_j = 0 invariant) within 2 x the emulation of tests/_attn_emul.py, once with the delta the model's
        backward used and once with the exact delta handed over (against the exact-delta emulation); the captured dqkv
        is bit for bit what flash_bwd returns for the captured inputs;
    (b) the plain inverse RoPE, per element with the bounds of test_qkv_bias_rope_autograd_routes;
    (c) the adapter gradients against fp64 from the captured gradient and x, within 2 x the emulation of
        _rowwise.lora_adapter_grad_refs.

    It prints, per layer, the ratio of the common part of q and k (the mean over tokens) to the rms of the rest per head
    as they enter the attention, and what each stage alone adds to the final q / k adapter gradients (every other stage
    in fp64). Measured on MI355X: profiles/attention_common_mode.md."""
    import _attn_emul as ae
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
    layers, grads = _capture_attention_stages(m, ids, labels, monkeypatch)
    nq, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
    nh, ops = nq + nkv, _ext.ops()
    problems = []
    for i, rec in enumerate(layers):
        a, rp, lo = rec["attn"], rec["rope"], rec["lora"]
        cu, max_seqlen, _, _, hd, scale, causal = a["args"]
        assert hd == D and rec["delta"] is None  # a LoRA layer has no o_proj hand-off: flash_bwd forms its own delta
        qkv, dout, M = a["qkv"], a["dout"].contiguous(), a["qkv"].shape[0]
        lens = (cu[1:] - cu[:-1]).tolist()
        X = ae.token_matrix(M, "cuda")
        # the common part of q and k as they enter the attention (after bias and rotation), per head
        qk = qkv[:, :nh * D].double().view(M, nh, D)
        mean = qk.mean(0)
        ratio = mean.norm(dim=-1) / (qk - mean).pow(2).sum(-1).mean(0).sqrt()
        vv = qkv[:, nh * D:].double().view(M, nkv, D)
        vr = vv.mean(0).norm(dim=-1) / (vv - vv.mean(0)).pow(2).sum(-1).mean(0).sqrt()
        print(f"layer {i} common / token-varying part of q heads {[f'{v:.2f}' for v in ratio[:nq].tolist()]}, "
              f"k heads {[f'{v:.2f}' for v in ratio[nq:].tolist()]}, v heads {[f'{v:.2f}' for v in vr.tolist()]}")
        # ---- (a) flash_bwd on its captured inputs
        out, lse = ops.flash_fwd(qkv, *a["args"])
        assert torch.equal(_bits(out), _bits(a["out"]))
        dqkv = ops.flash_bwd(dout, qkv, out, lse, *a["args"])
        assert torch.equal(_bits(dqkv), _bits(a["dqkv"]))  # the replay IS the model's stage
        o64, g64 = ae.reference64(qkv, dout, cu, nq, nkv, scale, causal)
        dqkv_x = ops.flash_bwd(dout, qkv, out, lse, *a["args"], ae.exact_delta(dout, o64, nq))
        for mode, got in (("kernel", dqkv), ("exact", dqkv_x)):
            eo, _, eg, _ = ae.emulate(qkv, dout, cu, nq, nkv, scale, causal, delta=mode, o64=o64)
            bounds = ae.bounds_from(ae.metrics(eo, eg, o64, g64, cu, nq, nkv, X))
            mt = ae.metrics(out, got, o64, g64, cu, nq, nkv, X)
            what = f"layer {i} (a) flash_bwd, {'own' if mode == 'kernel' else 'exact'} delta"
            problems += [(what,) + b for b in ae.check(mt, bounds, lens, what)]
        # ---- (b) the inverse rotation, per element
        assert rp["inverse"] and torch.equal(_bits(rp["pre"]), _bits(a["dqkv"]))
        want = ref.apply_rope(rp["pre"][:, :nh * D].double().view(M, nh, D), rp["cos"].double(), rp["sin"].double(),
                              inverse=True).reshape(M, nh * D)
        _assert_elements(rp["post"][:, :nh * D], want, nh, f"layer {i} (b) inverse RoPE")
        assert torch.equal(_bits(rp["post"][:, nh * D:]), _bits(rp["pre"][:, nh * D:]))
        # ---- (c) the adapter gradients of the qkv projection
        K, R, r, n, s, p, _, meta, _ = lo["state"]
        assert p == 0.0 and n == 3 and torch.equal(_bits(lo["dy"]), _bits(rp["post"]))
        x, As, Bs = lo["X"][:, :K], lo["ab"][:n], lo["ab"][n:]
        assert all(g is not None for g in (*lo["dAs"], *lo["dBs"]))

        def G(dy):  # the fp64 adapter gradients of a given (fp64 or bf16) gradient of the un-rotated qkv
            return rw.lora_adapter_grad_refs(x, dy, As, Bs, meta, s)

        def unrotate64(g):
            q = ref.apply_rope(g[:, :nh * D].double().view(M, nh, D), rp["cos"].double(), rp["sin"].double(), inverse=True)
            return torch.cat([q.reshape(M, nh * D), g[:, nh * D:].double()], dim=1)

        wA, wB = G(lo["dy"])
        eA, eB = rw.lora_adapter_grad_refs(x, lo["dy"], As, Bs, meta, s, ct=torch.float32, rounding=True)
        # each stage alone, everything after it in fp64: what it adds to the final adapter gradients
        tA, tB = G(unrotate64(g64))              # the whole chain in fp64 from the captured qkv / dout / x
        aA, aB = G(unrotate64(a["dqkv"]))        # flash_bwd as run
        xA, xB = G(unrotate64(dqkv_x))           # flash_bwd with the exact delta
        bA, bB = G(unrotate64(rp["pre"]))        # (b) as run is G(post) = wA, wB
        for j, name in enumerate("qkv"):
            for kind, got, want_, em, t, a_, x_, b_ in (("A", lo["dAs"][j], wA[j], eA[j], tA[j], aA[j], xA[j], bA[j]),
                                                        ("B", lo["dBs"][j], wB[j], eB[j], tB[j], aB[j], xB[j], bB[j])):
                e, bound = _rel(got, want_), 2 * _rel(em, want_)
                print(f"layer {i} (c) lora {kind}.{j} ({name}): {e:.3e} (bound {bound:.3e}); stages alone on the final "
                      f"gradient: flash_bwd {_rel(a_, t):.3e} (with the exact delta {_rel(x_, t):.3e}), inverse RoPE "
                      f"{_rel(want_, b_):.3e}, LoRA backward {e:.3e}, all three {_rel(got, t):.3e}")
                if not e <= bound:
                    problems.append((f"layer {i} (c) lora {kind}.{j}", e, bound))
                pn = f"model.layers.{i}.self_attn.lora.qkv.{kind}.{j}"
                assert torch.equal(grads[pn], got.float()), pn  # what the stage returned is what the parameter received
    assert not problems, problems


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
