"""Numerics of every HIP kernel vs a plain PyTorch fp32 reference of the same op (GPU only)."""
import contextlib
import math
import os

import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close, rounding_floor, swiglu_bwd_reference
from _rowwise import adamw_kernel_order, fp32_tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("H", [2048, 4096, 640])
@pytest.mark.parametrize("with_res", [False, True])
def test_rmsnorm(H, with_res):
    torch.manual_seed(0)
    M = 1000
    x = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)
    r = torch.randn(M, H, device=DEV, dtype=torch.bfloat16) if with_res else None
    w = (1 + 0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16)
    y, ro, rstd = _ext.ops().rmsnorm_fwd(x, r, w, 1e-6)
    h = x if r is None else (x.float() + r.float()).to(torch.bfloat16)
    y_ref, rstd_ref = ref.rms_norm(h, w, 1e-6)
    assert torch.equal(ro, h)
    assert rel_err(y, y_ref) < 1e-2
    assert torch.allclose(rstd, rstd_ref, rtol=1e-4)
    # backward vs autograd on fp32
    dy = torch.randn_like(x)
    dres = torch.randn_like(x) if with_res else None
    dx, dw = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, dres)
    hf = h.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    yf = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-6) * wf
    gx, gw = torch.autograd.grad(yf, (hf, wf), dy.float())
    if dres is not None:
        gx = gx + dres.float()
    assert rel_err(dx, gx) < 1e-2
    assert rel_err(dw, gw) < 1e-3


def test_rmsnorm_bwd_training_shape_deterministic():
    """M = 8192 tokens x H = 2048 (the bench micro-batch): many rows per wave, two-level dW reduce."""
    torch.manual_seed(1)
    M, H = 8192, 2048
    h = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16)
    _, _, rstd = _ext.ops().rmsnorm_fwd(h, None, w, 1e-6)
    dy = torch.randn_like(h)
    dres = torch.randn_like(h)
    dx, dw = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, dres)
    dx2, dw2 = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, dres)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)  # fixed-order reductions
    hf = h.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    yf = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-6) * wf
    gx, gw = torch.autograd.grad(yf, (hf, wf), dy.float())
    assert rel_err(dx, gx + dres.float()) < 1e-2
    assert rel_err(dw, gw) < 1e-3


def test_rmsnorm_bwd_direct_dw_out():
    """dW written / accumulated straight into a bf16 gradient buffer (the flat DDP slice)."""
    torch.manual_seed(2)
    M, H = 1024, 2048
    h = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(H, device=DEV)).to(torch.bfloat16)
    _, _, rstd = _ext.ops().rmsnorm_fwd(h, None, w, 1e-6)
    dy = torch.randn_like(h)
    dx_ref, dw_ref = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, None)
    buf = torch.full((H + 64,), 7.0, device=DEV, dtype=torch.bfloat16)
    out = buf[64:]
    dx, dw = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, None, out, False)
    assert dw.numel() == 0 and torch.equal(dx, dx_ref)
    assert torch.equal(out, dw_ref.to(torch.bfloat16)) and (buf[:64] == 7.0).all()
    _ext.ops().rmsnorm_bwd(dy, h, w, rstd, None, out, True)
    assert rel_err(out, 2 * dw_ref) < 1e-2


@pytest.mark.parametrize("M,I", [(777, 1376), (1, 8), (3, 24), (2048, 11008)])
def test_swiglu(M, I):
    torch.manual_seed(0)
    gu = torch.randn(M, 2 * I, device=DEV, dtype=torch.bfloat16)
    out = _ext.ops().swiglu_fwd(gu)
    assert rel_err(out, ref.swiglu(gu.float())) < 1e-2
    dy = torch.randn_like(out)
    g = gu.float().requires_grad_(True)
    o = ref.swiglu(g)
    (gref,) = torch.autograd.grad(o, g, dy.float())
    assert rel_err(_ext.ops().swiglu_bwd(dy, gu), gref) < 1e-2


@pytest.mark.parametrize("inverse", [False, True])
def test_rope(inverse):
    torch.manual_seed(0)
    M, nq, nkv, D = 300, 16, 4, 128
    qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    pos = torch.randint(0, 4000, (M,), device=DEV)
    cos, sin = ref.rope_cos_sin(pos, D, 2e6)
    exp = qkv.clone()
    qk = exp[:, : (nq + nkv) * D].view(M, nq + nkv, D)
    qk.copy_(ref.apply_rope(qk.float(), cos, sin, inverse=inverse))
    got = qkv.clone()
    _ext.ops().rope_(got, cos.contiguous(), sin.contiguous(), nq, nkv, D, inverse)
    assert rel_err(got, exp) < 1e-2
    assert torch.equal(got[:, (nq + nkv) * D:], qkv[:, (nq + nkv) * D:])  # V untouched


def test_embedding():
    torch.manual_seed(0)
    V, H, M = 5000, 2048, 3000
    w = torch.randn(V, H, device=DEV, dtype=torch.bfloat16)
    ids = torch.randint(0, 300, (M,), device=DEV)  # many repeats
    assert torch.equal(_ext.ops().embedding_fwd(ids, w), w[ids])
    dy = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)
    g = torch.zeros(V, H, device=DEV, dtype=torch.bfloat16)
    s, perm = torch.sort(ids.to(torch.int32))
    _ext.ops().embedding_bwd(dy, s, perm.to(torch.int32), g)
    gr = torch.zeros(V, H, device=DEV).index_add_(0, ids, dy.float())
    assert rel_err(g, gr) < 1e-2
    g2 = torch.zeros_like(g)
    _ext.ops().embedding_bwd(dy, s, perm.to(torch.int32), g2)
    assert torch.equal(g, g2)  # deterministic


def test_embedding_bwd_skewed_runs():
    """Real chat data: a few ids repeat hundreds of times (system prompt in every sample). Runs of 1, 7, 8, 9,
    17 and 700 rows (the batched-load tails) against the fp32 sum; bf16 rows accumulate into an existing grad."""
    torch.manual_seed(2)
    H = 2048
    ids = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate([1, 7, 8, 9, 17, 700, 3])])
    ids = ids[torch.randperm(ids.numel())].to(DEV)
    M, V = ids.numel(), 16
    dy = torch.randn(M, H, device=DEV, dtype=torch.bfloat16)
    g = torch.randn(V, H, device=DEV, dtype=torch.bfloat16)
    want = g.float().index_add_(0, ids, dy.float())
    s, perm = torch.sort(ids.to(torch.int32), stable=True)
    _ext.ops().embedding_bwd(dy, s, perm.to(torch.int32), g)
    assert rel_err(g, want) < 1e-2


@pytest.mark.parametrize("V", [128256, 8008, 512])
def test_cross_entropy(V):
    torch.manual_seed(0)
    M = 257
    logits = (3 * torch.randn(M, V, device=DEV)).to(torch.bfloat16)
    labels = torch.randint(0, V, (M,), device=DEV)
    labels[::7] = -100
    inv = torch.tensor([1.0 / 100.0], device=DEV)
    lg = logits.clone()
    stats = _ext.ops().ce_fwd(lg, labels, inv, True)
    loss, lse, correct, ent = ref.cross_entropy(logits, labels)
    assert torch.allclose(stats[0], loss, atol=2e-3, rtol=1e-3)
    assert torch.allclose(stats[1], lse, atol=2e-3, rtol=1e-3)
    assert torch.allclose(stats[2], ent, atol=2e-2, rtol=1e-2)
    assert torch.equal(stats[3].bool(), correct)
    lf = logits.float().requires_grad_(True)
    l = torch.nn.functional.cross_entropy(lf, labels, ignore_index=-100, reduction="sum") * inv[0]
    (gref,) = torch.autograd.grad(l, lf)
    assert rel_err(lg, gref) < 2e-2


@contextlib.contextmanager
def _env(**kv):
    """Set SFTAMD_* dispatch overrides for one case and restore the previous values afterwards."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _attn_case(lens, nq, nkv, causal, ds_mb=""):
    # ds_mb: "" = default budget (materialised dS^T + dq32), "0" = the dq3 recompute path
    with _env(SFTAMD_ATTN_DS_MB=ds_mb):
        _attn_case_body(lens, nq, nkv, causal)


def _attn_case_body(lens, nq, nkv, causal):
    torch.manual_seed(0)
    D = 128
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    M = int(cu[-1])
    qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    out, lse = _ext.ops().flash_fwd(qkv, cu, max(lens), nq, nkv, D, scale, causal)
    q32 = qkv.float().requires_grad_(True)
    o_ref = ref.attention(q32, nq, nkv, D, cu, scale, causal)
    assert rel_err(out, o_ref) < 2e-2, rel_err(out, o_ref)
    dout = torch.randn_like(out)
    (g_ref,) = torch.autograd.grad(o_ref, q32, dout.float())
    dqkv = _ext.ops().flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, causal)
    for name, sl in (("dq", slice(0, nq * D)), ("dk", slice(nq * D, (nq + nkv) * D)), ("dv", slice((nq + nkv) * D, None))):
        e = rel_err(dqkv[:, sl], g_ref[:, sl])
        per_seq = [(int(cu[b + 1] - cu[b]), round(float((dqkv[cu[b]:cu[b + 1], sl].float() - g_ref[cu[b]:cu[b + 1], sl])
                                                        .abs().max()), 4)) for b in range(len(lens))]
        assert e < 3e-2, (name, e, per_seq)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("ds_mb", ["", "0"])
def test_flash_attention_varlen_gqa(causal, ds_mb):
    """fwd32 + the GQA-grouped dK/dV (dkdv32) with either dQ path (materialised dS^T + dq32, or the dq3
    recompute past the dS^T budget) vs the fp32 reference: ragged lengths off the 64 / 128 tile grid, even GQA
    ratios (two head groups, LDS-DMA Q / dO), odd ones (one group), MHA (rep 1) and the SmolLM3 shape."""
    _attn_case([100, 255, 64, 1, 300, 129], 8, 2, causal, ds_mb)
    _attn_case([512, 511, 7], 16, 4, causal, ds_mb)
    _attn_case([200, 65], 12, 3, causal, ds_mb)
    _attn_case([130, 64], 12, 2, causal, ds_mb)
    _attn_case([621, 700, 553, 754], 16, 4, causal, ds_mb)
    _attn_case([300, 17, 129], 4, 4, causal, ds_mb)


@pytest.mark.parametrize("causal", [True, False])
def test_flash_fwd_out_and_lse(causal):
    """The 32x32x16 forward (fwd32: HW = gcd(rep, 4) heads per workgroup -> rep 4 / 8, 2 / 6, 1 / 3 paths) vs fp32
    softmax(QK^T) V and logsumexp, on lengths off the 32 / 64 grids."""
    torch.manual_seed(1)
    D = 128
    for lens, nq, nkv in (([512, 511, 7, 33], 16, 4), ([100, 255, 64, 1, 300, 129], 8, 2), ([200, 65], 12, 3),
                          ([130, 64, 31], 12, 2), ([300, 17, 129], 4, 4), ([257, 96], 16, 2)):
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
        M = int(cu[-1])
        qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
        scale = 1 / math.sqrt(D)
        out, lse = _ext.ops().flash_fwd(qkv, cu, max(lens), nq, nkv, D, scale, causal)
        q32 = qkv.float()
        o_ref = ref.attention(q32, nq, nkv, D, cu, scale, causal)
        assert rel_err(out, o_ref) < 1e-2, (lens, nq, nkv, rel_err(out, o_ref))
        rep = nq // nkv
        for b in range(len(lens)):
            s, e = int(cu[b]), int(cu[b + 1])
            q = q32[s:e, :nq * D].view(e - s, nq, D).transpose(0, 1)
            k = q32[s:e, nq * D:(nq + nkv) * D].view(e - s, nkv, D).transpose(0, 1).repeat_interleave(rep, 0)
            sc = (q @ k.transpose(1, 2)) * scale
            if causal:
                sc = sc.masked_fill(torch.ones(e - s, e - s, device=DEV, dtype=torch.bool).triu(1), float("-inf"))
            want = torch.logsumexp(sc, -1)
            torch.testing.assert_close(lse[:, s:e], want, atol=2e-3, rtol=1e-3)


def test_flash_attention_mha_and_long():
    _attn_case([1000, 37], 4, 4, True)
    _attn_case([2048, 5], 16, 4, True)


def test_flash_attention_smollm3_shape():
    _attn_case([512] * 4, 16, 4, True)


@pytest.mark.parametrize("path", ["default", "ds0"])
def test_flash_bwd_precomputed_delta(path, monkeypatch):
    """flash_bwd / flash_bwd_rope given delta (as dgrad_gemm_delta's epilogue computes it) skip the delta kernel and
    match the self-computed backward; a wrongly shaped delta is refused."""
    monkeypatch.setenv("SFTAMD_ATTN_DS_MB", "0" if path == "ds0" else "")
    torch.manual_seed(9)
    D, nq, nkv = 128, 8, 2
    lens = [300, 17, 512, 129]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    M = int(cu[-1])
    qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    out, lse = _ext.ops().flash_fwd(qkv, cu, max(lens), nq, nkv, D, scale, True)
    dout = torch.randn_like(out)
    delta = (dout.float() * out.float()).view(M, nq, D).sum(-1).t().contiguous()
    want = _ext.ops().flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True)
    got = _ext.ops().flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, delta)
    assert rel_err(got, want) < 1e-3
    pos = torch.cat([torch.arange(l) for l in lens]).to(DEV).float()
    ang = pos[:, None] / (10000 ** (torch.arange(0, 64, device=DEV).float() / 64))[None]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    want_r = _ext.ops().flash_bwd_rope(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, cos, sin)
    got_r = _ext.ops().flash_bwd_rope(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, cos, sin, delta)
    assert rel_err(got_r, want_r) < 1e-3
    with pytest.raises(RuntimeError):
        _ext.ops().flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, delta.t())


@pytest.mark.parametrize("path", ["default", "ds0", "mha"])
def test_flash_bwd_rope(path, monkeypatch):
    """flash_bwd_rope == inverse-RoPE(flash_bwd): fused into the dq / dK epilogues on the default path (one bf16
    rounding instead of two: close), the rope kernel after the backward on the dq3 path (bitwise)."""
    monkeypatch.setenv("SFTAMD_ATTN_DS_MB", "0" if path == "ds0" else "")
    torch.manual_seed(5)
    D = 128
    nq, nkv = (4, 4) if path == "mha" else (8, 2)
    lens = [300, 17, 512, 129]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    M = int(cu[-1])
    qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    pos = torch.cat([torch.arange(l) for l in lens]).to(DEV).float()
    inv = 1.0 / (10000 ** (torch.arange(0, 64, device=DEV).float() / 64))
    ang = pos[:, None] * inv[None]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    scale = 1 / math.sqrt(D)
    out, lse = _ext.ops().flash_fwd(qkv, cu, max(lens), nq, nkv, D, scale, True)
    dout = torch.randn_like(out)
    got = _ext.ops().flash_bwd_rope(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, cos, sin)
    want = _ext.ops().flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True)
    _ext.ops().rope_(want, cos, sin, nq, nkv, D, True)
    if path in ("default", "mha"):
        assert rel_err(got, want) < 1e-2
        assert torch.equal(got[:, (nq + nkv) * D:], want[:, (nq + nkv) * D:])  # dV untouched by the rotation
    else:
        assert torch.equal(got, want)


def test_flash_attention_deferred_rescale_branch():
    """Force the online-softmax max to jump past THR mid-sequence (CDNA guide rule 26)."""
    torch.manual_seed(1)
    D, nq, nkv = 128, 4, 2
    T = 384
    cu = torch.tensor([0, T], dtype=torch.int32, device=DEV)
    qkv = (0.3 * torch.randn(T, (nq + 2 * nkv) * D, device=DEV)).to(torch.bfloat16)
    k = qkv[:, nq * D:(nq + nkv) * D].view(T, nkv, D)
    q = qkv[:, :nq * D].view(T, nq, D)
    k[200] = (20.0 * q[300, 0].float()).to(k.dtype)  # key 200 spikes for query 300: max jumps ~27 (log2) at tile 3
    scale = 1 / math.sqrt(D)
    out, lse = _ext.ops().flash_fwd(qkv, cu, T, nq, nkv, D, scale, True)
    o_ref = ref.attention(qkv.float(), nq, nkv, D, cu, scale, True)
    assert rel_err(out, o_ref) < 2e-2


def test_adamw_and_norm():
    torch.manual_seed(0)
    n = 100003
    p = torch.randn(n, device=DEV).to(torch.bfloat16)
    g = torch.randn(n, device=DEV).to(torch.bfloat16)
    master = p.float()
    m = torch.randn(n, device=DEV).abs() * 0.01
    v = torch.randn(n, device=DEV).abs() * 0.001
    coef = torch.tensor([0.5], device=DEV)
    p2, master2, m2, v2 = p.clone(), master.clone(), m.clone(), v.clone()
    _ext.ops().adamw_flat(p, g, master, m, v, coef, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** 3, 1 - 0.999 ** 3)
    ref.adamw_(p2, g.float() * 0.5, m2, v2, master2, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3)
    assert torch.allclose(master, master2, atol=1e-6, rtol=1e-5)
    assert torch.allclose(m, m2, atol=1e-6) and torch.allclose(v, v2, atol=1e-7)
    assert torch.equal(p, master.to(torch.bfloat16))
    part = _ext.ops().sumsq(g)
    assert abs(part.sum().item() - g.float().pow(2).sum().item()) / g.float().pow(2).sum().item() < 1e-5


def test_adamw_stochastic_rounding_unbiased():
    torch.manual_seed(0)
    n = 1 << 20
    p = torch.full((n,), 1.0, device=DEV).to(torch.bfloat16)
    g = torch.ones(n, device=DEV).to(torch.bfloat16)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    coef = torch.ones(1, device=DEV)
    # one Adam step moves every weight by -lr (first step: m/sqrt(v) = 1); lr far below bf16 ulp(1)=2^-7
    lr = 1e-4
    _ext.ops().adamw_flat(p, g, None, m, v, coef, lr, 0.9, 0.999, 1e-12, 0.0, 1 - 0.9, 1 - 0.999, 1234)
    pf = p.float()
    assert ((pf - (1 - lr)).abs() <= 2 ** -7).all()  # within one ulp
    assert abs(pf.mean().item() - (1 - lr)) < 2e-5  # unbiased: RNE would leave every weight at 1.0
    p2 = torch.full((n,), 1.0, device=DEV).to(torch.bfloat16)
    m.zero_(), v.zero_()
    _ext.ops().adamw_flat(p2, g, None, m, v, coef, lr, 0.9, 0.999, 1e-12, 0.0, 1 - 0.9, 1 - 0.999, 0)
    assert (p2.float() == 1.0).all()  # round-to-nearest loses the update


@pytest.mark.parametrize("off", [4096, 4097])
@pytest.mark.parametrize("state", [torch.float32, torch.bfloat16])
def test_adamw_sr_matches_reference_twin(state, off):
    """bf16 params (+ optionally bf16 moments) with stochastic rounding: the kernel and the PyTorch
    twin use the same hash streams (one hash per element pair; an odd offset makes the pairs straddle the kernel's
    8-element vectors), so they agree except where fp32 op ordering moves a value across a rounding threshold (rare,
    and then by one bf16 ulp)."""
    torch.manual_seed(0)
    n, seed = 200003, 777
    p = torch.randn(n, device=DEV).to(torch.bfloat16)
    g = torch.randn(n, device=DEV).to(torch.bfloat16)
    m = (torch.randn(n, device=DEV) * 0.01).to(state)
    v = (torch.randn(n, device=DEV).abs() * 0.001).to(state)
    coef = torch.tensor([0.7], device=DEV)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    _, alt_m, alt_v = adamw_kernel_order(p.float(), g.float() * 0.7, m.float(), v.float(), 1e-3, 0.9, 0.999, 1e-8, 0.01,
                                         1 - 0.9 ** 5, 1 - 0.999 ** 5)
    _ext.ops().adamw_flat(p, g, None, m, v, coef, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** 5, 1 - 0.999 ** 5,
                          seed, off)
    ref.adamw_(p2, g.float() * 0.7, m2, v2, None, 1e-3, 0.9, 0.999, 1e-8, 0.01, 5, sr_seed=seed, sr_offset=off)
    for a, b, alt in ((p, p2, None), (m, m2, alt_m), (v, v2, alt_v)):
        assert a.dtype == b.dtype
        diff = (a.float() - b.float()).abs()
        bf = b.float().abs()
        # fp32: the kernel receives 1 - beta computed in double, as torch does, so the two differ only in how fp32
        # associates the update: rel |ref| + abs from an fp32 torch evaluation in the kernel's order against ref.adamw_
        # (_rowwise.fp32_tolerance: 2^-21 and 2^-22 max|ref|; values near zero come out of the cancellation
        # m = 0.9 m + 0.1 g, which the abs term covers)
        # bf16: an SR decision flipped by fp32 op ordering costs one ulp (two when it crosses a binade)
        if a.dtype == torch.bfloat16:
            tol = bf * 2 ** -6 + 1e-6 * bf.max()
        else:
            rel, ab = fp32_tolerance(alt, b)
            assert rel <= 1e-6 and ab <= 1e-6 * bf.max().item()  # never looser than the 2e-4 / 1e-6 it replaces
            tol = bf * rel + ab
        bad = diff > tol
        assert not bad.any(), (a.dtype, int(bad.sum()), a.float()[bad][:4].tolist(), b.float()[bad][:4].tolist())
        if a.dtype == torch.bfloat16:
            assert (diff > 0).float().mean().item() < 1e-3


@pytest.mark.parametrize("L", [1, 200, 777])
def test_decode_attention(L):
    torch.manual_seed(0)
    D, nq, nkv, S = 128, 16, 4, 1024
    q = torch.randn(nq * D, device=DEV, dtype=torch.bfloat16)
    kc = torch.randn(S, nkv, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn(S, nkv, D, device=DEV, dtype=torch.bfloat16)
    ln = torch.tensor([L], dtype=torch.int32, device=DEV)
    out = _ext.ops().decode_attention(q, kc, vc, ln, nq, nkv, 1 / math.sqrt(D))
    qf = q.float().view(nkv, nq // nkv, D)
    att = torch.einsum("grd,sgd->grs", qf, kc[:L].float()) / math.sqrt(D)
    ref_o = torch.einsum("grs,sgd->grd", att.softmax(-1), vc[:L].float()).reshape(-1)
    assert rel_err(out, ref_o) < 1e-2


@pytest.mark.parametrize("cfg,T,N,K", [(9, 416, 512, 384), (9, 32, 256, 128), (10, 352, 512, 512), (10, 96, 256, 256),
                                       # split-K ring (cfg = 100 * splits + variant): fp32 slabs + ordered reduce
                                       (210, 512, 512, 512), (410, 1024, 256, 256), (309, 384, 512, 384),
                                       (209, 64, 256, 128), (310, 320, 256, 256),
                                       # hybrid (1000 + ...): 256 whole tiles + the rest split (uneven pieces)
                                       (1310, 96, 4096, 4352), (1309, 128, 4096, 2304), (1210, 160, 4352, 4096)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_gemm(cfg, T, N, K, accumulate):
    torch.manual_seed(0)
    dy = torch.randn(T, N, device="cuda", dtype=torch.bfloat16)
    x = torch.randn(T, K, device="cuda", dtype=torch.bfloat16)
    out = torch.randn(N, K, device="cuda", dtype=torch.bfloat16)
    base = out.float().clone()
    _ext.ops().wgrad_gemm(out, dy, x, accumulate, cfg)
    want = dy.float().t() @ x.float() + (base if accumulate else 0)
    err = (out.float() - want).abs().max().item()
    assert err <= 0.02 * want.abs().max().item(), err


@pytest.mark.parametrize("cfg,T,N,K", [(9, 416, 512, 384), (10, 352, 512, 512), (210, 512, 512, 512), (309, 384, 512, 384),
                                       (1310, 96, 4096, 4352), (1309, 128, 4096, 2304)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_gemm_norm_slots(cfg, T, N, K, accumulate):
    """The ring wgrad kernels' norm partials (epilogue / split-K fixup) sum to the squared norm of the bf16
    gradient they stored; the slots a launch does not own stay untouched."""
    torch.manual_seed(0)
    dy = torch.randn(T, N, device="cuda", dtype=torch.bfloat16)
    x = torch.randn(T, K, device="cuda", dtype=torch.bfloat16)
    out = torch.randn(N, K, device="cuda", dtype=torch.bfloat16)
    cap = -(-N // 256) * -(-K // 128) * 32
    slots = torch.zeros(cap + 64, device="cuda")
    slots[cap:] = 7.0  # sentinel past the capacity handed to the kernel
    _ext.ops().wgrad_gemm(out, dy, x, accumulate, cfg, slots[:cap])
    want = out.float().pow(2).sum().item()
    assert abs(slots[:cap].sum().item() - want) <= 1e-4 * want
    assert torch.all(slots[cap:] == 7.0)
    with pytest.raises(RuntimeError):  # configurations that are not built are refused
        _ext.ops().wgrad_gemm(out, dy, x, accumulate, 1, slots[:cap])


def test_sumsq_chunks():
    torch.manual_seed(0)
    x = torch.randn(5_000_003, device="cuda").to(torch.bfloat16)
    tab = [(0, 1 << 20), (1 << 20, 3), (1_500_001, 77_777), (4_000_000, 1_000_003), (17, 0)]
    chunks = torch.tensor(tab, dtype=torch.int64, device="cuda")
    part = _ext.ops().sumsq_chunks(x, chunks)
    xf = x.float()
    for i, (o, n) in enumerate(tab):
        want = xf[o:o + n].pow(2).sum().item()
        assert abs(part[i].item() - want) <= 1e-4 * max(want, 1.0)


def test_dropout_add_matches_reference_mask():
    torch.manual_seed(0)
    wide = torch.randn(300, 528, device="cuda", dtype=torch.bfloat16)
    a, b = wide[:, 16:272], wide[:, 272:528]  # strided column slices (row stride 528)
    for p, seed in ((0.05, 11), (0.5, 12345)):
        got = _ext.ops().dropout_add(a, b, p, seed)
        want = ref.dropout_add(a.cpu(), b.cpu(), p, seed)
        assert (got.float().cpu() - want.float()).abs().max().item() < 0.02
        got0 = _ext.ops().dropout_add(None, b, p, seed)
        assert torch.equal(got0 != 0, ref.dropout_add(None, b.cpu(), p, seed).cuda() != 0)


@pytest.mark.parametrize("K,R,p", [(2048, 48, 0.05), (2048, 16, 0.0), (1024, 32, 0.3), (11008, 16, 0.05)])
def test_lora_fwd_bwd_kernels(K, R, p):
    torch.manual_seed(0)
    T = 200
    x = torch.randn(T, K, device="cuda", dtype=torch.bfloat16)
    A = (torch.randn(R, K, device="cuda") * 0.05).to(torch.bfloat16)
    for ldX in (0, K + 128):  # unpadded and padded to a whole 128-column K-tile pair (zeros past K + R)
        X, xd = _ext.ops().lora_fwd(x, A, 0.5, p, 99, ldX, True)
        Xr, xdr = ref.lora_fwd(x, A, 0.5, p, 99, ldX)
        X2, xd2 = _ext.ops().lora_fwd(x, A, 0.5, p, 99, ldX)  # default: no saved dropout(x)
        assert torch.equal(X2[:, :K], X[:, :K]) and xd2.numel() == 0 and torch.equal(X2[:, K + R:], X[:, K + R:])
        assert (X2[:, K:K + R].float() - X[:, K:K + R].float()).abs().max().item() <= 2e-2 * (X[:, K:].float().abs().max().item() + 1)
        assert X.shape == Xr.shape == (T, ldX or K + R)
        assert torch.equal(X[:, :K], x)
        assert (X[:, K:].float() - Xr[:, K:].float()).abs().max().item() < 2e-2 * (Xr[:, K:].float().abs().max().item() + 1)
        assert not X[:, K + R:].any()
    if p > 0:
        assert torch.equal(xd, xdr)
    # in place: x already in the left block of X (the producer wrote it there), only [K, ldX) filled
    Xi = torch.full((T, K + 128), 7.0, device="cuda", dtype=torch.bfloat16)
    Xi[:, :K] = x
    _ext.ops().lora_fwd_inplace(Xi, K, A, 0.5, p, 99)
    assert torch.equal(Xi, _ext.ops().lora_fwd(x, A, 0.5, p, 99, K + 128)[0])
    # swiglu: the widening pass reads gu [T, 2K] and forms silu(gate) * up itself == the SwiGLU kernel then lora_fwd
    gu = torch.randn(T, 2 * K, device="cuda", dtype=torch.bfloat16)
    act = _ext.ops().swiglu_fwd(gu)
    Xs = _ext.ops().lora_fwd(gu, A, 0.5, p, 99, K + 128, False, True)[0]
    Xa = _ext.ops().lora_fwd(act, A, 0.5, p, 99, K + 128)[0]
    assert torch.equal(Xs, Xa)
    wideb =torch.randn(T, K + 64, device="cuda", dtype=torch.bfloat16)
    base = wideb[:, :K]
    dxa = (torch.randn(T, R, device="cuda") * 0.1).to(torch.bfloat16)
    dx = _ext.ops().lora_bwd_dx(base, dxa, A, p, 99)
    dxr = ref.lora_bwd_dx(base, dxa, A, p, 99)
    assert (dx.float() - dxr.float()).abs().max().item() < 3e-2
    # with the SwiGLU input: dgu = swiglu_bwd(dx, gu) in the same pass == the two kernels back to back
    gu = torch.randn(T, 2 * K, device="cuda", dtype=torch.bfloat16)
    dgu = _ext.ops().lora_bwd_dx(base, dxa, A, p, 99, gu)
    assert torch.equal(dgu, _ext.ops().swiglu_bwd(dx, gu))
    # dA = dxa^T dropout(x) with the mask regenerated from the seed, x read from the widened activation X'
    dA = _ext.ops().lora_tsum(X, K, dxa, p, 99).sum(0)  # [splits, R, K] partial sums
    xs = ref.dropout_add(None, x, p, 99) if p > 0 else x
    dAr = dxa.float().t() @ xs.float()
    assert dA.dtype == torch.float32 and dA.shape == (R, K)
    assert rel_err(dA, dAr) < 1e-2
    # dB^T = (s xa)^T dy with S a column slice of X' (row stride ldX), no dropout; then the one-launch scatter into
    # bf16 / fp32 gradients, written and accumulated, transposed
    n_out = 640
    dy = torch.randn(T, n_out, device="cuda", dtype=torch.bfloat16)
    S = X[:, K:K + R]
    sBp = _ext.ops().lora_tsum(dy, n_out, S, 0.0, 0)
    sB = sBp.sum(0)
    assert rel_err(sB, S.float().t() @ dy.float()) < 1e-2
    o1 = torch.randn(n_out // 2, 16, device="cuda", dtype=torch.bfloat16)
    o2 = torch.zeros(n_out - n_out // 2, 16, device="cuda", dtype=torch.float32)
    o1_ref = o1.float() + sB[0:16, 0:n_out // 2].t()
    _ext.ops().lora_grad_out(sBp, [o1, o2], [0, R - 16], [0, n_out // 2], True, [1, 0])  # sums the slabs
    assert rel_err(o1, o1_ref) < 1e-2
    assert torch.allclose(o2, sB[R - 16:R, n_out // 2:].t())
    # both of a projection's scatters in one launch: dB^T blocks transposed from sBp, dA blocks straight from the dA
    # slabs, written / accumulated, bf16 / fp32
    dAp = _ext.ops().lora_tsum(X, K, dxa, p, 99)
    b1 = torch.randn(n_out // 2, 16, device="cuda", dtype=torch.bfloat16)
    b2 = torch.zeros(n_out - n_out // 2, 16, device="cuda", dtype=torch.float32)
    a1 = torch.zeros(16, K, device="cuda", dtype=torch.float32)
    a2 = torch.randn(16, K, device="cuda", dtype=torch.bfloat16)
    b1_ref, a2_ref = b1.float() + sB[0:16, 0:n_out // 2].t(), a2.float() + dA[R - 16:R]
    _ext.ops().lora_grad_out2(sBp, [b1, b2], [0, R - 16], [0, n_out // 2], True, [1, 0],
                              dAp, [a1, a2], [0, R - 16], [0, 0], False, [0, 1])
    assert rel_err(b1, b1_ref) < 1e-2 and torch.allclose(b2, sB[R - 16:R, n_out // 2:].t())
    assert torch.allclose(a1, dA[0:16]) and rel_err(a2, a2_ref) < 1e-2


@pytest.mark.parametrize("T,n,R,ldb", [(8192, 22016, 32, 2176), (256, 2048, 16, 2048 + 128), (300, 3072, 48, 2176),
                                        (64, 11008 // 8 * 8, 64, 11008 + 128), (33, 520, 32, 600),
                                        (96, 4104, 16, 2176)])
def test_lora_dxa_vs_fp32(T, n, R, ldb):
    """dxa = s dy Bc (the adapter-dx thin GEMM, csrc/lora.hip dxa_kernel): Bc a column slice of a wider weight, ragged
    token counts (T % 32 != 0) and reductions that are not a multiple of the 256-column chunk, every element checked."""
    torch.manual_seed(3)
    dy = torch.randn(T, n, device=DEV, dtype=torch.bfloat16)
    wide = torch.randn(n, ldb, device=DEV, dtype=torch.bfloat16)
    bc = wide[:, ldb - R - 8:ldb - 8] if ldb - R - 8 >= 0 else wide[:, :R]
    bc = bc if bc.data_ptr() % 16 == 0 else wide[:, :R]
    got = _ext.ops().lora_dxa(dy, bc, 0.5)
    want = 0.5 * (dy.float() @ bc.float())
    assert got.shape == (T, R)
    assert rel_err(got, want) < 5e-3 and _elem_ok(got, want)


@pytest.mark.parametrize("T,blocks,r", [(8192, (11008, 11008), 16), (200, (2048, 512, 512), 16), (77, (1000, 1512), 32),
                                        (640, (3000,), 16), (130, (256, 264, 8, 4096), 16),
                                        (64, (2048, 2048, 2048, 30000), 16)])  # piece table at its 16-entry limit
def test_lora_dxa_blocks_vs_fp32(T, blocks, r):
    """dxa = s dy Bc for a block-diagonal Bc (csrc/lora.hip dxa_piece_kernel + dxa_finish_kernel): each block's dy
    columns cut into pieces, partials summed per block; ragged T, blocks that are not a multiple of the 256-column
    chunk, up to 4 blocks, every element checked (columns outside every block stay zero)."""
    torch.manual_seed(5)
    n, K = sum(blocks), 64
    R = r * len(blocks)
    dy = torch.randn(T, n, device=DEV, dtype=torch.bfloat16)
    wide = torch.zeros(n, K + R + 64, device=DEV, dtype=torch.bfloat16)
    o = [sum(blocks[:i]) for i in range(len(blocks))]
    c = [r * i for i in range(len(blocks))]
    for i, rows in enumerate(blocks):
        wide[o[i]:o[i] + rows, K + c[i]:K + c[i] + r] = torch.randn(rows, r, device=DEV).to(torch.bfloat16)
    bc = wide[:, K:K + R]
    got = _ext.ops().lora_dxa_blocks(dy, bc, o, list(blocks), c, r, 0.5)
    want = 0.5 * (dy.float() @ bc.float())
    assert got.shape == (T, R)
    assert rel_err(got, want) < 5e-3 and _elem_ok(got, want)


@pytest.mark.parametrize("cfg", [5, 11])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 512, 128), (256, 512, 192), (512, 768, 256), (768, 512, 2112),
                                   (2048, 3072, 320)])
def test_gemm_tn_plain(cfg, M, N, K):
    torch.manual_seed(0)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16)
    c = _ext.ops().gemm_tn(x, w, cfg)
    assert rel_err(c, x.float() @ w.float().t()) < 5e-3
    want64 = x.double() @ w.double().t()  # every 32 x 32 block on its own: within twice the output rounding
    floor = rounding_floor(want64, 32, 32)
    worst = assert_blocks_close(c, want64, 32, 32, 2 * floor, f"gemm_tn cfg {cfg}")
    print(f"gemm_tn_plain cfg {cfg} {M}x{N}x{K}: worst 32x32 block {worst:.3e}, rounding floor {floor:.3e}")


def _elem_ok(out, exp, tol=1e-2):
    """every element within tol x max|exp| (a wrong column / row permutation or a skipped tail tile is O(max) off;
    bf16 rounding is 2^-8 of the element)."""
    d = (out.float() - exp.float()).abs()
    return bool((d <= tol * exp.float().abs().max()).all())


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 512, 256), (768, 2560, 2176), (4096, 4352, 256),
                                   (2304, 7424, 128), (8192, 3072, 2048)])
@pytest.mark.parametrize("cfg", [60, 61])
def test_gemm_tn_rowc(cfg, M, N, K):
    """cfg 60 / 61: the persistent 4-wave kernel with the row-contiguous store epilogue (B image rows permuted so a
    lane holds 8 consecutive output columns; 61 = nt stores). Plain, SwiGLU and RoPE epilogues vs the fp32 reference,
    every element checked: grids with several tiles per workgroup (> 256 tiles), the K = 128 single-pair path and
    the ragged last round."""
    torch.manual_seed(0)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16)
    ref32 = x.float() @ w.float().t()
    c = _ext.ops().gemm_tn(x, w, cfg)
    assert rel_err(c, ref32) < 5e-3 and _elem_ok(c, ref32)
    w1 = w * 0.1
    gu_ref = x.float() @ w1.float().t()
    gu, act = _ext.ops().gemm_tn_swiglu(x, w1, cfg)
    assert rel_err(gu, gu_ref) < 5e-3 and _elem_ok(gu, gu_ref)
    act_ref = _ext.ops().swiglu_fwd(gu)  # act from the bf16 gate / up, as the unfused kernel computes it
    assert rel_err(act, act_ref) < 2e-3 and _elem_ok(act, act_ref.float())
    D, nkv = 128, 1
    nq = N // D - 2 * nkv
    pos = (torch.arange(M, device=DEV) % 1000).float()
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    fr = pos[:, None] * inv[None, :]
    cs, sn = fr.cos().contiguous(), fr.sin().contiguous()
    y = (x.float() @ w.float().t()).to(torch.bfloat16)
    qk = y[:, :(nq + nkv) * D].view(M, nq + nkv, D)
    exp = torch.cat([ref.apply_rope(qk, cs, sn).reshape(M, -1), y[:, (nq + nkv) * D:]], dim=1)
    out = _ext.ops().gemm_tn_rope(x, w, cs, sn, (nq + nkv) * D, cfg)
    assert rel_err(out, exp) < 1e-2 and _elem_ok(out, exp, 2e-2)


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 512, 256), (768, 2560, 2176)])
def test_gemm_tn_rope_elementwise(M, N, K):
    """qkv + RoPE on the route the model takes (the ping-pong kernel, cfg 11), every element checked (a wrong column
    pairing or a shifted RoPE boundary in one lane is O(max) off there and invisible in a norm): one tile, four tiles,
    30 tiles with a 34-step reduction. Operands, tables and tolerances of test_gemm_tn_rowc's RoPE third."""
    torch.manual_seed(0)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16)
    D, nkv = 128, 1
    nq = N // D - 2 * nkv
    pos = (torch.arange(M, device=DEV) % 1000).float()
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    fr = pos[:, None] * inv[None, :]
    cs, sn = fr.cos().contiguous(), fr.sin().contiguous()
    y = (x.float() @ w.float().t()).to(torch.bfloat16)
    qk = y[:, :(nq + nkv) * D].view(M, nq + nkv, D)
    exp = torch.cat([ref.apply_rope(qk, cs, sn).reshape(M, -1), y[:, (nq + nkv) * D:]], dim=1)
    out = _ext.ops().gemm_tn_rope(x, w, cs, sn, (nq + nkv) * D, 11)
    assert rel_err(out, exp) < 1e-2 and _elem_ok(out, exp, 2e-2)


@pytest.mark.parametrize("cfg", [11, 60])
def test_gemm_tn_strided_rows(cfg):
    """a may be a row-strided view (e.g. a column slice of a wider activation)."""
    torch.manual_seed(0)
    xw = torch.randn(512, 384, device=DEV, dtype=torch.bfloat16)
    x = xw[:, :256]
    w = torch.randn(256, 256, device=DEV, dtype=torch.bfloat16)
    assert rel_err(_ext.ops().gemm_tn(x, w, cfg), x.float() @ w.float().t()) < 5e-3


@pytest.mark.parametrize("cfg", [5, 11])
@pytest.mark.parametrize("I,K", [(128, 320), (384, 320), (128, 384), (384, 2048)])
def test_gemm_tn_swiglu(I, K, cfg):
    torch.manual_seed(0)
    M = 512
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(2 * I, K, device=DEV, dtype=torch.bfloat16) * 0.1
    gu, act = _ext.ops().gemm_tn_swiglu(x, w, cfg)
    gu_ref = x.float() @ w.float().t()
    assert rel_err(gu, gu_ref) < 5e-3
    assert rel_err(act, ref.swiglu(gu_ref)) < 1e-2
    # act is computed from the bf16 gate/up the backward sees: identical to the unfused kernel on gu
    assert rel_err(act, _ext.ops().swiglu_fwd(gu)) < 2e-3


@pytest.mark.parametrize("cfg", [5, 11])
def test_gemm_tn_rope(cfg):
    torch.manual_seed(0)
    M, K, nq, nkv, D = 512, 256, 2, 1, 128
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn((nq + 2 * nkv) * D, K, device=DEV, dtype=torch.bfloat16) * 0.1
    pos = torch.arange(M, device=DEV).float()
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    fr = pos[:, None] * inv[None, :]
    cs, sn = fr.cos().contiguous(), fr.sin().contiguous()
    out = _ext.ops().gemm_tn_rope(x, w, cs, sn, (nq + nkv) * D, cfg)
    y = (x.float() @ w.float().t()).to(torch.bfloat16)
    qk = y[:, :(nq + nkv) * D].view(M, nq + nkv, D)
    exp = torch.cat([ref.apply_rope(qk, cs, sn).reshape(M, -1), y[:, (nq + nkv) * D:]], dim=1)
    assert rel_err(out, exp) < 1e-2
    assert torch.equal(out[:, (nq + nkv) * D:], y[:, (nq + nkv) * D:]) or rel_err(out[:, (nq + nkv) * D:], y[:, (nq + nkv) * D:]) < 5e-3


@pytest.mark.parametrize("tail", ["1", "0"])
def test_gemm_tn_rope_wave_tail(tail, monkeypatch):
    """SmolLM3 qkv grid (32 x 12 tiles = 1.5 rounds): the whole round + a 256 x 128 tail launch whose RoPE
    boundary (k heads rotated, v heads not) is shifted with its pointers == the fp32 reference."""
    monkeypatch.setenv("SFTAMD_TN_TAIL", tail)
    torch.manual_seed(1)
    M, K, nq, nkv, D = 8192, 128, 16, 4, 128
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn((nq + 2 * nkv) * D, K, device=DEV, dtype=torch.bfloat16) * 0.1
    pos = (torch.arange(M, device=DEV) % 512).float()
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    fr = pos[:, None] * inv[None, :]
    cs, sn = fr.cos().contiguous(), fr.sin().contiguous()
    out = _ext.ops().gemm_tn_rope(x, w, cs, sn, (nq + nkv) * D, 11)
    y = (x.float() @ w.float().t()).to(torch.bfloat16)
    qk = y[:, :(nq + nkv) * D].view(M, nq + nkv, D)
    exp = torch.cat([ref.apply_rope(qk, cs, sn).reshape(M, -1), y[:, (nq + nkv) * D:]], dim=1)
    for lo, hi in ((0, 2048), (2048, (nq + nkv) * D), ((nq + nkv) * D, (nq + 2 * nkv) * D)):
        assert rel_err(out[:, lo:hi], exp[:, lo:hi]) < 1e-2, (lo, hi)


@pytest.mark.parametrize("M,K,N,wpad", [(256, 64, 256, 0), (512, 2048, 768, 0), (256, 96, 512, 64), (768, 1024, 256, 0)])
def test_dgrad_gemm_plain(M, K, N, wpad):
    """dX = dy @ w (w [K, N], optionally a column-sliced view): the hand-written NN dgrad vs fp32."""
    torch.manual_seed(0)
    dy = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    wfull = torch.randn(K, N + wpad, device="cuda", dtype=torch.bfloat16)
    w = wfull[:, :N]
    for cfg in (2, 5, 7) if K % 64 == 0 else (2, 5):
        out = _ext.ops().dgrad_gemm(dy, w, None, cfg)
        want = dy.float() @ w.float()
        assert out.shape == (M, N)
        assert rel_err(out, want) < 1e-2, rel_err(out, want)
    # asymmetric structure: a row-shifted identity catches any transposed / permuted k mapping
    eye = torch.zeros(K, N, device="cuda")
    eye[torch.arange(min(K, N)), (torch.arange(min(K, N)) + 5) % N] = 1.0
    ramp = (torch.arange(M * K, device="cuda") % 251).float().view(M, K).to(torch.bfloat16)
    for cfg in (5, 7) if K % 64 == 0 else (5,):
        got = _ext.ops().dgrad_gemm(ramp, eye.to(torch.bfloat16), None, cfg).float()
        assert torch.equal(got, ramp.float() @ eye), cfg


@pytest.mark.parametrize("M,K,N,swiglu", [(8192, 64, 11008, True), (2048, 96, 9472, False), (4096, 64, 4352, True)])
def test_dgrad_gemm_wave_tail_split(M, K, N, swiglu, monkeypatch):
    """Grids with a partial last round of 256 workgroups (SmolLM3 down projection: 43 x 32 tiles) run the whole
    rounds as one launch and the leftover columns as 256 x 128 half tiles (SFTAMD_DGRAD_TAIL): bit-identical to the
    single launch (same per-element fp32 sums: every ring reads k in the natural order), and equal to the fp32
    reference."""
    torch.manual_seed(2)
    dy = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = (0.05 * torch.randn(K, N, device="cuda")).to(torch.bfloat16)
    gu = torch.randn(M, 2 * N, device="cuda", dtype=torch.bfloat16) if swiglu else None
    res = {}
    for cfg in (5, 7) if K % 64 == 0 else (5,):
        for tail in ("0", "2"):
            monkeypatch.setenv("SFTAMD_DGRAD_TAIL", tail)
            res[tail] = _ext.ops().dgrad_gemm(dy, w, gu, cfg)
        assert torch.equal(res["0"], res["2"]), cfg
    dact = dy.float() @ w.float()
    if swiglu:
        g, u = gu.float().chunk(2, dim=-1)
        s = torch.sigmoid(g)
        want = torch.cat([dact * u * s * (1 + g * (1 - s)), dact * g * s], dim=-1)
    else:
        want = dact
    assert rel_err(res["2"], want) < 1e-2
    # every 32 x 32 block on its own (the leftover columns of the tail launch are 3 of 43 column tiles)
    dact64 = dy.double() @ w.double()
    want64, bound = swiglu_bwd_reference(dact64, gu) if swiglu else (dact64, 2 * rounding_floor(dact64, 32, 32))
    worst = assert_blocks_close(res["2"], want64, 32, 32, bound, f"dgrad wave tail {M}x{K}x{N} swiglu={swiglu}")
    print(f"dgrad_wave_tail_split {M}x{K}x{N} swiglu={swiglu}: worst 32x32 block {worst:.3e}, bound {bound:.3e}")


@pytest.mark.parametrize("M,K,N", [(256, 256, 256), (512, 2048, 512), (256, 64, 768), (2048, 2048, 2816)])
def test_dgrad_gemm_swiglu_bwd(M, K, N):
    """Down-projection dgrad with the SwiGLU backward fused into the epilogue == swiglu_bwd(dy @ w, gu) in fp32."""
    torch.manual_seed(1)
    dy = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = (0.05 * torch.randn(K, N, device="cuda")).to(torch.bfloat16)
    gu = torch.randn(M, 2 * N, device="cuda", dtype=torch.bfloat16)
    dgu = _ext.ops().dgrad_gemm(dy, w, gu, 5)
    assert torch.equal(_ext.ops().dgrad_gemm(dy, w, gu, 2), dgu)  # 256 x 128 tiles: same fp32 sums per element
    if K % 64 == 0:
        assert torch.equal(_ext.ops().dgrad_gemm(dy, w, gu, 7), dgu)  # BK 64: same k order within each 32-deep MFMA
    dact = dy.float() @ w.float()
    g, u = gu.float().chunk(2, dim=-1)
    s = torch.sigmoid(g)
    want = torch.cat([dact * u * s * (1 + g * (1 - s)), dact * g * s], dim=-1)
    assert dgu.shape == (M, 2 * N)
    assert rel_err(dgu, want) < 1e-2, rel_err(dgu, want)
    want64, bound = swiglu_bwd_reference(dy.double() @ w.double(), gu)
    worst = assert_blocks_close(dgu, want64, 32, 32, bound, f"dgrad swiglu {M}x{K}x{N}")
    print(f"dgrad_swiglu_bwd {M}x{K}x{N}: worst 32x32 block {worst:.3e}, bound {bound:.3e}")
