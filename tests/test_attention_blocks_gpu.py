"""flash_fwd / flash_bwd / flash_bwd_rope judged per (sequence, head) against the fp64 reference with autograd.

One relative error over all sequences and heads cannot see a fault in a short sequence: in [100, 255, 64, 1, 300, 129]
the length-1 sequence is 1/849 of the rows, and any error in it up to about 87 % stays under a 3e-2 whole-tensor
bound. Here every (sequence, head) block of out, dq, dk and dv is held to the project's bounds (2e-2 for out, 3e-2 for
the gradients) on its own; a block whose reference is zero or tiny (dq / dk of a length-1 sequence) is judged against
the rms of the whole gradient (tests/_blockwise.py). The lengths straddle the 32 / 64 / 128 tile edges and put the
awkward sequences at both ends of the packed buffer."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 128
OUT_BOUND, GRAD_BOUND = 2e-2, 3e-2

EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1]
COLLATED = [300, 17, 129, 41]
COLLATED = COLLATED + [-sum(COLLATED) % 256]  # the trailing pad segment of data.collator._pack_py: M = 512
CASES = {"edges_gqa": (EDGES, 8, 2), "edges_mha": (EDGES, 4, 4), "long_ends": ([1, 511, 512, 1], 16, 4),
         "ragged": ([257, 96, 7], 16, 4), "odd_ratio": ([200, 65, 1], 12, 3), "collated": (COLLATED, 16, 4)}


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()


def _rope_tables(lens):
    pos = torch.cat([torch.arange(l) for l in lens]).to(DEV).double()  # positions restart in every segment
    ang = pos[:, None] / (10000 ** (torch.arange(0, 64, device=DEV).double() / 64))[None]
    return ang.cos(), ang.sin()


def _inverse_rope64(g, cos, sin, nq, nkv):
    """The rotate_half rotation by -angle on the q and k heads of a packed [M, (nq + 2 nkv) * D] gradient, in fp64."""
    M = g.shape[0]
    qk = g[:, :(nq + nkv) * D].reshape(M, nq + nkv, D)
    x1, x2 = qk[..., :64], qk[..., 64:]
    c, s = cos[:, None, :], sin[:, None, :]
    rot = torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], dim=-1).reshape(M, -1)
    return torch.cat([rot, g[:, (nq + nkv) * D:]], dim=1)


@pytest.fixture(scope="module")
def attn_ref():
    """Inputs and the fp64 reference (out, dqkv, inverse-RoPE dqkv) per (case, causal): computed once, shared by the two
    dQ paths, never modified."""
    cache = {}

    def get(name, causal):
        key = (name, causal)
        if key not in cache:
            lens, nq, nkv = CASES[name]
            g = torch.Generator(device=DEV).manual_seed(2 * list(CASES).index(name) + int(causal) + 1)
            cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
            M = int(cu[-1])
            qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, generator=g).to(torch.bfloat16)
            dout = torch.randn(M, nq * D, device=DEV, generator=g).to(torch.bfloat16)
            q64 = qkv.double().requires_grad_(True)
            o64 = ref.attention(q64, nq, nkv, D, cu, 1 / math.sqrt(D), causal)
            (g64,) = torch.autograd.grad(o64, q64, dout.double())
            cos, sin = _rope_tables(lens)
            cache[key] = dict(lens=lens, nq=nq, nkv=nkv, cu=cu, qkv=qkv, dout=dout, o64=o64.detach(), g64=g64,
                              g64_rope=_inverse_rope64(g64, cos, sin, nq, nkv),
                              cos=cos.float().contiguous(), sin=sin.float().contiguous())
        return cache[key]
    yield get
    cache.clear()


def _grad_blocks(dqkv, want, r, what):
    nq, nkv, cu = r["nq"], r["nkv"], r["cu"].tolist()
    worst = {}
    for name, lo, hi in (("dq", 0, nq * D), ("dk", nq * D, (nq + nkv) * D), ("dv", (nq + nkv) * D, (nq + 2 * nkv) * D)):
        worst[name] = assert_blocks_close(dqkv[:, lo:hi], want[:, lo:hi], 0, D, GRAD_BOUND, f"{what} {name}",
                                          row_splits=cu)
    return worst


@pytest.mark.parametrize("ds_mb", ["", "0"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_attention_per_sequence_and_head(name, causal, ds_mb, attn_ref, monkeypatch):
    monkeypatch.setenv("SFTAMD_ATTN_DS_MB", ds_mb)  # "" = materialised dS^T + dq32, "0" = the dq3 recompute path
    r = attn_ref(name, causal)
    lens, nq, nkv, cu, qkv, dout = r["lens"], r["nq"], r["nkv"], r["cu"], r["qkv"], r["dout"]
    scale, rep = 1 / math.sqrt(D), r["nq"] // r["nkv"]
    ops = _ext.ops()
    out, lse = ops.flash_fwd(qkv, cu, max(lens), nq, nkv, D, scale, causal)
    what = f"{name} causal={causal} ds_mb={ds_mb!r}"
    w_out = assert_blocks_close(out, r["o64"], 0, D, OUT_BOUND, f"{what} out", row_splits=cu.tolist())
    dqkv = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, causal)
    w = _grad_blocks(dqkv, r["g64"], r, what)
    dqkv_r = ops.flash_bwd_rope(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, causal, r["cos"], r["sin"])
    w_r = _grad_blocks(dqkv_r, r["g64_rope"], r, what + " rope")
    print(f"attention_blocks {what}: worst (sequence, head) block out {w_out:.3e}, "
          + ", ".join(f"{k} {v:.3e}" for k, v in w.items()) + "; rope " + ", ".join(f"{k} {v:.3e}" for k, v in w_r.items()))
    # a sequence of one token: the softmax of its one score is 1, so out is the V row bit for bit, and dq = dk = 0
    v = qkv[:, (nq + nkv) * D:].view(-1, nkv, D).repeat_interleave(rep, 1).reshape(-1, nq * D)
    rms = {k: r["g64"][:, sl].pow(2).mean().sqrt().item() for k, sl in (("dq", slice(0, nq * D)),
                                                                         ("dk", slice(nq * D, (nq + nkv) * D)))}
    cul = cu.tolist()
    for b, l in enumerate(lens):
        if l != 1:
            continue
        s = cul[b]
        assert torch.equal(out[s], v[s]), (what, "length-1 sequence", b, (out[s] != v[s]).nonzero().flatten()[:8].tolist())
        for g in (dqkv, dqkv_r):
            assert g[s, :nq * D].abs().max().item() <= 1e-4 * rms["dq"], (what, b, g[s, :nq * D].abs().max().item())
            assert g[s, nq * D:(nq + nkv) * D].abs().max().item() <= 1e-4 * rms["dk"], (what, b)


def test_deferred_rescale_branch_per_head():
    """The case of test_flash_attention_deferred_rescale_branch (the online-softmax max jumps ~27 in log2 at one key
    for one query of one head), judged per head and per 64-row block: the spiked head cannot hide behind the others."""
    torch.manual_seed(1)
    nq, nkv, T = 4, 2, 384
    cu = torch.tensor([0, T], dtype=torch.int32, device=DEV)
    qkv = (0.3 * torch.randn(T, (nq + 2 * nkv) * D, device=DEV)).to(torch.bfloat16)
    k = qkv[:, nq * D:(nq + nkv) * D].view(T, nkv, D)
    q = qkv[:, :nq * D].view(T, nq, D)
    k[200] = (20.0 * q[300, 0].float()).to(k.dtype)
    scale = 1 / math.sqrt(D)
    out, _ = _ext.ops().flash_fwd(qkv, cu, T, nq, nkv, D, scale, True)
    o64 = ref.attention(qkv.double(), nq, nkv, D, cu, scale, True)
    assert_blocks_close(out, o64, 64, D, OUT_BOUND, "deferred rescale")
    assert_blocks_close(out[300:301], o64[300:301], 1, D, OUT_BOUND, "the spiked query row")


@pytest.mark.parametrize("path", ["default", "ds0"])
def test_precomputed_delta_per_sequence_and_head(path, monkeypatch):
    """The comparison of test_flash_bwd_precomputed_delta (backward given delta == backward computing it), per
    (sequence, head) at the same 1e-3."""
    monkeypatch.setenv("SFTAMD_ATTN_DS_MB", "0" if path == "ds0" else "")
    torch.manual_seed(9)
    nq, nkv = 8, 2
    lens = [300, 17, 512, 129, 1]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    M = int(cu[-1])
    qkv = torch.randn(M, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    ops = _ext.ops()
    out, lse = ops.flash_fwd(qkv, cu, max(lens), nq, nkv, D, scale, True)
    dout = torch.randn_like(out)
    delta = (dout.float() * out.float()).view(M, nq, D).sum(-1).t().contiguous()
    cos, sin = (t.float().contiguous() for t in _rope_tables(lens))
    want = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True)
    got = ops.flash_bwd(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, delta)
    want_r = ops.flash_bwd_rope(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, cos, sin)
    got_r = ops.flash_bwd_rope(dout, qkv, out, lse, cu, max(lens), nq, nkv, D, scale, True, cos, sin, delta)
    for name, lo, hi in (("dq", 0, nq * D), ("dk", nq * D, (nq + nkv) * D), ("dv", (nq + nkv) * D, (nq + 2 * nkv) * D)):
        for g, w, tag in ((got, want, ""), (got_r, want_r, " rope")):
            assert_blocks_close(g[:, lo:hi], w[:, lo:hi].double(), 0, D, 1e-3, f"{path} {name}{tag}",
                                row_splits=cu.tolist())
