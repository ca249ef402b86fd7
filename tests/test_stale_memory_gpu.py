"""No op's result may depend on what freed GPU memory holds (tests/_stale.py): every case runs its op with the caching
allocator's free blocks filled with 0x00, 0xFF (NaN / -1) and 0x4B (~1.3e7) and requires bit-equal results, at the
smallest shapes at which the buffer in question exists and has an edge. Where tests/_rowwise.py or ops.reference has an
fp64 reference, the NaN-fill run is also held to the bound of the op's own test file.

Covered: the poisoning itself; attention, decode attention, the norms, SwiGLU, sumsq and wgrad_gemm as tests of their
own (STANDALONE_OPS); every other op as a table of cases in groups (TABLE_OPS); sequence_scores forward + backward of
three presets on the packed batch of tests/test_reward_gpu.py. test_every_registered_op_has_a_case holds the ops that
csrc/bindings.cpp registers, minus the capped EXEMPT, to exactly these."""
import dataclasses
import math
import pathlib
import re

import pytest
import torch

import _rowwise as rw
import _stale
from _blockwise import assert_blocks_close, swiglu_bwd_reference
from llm_fine_tune_distributed_amd import ops as pkg_ops
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
OUT_BOUND, GRAD_BOUND = 2e-2, 3e-2  # tests/test_attention_blocks_gpu.py, test_attention_d64_gpu.py, test_sliding_window_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return c


# ------------------------------------------------------------------------------------------------ the helper itself
@pytest.mark.parametrize("byte", _stale.FILLS)
def test_poison_reaches_every_size_class(byte):
    """After poison(b, n) a torch.empty of every size class reads back as b: the small pool (512 B, 64 KB, the largest
    small request), the large pool's 1 MB and 8 MB requests and half of what was poisoned. Live tensors of odd sizes pin
    segments with free remnants, as a test's inputs do."""
    live = [torch.ones(n, dtype=torch.uint8, device=DEV) for n in (1000, 300_000, 1_500_000, 3_000_000)]
    tmp = [torch.ones(n, dtype=torch.uint8, device=DEV) for n in (700, 200_000, 2_500_000)]
    del tmp  # remnants beside the live tensors, holding ones
    n = 64 << 20
    _stale.poison(byte, n)
    for size in (512, 64 << 10, (1 << 20) - 512, 1 << 20, 8 << 20, n // 2):
        t = torch.empty(size, dtype=torch.uint8, device=DEV)
        h = t.cpu()  # compared on the host: a device temporary would itself land in (and overwrite) a poisoned block
        del t
        bad = (h != byte).nonzero()
        assert bad.numel() == 0, (f"fill 0x{byte:02X}: torch.empty({size}) has {bad.numel()} unpoisoned bytes, first at "
                                  f"{int(bad[0])} = {int(h[bad[0]])}")
    assert all(bool((t == 1).all()) for t in live)


def test_assert_fill_independent_sees_an_unwritten_element():
    """The assertion fires on an op that leaves one element of its at::empty-like result unwritten, and names it."""
    x = torch.arange(4096, dtype=torch.float32, device=DEV).view(64, 64)

    def leaky():
        out = torch.empty_like(x)
        out[:37].copy_(x[:37])
        out[38:].copy_(x[38:])
        return (out,)

    with pytest.raises(AssertionError, match=r"leaky.*output 0.*first rows \[37\]"):
        _stale.assert_fill_independent(leaky, "leaky")
    _stale.assert_fill_independent(lambda: (x * 2,), "whole")
    # the same for an op that works in place on one buffer, which every pass hands back: the passes must not compare
    # that buffer with itself
    buf = torch.empty_like(x)

    def leaky_inplace():
        buf.copy_(x)
        buf[37].copy_(torch.empty(64, device=DEV))
        return (buf,)

    with pytest.raises(AssertionError, match=r"leaky_inplace.*output 0.*first rows \[37\]"):
        _stale.assert_fill_independent(leaky_inplace, "leaky_inplace")


# ------------------------------------------------------------------------------------------------ attention
ATTN_LENS = [1, 33, 65, 129]


def _attn_inputs(lens, nq, nkv, D, spare=0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + nq * 10 + nkv)
    total = sum(lens) + spare
    qkv = torch.randn(total, (nq + 2 * nkv) * D, generator=g, device=DEV).to(BF16)
    dout = torch.randn(total, nq * D, generator=g, device=DEV).to(BF16)
    pos = torch.cat([torch.arange(n, device=DEV) for n in lens] + [torch.arange(spare, device=DEV)])
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    ang = pos.float()[:, None] * inv[None]
    return qkv, dout, ang.cos().contiguous(), ang.sin().contiguous()


def _attn_check(lens, nq, nkv, D, window, ds_mb, monkeypatch, max_seqlen=None, spare=0, reference=True):
    monkeypatch.setenv("SFTAMD_ATTN_DS_MB", ds_mb)
    o = _ext.ops()
    cul = _cu(lens)
    total = cul[-1] + spare
    cu = torch.tensor(cul, dtype=torch.int32, device=DEV)
    ms = max(lens) if max_seqlen is None else max_seqlen
    scale = 1 / math.sqrt(D)
    qkv, dout, cos, sin = _attn_inputs(lens, nq, nkv, D, spare)
    out0, lse0 = o.flash_fwd(qkv, cu, ms, nq, nkv, D, scale, True, window)
    splits = cul + ([total] if spare else [])
    what = f"D={D} lens={lens}+{spare} nq={nq} nkv={nkv} window={window} ds_mb={ds_mb!r} max_seqlen={ms}"

    def fwd():
        out, lse = o.flash_fwd(qkv, cu, ms, nq, nkv, D, scale, True, window)
        return out, lse.t()  # rows = tokens, so that a difference names its sequence

    out, lse = _stale.assert_fill_independent(fwd, "flash_fwd " + what, splits, D)
    dqkv, = _stale.assert_fill_independent(
        lambda: (o.flash_bwd(dout, qkv, out0, lse0, cu, ms, nq, nkv, D, scale, True, None, window),),
        "flash_bwd " + what, splits, D)
    _stale.assert_fill_independent(
        lambda: (o.flash_bwd_rope(dout, qkv, out0, lse0, cu, ms, nq, nkv, D, scale, True, cos, sin, None, window),),
        "flash_bwd_rope " + what, splits, D)
    if spare:  # rows past cu[-1] belong to no sequence: +0 in out, lse and dqkv
        assert not _stale.bits(out[cul[-1]:]).any() and not _stale.bits(lse[cul[-1]:]).any(), what
        assert not _stale.bits(dqkv[cul[-1]:]).any(), what
    if reference:
        T = cul[-1]
        q64 = qkv[:T].double().requires_grad_(True)
        o64 = ref.attention(q64, nq, nkv, D, cu, scale, True, window)
        (g64,) = torch.autograd.grad(o64, q64, dout[:T].double())
        assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
        assert_blocks_close(out[:T], o64.detach(), 0, D, OUT_BOUND, what + " out", row_splits=cul)
        assert_blocks_close(dqkv[:T], g64, 0, D, GRAD_BOUND, what + " dqkv", row_splits=cul)


@pytest.mark.parametrize("ds_mb", ["", "0"])
@pytest.mark.parametrize("window", [0, 40])
@pytest.mark.parametrize("nq,nkv", [(2, 1), (4, 1), (4, 4)])  # hw = 2, 4, 1
def test_attention_d128_fill_independent(nq, nkv, window, ds_mb, monkeypatch):
    _attn_check(ATTN_LENS, nq, nkv, 128, window, ds_mb, monkeypatch)


@pytest.mark.parametrize("nq,nkv", [(2, 1), (4, 1), (4, 4)])
def test_attention_d64_fill_independent(nq, nkv, monkeypatch):
    _attn_check(ATTN_LENS, nq, nkv, 64, 0, "", monkeypatch)


@pytest.mark.parametrize("D,ds_mb", [(128, ""), (128, "0"), (64, "")])
@pytest.mark.parametrize("nq,nkv", [(4, 1), (2, 1)])
def test_attention_max_seqlen_contract(nq, nkv, D, ds_mb, monkeypatch):
    """(a) a pad-like last segment longer than the sequences, max_seqlen the true maximum: every row of out, lse and
    dqkv is fill-independent and right. (b) rows past cu[-1]: +0, fill-independent."""
    _attn_check([129, 5, 164], nq, nkv, D, 0, ds_mb, monkeypatch, max_seqlen=164)
    _attn_check([129, 5], nq, nkv, D, 0, ds_mb, monkeypatch, spare=164)


def test_check_packed_meta():
    assert pkg_ops.check_packed_meta([0, 129, 134, 298], 164, 298) == 164
    with pytest.raises(ValueError, match="segment 2 .* 164 rows"):
        pkg_ops.check_packed_meta(torch.tensor([0, 129, 134, 298], dtype=torch.int32), 129)
    with pytest.raises(ValueError, match="pad segment"):
        pkg_ops.check_packed_meta([0, 129, 134], 129, 298)
    with pytest.raises(ValueError, match="start at 0"):
        pkg_ops.check_packed_meta([0, 5, 3], 129)
    with pytest.raises(ValueError, match="host"):
        pkg_ops.check_packed_meta(torch.tensor([0, 5], dtype=torch.int32, device=DEV), 5)


# ------------------------------------------------------------------------------------------------ decode attention
DEC_LENS = [1, 64, 257, 0]  # the last one is the bad length: its row of the output is zeros, its cache rows untouched


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 1)])
def test_decode_attention_fill_independent(nq, nkv, D):
    B, S = 4, 300
    o = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(nq + D)
    qkv = torch.randn(B, (nq + 2 * nkv) * D, generator=g, device=DEV).to(BF16)
    kc = torch.randn(B, S, nkv, D, generator=g, device=DEV).to(BF16)
    vc = torch.randn(B, S, nkv, D, generator=g, device=DEV).to(BF16)
    for b, L in enumerate(DEC_LENS):  # the append overwrites row L - 1; nothing at or past it may be read
        kc[b, max(L - 1, 0):] = float("nan")
        vc[b, max(L - 1, 0):] = float("nan")
    ln = torch.tensor(DEC_LENS, dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(D)
    k1, v1 = torch.empty_like(kc), torch.empty_like(vc)

    def batched():
        k1.copy_(kc)
        v1.copy_(vc)
        return o.decode_attention_batched(qkv, k1, v1, ln, nq, nkv, scale), k1, v1

    what = f"decode_attention_batched D={D} nq={nq} nkv={nkv}"
    out, ka, va = _stale.assert_fill_independent(batched, what, None, D)
    assert not _stale.bits(out[3]).any(), what + ": the bad-length row is not +0"
    assert torch.equal(_stale.bits(ka[3]), _stale.bits(kc[3])) and torch.equal(_stale.bits(va[3]), _stale.bits(vc[3]))
    ka, va = ka.clone(), va.clone()
    for b, L in enumerate(DEC_LENS[:3]):
        q = qkv[b, :nq * D].view(nq, D)
        want, em = rw.decode_refs(q, ka[b, :L], va[b, :L], scale)
        assert_blocks_close(out[b].view(nq, D), want, 1, D, rw.row_bound(em, want), f"{what} L={L}")
        qb = qkv[b, :nq * D].contiguous()
        one, = _stale.assert_fill_independent(
            lambda: (o.decode_attention(qb, ka[b], va[b], ln[b:b + 1], nq, nkv, scale),),
            f"decode_attention D={D} nq={nq} nkv={nkv} L={L}", None, D)
        assert torch.equal(_stale.bits(one.view(-1)), _stale.bits(out[b].view(-1))), (what, L, "single != batched")


# ------------------------------------------------------------------------------------------------ norms, elementwise
@pytest.mark.parametrize("rows", [1, 255, 257])
def test_rmsnorm_fill_independent(rows):
    H, eps = 256, 1e-6
    o = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(rows)
    x, res, dy, dres = (torch.randn(rows, H, generator=g, device=DEV).to(BF16) for _ in range(4))
    w = (1 + 0.1 * torch.randn(H, generator=g, device=DEV)).to(BF16)
    for r in (None, res):
        what = f"rmsnorm_fwd rows={rows} residual={r is not None}"
        y, h, rstd = _stale.assert_fill_independent(lambda: tuple(o.rmsnorm_fwd(x, r, w, eps)), what)
        hh, y64, rstd64, y_em, _ = rw.rmsnorm_fwd_refs(x, r, w, eps)
        assert torch.equal(_stale.bits(h), _stale.bits(hh)), what
        assert_blocks_close(y, y64, 1, H, rw.row_bound(y_em, y64), what)
        for dr in (None, dres):
            what = f"rmsnorm_bwd rows={rows} dres={dr is not None}"
            dx, dw = _stale.assert_fill_independent(lambda: tuple(o.rmsnorm_bwd(dy, h, w, rstd, dr)), what)
            dx64, dw64, dx_em, dw_em = rw.rmsnorm_bwd_refs(dy, h, w, rstd, dr)
            assert_blocks_close(dx, dx64, 1, H, rw.row_bound(dx_em, dx64), what + " dx")
            assert_blocks_close(dw.view(1, H), dw64.view(1, H), 1, 1, 2 * rw.rel_elem_err(dw_em, dw64), what + " dW")


@pytest.mark.parametrize("rows", [1, 255, 257])
def test_swiglu_and_sumsq_fill_independent(rows):
    o = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(rows)
    gu = torch.randn(rows, 512, generator=g, device=DEV).to(BF16)
    dy = torch.randn(rows, 256, generator=g, device=DEV).to(BF16)
    act, = _stale.assert_fill_independent(lambda: (o.swiglu_fwd(gu),), f"swiglu_fwd rows={rows}")
    want, em = rw.swiglu_fwd_refs(gu)
    assert_blocks_close(act, want, 1, 256, rw.row_bound(em, want), f"swiglu_fwd rows={rows}")
    dgu, = _stale.assert_fill_independent(lambda: (o.swiglu_bwd(dy, gu),), f"swiglu_bwd rows={rows}")
    want_b, bound_b = swiglu_bwd_reference(dy.double(), gu, 1, 512)  # tests/test_rowwise_gpu.py's bound
    assert_blocks_close(dgu, want_b, 1, 512, bound_b, f"swiglu_bwd rows={rows}")
    flat = gu.view(-1)[: rows * 512 - 3]  # not a multiple of any chunk
    _stale.assert_fill_independent(lambda: (o.sumsq(flat),), f"sumsq n={flat.numel()}")


# ------------------------------------------------------------------------------------------------ weight gradients
# the smallest shape of every cfg that tests/test_gemm_4w_gpu.py launches (register epilogue; every tile split 2, 3, 4
# ways; hybrid: 256 whole tiles + 16 split 2 ways, at 2 and 3 blocks of 128 tokens, so with a short last piece), then
# its norm-slot shapes where the split-K buffer is tens of MB and the whole tiles park their slots past the slabs
WGRAD_SHAPES = [(14, 128, 256, 256), (214, 512, 512, 512), (314, 384, 512, 256), (414, 1024, 256, 256),
                (1314, 256, 4096, 4352), (1214, 384, 4352, 4096), (414, 1024, 2048, 2048), (1214, 1024, 2048, 11008)]


@pytest.mark.parametrize("cfg,T,N,K", WGRAD_SHAPES)
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("norm", [False, True])
def test_wgrad_fill_independent(cfg, T, N, K, accumulate, norm):
    """The split-K partials, which splitk_fixup_kernel sums, and the norm slots parked in them."""
    o = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(cfg)
    dy = torch.randn(T, N, generator=g, device=DEV).to(BF16)
    x = torch.randn(T, K, generator=g, device=DEV).to(BF16)
    out0 = torch.randn(N, K, generator=g, device=DEV).to(BF16)
    cap = -(-N // 256) * -(-K // 128) * 32
    out, slots = torch.empty_like(out0), torch.empty(cap, device=DEV)

    def run():
        out.copy_(out0)
        slots.zero_()
        o.wgrad_gemm(out, dy, x, accumulate, cfg, slots if norm else None)
        return out, slots

    _stale.assert_fill_independent(run, f"wgrad_gemm cfg={cfg} T={T} N={N} K={K} accumulate={accumulate} norm={norm}")


# ------------------------------------------------------------------------------------------------ model level
LENS = [1 + (37 * i) % 131 for i in range(32)]          # tests/test_reward_gpu.py: 32 sequences, 2140 rows
ROWS = -(-(sum(LENS) + 1) // 256) * 256                 # 2304: a 164-row pad segment, longer than every sequence
COEF = [(-1.0) ** i * (0.3 + 0.11 * (i % 9)) for i in range(32)]


@pytest.mark.parametrize("stated", ["true_max", "sequences_only"])
@pytest.mark.parametrize("preset", ["tiny-gpu", "tiny-gpu-mistral", "tiny-gpu-d64"])
def test_sequence_scores_fill_independent(preset, stated, monkeypatch):
    """Forward + backward of sequence_scores on the HIP path, the free memory poisoned before the forward and again before
    the backward: scores and every parameter gradient are bit-equal across the fills.

    ``true_max``: max_seqlen is the maximum over all segments (164, the pad segment). ``sequences_only``: 129, the
    maximum over the scored sequences, as tests/test_reward_gpu.py stated it before the contract was written down: a
    caller error. The host check rejects it; on the device the pad segment's rows past max_seqlen are written as +0
    before the attention kernels run, so even then nothing reads memory that nothing wrote."""
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0")
    torch.manual_seed(0)
    cfg = dataclasses.replace(get_config(preset), num_labels=1)
    m = build_model(cfg, device=DEV, dtype=BF16, seed=1)
    m.train()
    gen = torch.Generator(device=DEV).manual_seed(3)
    ids = torch.randint(0, cfg.vocab_size, (ROWS,), generator=gen, device=DEV)
    cul = _cu(LENS) + [ROWS]
    cu = torch.tensor(cul, dtype=torch.int32, device=DEV)
    pos = torch.cat([torch.arange(b - a, device=DEV) for a, b in zip(cul[:-1], cul[1:])])
    ms = max(b - a for a, b in zip(cul[:-1], cul[1:])) if stated == "true_max" else max(LENS)
    assert (ms, ROWS - sum(LENS)) == (164 if stated == "true_max" else 129, 164)
    if stated == "sequences_only":
        with pytest.raises(ValueError, match="164 rows"):
            pkg_ops.check_packed_meta(cul, ms, ROWS)
        with pytest.raises(ValueError, match="164 rows"):
            m._hidden(ids, None, cu.cpu(), ms, pos, False)
    else:
        pkg_ops.check_packed_meta(cul, ms, ROWS)
    coef = torch.tensor(COEF, device=DEV)
    names = [n for n, p in m.named_parameters() if p.requires_grad]

    def run(poison_again):
        for p in m.parameters():
            p.grad = None
        m.reset_grad_use_counters()
        s = m.sequence_scores(input_ids=ids, cu_seqlens=cu, position_ids=pos, max_seqlen=ms, n_seqs=len(LENS))
        loss = (s * coef).sum()
        poison_again()
        loss.backward()
        grads = dict(m.named_parameters())
        out = (s.detach(), *(grads[n].grad.detach().clone() for n in names if grads[n].grad is not None))
        for p in m.parameters():  # freed here, so that the next poison overwrites them too
            p.grad = None
        return out

    got = _stale.assert_fill_independent(run, f"sequence_scores {preset} max_seqlen={ms} (outputs: scores, then "
                                              f"the gradients of {names[:3]}...)", takes_poison=True)
    assert len(got) > 1 and all(torch.isfinite(t.float()).all() for t in got)


# ------------------------------------------------------------------------------------------------ the op table
CALLED = set()


class _Recording:
    """The extension's op namespace, noting in CALLED the name of every op that is looked up on it."""

    def __getattr__(self, name):
        CALLED.add(name)
        return getattr(_ext.ops(), name)


def _r(*shape, seed=0, scale=1.0, dtype=BF16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def _quarter(M, D=128):
    ang = torch.arange(M, device=DEV).float()[:, None] * (1.0 / 10000.0 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    return ang.cos().contiguous(), ang.sin().contiguous()


def _inplace(op, pristine, *rest):
    """fn of an op that works in place on its first argument: a fresh copy of ``pristine`` into one buffer per call."""
    buf = torch.empty_like(pristine)

    def fn():
        buf.copy_(pristine)
        out = op(buf, *rest)
        return (buf,) if out is None else (buf, *(out if isinstance(out, (tuple, list)) else (out,)))
    return fn


def _gemm_cases():
    o = _Recording()
    t = {}
    for cfg, k1 in ((5, 64), (11, 64), (60, 128), (61, 128)):  # tests/test_gemm_exact_gpu.py's smallest M per route
        x, w = _r(256, k1, seed=1), _r(256, k1, seed=2)
        t[f"gemm_tn cfg={cfg}"] = ("gemm_tn", lambda x=x, w=w, cfg=cfg: (o.gemm_tn(x, w, cfg),))
        xr, wr = _r(512, 256, seed=3), _r(4 * 128, 256, seed=4)
        cs, sn = _quarter(512)
        t[f"gemm_tn_rope cfg={cfg}"] = ("gemm_tn_rope",
                                        lambda xr=xr, wr=wr, cfg=cfg: (o.gemm_tn_rope(xr, wr, cs, sn, 3 * 128, cfg),))
    for cfg, M, I, K in ((5, 512, 384, 320), (11, 512, 384, 320), (60, 256, 128, 128), (61, 256, 128, 128)):
        x, w = _r(M, K, seed=5), _r(2 * I, K, seed=6, scale=0.1)
        t[f"gemm_tn_swiglu cfg={cfg}"] = ("gemm_tn_swiglu", lambda x=x, w=w, cfg=cfg: tuple(o.gemm_tn_swiglu(x, w, cfg)))
    for M in (1, 17, 64):
        for N, K in ((512, 256), (512, 8192)):  # the second: fewer strips than CUs and a long K, split + reduce launch
            x, w = _r(64, K, seed=7)[:M], _r(N, K, seed=8, scale=0.05)
            t[f"gemm_skinny M={M} N={N} K={K}"] = ("gemm_skinny", lambda x=x, w=w: (o.gemm_skinny(x, w),))
    dy, w, a = _r(256, 256, seed=9), _r(256, 256, seed=10, scale=0.05), _r(256, 256, seed=11)
    gu = _r(256, 512, seed=12)
    t["dgrad_gemm cfg=14"] = ("dgrad_gemm", lambda: (o.dgrad_gemm(dy, w, None, 14),))
    t["dgrad_gemm cfg=5 swiglu"] = ("dgrad_gemm", lambda: (o.dgrad_gemm(dy, w, gu, 5),))
    t["dgrad_gemm cfg=7"] = ("dgrad_gemm", lambda: (o.dgrad_gemm(dy, w, None, 7),))
    t["dgrad_gemm cfg=7 swiglu"] = ("dgrad_gemm", lambda: (o.dgrad_gemm(dy, w, gu, 7),))
    t["dgrad_gemm_delta"] = ("dgrad_gemm_delta", lambda: tuple(o.dgrad_gemm_delta(dy, w, a)))
    # one tile and a reduction of 8192: the tile is split 8 ways over the reduction into fp32 slabs + the ordered fixup
    dyk, wk = _r(256, 8192, seed=13), _r(8192, 256, seed=14, scale=0.05)
    t["dgrad_gemm cfg=14 split-K"] = ("dgrad_gemm", lambda: (o.dgrad_gemm(dyk, wk, None, 14),))
    return t


def _multi_cases():
    o = _Recording()
    t = {}
    T = 1024
    shapes = [(512, 256), (256, 512), (768, 256)]
    dys = [_r(T, n, seed=20 + i) for i, (n, k) in enumerate(shapes)]
    xs = [_r(T, k, seed=30 + i) for i, (n, k) in enumerate(shapes)]
    base = [_r(n, k, seed=40 + i) for i, (n, k) in enumerate(shapes)]
    outs = [torch.empty_like(b) for b in base]
    empty = torch.empty(0, device=DEV)
    slots = [torch.empty((n // 256) * (k // 256) * 32, device=DEV) for n, k in shapes]  # 32 per split tile
    for acc in (0, 1):
        for norm in (False, True):
            def multi(acc=acc, norm=norm):
                for ob, b, sl in zip(outs, base, slots):
                    ob.copy_(b)
                    sl.zero_()
                o.wgrad_gemm_multi(outs, dys, xs, [acc] * 3, slots if norm else [empty] * 3, 2, 0)
                return (*outs, *slots)

            def pair(acc=acc, norm=norm):
                for ob, b, sl in zip(outs[:2], base[:2], slots):
                    ob.copy_(b)
                    sl.zero_()
                o.wgrad_gemm_pair(outs[0], dys[0], xs[0], bool(acc), slots[0] if norm else None,
                                  outs[1], dys[1], xs[1], bool(acc), slots[1] if norm else None, 3)
                return (*outs[:2], *slots[:2])
            t[f"wgrad_gemm_multi split_all=2 accumulate={acc} norm={norm}"] = ("wgrad_gemm_multi", multi)
            t[f"wgrad_gemm_pair split_all=3 accumulate={acc} norm={norm}"] = ("wgrad_gemm_pair", pair)
    # the hybrid rule: 17 x 16 = 272 tiles = one whole round of 256 + 16 tiles of the second problem split over the
    # tokens; the whole tiles of that problem park their norm slots past its slabs (the shape of test_gemm_4w_gpu.py)
    T2, big = 384, [(256, 256), (4096, 4352)]
    dy2 = [_r(T2, n, seed=50 + i) for i, (n, k) in enumerate(big)]
    x2 = [_r(T2, k, seed=52 + i) for i, (n, k) in enumerate(big)]
    base2 = [_r(n, k, seed=54 + i) for i, (n, k) in enumerate(big)]
    out2 = [torch.empty_like(b) for b in base2]
    slot2 = [torch.empty((n // 256) * (k // 256) * 32, device=DEV) for n, k in big]

    def hybrid(acc):
        for ob, b, sl in zip(out2, base2, slot2):
            ob.copy_(b)
            sl.zero_()
        o.wgrad_gemm_pair(out2[0], dy2[0], x2[0], acc, slot2[0], out2[1], dy2[1], x2[1], acc, slot2[1], 0)
        return (*out2, *slot2)
    for acc in (False, True):
        t[f"wgrad_gemm_pair hybrid accumulate={acc} norm=True"] = ("wgrad_gemm_pair", lambda acc=acc: hybrid(acc))
    return t


def _rowwise_cases():
    o = _Recording()
    t = {}
    D, nq, nkv = 128, 2, 1
    for rows in (1, 255, 257):
        qkv = _r(rows, (nq + 2 * nkv) * D, seed=rows)
        cs, sn = _quarter(rows)
        t[f"rope_ rows={rows}"] = ("rope_", _inplace(lambda b, cs=cs, sn=sn: o.rope_(b, cs, sn, nq, nkv, D, False), qkv))
        qw, kw = _r(D, seed=1, scale=0.1) + 1, _r(D, seed=2, scale=0.1) + 1
        t[f"qk_norm_rope_fwd rows={rows}"] = ("qk_norm_rope_fwd", _inplace(
            lambda b, cs=cs, sn=sn: o.qk_norm_rope_fwd(b, qw, kw, cs, sn, nq, nkv, D, 1e-6, True), qkv))
        raw = o.qk_norm_rope_fwd(qkv.clone(), qw, kw, cs, sn, nq, nkv, D, 1e-6, True)
        t[f"qk_norm_rope_bwd rows={rows}"] = ("qk_norm_rope_bwd", _inplace(
            lambda b, cs=cs, sn=sn, raw=raw: o.qk_norm_rope_bwd(b, raw, qw, kw, cs, sn, nq, nkv, D, 1e-6), qkv))
        bias = _r((nq + 2 * nkv) * D, seed=3)
        t[f"qkv_bias_rope_fwd rows={rows}"] = ("qkv_bias_rope_fwd", _inplace(
            lambda b, cs=cs, sn=sn: o.qkv_bias_rope_fwd(b, bias, cs, sn, nq, nkv, D), qkv))
        t[f"qkv_bias_rope_bwd rows={rows}"] = ("qkv_bias_rope_bwd", _inplace(
            lambda b, cs=cs, sn=sn: o.qkv_bias_rope_bwd(b, cs, sn, nq, nkv, D), qkv))
        a, b2 = _r(rows, 256, seed=4), _r(rows, 256, seed=5)
        t[f"dropout_add rows={rows}"] = ("dropout_add", lambda a=a, b2=b2: (o.dropout_add(a, b2, 0.1, 7),
                                                                          o.dropout_add(None, b2, 0.1, 7)))
        ids = torch.randint(0, 64, (rows,), generator=torch.Generator().manual_seed(rows)).to(DEV)
        emb, mag = _r(64, 256, seed=6), torch.rand(rows, generator=torch.Generator().manual_seed(1)).to(DEV)
        t[f"embedding_fwd rows={rows}"] = ("embedding_fwd", lambda ids=ids: (o.embedding_fwd(ids, emb),))
        t[f"embedding_noise_fwd rows={rows}"] = ("embedding_noise_fwd",
                                                 lambda ids=ids, mag=mag: (o.embedding_noise_fwd(ids, emb, mag, 5),))
        srt, perm = torch.sort(ids)
        dy = _r(rows, 256, seed=8)
        t[f"embedding_bwd rows={rows}"] = ("embedding_bwd", _inplace(
            lambda g, dy=dy, srt=srt, perm=perm: o.embedding_bwd(dy, srt.to(torch.int32), perm.to(torch.int32), g), emb))
    return t


def _loss_cases():
    o = _Recording()
    t = {}
    M, V = 257, 1024
    lens = [1, 100, 0, 150]                     # an empty sequence; 6 rows of pad past the last one
    cu = torch.tensor(_cu(lens), dtype=torch.int32, device=DEV)
    S = len(lens)
    lg, tl = _r(M, V, seed=1, scale=2.0), _r(M, V, seed=2, scale=2.0)
    labels = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(3)).to(DEV)
    labels[::7] = -100
    inv = torch.tensor([1.0 / 200], device=DEV)
    for wg in (False, True):
        t[f"ce_fwd write_grad={wg}"] = ("ce_fwd", _inplace(lambda b, wg=wg: o.ce_fwd(b, labels, inv, wg), lg))
        t[f"kd_fwd write_grad={wg}"] = ("kd_fwd", _inplace(lambda b, wg=wg: o.kd_fwd(b, tl, labels, inv, wg, 0.5, 2.0), lg))
    ids, lps = o.teacher_topk(tl, 16, 2.0)
    t["teacher_topk"] = ("teacher_topk", lambda: tuple(o.teacher_topk(tl, 16, 2.0)))
    t["kd_topk_fwd"] = ("kd_topk_fwd", _inplace(lambda b: o.kd_topk_fwd(b, ids, lps, labels, inv, True, 2.0), lg))
    nll = _r(M, seed=4, dtype=torch.float32).abs()
    t["seq_logp_sum"] = ("seq_logp_sum", lambda: (o.seq_logp_sum(nll, cu, S),))
    lp, rlp = _r(S, seed=5, dtype=torch.float32), _r(S, seed=6, dtype=torch.float32)
    t["dpo_pair_fwd"] = ("dpo_pair_fwd", lambda: (o.dpo_pair_fwd(lp, rlp, torch.tensor([0.5], device=DEV), 0.1),))
    h, w = _r(M, 256, seed=7), _r(256, seed=8, scale=0.05)
    g = _r(S, seed=9, dtype=torch.float32)
    t["seq_score_fwd"] = ("seq_score_fwd", lambda: (o.seq_score_fwd(h, w, cu, S),))
    t["seq_score_bwd"] = ("seq_score_bwd", lambda: tuple(o.seq_score_bwd(g, h, w, cu, S, True, True)))
    t["reward_pair_fwd"] = ("reward_pair_fwd",
                            lambda: (o.reward_pair_fwd(lp, None, torch.tensor([0.5], device=DEV), 0.01),))
    adv = _r(S, seed=10, dtype=torch.float32)
    old, rf = nll * -1.0 + 0.01, nll * -1.0 - 0.02
    t["grpo_token_fwd"] = ("grpo_token_fwd", lambda: tuple(o.grpo_token_fwd(
        nll, old, rf, labels, adv, cu, S, torch.tensor([1.0 / 200], device=DEV), 0.2, 0.2, 0.04, False)))
    x, coef, one = _r(M, 256, seed=11), _r(S, seed=12, dtype=torch.float32), torch.tensor([0.5], device=DEV)
    rowc = _r(M, seed=13, dtype=torch.float32)
    t["scale_rows_by_seq"] = ("scale_rows_by_seq", lambda: (o.scale_rows_by_seq(x, coef, cu, S, one),))
    t["scale_rows_by_seq_"] = ("scale_rows_by_seq_", _inplace(lambda b: o.scale_rows_by_seq_(b, coef, cu, S, one), x))
    t["scale_rows"] = ("scale_rows", lambda: (o.scale_rows(x, rowc, one),))
    t["scale_rows_"] = ("scale_rows_", _inplace(lambda b: o.scale_rows_(b, rowc, one), x))
    return t


def _restoring(call, bufs, pristine):
    """fn of an op that works in place on several tensors: ``pristine`` copied into ``bufs`` before every call."""
    def fn():
        for b, p in zip(bufs, pristine):
            b.copy_(p)
        out = call()
        return (*bufs, *(() if out is None else out if isinstance(out, (tuple, list)) else (out,)))
    return fn


def _lora_cases():
    o = _Recording()
    t = {}
    K, R, s, p, seed = 256, 16, 0.5, 0.25, 99
    A = _r(R, K, seed=1, scale=0.05)
    for rows in (1, 257):
        x, gu = _r(rows, K, seed=rows), _r(rows, 2 * K, seed=rows + 1)
        # X[:, K:] of lora_widen is documented as uninitialised (the caller's GEMM writes it): only the copy is a result
        t[f"lora_widen rows={rows}"] = ("lora_widen", lambda x=x: (lambda X, xd: (X[:, :K], xd))(*o.lora_widen(x, R, p, seed)))
        for ldX in (0, K + 128):  # unpadded, and padded: the columns past K + R are written as zeros
            t[f"lora_fwd rows={rows} ldX={ldX}"] = ("lora_fwd", lambda x=x, ldX=ldX: tuple(o.lora_fwd(x, A, s, p, seed, ldX, True)))
        t[f"lora_fwd rows={rows} swiglu"] = ("lora_fwd", lambda gu=gu: (o.lora_fwd(gu, A, s, p, seed, K + 128, False, True)[0],))
        Xi = torch.full((rows, K + 128), 7.0, device=DEV, dtype=BF16)
        Xi[:, :K] = x
        t[f"lora_fwd_inplace rows={rows}"] = ("lora_fwd_inplace", _inplace(lambda b: o.lora_fwd_inplace(b, K, A, s, p, seed), Xi))
        base, dxa = _r(rows, K + 64, seed=rows + 2)[:, :K], _r(rows, R, seed=rows + 3, scale=0.1)
        t[f"lora_bwd_dx rows={rows}"] = ("lora_bwd_dx", lambda base=base, dxa=dxa: (o.lora_bwd_dx(base, dxa, A, p, seed),))
        t[f"lora_bwd_dx rows={rows} swiglu"] = ("lora_bwd_dx", lambda base=base, dxa=dxa, gu=gu: (
            o.lora_bwd_dx(base, dxa, A, p, seed, gu),))
        X = o.lora_fwd(x, A, s, p, seed, 0, False)[0]
        t[f"lora_tsum rows={rows}"] = ("lora_tsum", lambda X=X, dxa=dxa: (o.lora_tsum(X, K, dxa, p, seed),))
        n = 520  # a reduction that is no multiple of the 256-column chunk
        dy, wide = _r(rows, n, seed=rows + 4), _r(n, 2 * R + 64, seed=rows + 5)
        t[f"lora_dxa rows={rows}"] = ("lora_dxa", lambda dy=dy, wide=wide: (o.lora_dxa(dy, wide[:, 16:16 + R], s),))
        t[f"lora_dxa_blocks rows={rows}"] = ("lora_dxa_blocks", lambda dy=dy, wide=wide: (
            o.lora_dxa_blocks(dy, wide[:, 16:16 + 2 * R], [0, 256], [256, 264], [0, R], R, s),))
    # the scatters: slabs [ns, R, K] summed into blocks of bf16 / fp32 outputs, written (0) or accumulated (1)
    sa, sb = _r(9, R, K, seed=20, dtype=torch.float32), _r(7, R, 136, seed=21, dtype=torch.float32)
    spec = [(BF16, 0, 0, 16, 40, 0), (torch.float32, 8, 8, 8, 24, 1)]  # dtype, r0, c0, rows, columns, accumulate

    def group(tr, sd):
        prist = [_r(*((nc, nr) if tr else (nr, nc)), seed=sd + i, dtype=dt) for i, (dt, _, _, nr, nc, _) in enumerate(spec)]
        bufs = [torch.empty_like(q) for q in prist]
        return bufs, prist, (bufs, [c[1] for c in spec], [c[2] for c in spec], tr, [c[5] for c in spec])
    for tr in (False, True):
        bufs, prist, args = group(tr, 30)
        t[f"lora_grad_out tr={tr}"] = ("lora_grad_out", _restoring(lambda args=args: o.lora_grad_out(sa, *args), bufs, prist))
    ba, pa, aa = group(True, 40)
    bb, pb, ab = group(False, 44)
    t["lora_grad_out2"] = ("lora_grad_out2", _restoring(lambda: o.lora_grad_out2(sa, *aa, sb, *ab), ba + bb, pa + pb))
    # (rows, columns, source pitch, destination pitch): the first above 64 x 256 elements, a second grid-stride pass
    cspec = [(70, 300, 320, 304), (1, 77, 77, 100), (0, 16, 16, 16), (33, 5, 9, 7)]
    srcs = [_r(max(r, 1) * lds + 16, seed=60 + i) for i, (r, c, lds, ldd) in enumerate(cspec)]
    prist = [torch.full(((max(r, 1) + 2) * ldd,), 7.0, device=DEV, dtype=BF16) for r, c, lds, ldd in cspec]
    dsts = [torch.empty_like(q) for q in prist]
    desc = torch.tensor([[sr.data_ptr() + 16, d.data_ptr() + 2 * (ldd + 3), r, c, lds, ldd]
                         for sr, d, (r, c, lds, ldd) in zip(srcs, dsts, cspec)], dtype=torch.int64).to(DEV)
    most = max(r * c for r, c, _, _ in cspec)
    # (the table holds addresses: the closure keeps the sources alive)
    t["copy2d_batch"] = ("copy2d_batch", _restoring(lambda keep=srcs: o.copy2d_batch(desc, most), dsts, prist))
    return t


def _sampler_cases():
    o = _Recording()
    t = {}
    B, V, cap, seed = 3, 1024, 2, 1234
    T, K, P, RP = 0.7, 12, 0.9, 1.2
    logits = _r(B, V, seed=1, scale=2.0, dtype=torch.float32)
    pres = torch.zeros(B, (V + 31) // 32, dtype=torch.int32, device=DEV)
    for b, hist in enumerate([[3, 17, 400], [1, 2, 1023], [512]]):
        for tok in hist:
            pres[b, tok >> 5] |= 1 << (tok & 31)
    prist = [pres, torch.zeros(B, 4, dtype=torch.long, device=DEV), torch.full((B,), -1, dtype=torch.long, device=DEV),
             torch.zeros(B, dtype=torch.long, device=DEV), torch.ones(B, dtype=torch.int32, device=DEV),
             torch.full((B, cap), -1, dtype=torch.long, device=DEV), torch.zeros(B, cap, device=DEV),
             torch.zeros(B, dtype=torch.int32, device=DEV)]
    bufs = [torch.empty_like(q) for q in prist]
    pr, st, tok, pos, ln, log, logp, done = bufs
    for lg, kind in ((logits, "fp32"), (logits.to(BF16), "bf16")):
        t[f"sample_tokens {kind}"] = ("sample_tokens", _restoring(
            lambda lg=lg: o.sample_tokens(lg, pr, st, tok, pos, ln, log, done, 7, T, K, P, RP, True, seed),
            bufs, prist))
        t[f"sample_tokens_full {kind}"] = ("sample_tokens_full", _restoring(
            lambda lg=lg: o.sample_tokens_full(lg, pr, st, tok, pos, ln, log, logp, done, 7, T, RP, seed), bufs, prist))
        row = lg[1].contiguous()
        t[f"sample_token {kind}"] = ("sample_token", _restoring(
            lambda row=row: o.sample_token(row, pr[1], st[1], tok[1:2], pos[1:2], ln[1:2], log[1], T, K, P, RP, True, seed),
            bufs, prist))
    return t


def _optim_cases():
    o = _Recording()
    n = 3 * 4096 + 5  # not a multiple of any chunk
    p0, g = _r(n, seed=1), _r(n, seed=2)
    m0, v0 = _r(n, seed=3, scale=0.01), _r(n, seed=4, scale=0.001).abs()
    p, m, v = torch.empty_like(p0), torch.empty_like(m0), torch.empty_like(v0)
    coef = torch.tensor([0.7], device=DEV)

    def step():
        p.copy_(p0), m.copy_(m0), v.copy_(v0)
        o.adamw_flat(p, g, None, m, v, coef, 1e-3, 0.9, 0.95, 1e-8, 0.01, 0.1, 0.05, 11, 0)
        return p, m, v
    # chunks (offset, length) that overlap, are empty and end at the last element; their lengths no multiple of a block
    tab = [(0, 4096), (4096, 3), (5001, 7001), (17, 0), (n - 5, 5)]
    assert all(0 <= off and off + ln <= n for off, ln in tab)  # the op trusts its table: nothing past the operand
    chunks = torch.tensor(tab, dtype=torch.int64, device=DEV)
    return {"adamw_flat": ("adamw_flat", step),
            "sumsq_chunks": ("sumsq_chunks", lambda: (o.sumsq_chunks(g, chunks),))}


# What each group of the table must exercise. The completeness test reads this, so a new op needs a case in a group.
TABLE_OPS = {
    "_gemm_cases": {"gemm_tn", "gemm_tn_rope", "gemm_tn_swiglu", "gemm_skinny", "dgrad_gemm", "dgrad_gemm_delta"},
    "_multi_cases": {"wgrad_gemm_multi", "wgrad_gemm_pair"},
    "_rowwise_cases": {"rope_", "qk_norm_rope_fwd", "qk_norm_rope_bwd", "qkv_bias_rope_fwd", "qkv_bias_rope_bwd",
                       "dropout_add", "embedding_fwd", "embedding_noise_fwd", "embedding_bwd"},
    "_loss_cases": {"ce_fwd", "kd_fwd", "teacher_topk", "kd_topk_fwd", "seq_logp_sum", "dpo_pair_fwd", "seq_score_fwd",
                    "seq_score_bwd", "reward_pair_fwd", "grpo_token_fwd", "scale_rows_by_seq", "scale_rows_by_seq_",
                    "scale_rows", "scale_rows_"},
    "_lora_cases": {"lora_widen", "lora_fwd", "lora_fwd_inplace", "lora_bwd_dx", "lora_tsum", "lora_dxa",
                    "lora_dxa_blocks", "lora_grad_out", "lora_grad_out2", "copy2d_batch"},
    "_sampler_cases": {"sample_token", "sample_tokens", "sample_tokens_full"},
    "_optim_cases": {"adamw_flat", "sumsq_chunks"},
}
# The ops that a test of their own exercises, above.
STANDALONE_OPS = {
    "flash_fwd": "test_attention_d128_fill_independent", "flash_bwd": "test_attention_d128_fill_independent",
    "flash_bwd_rope": "test_attention_d128_fill_independent",
    "decode_attention": "test_decode_attention_fill_independent",
    "decode_attention_batched": "test_decode_attention_fill_independent",
    "rmsnorm_fwd": "test_rmsnorm_fill_independent", "rmsnorm_bwd": "test_rmsnorm_fill_independent",
    "swiglu_fwd": "test_swiglu_and_sumsq_fill_independent", "swiglu_bwd": "test_swiglu_and_sumsq_fill_independent",
    "sumsq": "test_swiglu_and_sumsq_fill_independent", "wgrad_gemm": "test_wgrad_fill_independent",
}
# Registered ops without a case, each with its reason. Nothing else may be exempt.
EXEMPT = {
    "ipc_ar_create": "multi-process: the IPC all-reduce has its own NaN poison (tests/test_ipc_allreduce_gpu.py)",
    "ipc_ar_handle": "multi-process, as ipc_ar_create",
    "ipc_ar_open": "multi-process, as ipc_ar_create",
    "ipc_ar_check": "multi-process, as ipc_ar_create",
    "ipc_ar_poll": "multi-process, as ipc_ar_create",
    "ipc_ar_uncached": "multi-process, as ipc_ar_create",
    "ipc_ar_destroy": "multi-process, as ipc_ar_create",
    "ipc_ar_allreduce": "multi-process, as ipc_ar_create",
    "ddp_plan": "host-side bucket planner of the multi-process DDP engine: no GPU memory",
    "ddp_tracker_create": "host-side ready tracker of the DDP engine: no GPU memory",
    "ddp_tracker_reset": "as ddp_tracker_create",
    "ddp_tracker_mark": "as ddp_tracker_create",
    "ddp_tracker_drain": "as ddp_tracker_create",
    "ddp_tracker_pending": "as ddp_tracker_create",
    "ddp_tracker_destroy": "as ddp_tracker_create",
    "dispatch_trace": "host-side switch of the dispatch trace: neither allocates nor launches",
    "dispatch_trace_read": "host-side read of the dispatch trace: neither allocates nor launches",
    "set_cu_budget": "host-side setting: neither allocates nor launches",
    "cu_hog": "a busy-wait kernel for overlap tests: writes one caller-owned sink, computes nothing",
    "pack_sequences": "host op of the data pipeline",
    "pad_batch": "host op of the data pipeline",
}
_EXEMPT_ALLOWED = re.compile(r"ipc_ar_\w+|ddp_\w+|dispatch_trace\w*|set_cu_budget|cu_hog|pack_sequences|pad_batch")


def test_every_registered_op_has_a_case():
    """The op names csrc/bindings.cpp registers, minus EXEMPT, are exactly the ops this file exercises. A new op fails
    here until it has a case (in a group of the table: add it to TABLE_OPS) built on tests/_stale.py."""
    src = pathlib.Path(__file__).resolve().parents[1] / "csrc" / "bindings.cpp"
    registered = set(re.findall(r'm\.def\(\s*"(\w+)\(', src.read_text()))
    assert len(registered) == src.read_text().count("m.def(") and {"flash_fwd", "set_cu_budget"} <= registered, \
        "the m.def pattern no longer matches every registration of csrc/bindings.cpp"
    assert all(_EXEMPT_ALLOWED.fullmatch(n) and reason for n, reason in EXEMPT.items()), "EXEMPT is capped"
    assert set(EXEMPT) <= registered, f"EXEMPT names ops that are not registered: {sorted(set(EXEMPT) - registered)}"
    exercised = set(STANDALONE_OPS).union(*TABLE_OPS.values())
    assert all(callable(globals().get(fn)) for fn in STANDALONE_OPS.values())
    missing, unknown = registered - set(EXEMPT) - exercised, exercised - registered
    assert not missing and not unknown, (f"registered ops without a stale-memory case: {sorted(missing)}; cases of ops "
                                         f"that are not registered: {sorted(unknown)}")


@pytest.mark.parametrize("group", sorted(TABLE_OPS))
def test_table_ops_fill_independent(group):
    """Every case of one group of the table. A case must call the op it is filed under (the recorder sees the call);
    the cases' failed assertions are reported together, each naming its case. Any other error ends the test at once:
    nothing more is launched after a kernel fault."""
    cases = globals()[group]()
    assert {op for op, _ in cases.values()} == TABLE_OPS[group]
    failed = []
    for name, (op, fn) in cases.items():
        CALLED.clear()
        try:
            _stale.assert_fill_independent(fn, name)
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:300]}")
        assert op in CALLED, f"{name}: the case never called {op}"
    assert not failed, "\n".join(failed)
