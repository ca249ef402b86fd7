"""Per-row checks of the RMSNorm, SwiGLU, RoPE, embedding and dropout kernels (csrc/rmsnorm.hip, csrc/elementwise.hip)
against fp64, at the shapes where their dispatch changes: every NV variant with a full and a predicated last vector
group, row counts that are no multiple of the rows per block, every partial count P of the dW reduction, the second
grid-stride pass with a ragged tail, more rows than gridDim.y holds.

Every bound is 2 x the worst per-row error of a torch fp32 emulation with the kernel's rounding points (tests/_rowwise.py)
against the fp64 reference, computed here from the references alone; what is exactly determined (the residual sum, the
gather, integer RoPE, dropout masks, copies, pass-through columns) is compared bit for bit. Each test prints its worst
measured error next to its bound (pytest -s); profiles/rowwise_kernel_errors.md records one run."""
import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

import _rowwise as rw
from _blockwise import assert_blocks_close, block_rel_err, int_operand, swiglu_bwd_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
EPS = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16)


def report(what, worst, bound):
    print(f"\n[rowwise] {what}: worst {worst:.3e} bound {bound:.3e}")


def randn(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV).to(BF16)


def norm_weight(H, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (1 + 0.1 * torch.randn(H, generator=g, device=DEV)).to(BF16)


# ------------------------------------------------------------------------------------------------ RMSNorm forward
# lanes of the last vector group predicated off: NV = 1 at H = 8 (one lane live) and 64, NV = 2 at 520 and 640, NV = 4
# at 1032, NV = 8 at 2056 and 2560 (qwen3-4b); every lane live: NV = 1 / 2 / 4 / 8 at 512 / 1024 / 2048 / 4096
FWD_H = [8, 64, 512, 520, 640, 1024, 1032, 2048, 2056, 2560, 4096]
FWD_M = [1, 3, 5, 67]


def _fwd_inputs(M, H, with_res):
    x = randn(M, H, seed=1000 + M * 7 + H)
    r = randn(M, H, seed=2000 + M * 7 + H) if with_res else None
    return x, r, norm_weight(H, 3000 + H)


@pytest.fixture(scope="module")
def rstd_bound():
    """2 x the worst relative error of the fp32 wave-order rstd emulation over every (M, H, residual) case of the grid:
    pooled, since one row (M = 1) is no sample of a rounding error."""
    worst = 0.0
    for M in FWD_M:
        for H in FWD_H:
            for with_res in (False, True):
                x, r, w = _fwd_inputs(M, H, with_res)
                _, _, rstd64, _, rstd_em = rw.rmsnorm_fwd_refs(x, r, w, EPS)
                worst = max(worst, ((rstd_em.double() - rstd64).abs() / rstd64).max().item())
    return 2 * worst


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("H", FWD_H)
@pytest.mark.parametrize("M", FWD_M)
def test_rmsnorm_fwd_rows(M, H, with_res, rstd_bound):
    x, r, w = _fwd_inputs(M, H, with_res)
    y, ro, rstd = _ext.ops().rmsnorm_fwd(x, r, w, EPS)
    h, y64, rstd64, y_em, _ = rw.rmsnorm_fwd_refs(x, r, w, EPS)
    assert torch.equal(bits(ro), bits(h))  # bf16(x + r), or x itself
    bound = rw.row_bound(y_em, y64)
    worst = assert_blocks_close(y, y64, 1, H, bound, f"rmsnorm_fwd y M={M} H={H}")
    e_rstd = ((rstd.double() - rstd64).abs() / rstd64).max().item()
    report(f"rmsnorm_fwd M={M} H={H} res={with_res}: rstd {e_rstd:.3e} (bound {rstd_bound:.3e}); y", worst, bound)
    assert rstd.dtype == torch.float32 and e_rstd <= rstd_bound


@pytest.mark.parametrize("M,H", [(5, 520), (67, 2560)])
def test_rmsnorm_fwd_wide_output_writes_the_left_block_only(M, H):
    x, r, w = _fwd_inputs(M, H, True)
    y0, ro0, rstd0 = _ext.ops().rmsnorm_fwd(x, r, w, EPS, 0)
    ld = H + 128
    y, ro, rstd = _ext.ops().rmsnorm_fwd(x, r, w, EPS, ld)
    assert y.shape == x.shape and y.stride(-2) == ld and y.stride(-1) == 1
    # the [M, ld] buffer behind y: fill its right block, then the left block must still hold what y_ld = 0 gives
    buf = torch.as_strided(y, (M, ld), (ld, 1))
    buf[:, H:] = 7.0
    torch.cuda.synchronize()
    assert torch.equal(bits(buf[:, :H]), bits(y0)) and bool((buf[:, H:] == 7.0).all())
    assert torch.equal(bits(y), bits(y0))  # the strided view reads the left block
    assert torch.equal(bits(ro), bits(ro0)) and torch.equal(rstd, rstd0)


# ------------------------------------------------------------------------------------------------ RMSNorm backward
# P = min(ceil(M / 16), 512) partial rows: 1, 5, 64, 65, 128, 129, 512
BWD_CASES = [(1, H) for H in FWD_H] + [(67, H) for H in FWD_H] + \
            [(M, H) for M in (1024, 1025, 2048, 2049, 8200) for H in (72, 520)]


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("M,H", BWD_CASES)
def test_rmsnorm_bwd_rows_and_columns(M, H, with_dres):
    assert min(-(-M // 16), 512) in (1, 5, 64, 65, 128, 129, 512)
    h = randn(M, H, seed=4000 + M + H)
    dy = randn(M, H, seed=5000 + M + H)
    dres = randn(M, H, seed=6000 + M + H) if with_dres else None
    w = norm_weight(H, 7000 + H)
    _, _, rstd = _ext.ops().rmsnorm_fwd(h, None, w, EPS)
    dx, dw = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, dres)
    dx2, dw2 = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, dres)
    assert torch.equal(bits(dx), bits(dx2)) and torch.equal(dw, dw2)  # fixed-order reductions
    dx64, dw64, dx_em, dw_em = rw.rmsnorm_bwd_refs(dy, h, w, rstd, dres)
    b_dx = rw.row_bound(dx_em, dx64)
    e_dx = assert_blocks_close(dx, dx64, 1, H, b_dx, f"rmsnorm_bwd dx M={M} H={H}")
    # dW per column, each against max(|dW_c|, rms(dW)); fp32, so the bound is the fp32 column sum's own error
    b_dw = 2 * rw.rel_elem_err(dw_em, dw64)
    e_dw = assert_blocks_close(dw.view(1, H), dw64.view(1, H), 1, 1, b_dw, f"rmsnorm_bwd dW M={M} H={H}")
    report(f"rmsnorm_bwd M={M} H={H} dres={with_dres}: dW {e_dw:.3e} (bound {b_dw:.3e}); dx", e_dx, b_dx)


@pytest.mark.parametrize("M,H", [(67, 520), (1025, 72), (2049, 520), (67, 4096)])
def test_rmsnorm_bwd_dw_out_slice(M, H):
    """dW written, then accumulated, into a slice of a sentinel buffer: per column against fp64, guards on both sides."""
    h = randn(M, H, seed=4100 + M + H)
    dy = randn(M, H, seed=5100 + M + H)
    w = norm_weight(H, 7100 + H)
    _, _, rstd = _ext.ops().rmsnorm_fwd(h, None, w, EPS)
    dx_ref, dw_ref = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, None)
    _, dw64, _, dw_em = rw.rmsnorm_bwd_refs(dy, h, w, rstd, None)
    G = 64
    buf = torch.full((G + H + G,), 7.0, device=DEV, dtype=BF16)
    out = buf[G:G + H]
    dx, dw = _ext.ops().rmsnorm_bwd(dy, h, w, rstd, None, out, False)
    assert dw.numel() == 0 and torch.equal(bits(dx), bits(dx_ref))
    assert torch.equal(bits(out), bits(dw_ref.to(BF16)))  # the fp32 dW rounded once
    b_w = 2 * rw.rel_elem_err(dw_em.to(BF16), dw64)
    e_w = assert_blocks_close(out.view(1, H), dw64.view(1, H), 1, 1, b_w, f"dw_out write M={M} H={H}")
    old = out.clone()
    _ext.ops().rmsnorm_bwd(dy, h, w, rstd, None, out, True)
    want_acc = dw64 + old.double()
    b_a = 2 * rw.rel_elem_err((dw_em + old.float()).to(BF16), want_acc)
    e_a = assert_blocks_close(out.view(1, H), want_acc.view(1, H), 1, 1, b_a, f"dw_out accumulate M={M} H={H}")
    assert bool((buf[:G] == 7.0).all()) and bool((buf[G + H:] == 7.0).all())
    report(f"rmsnorm_bwd dw_out M={M} H={H}: write {e_w:.3e} (bound {b_w:.3e}); accumulate", e_a, b_a)


# ------------------------------------------------------------------------------------------------ SwiGLU
# (2047, 8200): 2,098,175 vectors = one full pass of 2048 blocks x 256 threads x 4 vectors and a second pass of 1023
SWIGLU_SHAPES = [(1, 8), (3, 24), (5, 9728), (2047, 8200)]


@pytest.mark.parametrize("M,I", SWIGLU_SHAPES)
def test_swiglu_rows(M, I):
    if M * I // 8 > 2048 * 256 * 4:
        assert 0 < M * I // 8 - 2048 * 256 * 4 < 2048 * 256 * 4 and (M * I // 8) % 256 != 0
    gu = randn(M, 2 * I, seed=8000 + M + I)
    out = _ext.ops().swiglu_fwd(gu)
    want, em = rw.swiglu_fwd_refs(gu)
    b_f = rw.row_bound(em, want)
    e_f = assert_blocks_close(out, want, 1, I, b_f, f"swiglu_fwd M={M} I={I}")
    del want, em
    dy = randn(M, I, seed=9000 + M + I)
    dgu = _ext.ops().swiglu_bwd(dy, gu)
    want_b, b_b = swiglu_bwd_reference(dy.double(), gu, 1, 2 * I)
    e_b = assert_blocks_close(dgu, want_b, 1, 2 * I, b_b, f"swiglu_bwd M={M} I={I}")
    report(f"swiglu M={M} I={I}: fwd {e_f:.3e} (bound {b_f:.3e}); bwd", e_b, b_b)


# ------------------------------------------------------------------------------------------------ RoPE
# (4099, 48, 16, 32): 4099 * 64 heads * 2 chunks = 524,672 work items, 384 more than the 2048 x 256 of one pass
ROPE_SHAPES = [(37, 3, 2, 128), (37, 4, 1, 64), (67, 5, 3, 32), (4099, 48, 16, 32)]


def _cos_sin(M, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pos = torch.randint(0, 4000, (M,), generator=g, device=DEV)
    cos, sin = ref.rope_cos_sin(pos, D, 2e6)
    return cos.contiguous(), sin.contiguous()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("M,nq,nkv,D", ROPE_SHAPES)
def test_rope_rows_and_heads(M, nq, nkv, D, inverse):
    nh, ld = nq + nkv, (nq + 2 * nkv) * D
    qkv = randn(M, ld, seed=100 + M + D)
    cos, sin = _cos_sin(M, D, 200 + M + D)
    got = qkv.clone()
    _ext.ops().rope_(got, cos, sin, nq, nkv, D, inverse)
    want, em = rw.rope_refs(qkv[:, : nh * D].view(M, nh, D), cos, sin, inverse)
    want, em = want.reshape(M * nh, D), em.reshape(M * nh, D)
    bound = rw.row_bound(em, want)
    worst = assert_blocks_close(got[:, : nh * D].reshape(M * nh, D), want, 1, D, bound, f"rope M={M} D={D}")
    assert torch.equal(bits(got[:, nh * D:]), bits(qkv[:, nh * D:]))  # the V columns pass through
    report(f"rope M={M} nq={nq} nkv={nkv} D={D} inverse={inverse}", worst, bound)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_rope_integer_operands_bit_exact(D, inverse):
    """cos, sin in {0, +-1} on integers |x| <= 100: every output is an integer of magnitude <= 200, exact in bf16, so
    there is one right answer whatever the order of the two products."""
    M, nq, nkv = 133, 3, 2
    nh = nq + nkv
    qkv = int_operand((M, (nq + 2 * nkv) * D), -100, 100, 300 + D, DEV)
    cos = int_operand((M, D // 2), -1, 1, 400 + D, DEV).float()
    sin = int_operand((M, D // 2), -1, 1, 500 + D, DEV).float()
    got = qkv.clone()
    _ext.ops().rope_(got, cos, sin, nq, nkv, D, inverse)
    want = ref.apply_rope(qkv[:, : nh * D].view(M, nh, D).double(), cos.double(), sin.double(), inverse=inverse)
    assert want.abs().max().item() <= 200 and want.abs().max().item() > 100
    assert torch.equal(bits(got[:, : nh * D]), bits(want.reshape(M, nh * D).to(BF16)))
    assert torch.equal(bits(got[:, nh * D:]), bits(qkv[:, nh * D:]))


def test_rope_argument_checks():
    """rope_ goes through the checker of its siblings (csrc/qkv_rows.h): a good call still rotates, the inverse after
    the forward returns the input, and a call whose 16-byte accesses would leave the tensors or be misaligned raises
    on the host with the tensor untouched."""
    M, nq, nkv, D = 3, 2, 1, 128
    nh, ld = nq + nkv, (nq + 2 * nkv) * D
    rope = _ext.ops().rope_
    qkv = randn(M, ld, seed=700)
    cos, sin = _cos_sin(M, D, 701)
    qk = qkv[:, : nh * D].view(M, nh, D)

    got = qkv.clone()
    rope(got, cos, sin, nq, nkv, D, False)
    want, em = rw.rope_refs(qk, cos, sin, False)
    want, em = want.reshape(M * nh, D), em.reshape(M * nh, D)
    bound = rw.row_bound(em, want)
    worst = assert_blocks_close(got[:, : nh * D].reshape(M * nh, D), want, 1, D, bound, "rope good call")
    assert torch.equal(bits(got[:, nh * D:]), bits(qkv[:, nh * D:]))
    report("rope_ good call", worst, bound)

    # the inverse of the rotated bf16 output, emulated with the same two roundings
    rope(got, cos, sin, nq, nkv, D, True)
    back = qk.double().reshape(M * nh, D)
    em2 = rw.rope_refs(em.view(M, nh, D), cos, sin, True)[1].reshape(M * nh, D)
    bound = rw.row_bound(em2, back)
    worst = assert_blocks_close(got[:, : nh * D].reshape(M * nh, D), back, 1, D, bound, "rope inverse after forward")
    assert torch.equal(bits(got[:, nh * D:]), bits(qkv[:, nh * D:]))
    report("rope_ inverse after forward", worst, bound)

    def refused(x, c, s, msg):
        before = x.clone()
        with pytest.raises(RuntimeError, match=msg):
            rope(x, c, s, nq, nkv, D, False)
        assert torch.equal(bits(x), bits(before))  # nothing was launched

    refused(qkv.cpu(), cos, sin, "qkv must be")
    refused(qkv.clone(), cos, sin[: M - 1], "cos table")
    refused(randn(M, 2 * D, seed=702), cos, sin, "row width")       # narrower than the three rotated heads
    refused(randn(M, ld + 4, seed=703), cos, sin, "row width")      # rows not a multiple of 16 bytes
    off1 = torch.zeros(M * ld + 1, dtype=BF16, device=DEV)[1:].view(M, ld)  # contiguous, 2 bytes into its storage
    assert off1.is_contiguous() and off1.data_ptr() % 16 == 2
    refused(off1, cos, sin, "aligned")


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("H", [8, 520, 2560, 4096])
def test_embedding_fwd_bitwise(H):
    V, M = 50, 37
    # a last block of the grid that is only partly full (H = 4096 has 512 vectors per row: always whole blocks)
    assert (M * H // 8) % 256 != 0 or H == 4096
    w = randn(V, H, seed=600 + H)
    g = torch.Generator(device=DEV).manual_seed(601 + H)
    ids = torch.randint(0, V, (M,), generator=g, device=DEV)
    ids[3], ids[M - 1] = 0, V - 1
    out = _ext.ops().embedding_fwd(ids, w)
    assert out.shape == (M, H) and torch.equal(bits(out), bits(w[ids]))


RUNS = [1, 7, 8, 9, 16, 17]


@pytest.mark.parametrize("last_run", [3, 4, 5])  # M = 61, 62, 63: M % 4 = 1, 2, 3
@pytest.mark.parametrize("H", [64, 520, 1032, 2560, 4096])
def test_embedding_bwd_rows(H, last_run):
    V = 40
    run_ids = [0, 5, 6, 11, 20, 21, V - 1]  # ids 0 and V - 1 present, the last run ends at M
    ids = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in zip(run_ids, RUNS + [last_run])])
    M = ids.numel()
    assert M % 4 == last_run - 2 and M % 4 != 0
    ids = ids[torch.randperm(M, generator=torch.Generator().manual_seed(H + last_run))].to(DEV)
    dy = randn(M, H, seed=700 + H + last_run)
    g0 = randn(V, H, seed=800 + H)
    s, perm = torch.sort(ids.to(torch.int32), stable=True)
    assert int(s[-1]) == V - 1 and int(s[0]) == 0
    g = g0.clone()
    _ext.ops().embedding_bwd(dy, s, perm.to(torch.int32), g)
    g2 = g0.clone()
    _ext.ops().embedding_bwd(dy, s, perm.to(torch.int32), g2)
    assert torch.equal(bits(g), bits(g2))  # deterministic
    want, em = rw.embedding_bwd_refs(g0, ids, dy)
    bound = rw.row_bound(em, want)
    worst = assert_blocks_close(g, want, 1, H, bound, f"embedding_bwd H={H} M={M}")
    absent = torch.ones(V, dtype=torch.bool, device=DEV)
    absent[ids] = False
    assert int(absent.sum()) == V - len(run_ids)
    assert torch.equal(bits(g[absent]), bits(g0[absent]))  # rows whose id is absent: untouched
    report(f"embedding_bwd H={H} M={M}", worst, bound)


# ------------------------------------------------------------------------------------------------ dropout / widen
T_BIG = 65536 + 3  # gridDim.y is capped at 65535: rows 65535 .. 65538 come from the second pass of the row loop


@pytest.mark.parametrize("K", [8, 264])
def test_dropout_add_many_rows(K):
    p, seed = 0.25, 4321
    wide = randn(T_BIG, 2 * K + 16, seed=900 + K)
    a, b = wide[:, 8:8 + K], wide[:, 8 + K:8 + 2 * K]  # strided column slices
    keep, want, em = rw.dropout_add_refs(a, b, p, seed)
    got = _ext.ops().dropout_add(a, b, p, seed)
    bound = rw.row_bound(em, want)
    worst = assert_blocks_close(got, want, 1, K, bound, f"dropout_add K={K}")
    # the mask itself, bit for bit: without a, an output is non-zero exactly where it is kept and b is non-zero
    keep0, want0, em0 = rw.dropout_add_refs(None, b, p, seed)
    got0 = _ext.ops().dropout_add(None, b, p, seed)
    assert torch.equal(got0 != 0, keep0 & (b != 0))
    assert torch.equal(bits(got0), bits(em0))  # one fp32 product, one rounding: exactly determined
    assert 0.7 < keep.float().mean().item() < 0.8
    report(f"dropout_add T={T_BIG} K={K}", worst, bound)


@pytest.mark.parametrize("K", [8, 264])
def test_lora_widen_many_rows(K):
    p, seed, R = 0.25, 977, 16
    x = randn(T_BIG, K, seed=950 + K)
    X, xd = _ext.ops().lora_widen(x, R, p, seed)
    assert X.shape == (T_BIG, K + R) and torch.equal(bits(X[:, :K]), bits(x))  # the copy
    keep, _, em = rw.dropout_add_refs(None, x, p, seed)
    assert torch.equal(xd != 0, keep & (x != 0))
    assert torch.equal(bits(xd), bits(em))
    X0, xd0 = _ext.ops().lora_widen(x, R, 0.0, seed)
    assert xd0.numel() == 0 and torch.equal(bits(X0[:, :K]), bits(x))
