"""The LoRA adapter kernels (csrc/lora.hip: fwd_kernel, bwd_dx_kernel, tsum_kernel, grad_out_kernel,
copy2d_batch_kernel) bit for bit against the fp64 references of tests/_lora_exact.py, on small-integer operands for
which every output has exactly one right bit pattern (power-of-two adapter scale, dropout p in {0, 0.5}).

No comparison here uses a tolerance. The one exception in kind: the SwiGLU-fused instantiations (``swiglu=True``,
``gu``) take random bf16 gate / up values and are compared bit for bit with the two-kernel path, whose halves are pinned
exactly (the plain instantiation here, swiglu_fwd / swiglu_bwd in tests/test_rowwise_gpu.py).

The shapes reach every R (RF = 1 .. 4, the ``default:`` arms), the NCH = 4 and generic forward with the A prefetch on
and off, half and partial column chunks, one-lane and 8-column wave tails of the dx pass, token chunks of several
64-token stages with ragged last stages in the narrow and the wide reduction, partial column workgroups, the unrolled
body and the tail of the slab sum, second grid-stride passes, and the ops' refusals and empty inputs. Element indices
beyond 2^32 (T * K > 4.29e9) would need multi-gigabyte tensors and are left out. profiles/lora_exact_tests.md records
one run: wall times and the (T, K, R) -> splits table."""
import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext

import _lora_exact as lx
from _lora_exact import assert_bits_equal, case_id

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SEED = lx.SEED


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def ops():
    return _ext.ops()


def randn(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV).to(BF16)


def randint(shape, lo, hi, seed, dtype):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=DEV).to(dtype)


# ---------------------------------------------------------------------------------------------------- lora_fwd
@pytest.mark.parametrize("c", lx.FWD_CASES, ids=case_id)
def test_lora_fwd_exact(c):
    T, K, R, s, p = c["T"], c["K"], c["R"], c["s"], c["p"]
    ldX = lx.fwd_ldX(c)
    x, A = lx.fwd_operands(c, DEV)
    want_X, want_xd = lx.fwd_want(x, A, s, p, SEED, ldX)
    X, xd = ops().lora_fwd(x, A, s, p, SEED, ldX, c["save_xd"])
    assert X.shape == (T, ldX or K + R)
    assert_bits_equal(X, want_X, "X'")
    if c["save_xd"] and p > 0:
        assert_bits_equal(xd, want_xd, "xd")
    else:
        assert xd.numel() == 0
    # in place: x already in the left block, a sentinel everywhere else
    Xi = torch.full((T, ldX or K + R), 7.0, device=DEV, dtype=BF16)
    Xi[:, :K] = x
    ops().lora_fwd_inplace(Xi, K, A, s, p, SEED)
    assert_bits_equal(Xi[:, :K], x, "in place: left block")
    assert_bits_equal(Xi, want_X, "in place")


@pytest.mark.parametrize("c", lx.FWD_SW_CASES, ids=case_id)
def test_lora_fwd_swiglu_matches_two_kernels(c):
    T, K, R, s, p = c["T"], c["K"], c["R"], c["s"], c["p"]
    ldX = lx.fwd_ldX(c)
    gu = randn(T, 2 * K, seed=41 + T + K + R)
    A = lx.fwd_operands(c, DEV)[1]
    act = ops().swiglu_fwd(gu)
    Xs, xd = ops().lora_fwd(gu, A, s, p, SEED, ldX, False, True)
    assert xd.numel() == 0 and Xs.shape == (T, ldX or K + R)
    assert_bits_equal(Xs[:, :K], act, "activation")
    assert_bits_equal(Xs, ops().lora_fwd(act, A, s, p, SEED, ldX)[0], "X' of gu")


# ---------------------------------------------------------------------------------------------------- lora_bwd_dx
@pytest.mark.parametrize("c", lx.BWD_CASES, ids=case_id)
def test_lora_bwd_dx_exact(c):
    T, K, R, p = c["T"], c["K"], c["R"], c["p"]
    base, dxa, A = lx.bwd_operands(c, DEV)
    assert base.is_contiguous() != c["sliced"] or T == 1
    keep_base = base.clone()
    dx = ops().lora_bwd_dx(base, dxa, A, p, SEED)
    assert dx.shape == (T, K)
    assert_bits_equal(dx, lx.bwd_dx_want(base, dxa, A, p, SEED), "dx")
    assert_bits_equal(base, keep_base, "base (input)")
    # the SwiGLU-fused instantiation: dgu = swiglu_bwd(dx, gu) in the same pass
    gu = randn(T, 2 * K, seed=42 + T + K + R)
    dgu = ops().lora_bwd_dx(base, dxa, A, p, SEED, gu)
    assert_bits_equal(dgu, ops().swiglu_bwd(dx, gu), "dgu")


# ---------------------------------------------------------------------------------------------------- lora_tsum
@pytest.mark.parametrize("c", lx.TSUM_CASES, ids=case_id)
def test_lora_tsum_exact(c):
    T, K, R, p = c["T"], c["K"], c["R"], c["p"]
    X, S = lx.tsum_operands(c, DEV)
    assert X.stride(0) == K + 72 and S.stride(0) == R + 24 and S.data_ptr() % 16 == 0
    out = ops().lora_tsum(X, K, S, p, SEED)
    splits = out.shape[0]
    print(f"\n[lora_tsum] (T, K, R) = ({T}, {K}, {R}) -> splits {splits}")
    assert out.dtype == torch.float32 and out.shape == (splits, R, K)
    if c["prop"] == "multi":  # some chunk runs more than one 64-token stage
        assert splits * 64 < T, (splits, T)
    elif c["prop"] == "tail3":  # chunks are whole stages: this many of them are one stage each, the last 3 tokens
        assert splits == -(-T // 64) and T % 64 == 3, (splits, T)
    assert torch.isfinite(out).all()
    assert_bits_equal(out.sum(0), lx.tsum_want(X, K, S, p, SEED), "sum of the slabs")


# ---------------------------------------------------------------------------------------------------- lora_grad_out
PAD, SENT = 24, 12345.0  # sentinel elements on either side of every output (12345 rounds to 12352 in bf16)


class Out:
    """An output tensor that is the contiguous middle of a larger sentinel-filled buffer."""

    def __init__(self, shape, dtype, seed, r0, c0, tr, acc):
        n = shape[0] * shape[1]
        self.buf = torch.full((n + 2 * PAD,), SENT, device=DEV, dtype=dtype)
        self.t = self.buf[PAD:PAD + n].view(shape)
        self.t.copy_(randint(shape, -4, 4, seed, dtype))
        self.old, self.r0, self.c0, self.tr, self.acc = self.t.clone(), r0, c0, tr, acc

    def check(self, sum_, what):
        n = self.old.numel()
        assert_bits_equal(self.t, lx.grad_out_want(sum_, self.old, self.r0, self.c0, self.tr, self.acc), what)
        guard = torch.full((PAD,), SENT, device=DEV, dtype=self.buf.dtype)
        assert_bits_equal(self.buf[:PAD], guard, what + ": elements before")
        assert_bits_equal(self.buf[PAD + n:], guard, what + ": elements after")


def slabs(ns, R, K, seed):
    """Integer fp32 sums [ns, R, K], or the 2-D [R, K] form for ns == 0."""
    return randint((ns, R, K) if ns else (R, K), -4, 4, seed, torch.float32)


def four_outs(R, K, tr, seed):
    """bf16 / fp32, written / accumulated, blocks at zero and non-zero r0 / c0 (one touching the last row and column);
    ``tr``: out [nc, nr]."""
    spec = [(BF16, 0, 0, 16, 40, 0), (torch.float32, 16, 8, 8, 24, 1), (BF16, R - 16, K - 72, 16, 72, 1),
            (torch.float32, 3, 5, 7, 9, 0)]
    return [Out((nc, nr) if tr else (nr, nc), dt, seed + i, r0, c0, tr, acc)
            for i, (dt, r0, c0, nr, nc, acc) in enumerate(spec)]


def call_args(outs):
    return [o.t for o in outs], [o.r0 for o in outs], [o.c0 for o in outs], outs[0].tr, [int(o.acc) for o in outs]


@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("ns", [0, 1, 7, 8, 9, 17])  # 0: the 2-D [R, K] form
def test_lora_grad_out_exact(ns, tr):
    R, K = 32, 136
    sum_ = slabs(ns, R, K, 50 + ns)
    keep = sum_.clone()
    outs = four_outs(R, K, tr, 60 + ns)
    ops().lora_grad_out(sum_, *call_args(outs))
    for i, o in enumerate(outs):
        o.check(sum_, f"output {i}")
    assert_bits_equal(sum_, keep, "sum (input)")


@pytest.mark.parametrize("ns_a,ns_b", [(9, 0), (7, 17)])
def test_lora_grad_out2_exact(ns_a, ns_b):
    sa, sb = slabs(ns_a, 48, 136, 70), slabs(ns_b, 32, 200, 71)
    oa, ob = four_outs(48, 136, True, 72), four_outs(32, 200, False, 76)
    ops().lora_grad_out2(sa, *call_args(oa), sb, *call_args(ob))
    for i, o in enumerate(oa):
        o.check(sa, f"group a output {i}")
    for i, o in enumerate(ob):
        o.check(sb, f"group b output {i}")


@pytest.mark.parametrize("tr", [False, True])
def test_lora_grad_out_grid_stride(tr):
    """One output of 16 x 16392 = 262272 elements, more than the 1024 x 256 threads of the largest grid: a second
    grid-stride pass; the small output of the same launch is not touched beyond its own extent."""
    R, K = 16, 16392
    sum_ = slabs(2, R, K, 80)
    big = Out((K, R) if tr else (R, K), torch.float32, 81, 0, 0, tr, 1)
    small = Out((8, 8), BF16, 82, 8, K - 8, tr, 0)
    assert big.old.numel() > 1024 * 256
    ops().lora_grad_out(sum_, *call_args([big, small]))
    big.check(sum_, "big")
    small.check(sum_, "small")


# ---------------------------------------------------------------------------------------------------- copy2d_batch
def test_copy2d_batch_exact():
    # (rows, cols, src row stride, dst row stride): the first two above 64 x 256 elements (a second grid-stride pass)
    spec = [(70, 300, 320, 304), (16, 2048, 2048, 2048 + 64), (1, 77, 77, 100), (0, 16, 16, 16), (33, 5, 9, 7),
            (48, 16, 16, 2176)]
    most = max(r * c for r, c, _, _ in spec)
    assert most > 64 * 256
    srcs, dsts, wants, rows = [], [], [], []
    for i, (r, c, lds, ldd) in enumerate(spec):
        src = lx.int_operand((max(r, 1) * lds + 16,), -200, 200, 90 + i, DEV)
        dst = torch.full(((max(r, 1) + 2) * ldd,), 7.0, device=DEV, dtype=BF16)
        so, do = 8, ldd + 3  # the copies start inside their buffers
        want = dst.clone()
        for j in range(r):
            want[do + j * ldd:do + j * ldd + c] = src[so + j * lds:so + j * lds + c]
        srcs.append(src), dsts.append(dst), wants.append(want)
        rows.append([src.data_ptr() + 2 * so, dst.data_ptr() + 2 * do, r, c, lds, ldd])
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    keep_src = [s.clone() for s in srcs]
    ops().copy2d_batch(table[:0], most)  # no copies
    ops().copy2d_batch(table, 0)  # nothing to copy
    for i, d in enumerate(dsts):
        assert_bits_equal(d, torch.full_like(d, 7.0), f"no-op call, destination {i}")
    ops().copy2d_batch(table, most)
    for i, (d, w) in enumerate(zip(dsts, wants)):
        assert_bits_equal(d, w, f"destination {i} {spec[i]}")
        assert_bits_equal(srcs[i], keep_src[i], f"source {i}")


# ---------------------------------------------------------------------------------------------------- refusals
def z(*shape, dtype=BF16):
    return torch.zeros(*shape, device=DEV, dtype=dtype)


def refused(fn, *args):
    with pytest.raises(RuntimeError):
        fn(*args)
    torch.cuda.synchronize()  # a refusal is made on the host: nothing was launched, nothing is pending


def test_lora_fwd_refusals():
    f = ops().lora_fwd
    refused(f, z(4, 264), z(16, 264), 0.5, 0.0, 1)  # K % 256 != 0
    refused(f, z(4, 0), z(16, 0), 0.5, 0.0, 1)  # K == 0
    refused(f, z(4, 256), z(8, 256), 0.5, 0.0, 1)  # R = 8
    refused(f, z(4, 256), z(80, 256), 0.5, 0.0, 1)  # R = 80
    refused(f, z(4, 256), z(16, 256), 0.5, 0.0, 1, 256 + 8)  # ldX < K + R
    refused(f, z(4, 256), z(16, 256), 0.5, 0.0, 1, 256 + 16 + 4)  # ldX % 8 != 0
    refused(f, z(4, 512), z(16, 256), 0.5, 0.5, 1, 0, True, True)  # swiglu with save_xd
    fi = ops().lora_fwd_inplace
    refused(fi, z(4, 264 + 16), 264, z(16, 264), 0.5, 0.0, 1)
    refused(fi, z(4, 16), 0, z(16, 0), 0.5, 0.0, 1)  # K == 0
    refused(fi, z(4, 256 + 8), 256, z(16, 256), 0.5, 0.0, 1)  # ldX < K + R
    refused(fi, z(4, 256 + 80), 256, z(80, 256), 0.5, 0.0, 1)


def test_lora_bwd_dx_refusals():
    f = ops().lora_bwd_dx
    refused(f, z(4, 64), z(4, 80), z(80, 64), 0.0, 1)  # R = 80
    refused(f, z(4, 64), z(4, 0), z(0, 64), 0.0, 1)  # R = 0
    refused(f, z(4, 64), z(4, 16), z(16, 64), 0.0, 1, z(4, 64))  # gu of the wrong width
    refused(f, z(4, 72)[:, 4:68], z(4, 16), z(16, 64), 0.0, 1)  # base rows not 16-byte aligned
    refused(f, z(4, 0), z(4, 16), z(16, 0), 0.0, 1)  # K == 0


def test_lora_tsum_refusals():
    f = ops().lora_tsum
    refused(f, z(4, 64), 64, z(4, 80), 0.0, 1)  # R = 80
    refused(f, z(4, 64), 64, z(5, 16), 0.0, 1)  # S with the wrong row count
    refused(f, z(4, 24)[:, 4:], 16, z(4, 16), 0.0, 1)  # X rows not 16-byte aligned
    refused(f, z(4, 24)[:, 4:20], 16, z(4, 16), 0.0, 1)
    refused(f, z(4, 64), 64, z(4, 24)[:, 4:20], 0.0, 1)  # S rows not 16-byte aligned
    refused(f, z(4, 64), 0, z(4, 16), 0.0, 1)  # K == 0


def test_lora_dxa_blocks_refusals():
    f = ops().lora_dxa_blocks
    dy = z(4, 80)
    refused(f, dy, z(80, 80), [0, 16, 32, 48, 64], [16] * 5, [0, 16, 32, 48, 64], 16, 0.5)  # five blocks
    refused(f, dy, z(80, 48), [0], [80], [0], 48, 0.5)  # r = 48
    refused(f, dy, z(80, 32), [0, 48], [48, 40], [0, 16], 16, 0.5)  # a block past n


def test_lora_grad_out_refusals():
    f = ops().lora_grad_out
    sum_ = z(2, 16, 64, dtype=torch.float32)
    refused(f, sum_, [z(8, 8)], [9], [0], False, [0])  # rows past R
    refused(f, sum_, [z(8, 8)], [0], [60], False, [0])  # columns past K
    refused(f, sum_, [z(8, 8)], [0], [60], True, [0])
    refused(f, sum_, [z(1, 1) for _ in range(9)], [0] * 9, [0] * 9, False, [0] * 9)  # nine outputs


def test_copy2d_batch_refusals():
    f = ops().copy2d_batch
    refused(f, z(2, 5, dtype=torch.int64), 16)
    refused(f, z(12, dtype=torch.int64), 16)
    refused(f, z(2, 6, dtype=torch.int32), 16)


# ---------------------------------------------------------------------------------------------------- empty inputs
@pytest.mark.parametrize("R", [16, 64])
def test_lora_ops_without_tokens(R):
    K = 256
    A = lx.int_operand((R, K), -2, 2, 1, DEV)
    for save_xd in (False, True):
        X, xd = ops().lora_fwd(z(0, K), A, 0.5, 0.5, SEED, K + R + 8, save_xd)
        assert X.shape == (0, K + R + 8) and X.dtype == BF16
        assert xd.shape == ((0, K) if save_xd else (0,))
    X, xd = ops().lora_fwd(z(0, 2 * K), A, 0.5, 0.0, SEED, 0, False, True)
    assert X.shape == (0, K + R) and xd.numel() == 0
    assert ops().lora_fwd_inplace(z(0, K + R), K, A, 0.5, 0.0, SEED) is None
    assert ops().lora_bwd_dx(z(0, K), z(0, R), A, 0.5, SEED).shape == (0, K)
    assert ops().lora_bwd_dx(z(0, K), z(0, R), A, 0.5, SEED, z(0, 2 * K)).shape == (0, 2 * K)
    out = ops().lora_tsum(z(0, K + 8), K, z(0, R), 0.5, SEED)
    assert out.shape == (1, R, K) and out.dtype == torch.float32 and not out.any()
    assert ops().lora_dxa(z(0, K), z(K, R), 0.5).shape == (0, R)
    assert ops().lora_dxa_blocks(z(0, K), z(K, R), [0], [K], [0], 16, 0.5).shape == (0, R)
    torch.cuda.synchronize()
