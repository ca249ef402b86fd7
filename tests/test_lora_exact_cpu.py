"""tests/_lora_exact.py on the CPU, no kernel involved: its fp64 references against the twins of ops/reference.py where
those round at the same points, the proof that every case of tests/test_lora_exact_gpu.py is in the exact regime (every
partial sum below 2^24 whatever the summation order), the coverage the case tables promise, and the sensitivity of the
bit-for-bit comparison: single defects of the kinds csrc/lora.hip can have, planted into a correct result, are each
reported with their place, while the whole-tensor tolerances of tests/test_kernels_gpu.py::test_lora_fwd_bwd_kernels,
applied to that test's own operands, mostly let the same defects through (figures printed with pytest -s):

    planted defect                                              old check            old figure               old bound
    mask of one 8-element chunk shifted by one chunk, p = 0.05  adapter cols, max    7.8e-3                   1.2e-1
      at p = 0.3 / 0.5 (the forward's max norm sees these)                           3.1e-1 / 3.6e-1          1.3 / 1.7e-1
    the same in lora_tsum's dA, p = 0.05 / 0.3 / 0.5            rel_err              2.3e-4 / 6.6e-3 / 7.0e-3 1e-2
    last token of a chunk left out of one 64-column slab        rel_err              3.3e-3 (old operands:    1e-2
      (T = 1100, K = 4096)                                                           4.3e-3)
    the adapter terms of two columns of one 8-column group      max |dx - ref|       below the bound at 69 %  3e-2
      swapped in one row of dx (the old terms are ~ 0.02)                            of all (row, group)

An ``xd`` element scaled by 1 instead of 2 is seen by the old test's torch.equal on xd (when xd is saved), a slab left
out of a grad_out sum by its rel_err; the new comparison reports both with their place."""
import pytest
import torch

from llm_fine_tune_distributed_amd.ops import reference as ref

import _lora_exact as lx
from _lora_exact import assert_bits_equal, case_id

BF16 = torch.bfloat16
SEED = lx.SEED


def rel_err(a, b):  # the metric of tests/test_kernels_gpu.py
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


# ------------------------------------------------------------------------------------------------ references vs twins
@pytest.mark.parametrize("c", lx.FWD_CASES[::3], ids=case_id)
def test_fwd_want_equals_reference_twin(c):
    x, A = lx.fwd_operands(c, "cpu")
    ldX = lx.fwd_ldX(c)
    X, xd = lx.fwd_want(x, A, c["s"], c["p"], SEED, ldX)
    Xr, xdr = ref.lora_fwd(x, A, c["s"], c["p"], SEED, ldX)
    assert_bits_equal(X, Xr, "X'")
    if c["p"] > 0:
        assert_bits_equal(xd, xdr, "xd")
        kept = lx.keep_mask(c["T"], c["K"], SEED, 0.5).float().mean().item()
        assert c["T"] * c["K"] < 4096 or 0.47 < kept < 0.53, kept
    else:
        assert xdr is None and torch.equal(xd, x)


@pytest.mark.parametrize("c", lx.BWD_CASES[::2], ids=case_id)
def test_bwd_dx_want_equals_reference_twin(c):
    """The twin rounds dxa @ A to bf16 before the add: the same result while the product stays within 256."""
    base, dxa, A = lx.bwd_operands(c, "cpu")
    assert c["R"] * 2 * 2 <= 256
    assert_bits_equal(lx.bwd_dx_want(base, dxa, A, c["p"], SEED), ref.lora_bwd_dx(base, dxa, A, c["p"], SEED))


def test_grad_out_want_by_hand():
    s = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)  # slab sum [r][k] = 12 + 2 (4 r + k)
    old = torch.ones(2, 2, dtype=BF16)
    # rows 1 .., columns 2 .., transposed
    want = torch.tensor([[12 + 2 * 6, 12 + 2 * 10], [12 + 2 * 7, 12 + 2 * 11]], dtype=torch.float32)
    assert torch.equal(lx.grad_out_want(s, old, 1, 2, True, False), want.to(BF16))
    assert torch.equal(lx.grad_out_want(s, old, 1, 2, True, True), (want + 1).to(BF16))
    assert torch.equal(lx.grad_out_want(s[0], old.float(), 1, 2, False, False), s[0, 1:3, 2:4])


# ------------------------------------------------------------------------------------------------ the exact regime
def test_every_gpu_case_is_exact():
    """Worst-case magnitudes (every operand at its largest, every element kept): they bound every partial sum of every
    summation order, whatever values the generator draws on the other device."""
    for c in lx.FWD_CASES + lx.FWD_SW_CASES:
        assert lx.fwd_bound(c) < lx.EXACT_LIMIT and c["K"] % 256 == 0
        assert c["s"] / (1 - c["p"]) in (0.5, 1.0, 2.0, 4.0)
    for c in lx.BWD_CASES:
        assert lx.bwd_bound(c) < lx.EXACT_LIMIT and c["K"] % 8 == 0
    for c in lx.TSUM_CASES:
        assert lx.tsum_bound(c) < lx.EXACT_LIMIT and c["K"] % 8 == 0
    for c in lx.FWD_CASES + lx.FWD_SW_CASES + lx.BWD_CASES + lx.TSUM_CASES:
        assert c["p"] in (0.0, 0.5) and c["R"] in (16, 32, 48, 64)


@pytest.mark.parametrize("c", lx.TSUM_CASES, ids=case_id)
def test_tsum_cases_pass_exact_or_fail(c):
    X, S = lx.tsum_operands(c, "cpu")
    want = lx.tsum_want(X, c["K"], S, c["p"], SEED)  # exact_or_fail inside
    assert want.dtype == torch.float32 and want.shape == (c["R"], c["K"])
    assert want.abs().max().item() <= lx.tsum_bound(c)
    assert torch.equal(want, want.round())


def test_fwd_and_bwd_cases_pass_exact_or_fail():
    for c in lx.FWD_CASES:
        x, A = lx.fwd_operands(c, "cpu")
        X, _ = lx.fwd_want(x, A, c["s"], c["p"], SEED, lx.fwd_ldX(c))
        assert X.float().abs().max().item() <= lx.fwd_bound(c)
    for c in lx.BWD_CASES:
        base, dxa, A = lx.bwd_operands(c, "cpu")
        assert lx.bwd_dx_want(base, dxa, A, c["p"], SEED).float().abs().max().item() <= lx.bwd_bound(c)


def test_exact_or_fail_refuses_and_folds_zero():
    with pytest.raises(AssertionError):
        lx.exact_or_fail(torch.tensor([2.0 ** 24], dtype=torch.float64))
    z = lx.exact_or_fail(torch.tensor([-0.0], dtype=torch.float64))
    assert z.view(torch.int64).item() == 0


# ------------------------------------------------------------------------------------------------ the tables' coverage
def test_case_tables_cover_what_they_promise():
    for R in lx.FWD_R:
        mine = [c for c in lx.FWD_CASES if c["R"] == R]
        assert {c["K"] for c in mine} == set(lx.FWD_K) and {c["T"] for c in mine} == set(lx.FWD_T)
        assert {c["pad"] for c in mine} == set(lx.FWD_PAD) and {c["p"] for c in mine} == {0.0, 0.5}
        assert {c["s"] for c in mine} == {0.5, 2.0}
        assert {(c["save_xd"], c["p"]) for c in mine} >= {(True, 0.5), (False, 0.5), (True, 0.0)}
        mine = [c for c in lx.BWD_CASES if c["R"] == R]
        assert {c["K"] for c in mine} == set(lx.BWD_K) and {c["T"] for c in mine} == set(lx.BWD_T)
        assert {(c["p"], c["sliced"]) for c in mine} == {(p, sl) for p in (0.0, 0.5) for sl in (False, True)}
        for TK in ((1100, 4096), (1000, 8200)):
            assert {c["p"] for c in lx.TSUM_CASES if c["R"] == R and (c["T"], c["K"]) == TK} == {0.0, 0.5}
    assert 20 <= len(lx.FWD_CASES) <= 32
    assert {(c["K"], c["R"]) for c in lx.FWD_SW_CASES} == {(K, R) for K in (256, 768, 2560) for R in (16, 64)}
    shapes = {(c["T"], c["K"]) for c in lx.TSUM_CASES}
    assert shapes >= {(1100, 4096), (1000, 8200), (67, 8200), (203, 520), (2051, 1032), (1, 64)}


# ------------------------------------------------------------------------------------------------ sensitivity
def _caught(bad, good, row=None, group=None):
    """The comparison reports the defect, and names its row and 8-column group."""
    with pytest.raises(AssertionError) as e:
        assert_bits_equal(bad, good)
    msg = str(e.value)
    if row is not None:
        assert f"(row {row}," in msg and f"rows [{row}]" in msg, msg
    if group is not None:
        assert f"8-column groups [{group}]" in msg, msg
    return msg


def _shift_chunk(keep, row, chunk):
    """The mask of one 8-element chunk of one row replaced by that of the chunk after it."""
    bad = keep.clone()
    bad[row, 8 * chunk:8 * chunk + 8] = keep[row, 8 * chunk + 8:8 * chunk + 16]
    return bad


def _old_operands(T, K, R, seed=0):
    """The operands of test_lora_fwd_bwd_kernels (its distributions; drawn on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g).to(BF16)
    A = (torch.randn(R, K, generator=g) * 0.05).to(BF16)
    dxa = (torch.randn(T, R, generator=g) * 0.1).to(BF16)
    base = torch.randn(T, K, generator=g).to(BF16)
    return x, A, dxa, base


def test_shifted_mask_chunk_is_caught_and_passes_the_old_tolerances():
    c = dict(T=203, K=768, R=48, pad=8, p=0.5, s=0.5)
    x, A = lx.fwd_operands(c, "cpu")
    keep = lx.keep_mask(c["T"], c["K"], SEED, 0.5)
    row, chunk = 100, 37
    bad_keep = _shift_chunk(keep, row, chunk)
    assert not torch.equal(bad_keep[row] & (x[row] != 0), keep[row] & (x[row] != 0))  # the defect changes the input
    good = lx.fwd_want(x, A, 0.5, 0.5, SEED, lx.fwd_ldX(c))
    bad = lx.fwd_want(x, A, 0.5, 0.5, SEED, lx.fwd_ldX(c), keep=bad_keep)
    msg = _caught(bad[0], good[0], row=row)
    assert all(g >= c["K"] // 8 for g in (int(v) for v in msg.split("groups [")[1].split("]")[0].split(",")))
    _caught(bad[1], good[1], row=row, group=chunk)
    # lora_tsum's dA under the same defect: the 8 columns of the chunk, every r
    ct = dict(T=203, K=520, R=32, p=0.5)
    X, S = lx.tsum_operands(ct, "cpu")
    keep = lx.keep_mask(203, 520, SEED, 0.5)
    bad_keep = _shift_chunk(keep, row, chunk)
    _caught(lx.tsum_want(X, 520, S, 0.5, SEED, keep=bad_keep), lx.tsum_want(X, 520, S, 0.5, SEED), group=chunk)

    # the old checks on the old operands (T = 200, K = 2048, R = 48, s = 0.5) at the old test's p = 0.05 and 0.3 and
    # at 0.5: dA's rel_err misses the defect at every p; the forward's max norm over the adapter columns misses it at
    # the p = 0.05 this shape is run with (one element of the chunk changes) and sees it from p = 0.3 on
    T, K, R = 200, 2048, 48
    x, A, dxa, _ = _old_operands(T, K, R)
    for p in (0.05, 0.3, 0.5):
        keep = lx.keep_mask(T, K, SEED, p)
        bad_keep = _shift_chunk(keep, row, chunk)
        assert not torch.equal(bad_keep, keep)
        sc = 0.5 / (1 - p)
        z = torch.zeros((), dtype=torch.float64)
        xa = [(sc * (torch.where(k, x.double(), z) @ A.double().t())).float().to(BF16) for k in (keep, bad_keep)]
        err, bound = (xa[1].float() - xa[0].float()).abs().max().item(), 2e-2 * (xa[0].float().abs().max().item() + 1)
        print(f"\n[old] p {p}: adapter columns, max |diff| {err:.3e} bound {bound:.3e}")
        assert err > 0 and (err < bound or p > 0.05)
        dA = [dxa.double().t() @ torch.where(k, x.double(), z) / (1 - p) for k in (keep, bad_keep)]
        print(f"[old] p {p}: dA rel_err {rel_err(dA[1], dA[0]):.3e} bound 1e-2")
        assert 0 < rel_err(dA[1], dA[0]) < 1e-2


def test_dropped_token_of_one_slab_is_caught_and_passes_the_old_tolerance():
    """One workgroup (64 columns, one token chunk) of lora_tsum leaves out the last token of its chunk."""
    c = dict(T=1100, K=4096, R=16, p=0.0)
    X, S = lx.tsum_operands(c, "cpu")
    good = lx.tsum_want(X, c["K"], S, 0.0, SEED)
    t, k0 = 127, 64 * 5  # the last token of a first chunk of 128, the sixth workgroup's columns
    bad = good.clone()
    bad[:, k0:k0 + 64] -= (S[t].double()[:, None] * X[t, k0:k0 + 64].double()[None, :]).float()
    msg = _caught(bad, good)
    assert "8-column groups [40, 41, 42, 43, 44, 45, 46, 47]" in msg, msg
    old = rel_err(bad, good)
    print(f"\n[old] integer operands: dA rel_err {old:.3e} bound 1e-2")
    assert old < 1e-2
    x, A, dxa, _ = _old_operands(1100, 4096, 16)  # the same defect on the old test's distributions, at this T and K
    dA = dxa.double().t() @ x.double()
    badA = dA.clone()
    badA[:, k0:k0 + 64] -= dxa[t].double()[:, None] * x[t, k0:k0 + 64].double()[None, :]
    print(f"[old] old operands: dA rel_err {rel_err(badA, dA):.3e} bound 1e-2")
    assert rel_err(badA, dA) < 1e-2


def test_swapped_columns_of_one_lane_group_are_caught_and_mostly_pass_the_old_tolerance():
    """bwd_dx_kernel's lane holds 8 contiguous output columns, one per MFMA tile: tiles 2 and 3 of one lane swapped."""
    c = dict(T=19, K=136, R=32, p=0.0, sliced=False)
    base, dxa, A = lx.bwd_operands(c, "cpu")
    good = lx.bwd_dx_want(base, dxa, A, 0.0, SEED)
    term = dxa.double() @ A.double()
    row, group = 7, 16  # the 8 columns past the full 128-column wave
    a, b = 8 * group + 2, 8 * group + 3
    assert term[row, a] != term[row, b]  # the defect changes the result
    sw = term.clone()
    sw[row, a], sw[row, b] = term[row, b], term[row, a]
    bad = (base.double() + sw).float().to(BF16)
    _caught(bad, good, row=row, group=group)
    # the old check, |dx - ref| < 3e-2 on operands whose adapter terms are ~ 0.1 * 0.05 * sqrt(R) = 0.02: the same swap
    # at every (row, group) of the old test's R = 16, p = 0 case; two terms differ by N(0, 2 * 0.02^2), within 3e-2
    # with probability 0.7, and more than half a bf16 ulp of base on top cannot be seen at all
    T, K, R = 200, 2048, 16
    _, A, dxa, base = _old_operands(T, K, R)
    term = dxa.double() @ A.double()
    good = (base.double() + term).float().to(BF16)
    sw = term.clone()
    sw[:, 2::8], sw[:, 3::8] = term[:, 3::8], term[:, 2::8]
    bad = (base.double() + sw).float().to(BF16)
    err = (bad.float() - good.float()).abs().view(T, K // 8, 8).amax(-1)  # per (row, group): the old figure of one swap
    missed = (err < 3e-2).float().mean().item()
    differs = (err > 0).float().mean().item()
    print(f"\n[old] swap in one lane group: changes dx at {differs:.1%} of all places, |diff| < 3e-2 at {missed:.1%}")
    assert differs > 0.9 and missed > 0.4


def test_missing_slab_and_unscaled_xd_are_caught():
    g = torch.Generator().manual_seed(3)
    s = torch.randint(-4, 5, (9, 32, 136), generator=g).float()
    for dtype, tr, acc in ((BF16, True, True), (torch.float32, False, False)):
        old = torch.randint(-4, 5, (24, 8) if tr else (8, 24), generator=g).to(dtype)
        good = lx.grad_out_want(s, old, 16, 8, tr, acc)
        bad = lx.grad_out_want(s[:-1], old, 16, 8, tr, acc)  # the tail of slab_sum not run
        assert "elements differ" in _caught(bad, good)
        assert rel_err(bad, good) > 1e-2  # the old tolerance sees this one too
    c = dict(T=17, K=256, R=16, pad=None, p=0.5, s=2.0)
    x, A = lx.fwd_operands(c, "cpu")
    xd = lx.fwd_want(x, A, 2.0, 0.5, SEED, 0)[1]
    keep = lx.keep_mask(17, 256, SEED, 0.5)
    row, col = 16, next(k for k in range(248, 256) if keep[16, k] and x[16, k] != 0)
    bad = xd.clone()
    bad[row, col] = x[row, col]
    _caught(bad, xd, row=row, group=31)


def test_report_names_rows_and_groups():
    want = torch.zeros(40, 64, dtype=BF16)
    got = want.clone()
    got[3, 17] = 1
    got[30, 63] = 1
    with pytest.raises(AssertionError) as e:
        assert_bits_equal(got, want, "dx")
    msg = str(e.value)
    assert msg.startswith("dx: first difference at (row 3, column 17)") and "2 of 2560 elements differ" in msg
    assert "2 rows [3, 30]" in msg and "2 8-column groups [2, 7]" in msg
    assert_bits_equal(got, got.clone())
    with pytest.raises(AssertionError):  # +0 and -0 are different bit patterns
        assert_bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
