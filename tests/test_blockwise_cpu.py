"""tests/_blockwise.py on the CPU, no kernel involved: faults planted in one block, tile or row of a bf16-rounded
4096 x 4096 result pass the whole-matrix Frobenius bounds the GPU tests used alone (5e-3 / 1e-2) and fail the per-block
bound of 2 x rounding_floor.

    planted fault                                 global error   old bound   damaged block
    none                                          1.66e-3        -           1.85e-3 (worst 32 x 32 block)
    one 32 x 32 block loses 1/8 of its reduction  1.91e-3        5e-3        1.22e-1
    one 256 x 256 tile loses 1 of 64 token blocks 1.92e-3        5e-3        1.57e-2
    the last row is halved                        7.98e-3        1e-2        4.99e-1

A lost share s of a reduction is modelled as the block scaled by 1 - s (the mean effect; dropping s of K independent
terms would be sqrt(s), i.e. larger). Margins: the block and the row exceed the 2 x floor bound (3.7e-3) more than 5
times over. The tile that lost 1/64 sits at 1.57e-2 = 4.2 x the bound — (1/64) / (2 x 1.85e-3) whatever the code does —
so that case asserts 4 x: it fails the block check by a wide margin, though not by the 5 x of the other two."""
import math

import pytest
import torch

from _blockwise import assert_blocks_close, block_rel_err, global_rel_err, int_operand, rounding_floor

N = 4096


@pytest.fixture(scope="module")
def clean():
    g = torch.Generator().manual_seed(0)
    want = torch.randn(N, N, generator=g, dtype=torch.float64)
    got = want.float().to(torch.bfloat16)
    return want, got, rounding_floor(want, 32, 32)


def test_clean_matrix_passes(clean):
    want, got, floor = clean
    assert 1.5e-3 < global_rel_err(got, want) < 1.8e-3       # bf16 rounding: 2^-9 / sqrt(3) x the spread of mantissas
    assert 1.7e-3 < floor < 2.1e-3                           # the worst of 16384 blocks sits a little above the mean
    assert assert_blocks_close(got, want, 32, 32, 2 * floor) == pytest.approx(floor)
    assert assert_blocks_close(got, want, 256, 256, 2 * rounding_floor(want, 256, 256)) < floor


def _plant(clean, rows, cols, factor):
    want, got, _ = clean
    bad = got.clone()
    bad[rows, cols] = (want[rows, cols] * factor).float().to(torch.bfloat16)
    return want, bad


@pytest.mark.parametrize("name,rows,cols,factor,old_bound,br,bc,margin", [
    ("block_loses_an_eighth", slice(1024, 1056), slice(2048, 2080), 7 / 8, 5e-3, 32, 32, 5),
    ("tile_loses_a_token_block", slice(512, 768), slice(3072, 3328), 63 / 64, 5e-3, 32, 32, 4),
    ("tile_loses_a_token_block_256", slice(512, 768), slice(3072, 3328), 63 / 64, 5e-3, 256, 256, 4),
    ("last_row_halved", slice(N - 1, N), slice(0, N), 0.5, 1e-2, 32, 32, 5),      # 0.5 / sqrt(32) per 32 x 32 block
    ("last_row_as_row_blocks", slice(N - 1, N), slice(0, N), 0.5, 1e-2, 1, N, 5),  # 4.99e-1 on the row itself
])
def test_planted_fault_passes_the_global_metric_and_fails_the_block_metric(clean, name, rows, cols, factor, old_bound,
                                                                           br, bc, margin):
    want, bad = _plant(clean, rows, cols, factor)
    floor = clean[2] if (br, bc) == (32, 32) else rounding_floor(want, br, bc)
    g = global_rel_err(bad, want)
    e = block_rel_err(bad, want, br, bc)
    i, j = (rows.start or 0) // br, (cols.start or 0) // bc
    print(f"{name}: global {g:.3e} (old bound {old_bound:g}), damaged block {e[i, j].item():.3e}, "
          f"bound {2 * floor:.3e}")
    assert g < old_bound                                     # the old metric lets it through
    wi, wj = divmod(int(e.argmax()), e.shape[1])             # the worst block lies in the damaged region
    assert i <= wi < -(-rows.stop // br) and j <= wj < -(-cols.stop // bc)
    i, j = wi, wj
    assert e.max().item() >= margin * 2 * floor              # and is far over the block bound
    with pytest.raises(AssertionError) as info:
        assert_blocks_close(bad, want, br, bc, 2 * floor, name)
    msg = str(info.value)
    assert f"block ({i}, {j})" in msg and "global error" in msg and "blocks over the bound" in msg
    nbad = int((e > 2 * floor).sum())
    assert f"{nbad} of {e.numel()} blocks" in msg
    if name == "last_row_halved":
        assert nbad == N // bc                               # every block of the last block row, no other
    elif br == 32 and name.startswith("tile"):
        assert nbad == 64
    else:
        assert nbad == 1


def test_zero_and_tiny_reference_blocks():
    """A block whose reference is all zero (dq / dk of a length-1 sequence) is judged against the typical magnitude of
    the whole reference: exact zeros pass, noise far below the rms passes, an rms-sized value fails; nothing divides
    by zero, and an all-zero reference accepts only an all-zero output."""
    g = torch.Generator().manual_seed(1)
    want = torch.randn(96, 160, generator=g, dtype=torch.float64)
    want[32:64, 32:64] = 0
    got = want.float().to(torch.bfloat16).float()
    floor = rounding_floor(want, 32, 32)
    e = block_rel_err(got, want, 32, 32)
    assert e.shape == (3, 5) and torch.isfinite(e).all() and e[1, 1] == 0
    assert_blocks_close(got, want, 32, 32, 2 * floor)
    noisy = got.clone()
    noisy[32:64, 32:64] = 1e-5
    assert_blocks_close(noisy, want, 32, 32, 2 * floor)
    assert block_rel_err(noisy, want, 32, 32)[1, 1].item() == pytest.approx(1e-5 / want.pow(2).mean().sqrt().item(), rel=1e-6)
    wrong = got.clone()
    wrong[40, 40] = 1.0
    with pytest.raises(AssertionError, match=r"block \(1, 1\)"):
        assert_blocks_close(wrong, want, 32, 32, 2 * floor)
    zero = torch.zeros(64, 64, dtype=torch.float64)
    assert block_rel_err(zero.float(), zero, 32, 32).max().item() == 0
    off = zero.float().clone()
    off[3, 3] = 1e-20
    assert math.isinf(block_rel_err(off, zero, 32, 32)[0, 0].item())
    nan = got.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_blocks_close(nan, want, 32, 32, 2 * floor)


def test_ragged_blocks_cover_every_element():
    """Shapes that are no multiple of the block: the last partial blocks are judged too (no element is left out)."""
    g = torch.Generator().manual_seed(2)
    want = torch.randn(70, 45, generator=g, dtype=torch.float64)
    got = want.clone()
    assert block_rel_err(got, want, 32, 32).shape == (3, 2)
    got[69, 44] += 1.0
    e = block_rel_err(got, want, 32, 32)
    assert e[2, 1] > 0 and e.sum() == e[2, 1]


def test_int_operand():
    a = int_operand((512, 384), -2, 2, 7, "cpu")
    assert a.dtype == torch.bfloat16 and torch.equal(a, int_operand((512, 384), -2, 2, 7, "cpu"))
    assert not torch.equal(a, int_operand((512, 384), -2, 2, 8, "cpu"))
    assert set(a.float().unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    # not periodic: no row or column shift maps the operand onto itself
    for s in (1, 2, 5, 7, 64, 128, 256):
        assert not torch.equal(a, a.roll(s, 0)) and not torch.equal(a, a.roll(s, 1))
    # nnz_per_col: at most that many non-zeros in every column, at rows that differ from column to column
    w = int_operand((2048, 256), -1, 1, 3, "cpu", nnz_per_col=200)
    nz = w != 0
    assert int(nz.sum(0).max()) <= 200 and int(nz.sum(0).min()) > 100
    assert not torch.equal(nz[:, 0], nz[:, 1])
    dy = int_operand((64, 2048), -1, 1, 4, "cpu").double()
    assert (dy @ w.double()).abs().max() <= 200              # bounded by the non-zeros: exact in bf16
    # small integers: fp32 sums equal fp64 sums whatever the order
    x = int_operand((8192, 64), -3, 3, 5, "cpu")
    y = int_operand((8192, 64), -2, 2, 6, "cpu")
    p64 = y.double().t() @ x.double()
    assert torch.equal((y.float().t() @ x.float()).double(), p64) and p64.abs().max() < 2 ** 24
