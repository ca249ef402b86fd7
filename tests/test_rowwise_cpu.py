"""The per-row checks of tests/test_rowwise_gpu.py and tests/test_decode_edges_gpu.py on the CPU, no kernel involved:
faults planted in one row of the torch emulation's output pass the whole-output Frobenius bound of 1e-2 that
tests/test_kernels_gpu.py applies and fail the per-row bound (2 x the emulation's own worst row) at least 4 times over;
and the sampler twin of tests/_rowwise.py against the rule of inference/generation.py sample_next.

    planted fault (RMSNorm dx 1000 x 2048, embedding gradient 1000 x 2048,     global    old bound   damaged row
    decode output of one 600-key sequence, 16 heads x 128)
    one row scaled by 1 - 1/64                                                 < 1e-2    1e-2        1.57e-2 = 4.3 x bound
    one row's last 8 columns zeroed (dx, embedding)                            < 1e-2    1e-2        6.2e-2
    one head's last 8 of 128 dims zeroed (decode)                              5.7e-2    1e-2        2.1e-1
    one head of one sequence swapped with its neighbour (decode)               3.8e-1    1e-2        1.05

The decode test's old bound is already taken per sequence (16 heads), so it sees the last two faults as well; the
per-head check sees them 3 to 4 x larger, and the first only there. The row scaled by 1 - 1/64 sits at
(1/64) / (2 x 1.8e-3) = 4.3 x the bound whatever the code does, so every case asserts 4 x."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import sample_next

import _rowwise as rw
from _blockwise import assert_blocks_close, block_rel_err, global_rel_err

BF16 = torch.bfloat16
OLD_BOUND = 1e-2
MARGIN = 4


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(BF16)


def _scale_row(got, want, row):
    bad = got.clone()
    bad[row] = (want[row] * (1 - 1 / 64)).float().to(BF16)
    return bad


def _zero_tail(got, want, row):
    bad = got.clone()
    bad[row, -8:] = 0
    return bad


def _swap_rows(got, want, row):
    bad = got.clone()
    bad[row], bad[row + 1] = got[row + 1], got[row]
    return bad


def _judge(got, want, bad, row, bound, rms=None):
    """(global error of the faulty output, damaged row's error / bound); the clean output passes the row check."""
    C = want.shape[1]
    assert block_rel_err(got, want, 1, C, rms).max().item() <= bound
    e = block_rel_err(bad, want, 1, C, rms)
    assert int(e.argmax()) in (row, row + 1)
    return global_rel_err(bad, want), e.max().item() / bound


@pytest.fixture(scope="module")
def dx_case():
    M, H = 1000, 2048
    h, dy, dres = _randn(M, H, seed=1), _randn(M, H, seed=2), _randn(M, H, seed=3)
    w = (1 + 0.1 * torch.randn(H, generator=torch.Generator().manual_seed(4))).to(BF16)
    rstd = torch.rsqrt(h.float().pow(2).mean(-1) + 1e-6)
    dx64, _, dx_em, _ = rw.rmsnorm_bwd_refs(dy, h, w, rstd, dres)
    return dx_em, dx64, rw.row_bound(dx_em, dx64)


@pytest.fixture(scope="module")
def emb_case():
    V, H = 1000, 2048
    ids = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in zip([0, 5, 6, 11, 20, 21, V - 1],
                                                                           [1, 7, 8, 9, 16, 17, 3])])
    ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(5))]
    want, em = rw.embedding_bwd_refs(_randn(V, H, seed=6), ids, _randn(ids.numel(), H, seed=7))
    return em, want, rw.row_bound(em, want)


@pytest.mark.parametrize("fault", [_scale_row, _zero_tail])
@pytest.mark.parametrize("case,row", [("dx_case", 777), ("emb_case", 20)])
def test_row_fault_passes_the_global_bound_and_fails_the_row_bound(case, row, fault, request):
    got, want, bound = request.getfixturevalue(case)
    assert 3e-3 < bound < 4.2e-3  # 2 x the bf16 rounding of a row (2^-9 / sqrt 3 x the spread of the mantissas)
    g, over = _judge(got, want, fault(got, want, row), row, bound)
    assert g < OLD_BOUND and over >= MARGIN, (g, over)
    with pytest.raises(AssertionError, match=rf"rows {row}\.\."):
        assert_blocks_close(fault(got, want, row), want, 1, want.shape[1], bound)


@pytest.fixture(scope="module")
def decode_case():
    """One 600-key sequence of 16 query heads over 2 kv heads: [16, 128] emulation, fp64 reference, per-head bound."""
    nq, nkv, D, L = 16, 2, 128, 600
    q, K, V = _randn(nq, D, seed=8), _randn(L, nkv, D, seed=9), _randn(L, nkv, D, seed=10)
    want, em = rw.decode_refs(q, K, V, 1 / math.sqrt(D))
    return em, want, rw.row_bound(em, want)


def test_decode_head_faults(decode_case):
    got, want, bound = decode_case
    # one head scaled by 1 - 1/64: the per-sequence norm the old test takes does not see it, the per-head check does
    g, over = _judge(got, want, _scale_row(got, want, 5), 5, bound)
    assert g < OLD_BOUND and over >= MARGIN, (g, over)
    # the last 8 dims of one head zeroed, one head swapped with its neighbour (same kv head: only q differs): the
    # per-sequence norm sees these too (it is taken over 16 heads only), the per-head check 3 to 4 x larger
    for fault in (_zero_tail, _swap_rows):
        g, over = _judge(got, want, fault(got, want, 4), 4, bound)
        assert g >= OLD_BOUND and over >= MARGIN and over * bound >= 2 * g, (fault.__name__, g, over)


# ------------------------------------------------------------------------------------------------ sampler twin
V, K, T, RP, SEED = 5000, 12, 0.7, 1.2, 1234
HIST = [3, 17, 400]


@pytest.mark.parametrize("P", [0.9, 1.0])
def test_twin_support_and_argmax_follow_sample_next(P):
    """The twin's kept set is the support of sample_next's distribution (penalty, temperature, top-k, top-p with the
    same 'mass ranked above' rule), and its first rank is sample_next's greedy token."""
    logits = rw.sampler_logits(40, V, HIST, SEED)
    present = rw.history_mask(V, HIST)
    hist = torch.tensor(HIST)
    for t in range(logits.shape[0]):
        tok, amb, support = rw.sampler_twin(logits[t], present, t, SEED, T, K, P, RP)
        assert tok in support and len(set(support)) == len(support) <= K
        assert support[0] == sample_next(logits[t], hist, T, K, P, RP, do_sample=False)
        if amb:
            continue
        # the support of sample_next's distribution: every draw lies in it, and its size is the twin's
        lg = logits[t].clone()
        sc = lg[hist]
        lg[hist] = torch.where(sc < 0, sc * RP, sc / RP)
        lg = lg / T
        kth = torch.topk(lg, K).values[-1]
        lg[lg < kth] = -float("inf")
        sl, si = torch.sort(lg, descending=True)
        cp = sl.softmax(-1).cumsum(-1)
        remove = cp > P
        remove[1:] = remove[:-1].clone()
        remove[0] = False
        want = set(si[~remove & torch.isfinite(sl)].tolist()) if P < 1.0 else set(si[torch.isfinite(sl)].tolist())
        assert set(support) == want, (t, support, sorted(want))
        g = torch.Generator().manual_seed(t)
        assert sample_next(logits[t], hist, T, K, P, RP, True, g) in want


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("P", [0.9, 1.0])
@pytest.mark.parametrize("Vv", [5000, 2048, 2049])
def test_share_of_steps_too_close_to_call(Vv, P, dtype):
    """At most 3 % of 400 steps fall within the skip margins, computed from the twin alone (4 of 400 for V = 5000,
    P = 0.9, fp32): the exact GPU test keeps at least 97 % of its steps."""
    logits = rw.sampler_logits(400, Vv, HIST, SEED).to(dtype)
    toks, amb = rw.twin_run(logits, HIST, SEED, T, K, P, RP)
    print(f"\n[twin] V={Vv} P={P} {dtype}: {sum(amb)} of {len(amb)} steps too close to call")
    assert sum(amb) <= 0.03 * len(amb)
    assert len(set(toks)) > 100  # a draw, not a constant
