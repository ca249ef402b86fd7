"""ce_fwd (csrc/cross_entropy.hip) at its edges, every row judged on its own against fp64 on the same bf16 logits.

The row loop consumes 1024 16-byte vectors per unrolled pass (4 loads in flight per thread x 256 threads), then 256 per
pass: the vocabularies straddle both steps. The rows of each case carry labels at 0, at V - 1, inside the last vector,
inside the remainder loop and -100, a row of all-equal logits, a row with one logit at +80 over -80, and argmax ties
between two threads of a wave and between two waves. With the gradient written the launch reserves dynamic LDS to cap
the rows in flight: 51 KB at V = 128,256, 79 KB at 151,936, 159 KB at 262,144 — above 64 KB only with the limit raised
(ce_fwd does that once)."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE = 1.0 / 7.0


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()


def _first_max(x):
    """The first index where x == x.max(), per row (not argmax: which of several equal maxima argmax returns is not
    specified)."""
    V = x.shape[-1]
    idx = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values


def _check(logits, labels, write_grad):
    """One ce_fwd call on a copy of ``logits``; every row of loss, lse, entropy, correct and the gradient against
    fp64. Returns the measured maxima (loss / lse absolute error, gradient error in units of its bound)."""
    inv = torch.tensor([SCALE], device=DEV)
    lg = logits.clone()
    stats = _ext.ops().ce_fwd(lg, labels, inv, write_grad)
    torch.cuda.synchronize()
    return compare_rows(logits, labels, stats, lg, write_grad)


def compare_rows(logits, labels, stats, lg, write_grad):
    """Rows of one ce_fwd call against fp64: ``logits`` [M, V] as they went in, ``stats`` [4, M] and ``lg`` [M, V] (the
    same memory after the call) as they came out: all of a call, or the same rows taken from a larger one. Returns
    the measured maxima (loss and lse absolute error; with the gradient, its worst error in units of its bound)."""
    M, V = logits.shape
    assert stats.shape == (4, M) and stats.dtype == torch.float32
    x = logits.double()
    valid = labels != -100
    lse = torch.logsumexp(x, -1)
    tgt = x.gather(-1, labels.clamp(min=0)[:, None]).squeeze(-1)
    loss = torch.where(valid, lse - tgt, torch.zeros_like(lse))
    p = torch.softmax(x, -1)
    ent = lse - (p * x).sum(-1)
    correct = (_first_max(x) == labels) & valid
    got = stats.double()
    assert torch.isfinite(stats).all(), stats
    figs = {}
    for name, g, w in (("loss", got[0], loss), ("lse", got[1], lse)):
        err = (g - w).abs()
        figs[name] = err.max().item()
        print(f"ce V={V} M={M} grad={write_grad}: max {name} error {err.max().item():.3e}")
        bad = err > 1e-4 + 1e-5 * w.abs()
        assert not bool(bad.any()), (name, bad.nonzero().flatten().tolist(), g[bad].tolist(), w[bad].tolist())
    e_ent = (got[2] - ent).abs()
    assert bool((e_ent <= 2e-2 + 1e-2 * ent.abs()).all()), ("entropy", got[2].tolist(), ent.tolist())
    assert torch.equal(stats[3].bool(), correct), (stats[3].tolist(), correct.tolist(), labels.tolist())
    if not write_grad:
        assert torch.equal(lg.view(torch.int16), logits.view(torch.int16))  # untouched, bit for bit
        return figs
    assert not bool(torch.isnan(lg).any())
    onehot = torch.zeros_like(p)
    onehot[valid, labels[valid]] = 1.0
    want = (p - onehot) * SCALE * valid[:, None]
    # one bf16 half-ulp (2^-8) for the store plus one of margin for the fp32 exp / lse
    over = (lg.double() - want).abs() / (2.0 ** -7 * want.abs() + 1e-30)
    print(f"ce V={V} M={M}: max gradient error {over.max().item():.3f} of its bound")
    assert bool((over <= 1).all()), ((over > 1).nonzero()[:4].tolist(), over.max().item())
    assert bool((lg[~valid] == 0).all())  # ignored rows: exactly zero
    figs["grad"] = over.max().item()
    return figs


def _edge_rows(V, seed):
    """M = 9 rows of bf16 logits and their labels (see the module docstring); returns (logits, labels)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (3 * torch.randn(9, V, device=DEV, generator=g)).to(torch.bfloat16)
    nvec = V // 8
    in_rem = 8 * max(0, nvec - 300) + 2   # past the last whole 1024-vector pass whenever nvec % 1024 >= 300
    labels = [0, V - 1, V - 3, in_rem, -100]
    x[5] = 1.5                            # all equal: lse = x + ln V, entropy = ln V, argmax index 0
    labels.append(0)
    hot = V // 2
    x[6] = -80.0
    x[6, hot] = 80.0                      # p = 1 at the label: loss ~ 0 and finite, gradient 0 there
    labels.append(hot)
    # ties: the maximum at two indices, owned by neighbouring threads (vectors v0, v0 + 1: lanes of one wave) and by
    # threads 64 apart (two waves); where the row has too few vectors, two elements as far apart as it allows
    v0 = min(3, max(0, nvec - 2))
    a, b = 8 * v0 + 5, 8 * min(v0 + 1, nvec - 1) + 2
    a, b = (a, b) if a != b and a < b else (8 * v0 + 2, 8 * v0 + 5)
    x[7, a] = x[7, b] = 24.0
    labels.append(a)                      # the lower index: counted correct
    c, d = 8 * v0 + 6, 8 * min(v0 + 64, nvec - 1) + 1
    c, d = (c, d) if c < d else (8 * v0 + 1, 8 * v0 + 6)
    x[8, c] = x[8, d] = 24.0
    labels.append(d)                      # the higher index: must NOT be counted correct
    return x.contiguous(), torch.tensor(labels, device=DEV, dtype=torch.int64)


@pytest.mark.parametrize("write_grad", [True, False])
@pytest.mark.parametrize("V", [8 * n for n in (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2049)]
                         + [128256, 151936, 262144])
def test_ce_edges(V, write_grad):
    logits, labels = _edge_rows(V, V)
    _check(logits, labels, write_grad)
    # the analytic rows, from the kernel's own numbers
    stats = _ext.ops().ce_fwd(logits.clone(), labels, torch.tensor([SCALE], device=DEV), False)
    assert abs(stats[1, 5].item() - (1.5 + math.log(V))) <= 1e-4 + 1e-5 * (1.5 + math.log(V))
    assert abs(stats[2, 5].item() - math.log(V)) <= 2e-2 + 1e-2 * math.log(V)
    assert stats[3, 5].item() == 1.0      # all equal: the argmax is index 0, the label
    assert abs(stats[0, 6].item()) <= 1e-4 and stats[3, 6].item() == 1.0
    assert stats[3, 7].item() == 1.0 and stats[3, 8].item() == 0.0


@pytest.mark.parametrize("V", [8, 2056, 128256])
def test_ce_single_row(V):
    g = torch.Generator(device=DEV).manual_seed(5)
    logits = (3 * torch.randn(1, V, device=DEV, generator=g)).to(torch.bfloat16)
    for label in (V - 1, -100):
        _check(logits, torch.tensor([label], device=DEV), True)


def test_ce_hot_row_gradient():
    """One logit at +80 over -80 everywhere else, labelled elsewhere too: no NaN, the loss is 160, the gradient is
    +scale at the hot index, -scale at the label and zero (p = e^-160) everywhere else."""
    V = 8 * 1025
    x = torch.full((2, V), -80.0, device=DEV, dtype=torch.bfloat16)
    x[:, 4097] = 80.0
    labels = torch.tensor([4097, 11], device=DEV)
    _check(x, labels, True)
    lg = x.clone()
    stats = _ext.ops().ce_fwd(lg, labels, torch.tensor([SCALE], device=DEV), True)
    assert abs(stats[0, 1].item() - 160.0) <= 1e-4 + 1e-5 * 160
    assert lg[0, 4097].item() == 0.0 and bool((lg[0] == 0).all())
    s = torch.tensor(SCALE).to(torch.bfloat16).item()
    assert lg[1, 4097].item() == s and lg[1, 11].item() == -s and int((lg[1] != 0).sum()) == 2
