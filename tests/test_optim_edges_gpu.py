"""csrc/optim.hip at its edges: all six built AdamW variants (master / no master with round-to-nearest / no master with
stochastic rounding, each with fp32 and bf16 moments) element by element against ops/reference.py adamw_, at sizes that
run only the scalar tail (1, 7), only whole vectors (8), both (2051) and the grid-stride loop with the tail after it
(16,777,216 + 8,003), with stochastic-rounding offsets on both sides of 2^32; sumsq / sumsq_chunks against fp64.

Tolerances. fp32 state: |x - ref| <= rel |ref| + abs with (rel, abs) from _rowwise.fp32_tolerance, i.e. from an fp32
torch evaluation of the step in the kernel's association order against ref.adamw_ (the two differ in how they
associate the bias corrections and the g^2 term), never from the kernel's output. bf16 state: at most one decision
flipped by fp32 ordering per 1000 elements, and then by one ulp (two when it crosses a binade): the rule of
test_kernels_gpu.py::test_adamw_sr_matches_reference_twin. Measured figures: profiles/rowwise_kernel_errors.md."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

import _rowwise as rw

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
N_BIG = 2048 * 256 * 4 * 8 + 8 * 1000 + 3  # one full grid-stride pass, 1000 vectors of a second one, 3 tail elements
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)
STEP, COEF = 5, 0.7


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def _state(n, moments, master, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, generator=g, device=DEV).to(BF16)
    grad = torch.randn(n, generator=g, device=DEV).to(BF16)
    m = (torch.randn(n, generator=g, device=DEV) * 0.01).to(moments)
    v = (torch.randn(n, generator=g, device=DEV).abs() * 0.001).to(moments)
    ms = (p.float() + 1e-3 * torch.randn(n, generator=g, device=DEV)) if master else None
    return p, grad, ms, m, v


def _kernel_step(p, grad, ms, m, v, sr_seed, sr_offset):
    h = HYPER
    coef = torch.tensor([COEF], device=DEV)
    _ext.ops().adamw_flat(p, grad, ms, m, v, coef, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                          1 - h["b1"] ** STEP, 1 - h["b2"] ** STEP, sr_seed, sr_offset)


def _check_bf16(a, b, what):
    diff = (a.float() - b.float()).abs()
    tol = b.float().abs() * 2 ** -6 + 1e-6 * b.float().abs().max()
    assert not (diff > tol).any(), (what, int((diff > tol).sum()))
    ndiff = int((diff > 0).sum())
    assert ndiff <= math.ceil(1e-3 * a.numel()), (what, ndiff, a.numel())
    return ndiff


def _check_fp32(a, b, alt, what):
    rel, ab = rw.fp32_tolerance(alt, b)
    diff = (a.double() - b.double()).abs()
    over = diff > rel * b.double().abs() + ab
    need = ((diff - ab).clamp_min(0) / b.double().abs().clamp_min(1e-300)).max().item()
    assert not over.any(), (what, int(over.sum()), need, rel)
    return f"{(diff.max() / b.double().abs().max()).item():.2e} of max", need, rel


OFFSETS = [0, 1, 2 ** 32 - 3, 2 ** 33 + 1]
# the offset only enters the stochastic-rounding streams: the other variants take two of the values (it is ignored)
ADAMW_CASES = [(variant, seed, moments, n, off)
               for variant, seed, offs in (("master", 0, OFFSETS[::2]), ("rne", 0, OFFSETS[::2]), ("sr", 777, OFFSETS))
               for moments in (torch.float32, BF16) for n in (1, 7, 8, 2051, N_BIG) for off in offs]


@pytest.mark.parametrize("variant,sr_seed,moments,n,sr_offset", ADAMW_CASES)
def test_adamw_variants_match_reference(variant, sr_seed, moments, n, sr_offset):
    before = _state(n, moments, variant == "master", 11 + n % 1000)
    after = [None if t is None else t.clone() for t in before]
    _kernel_step(*after, sr_seed, sr_offset)
    figs = check_against_reference(before, after, moments, sr_seed, sr_offset)
    print(f"\n[optim] adamw {variant} moments={moments} n={n} off={sr_offset}: {figs}")


def check_against_reference(before, after, moments, sr_seed, sr_offset):
    """``before`` = (p, grad, master or None, m, v) as they went into one kernel step (left unchanged), ``after`` the
    same tensors as the kernel left them (all of a call, or a range of a larger one with ``sr_offset`` advanced by its
    start): against ops/reference.py adamw_ under the tolerances of the module docstring. Returns the figures."""
    h = HYPER
    p2, grad, ms2, m2, v2 = [None if t is None else t.clone() for t in before]
    p, _, ms, m, v = after
    w0 = ms2.clone() if ms2 is not None else p2.float()
    alt_w, alt_m, alt_v = rw.adamw_kernel_order(w0, grad.float() * COEF, m2.float(), v2.float(), h["lr"], h["b1"],
                                                h["b2"], h["eps"], h["wd"], 1 - h["b1"] ** STEP, 1 - h["b2"] ** STEP)
    ref.adamw_(p2, grad.float() * COEF, m2, v2, ms2, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], STEP,
               sr_seed=sr_seed, sr_offset=sr_offset)
    assert torch.equal(after[1], grad)  # the gradient is only read
    figs = []
    for name, a, b, alt in (("m", m, m2, alt_m), ("v", v, v2, alt_v)):
        assert a.dtype == b.dtype == moments
        if moments == BF16:
            figs.append((name, _check_bf16(a, b, name)))
        else:
            figs.append((name,) + _check_fp32(a, b, alt, name))
    if ms is not None:
        figs.append(("master",) + _check_fp32(ms, ms2, alt_w, "master"))
        assert torch.equal(p, ms.to(BF16))  # the working copy is the master rounded once
    else:
        figs.append(("p", _check_bf16(p, p2, "p")))
    return figs


@pytest.mark.parametrize("moments", [torch.float32, BF16])
@pytest.mark.parametrize("n", [7, 2051])
def test_adamw_master_ignores_the_sr_seed(moments, n):
    a = _state(n, moments, True, 5)
    b = tuple(t.clone() for t in a)
    _kernel_step(*a, 0, 0)
    _kernel_step(*b, 12345, 2 ** 32 - 3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ sumsq
SUMSQ_N = [0, 1, 7, 8, 9, 2 ** 21 + 5]
CHUNK_BUF = 300_000
SMALL = 4096  # up to here one lost or doubled element moves the sum by >= 2e-4 of itself: far above the bound
# (start, length): whole vectors and a tail; misaligned; empty; shorter than a vector (aligned and not); ending at the
# buffer's last element (aligned start and not); a single element; one vector; long ones, aligned and not
CHUNKS = [(0, 1024 + 5), (3, 1000), (17, 0), (64, 5), (70, 7), (CHUNK_BUF - 4096, 4096), (CHUNK_BUF - 1001, 1001),
          (0, 0), (CHUNK_BUF - 1, 1), (8, 8), (16, 2048 + 256 * 8 - 1), (0, 262_144 + 5), (262_151, 30_011)]


def _x(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, generator=g, device=DEV).to(BF16)


@pytest.fixture(scope="module")
def sumsq_bound():
    """n -> 2 x the worst relative error of the fp32 256-way strided sum against fp64, over every tested buffer and
    chunk of n's size class (up to 4096 elements, or more). Pooled: a sum of one or seven exact squares has no rounding
    error of its own to measure, and one sum's error is one draw of a random walk. Never below 2^-21: eight additions
    of half an ulp each, the depth of the shortest sums."""
    worst = {True: 0.0, False: 0.0}
    x = _x(CHUNK_BUF, 99)
    for c in [_x(n, 40 + i) for i, n in enumerate(SUMSQ_N)] + [x[s:s + n] for s, n in CHUNKS]:
        if c.numel():
            want = c.double().pow(2).sum().item()
            err = abs(rw.strided_sum_emul(c.float().pow(2)).double().item() - want) / want
            worst[c.numel() <= SMALL] = max(worst[c.numel() <= SMALL], err)
    return lambda n: max(2 * worst[n <= SMALL], 2.0 ** -21)


@pytest.mark.parametrize("i,n", list(enumerate(SUMSQ_N)))
def test_sumsq_sizes(i, n, sumsq_bound):
    x = _x(n, 40 + i)
    part = _ext.ops().sumsq(x)
    got, want = part.double().sum().item(), x.double().pow(2).sum().item()
    err = abs(got - want) / want if want else abs(got)
    print(f"\n[optim] sumsq n={n}: error {err:.3e} bound {sumsq_bound(n):.3e}")
    assert err <= sumsq_bound(n)


def test_sumsq_chunks_edges(sumsq_bound):
    x = _x(CHUNK_BUF, 99)
    assert any(s % 8 for s, _ in CHUNKS) and any(s + n == CHUNK_BUF for s, n in CHUNKS)
    part = _ext.ops().sumsq_chunks(x, torch.tensor(CHUNKS, dtype=torch.int64, device=DEV))
    assert part.shape == (len(CHUNKS),)
    figs = []
    for i, (s, n) in enumerate(CHUNKS):
        got, want = part[i].double().item(), x[s:s + n].double().pow(2).sum().item()
        err = abs(got - want) / want if want else abs(got)
        figs.append((s, n, f"{err:.2e}", f"{sumsq_bound(n):.2e}"))
        assert err <= sumsq_bound(n), (i, s, n, err, sumsq_bound(n))
    print(f"\n[optim] sumsq_chunks (start, length, error, bound): {figs}")
