"""Offline distillation on the GPU: teacher_topk and kd_topk_fwd (csrc/distill_topk.hip) per row against fp64, the
LM-head op built on them (ops.lm_head_distill_topk_loss), CausalLM.distill_topk_loss on the HIP path against the
PyTorch reference path, and GKDTrainer steps from the teacher's cached top-k with the dispatch trace.

Bounds follow tests/test_distill_gpu.py: each is 2 x the worst error of an fp32 torch emulation with the kernel's
rounding points against the fp64 reference, computed here from the references alone and pooled over the grid per
kernel; errors are in fp32 ulps (_ulps) for loss, lse, mass and log-probabilities and per row (block_rel_err) for
gradients; every test prints its worst measured error next to the bound (pytest -s); profiles/distill_topk.md records
one run. The model tests use the project's bounds of tests/test_distill_gpu.py::test_distill_loss_hip_vs_reference."""
import dataclasses
import math
import os
import shutil

import pytest
import torch

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.models import CausalLM, build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close, block_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SCALE = 1.0 / 7.0
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

SMALL_V = [8 * n for n in (32, 255, 257, 1025, 2049)]
BIG_V = [128256, 151936]
KS = [1, 7, 64, 256]
TOPK_GRID = [(V, k, tau) for V in SMALL_V + BIG_V for k in KS for tau in (0.9, 2.0) if k <= V]
KD_GRID = [(V, k, tau) for V in SMALL_V + BIG_V for k in KS for tau in (1.0, 0.9, 2.0) if k <= V]


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def report(what, worst, bound):
    print(f"\n[distill_topk] {what}: worst {worst:.3e} bound {bound:.3e}")


def first_argmax(x):
    """argmax over the last dimension, ties resolved to the first index."""
    V = x.shape[-1]
    cols = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, cols, torch.full_like(cols, V)).min(-1).values


def _ulps(err, *mags):
    """An absolute error in fp32 ulps of the largest of ``mags`` (at least 1), as in tests/test_distill_gpu.py: every
    quantity here is a sum of an lse and of logit differences, so one ulp of the largest of them is the unit a rounding
    of any term moves it by."""
    top = torch.stack([m.abs() for m in mags]).max(0).values.clamp(min=1.0)
    return err / torch.exp2(torch.floor(torch.log2(top)) - 23)


def f32(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def exp32(x):
    """__expf: the hardware exp2 of fp32(x log2 e)."""
    return torch.exp2(x * f32(LOG2E))


def log32(x):
    """__logf: fp32(log2(x) ln 2)."""
    return torch.log2(x) * f32(LN2)


def lse32(a):
    """(lse, max) of fp32 rows as the kernels build it: m + log(sum e^(a - m))."""
    m = a.max(-1, keepdim=True).values
    return m[:, 0] + log32(exp32(a - m).sum(-1))


# ------------------------------------------------------------------------------------------------ teacher_topk
TOPK_KINDS = ["3 * randn", "all equal: ids 0 .. k - 1", "the maximum at column V - 1, the runner-up at column 5",
              "ties planted across two threads, inside one 16-byte vector and (V = 8 x 1025) across the unrolled part "
              "and the tail vector", "gaps of 150"]
TOPK_BIG_KINDS = [0, 1, 3]  # the three rows of the training vocabularies


def _topk_rows(V):
    """bf16 logits [5, V], one row per kind of TOPK_KINDS (TOPK_BIG_KINDS for the two training vocabularies)."""
    g = torch.Generator(device=DEV).manual_seed(1000 + V)
    x = (3 * torch.randn(5, V, device=DEV, generator=g)).to(BF16)
    x[1] = 1.25
    x[2, V - 1] = x[2].float().max() + 2.0
    x[2, 5] = x[2, V - 1].float() - 1.0
    hi = x[3].float().max() + 4.0
    x[3, 8 * 3 + 1], x[3, 8 * 20 + 1] = hi, hi                           # vectors 3 and 20: two threads
    x[3, 16], x[3, 19], x[3, 21] = hi - 1.0, hi - 1.0, hi - 1.0           # vector 2: one 16-byte load
    if V == 8 * 1025:
        x[3, 8 * 1024 + 3], x[3, 17] = hi - 2.0, hi - 2.0                 # the tail vector and the unrolled part
    n = max(1, V // 16)
    x[4, :n] += 150.0
    x[4, V - n:] -= 150.0
    if V > 100000:
        x = x[torch.tensor(TOPK_BIG_KINDS, device=DEV)]
    return x.contiguous()


def _topk_refs(x, k, tau):
    """(ids of the stable descending sort, fp64 log-probabilities, fp64 lse) and the fp32 emulation of the
    log-probabilities: logits times fp32(1 / tau), lse = m + log(sum e^(a - m)), the entry minus the lse."""
    ids, lps = ref.teacher_topk(x.double(), k, tau)
    lse = torch.logsumexp(x.double() / tau, -1)
    a = x.float() * f32(1.0 / tau)
    emul = a.gather(1, ids.long()) - lse32(a)[:, None]
    return ids, lps, lse, emul


@pytest.fixture(scope="module")
def topk_cases():
    rows = {V: _topk_rows(V) for V in SMALL_V + BIG_V}
    cases, bound = {}, 0.0
    for V, k, tau in TOPK_GRID:
        x = rows[V]
        ids, lps, lse, emul = _topk_refs(x, k, tau)
        cases[V, k, tau] = (x, ids, lps, lse)
        bound = max(bound, _ulps((emul.double() - lps).abs(), lse[:, None].expand_as(lps), lps).max().item())
    return cases, 2 * bound


@pytest.mark.parametrize("V,k,tau", TOPK_GRID)
def test_teacher_topk_rows(V, k, tau, topk_cases):
    cases, bound = topk_cases
    x, want_ids, want_lps, lse = cases[V, k, tau]
    x0 = x.clone()
    ids, lps = ops.teacher_topk(x, k, tau)
    torch.cuda.synchronize()
    M = x.shape[0]
    assert ids.shape == (M, k) and ids.dtype == torch.int32 and lps.shape == (M, k) and lps.dtype == torch.float32
    assert torch.equal(bits(x), bits(x0))                       # the logits are only read
    stable = torch.sort(x.float(), dim=-1, descending=True, stable=True).indices[:, :k]
    assert torch.equal(want_ids.long(), stable)
    assert torch.equal(ids, want_ids), (ids != want_ids).nonzero()[:8].tolist()
    assert ids[1].tolist() == list(range(k))                    # the all-equal row
    if M == 5:
        assert ids[2, 0].item() == V - 1 and (k == 1 or ids[2, 1].item() == 5)
    tie_row = 3 if M == 5 else 2
    assert ids[tie_row, :min(k, 5)].tolist() == [25, 161, 16, 19, 21][:min(k, 5)]
    if V == 8 * 1025 and k >= 7:
        assert ids[3, 5:7].tolist() == [17, 8 * 1024 + 3]
    e = _ulps((lps.double() - want_lps).abs(), lse[:, None].expand_as(want_lps), want_lps).max().item()
    report(f"teacher_topk V={V} k={k} tau={tau}: log-probabilities (fp32 ulps of the larger of lse and entry)", e, bound)
    assert 0 < bound and e <= bound


@pytest.mark.parametrize("V,k", [(8 * 257, 7), (8 * 2049, 64), (8 * 2049, 256)])
def test_teacher_topk_row_isolation_and_repeat(V, k):
    """One row replaced by large values: every other row's outputs keep their bits; and a second call on the same
    input returns the same bits (the LDS counters are integers)."""
    x = _topk_rows(V)
    ids0, lps0 = ops.teacher_topk(x, k, 0.9)
    ids1, lps1 = ops.teacher_topk(x, k, 0.9)
    assert torch.equal(ids0, ids1) and torch.equal(bits(lps0), bits(lps1))
    for r in (0, 3):
        xp = x.clone()
        xp[r] = (1e4 * torch.randn(V, device=DEV)).to(BF16)
        ids2, lps2 = ops.teacher_topk(xp, k, 0.9)
        others = torch.arange(5, device=DEV) != r
        assert torch.equal(ids2[others], ids0[others]) and torch.equal(bits(lps2[others]), bits(lps0[others]))
        assert not torch.equal(ids2[r], ids0[r])
        assert torch.equal(ids2[r].long(), torch.sort(xp[r].float(), descending=True, stable=True).indices[:k])


def test_teacher_topk_refusals():
    x = _topk_rows(8 * 32)
    o = _ext.ops()
    bad = [lambda: o.teacher_topk(x.float(), 4, 1.0),                      # fp32 input
           lambda: o.teacher_topk(x[:, :252].contiguous(), 4, 1.0),        # V % 8 != 0
           lambda: o.teacher_topk(x, 0, 1.0),
           lambda: o.teacher_topk(x, 257, 1.0),
           lambda: o.teacher_topk(x[:, :64].contiguous(), 65, 1.0),        # k > V
           lambda: o.teacher_topk(x, 4, 0.0),
           lambda: o.teacher_topk(x, 4, -1.0),
           lambda: o.teacher_topk(x[:, ::2], 4, 1.0),                      # not contiguous
           lambda: o.teacher_topk(x.cpu(), 4, 1.0)]
    for fn in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
    with pytest.raises(ValueError):
        ops.teacher_topk(x, 4, 0.0)
    ids, lps = o.teacher_topk(x[:0], 4, 1.0)
    assert ids.shape == (0, 4) and lps.shape == (0, 4)


# ------------------------------------------------------------------------------------------------ kd_topk_fwd
KD_KINDS = ["random", "the teacher's top-k taken from the student itself", "label -100",
            "near-one-hot teacher at column V - 1 where the student is near its minimum",
            "near-one-hot student where the teacher is near its minimum", "gaps of 150"]
KD_BIG_KINDS = [0, 5, 2]


def _kd_rows(V):
    """bf16 student / teacher logits [M, V] and labels, one row per kind of KD_KINDS (KD_BIG_KINDS for the two training
    vocabularies)."""
    g = torch.Generator(device=DEV).manual_seed(V)
    s = (3 * torch.randn(6, V, device=DEV, generator=g)).to(BF16)
    t = (3 * torch.randn(6, V, device=DEV, generator=g)).to(BF16)
    labels = torch.randint(0, V, (6,), device=DEV, generator=g)
    labels[0] = int(s[0].float().argmax())                 # a row the student gets right
    t[1] = s[1]
    labels[2] = -100
    t[3, V - 1] = t[3].float().max() + 30.0
    s[3, V - 1] = s[3].float().min()
    c = int(torch.randint(0, V, (1,), device=DEV, generator=g))
    s[4, c] = s[4].float().max() + 30.0
    t[4, c] = t[4].float().min()
    n = max(1, V // 16)
    s[5, :n] += 150.0
    t[5, V - n:] += 150.0
    if V > 100000:
        keep = torch.tensor(KD_BIG_KINDS, device=DEV)
        s, t, labels = s[keep], t[keep], labels[keep]
    return s.contiguous(), t.contiguous(), labels.contiguous()


def _cache_of(t, k, tau):
    """The cached (ids, logps) of teacher logits t: the fp64 reference top-k, rounded to fp32."""
    ids, lps = ref.teacher_topk(t.double(), k, tau)
    return ids.contiguous(), lps.float().contiguous()


def _kd_topk_refs(s, ids, lps, labels, tau):
    """fp64 (loss, grad, lse, mass) of the definition on the bf16 logits and the fp32 cache, and the fp32 emulation
    (loss, bf16 grad, lse, mass) with the kernel's rounding points: logits times fp32(1 / tau), lse = m + log s, p_k
    = exp(tlp_k), the loss terms p_k (tlp_k - (a_k - lse)), the gradient (m e^lp) scale with the K corrected elements
    (m e^lp_k - p_k) scale, each rounded once to bf16."""
    sc = torch.tensor([SCALE], dtype=torch.float64, device=DEV)
    loss, lse, mass, _, _ = ref.distill_topk(s.double(), ids, lps.double(), labels, tau)
    grad = ref.distill_topk_grad(s.double(), ids, lps.double(), labels, sc, tau)
    valid = (labels != -100).float()
    it = f32(1.0 / tau)
    a = s.float() * it
    ls = lse32(a)
    idx = ids.long()
    lpk = a.gather(1, idx) - ls[:, None]
    p = exp32(lps)
    m32 = p.sum(-1)
    loss32 = (p * (lps - lpk)).sum(-1)
    scale = f32(SCALE) * it
    g32 = (m32[:, None] * exp32(a - ls[:, None])) * scale
    g32 = g32.scatter(1, idx, (m32[:, None] * exp32(lpk) - p) * scale)
    return (loss, grad, lse, mass), (loss32 * valid, (g32 * valid[:, None]).to(BF16), ls, m32)


def _errs(got, want, ids):
    """(loss ulps, lse ulps, mass ulps, worst gradient row, worst row of the K corrected elements) of (loss, grad, lse,
    mass) against the fp64 ``want``."""
    loss, grad, lse, mass = want
    V = grad.shape[1]
    idx = ids.long()
    k = idx.shape[1]
    gk, wk = got[1].double().gather(1, idx), grad.gather(1, idx)
    return (_ulps((got[0].double() - loss).abs(), lse, loss).max().item(),
            _ulps((got[2].double() - lse).abs(), lse).max().item(),
            _ulps((got[3].double() - mass).abs(), mass).max().item(),
            block_rel_err(got[1], grad, 1, V).max().item(),
            block_rel_err(gk, wk, 1, k).max().item())


@pytest.fixture(scope="module")
def kd_cases():
    """Per (V, k, tau): inputs and fp64 references, computed once and left unchanged; the bounds pooled over the grid:
    (loss, lse, mass, gradient rows, corrected elements). The K corrected elements of a row are judged as a block of
    their own, [M, K] gathered at the ids, against the larger of their norm and the typical norm of such a block (the
    floor of block_rel_err): a row whose gradient vanishes (the teacher taken from the student at k = V) counts against
    the typical magnitude, as it does in the row check."""
    rows = {V: _kd_rows(V) for V in SMALL_V + BIG_V}
    cases, bound = {}, [0.0] * 5
    for V, k, tau in KD_GRID:
        s, t, labels = rows[V]
        ids, lps = _cache_of(t, k, tau)
        want, emul = _kd_topk_refs(s, ids, lps, labels, tau)
        cases[V, k, tau] = (s, ids, lps, labels, want)
        bound = [max(b, e) for b, e in zip(bound, _errs(emul, want, ids))]
    return cases, [2 * b for b in bound]


def _call(s, ids, lps, labels, write_grad, tau):
    lg, i0, l0 = s.clone(), ids.clone(), lps.clone()
    stats = _ext.ops().kd_topk_fwd(lg, ids, lps, labels, torch.tensor([SCALE], device=DEV), write_grad, tau)
    assert torch.equal(ids, i0) and torch.equal(bits(lps), bits(l0))  # the cache is only read
    return lg, stats


def _check(what, s, ids, lps, labels, tau, want, bounds):
    loss, grad, lse, mass = want
    M, V = s.shape
    valid = labels != -100
    lg, stats = _call(s, ids, lps, labels, True, tau)
    torch.cuda.synchronize()
    assert stats.shape == (5, M) and stats.dtype == torch.float32
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(lg.float()).all())
    errs = _errs((stats[0], lg, stats[1], stats[2]), want, ids)
    names = ["loss (fp32 ulps of the row's largest term)", "lse (fp32 ulps)", "teacher mass (fp32 ulps)",
             "gradient rows", "the K corrected gradient elements, per row"]
    for n, e, b in zip(names, errs, bounds):
        report(f"{what}: {n}", e, b)
    assert all(0 < b for b in bounds) and bounds[3] < 1e-2 and bounds[4] < 1e-2
    for n, e, b in zip(names, errs, bounds):
        assert e <= b, (n, e, b)
    assert bool((stats[0][~valid] == 0).all())
    assert not bits(lg[~valid]).any()               # a label of -100: every gradient element has zero bits
    top = first_argmax(s.float())
    assert torch.equal(stats[3], ((top == labels) & valid).float())
    assert torch.equal(stats[4], ((top == ids[:, 0]) & valid).float())
    return lg, stats


@pytest.mark.parametrize("V,k,tau", KD_GRID)
def test_kd_topk_fwd_rows(V, k, tau, kd_cases):
    cases, bounds = kd_cases
    s, ids, lps, labels, want = cases[V, k, tau]
    _, stats = _check(f"kd_topk_fwd V={V} k={k} tau={tau}", s, ids, lps, labels, tau, want, bounds)
    assert stats[3][0].item() == 1.0                # the row the student gets right
    if s.shape[0] == 6:
        assert stats[4][1].item() == 1.0            # the teacher taken from the student agrees with it
        assert int(ids[3, 0]) == V - 1


@pytest.mark.parametrize("V", [8 * 1025, 128256])
def test_kd_topk_fwd_planted_ids(V, kd_cases):
    """ids at column 0, at column V - 1, two in one 16-byte vector, one in the tail vector, one equal to the label, one
    equal to the student's argmax; the rest random and distinct. The log-probabilities are a second teacher's at those
    columns (the kernel does not ask for the largest)."""
    _, bounds = kd_cases
    k, tau = 64, 0.9
    s, t, labels = _kd_rows(V)
    M = s.shape[0]
    g = torch.Generator(device=DEV).manual_seed(11)
    valid = labels != -100
    lab = torch.where(valid, labels, torch.full_like(labels, 40))
    top = first_argmax(s.float())
    tail = 8 * (V // 8 - 1) + 3  # (V / 8 = 1025 and 16032: the last vector is past the 4 x 256 unrolled rounds)
    planted = torch.stack([torch.zeros_like(lab), torch.full_like(lab, V - 1), torch.full_like(lab, 16),
                           torch.full_like(lab, 19), torch.full_like(lab, tail), lab, top], 1)
    ids = []
    for r in range(M):
        seen, row = set(), []
        for c in planted[r].tolist() + torch.randperm(V, device=DEV, generator=g)[:k + 8].tolist():
            if c not in seen and len(row) < k:
                seen.add(c)
                row.append(c)
        ids.append(row)
    ids = torch.tensor(ids, dtype=torch.int32, device=DEV)
    lps = torch.log_softmax(t.double() / tau, -1).gather(1, ids.long()).float().contiguous()
    want, _ = _kd_topk_refs(s, ids, lps, labels, tau)
    lg, _ = _check(f"kd_topk_fwd planted ids V={V}", s, ids, lps, labels, tau, want, bounds)
    # the planted elements one by one: each within one bf16 rounding (2^-8) of the reference, plus the row's fp32 noise
    got, ref64 = lg.double().gather(1, ids[:, :7].long()), want[1].gather(1, ids[:, :7].long())
    floor = want[1].abs().max(-1, keepdim=True).values * 2.0 ** -20
    assert bool(((got - ref64).abs() <= ref64.abs() * 2.0 ** -8 + floor).all())


@pytest.mark.parametrize("V,k", [(8 * 32, 7), (8 * 1025, 64), (128256, 256)])
def test_kd_topk_fwd_stats_only(V, k):
    """write_grad=False: the student's logits stay untouched, bit for bit, and the stats equal those of a
    write_grad=True call on a clone."""
    s, t, labels = _kd_rows(V)
    ids, lps = _cache_of(t, k, 0.9)
    lg, st = _call(s, ids, lps, labels, False, 0.9)
    assert torch.equal(bits(lg), bits(s))
    lg1, st1 = _call(s, ids, lps, labels, True, 0.9)
    assert torch.equal(bits(st), bits(st1)) and not torch.equal(bits(lg1), bits(s))


@pytest.mark.parametrize("V,k", [(8 * 257, 7), (8 * 2049, 64)])
def test_kd_topk_fwd_row_isolation(V, k):
    """One row's student logits replaced by large values: that row's stats and gradient move, every other row's bits
    stay."""
    s, t, labels = _kd_rows(V)
    ids, lps = _cache_of(t, k, 0.9)
    lg0, st0 = _call(s, ids, lps, labels, True, 0.9)
    for r in (0, 3):
        sp = s.clone()
        sp[r] = (1e4 * torch.randn(V, device=DEV)).to(BF16)
        lg1, st1 = _call(sp, ids, lps, labels, True, 0.9)
        others = torch.arange(6, device=DEV) != r
        assert torch.equal(bits(st1[:, others]), bits(st0[:, others]))
        assert torch.equal(bits(lg1[others]), bits(lg0[others]))
        assert st1[0, r].item() != st0[0, r].item() and not torch.equal(bits(lg1[r]), bits(lg0[r]))


def test_kd_topk_fwd_full_support_is_kd_fwd_forward_kl(kd_cases):
    """V = k = 256: loss and gradient agree with kd_fwd(beta=0) on the dense teacher within the two kernels' bounds, and
    the teacher mass is 1 within its bound. The cache holds the teacher's log-probabilities rounded to fp32, so the two
    fp64 references differ by that rounding: their own distance is added to each bound, computed from the references."""
    _, bounds = kd_cases
    V = k = 256
    rel = {}
    for tau in (1.0, 0.9, 2.0):
        s, t, labels = _kd_rows(V)
        ids, lps = _cache_of(t, k, tau)
        want, _ = _kd_topk_refs(s, ids, lps, labels, tau)
        sc = torch.tensor([SCALE], dtype=torch.float64, device=DEV)
        d_loss, d_lse_s, d_lse_t, _, _ = ref.generalized_jsd(s.double(), t.double(), labels, 0.0, tau)
        d_grad = ref.generalized_jsd_grad(s.double(), t.double(), labels, sc, 0.0, tau)
        # kd_fwd's forward-KL emulation (tests/test_distill_gpu.py _kd_refs) for its two bounds
        it = f32(1.0 / tau)
        a, b = s.float() * it, t.float() * it
        ls, lt = lse32(a), lse32(b)
        mt = b.max(-1, keepdim=True).values
        et = exp32(b - mt)
        vf = (labels != -100).float()
        e_loss = ((et * (b - a)).sum(-1) / et.sum(-1) + (ls - lt)) * vf
        e_grad = (((exp32(a - ls[:, None]) - exp32(b - lt[:, None])) * (f32(SCALE) * it)) * vf[:, None]).to(BF16)
        b_loss = 2 * _ulps((e_loss.double() - d_loss).abs(), d_lse_s, d_lse_t, d_loss).max().item()
        b_grad = 2 * block_rel_err(e_grad, d_grad, 1, V).max().item()
        lg_k, st_k = _call(s, ids, lps, labels, True, tau)
        lg_d = s.clone()
        st_d = _ext.ops().kd_fwd(lg_d, t, labels, torch.tensor([SCALE], device=DEV), True, 0.0, tau)
        torch.cuda.synchronize()
        between = _ulps((want[0] - d_loss).abs(), d_lse_s, d_lse_t, d_loss).max().item()
        e = _ulps((st_k[0].double() - st_d[0].double()).abs(), d_lse_s, d_lse_t, d_loss).max().item()
        report(f"kd_topk_fwd vs kd_fwd V=k=256 tau={tau}: loss (fp32 ulps)", e, bounds[0] + b_loss + between)
        assert e <= bounds[0] + b_loss + between
        g_between = block_rel_err(want[1], d_grad, 1, V).max().item()
        eg = block_rel_err(lg_k, lg_d.double(), 1, V, rms=d_grad.pow(2).mean().sqrt()).max().item()
        report(f"kd_topk_fwd vs kd_fwd V=k=256 tau={tau}: gradient rows", eg, bounds[3] + b_grad + g_between)
        assert eg <= bounds[3] + b_grad + g_between
        one = torch.ones_like(want[3])
        m_between = _ulps((want[3] - one).abs(), one).max().item()
        em = _ulps((st_k[2].double() - one).abs(), one).max().item()
        report(f"kd_topk_fwd V=k=256 tau={tau}: teacher mass against 1 (fp32 ulps)", em, bounds[2] + m_between)
        assert em <= bounds[2] + m_between
        rel[tau] = (e, eg, em)
    assert len(rel) == 3


def test_kd_topk_fwd_refusals():
    s, t, labels = _kd_rows(64)
    ids, lps = _cache_of(t, 7, 1.0)
    inv = torch.tensor([SCALE], device=DEV)
    o = _ext.ops()
    big = torch.zeros(6, 257, dtype=torch.int32, device=DEV)
    bad = [lambda: o.kd_topk_fwd(s.float(), ids, lps, labels, inv, True, 1.0),                  # fp32 logits
           lambda: o.kd_topk_fwd(s[:, :60].contiguous(), ids, lps, labels, inv, True, 1.0),     # V % 8
           lambda: o.kd_topk_fwd(s.clone(), ids.long(), lps, labels, inv, True, 1.0),           # int64 ids
           lambda: o.kd_topk_fwd(s.clone(), ids, lps.double(), labels, inv, True, 1.0),
           lambda: o.kd_topk_fwd(s.clone(), ids[:5], lps[:5], labels, inv, True, 1.0),          # rows
           lambda: o.kd_topk_fwd(s.clone(), ids, lps[:, :6].contiguous(), labels, inv, True, 1.0),
           lambda: o.kd_topk_fwd(s.clone(), ids[:, ::2], lps[:, ::2], labels, inv, True, 1.0),  # not contiguous
           lambda: o.kd_topk_fwd(s.clone(), big, big.float(), labels, inv, True, 1.0),          # k > 256 (and > V)
           lambda: o.kd_topk_fwd(s.clone(), ids[:, :0], lps[:, :0], labels, inv, True, 1.0),    # k = 0
           lambda: o.kd_topk_fwd(s.clone(), ids.cpu(), lps, labels, inv, True, 1.0),
           lambda: o.kd_topk_fwd(s.clone(), ids, lps, labels, inv, True, 0.0),
           lambda: o.kd_topk_fwd(s.clone(), ids, lps, labels, inv.cpu(), True, 1.0),
           lambda: o.kd_topk_fwd(s.clone(), ids, lps, labels.int(), inv, True, 1.0),
           lambda: o.kd_topk_fwd(s.clone(), ids, lps, labels[:5], inv, True, 1.0)]
    for fn in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
    empty = o.kd_topk_fwd(s[:0], ids[:0], lps[:0], labels[:0], inv, True, 1.0)
    assert empty.shape == (5, 0) and empty.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ lm_head_distill_topk_loss
T_ROWS, HID, VOC, TOPK = 70, 256, 1024, 64


def _head_case():
    g = torch.Generator(device=DEV).manual_seed(5)
    h = torch.randn(T_ROWS, HID, generator=g, device=DEV).to(BF16)
    w = (0.06 * torch.randn(VOC, HID, generator=g, device=DEV)).to(BF16)
    teacher = (2.0 * torch.randn(T_ROWS, VOC, generator=g, device=DEV)).to(BF16)
    labels = torch.randint(0, VOC, (T_ROWS,), generator=g, device=DEV)
    labels[:9] = -100
    labels[33] = -100
    labels[-1] = -100
    return h, w, teacher, labels


def _head_refs(h, w, ids, lps, labels, tau, gl, dt):
    """(loss, dh, dW) of gl * loss in ``dt``; dt fp32 rounds where the HIP path does: bf16 logits, the bf16 gradient
    over them, the loss gradient rounded to bf16 on the bf16 G W and on h, one bf16 rounding of each result."""
    emul = dt == torch.float32
    rnd = (lambda x: x.to(BF16).to(dt)) if emul else (lambda x: x)
    n = (labels != -100).sum().to(dt)
    inv = (1.0 / n).reshape(1)
    logits = rnd(h.to(dt) @ w.to(dt).t())
    loss = ref.distill_topk(logits, ids, lps.to(dt), labels, tau)[0].sum() * inv[0]
    G = rnd(ref.distill_topk_grad(logits, ids, lps.to(dt), labels, inv, tau))
    g = rnd(torch.tensor(gl, dtype=dt, device=DEV))
    dh = rnd(rnd(G @ w.to(dt)) * g)
    dw = rnd(G.t() @ rnd(h.to(dt) * g))
    return loss, dh, dw


@pytest.mark.parametrize("gl", [1.0, 1.0 / 7.0])
def test_lm_head_distill_topk_loss_against_fp64(gl):
    tau = 0.9
    h, w, teacher, labels = _head_case()
    ids, lps = _cache_of(teacher, TOPK, tau)
    want = _head_refs(h, w, ids, lps, labels, tau, gl, torch.float64)
    emul = _head_refs(h, w, ids, lps, labels, tau, gl, torch.float32)
    inv = (1.0 / (labels != -100).sum().float()).reshape(1)
    hh, ww = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    i0, l0 = ids.clone(), lps.clone()
    loss, stats = ops.lm_head_distill_topk_loss(hh, ww, ids, lps, labels, inv, tau)
    assert stats.shape == (5, T_ROWS) and loss.dtype == torch.float32
    (loss * gl).backward()
    assert torch.equal(ids, i0) and torch.equal(bits(lps), bits(l0))
    bl = 2 * abs(emul[0].item() - want[0].item()) / abs(want[0].item())
    el = abs(loss.item() - want[0].item()) / abs(want[0].item())
    report(f"lm_head_distill_topk_loss dloss={gl:.3f}: loss", el, bl)
    assert bl > 0 and el <= bl
    bh = 2 * block_rel_err(emul[1], want[1], 1, HID).max().item()
    eh = assert_blocks_close(hh.grad, want[1], 1, HID, bh, "dh")
    report(f"lm_head_distill_topk_loss dloss={gl:.3f}: dh rows", eh, bh)
    bw = 2 * block_rel_err(emul[2], want[2], 32, 32).max().item()
    ew = assert_blocks_close(ww.grad, want[2], 32, 32, bw, "dW")
    report(f"lm_head_distill_topk_loss dloss={gl:.3f}: dW (32 x 32 blocks)", ew, bw)
    assert not (hh.grad[labels == -100] != 0).any()
    # a frozen weight: no dW, the same dh
    h2, wf = h.clone().requires_grad_(True), w.clone()
    loss2, _ = ops.lm_head_distill_topk_loss(h2, wf, ids, lps, labels, inv, tau)
    (loss2 * gl).backward()
    assert wf.grad is None and torch.equal(bits(h2.grad), bits(hh.grad)) and loss2.item() == loss.item()
    # the teacher's side: the forward GEMM and teacher_topk, against the stable sort of the same logits
    tid, tlp = ops.lm_head_topk_logps(h, w, TOPK, tau)
    lg = ops.lm_head_logits(h, w)
    assert torch.equal(tid.long(), torch.sort(lg.float(), dim=-1, descending=True, stable=True).indices[:, :TOPK])
    assert not tlp.requires_grad and tlp.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ model, HIP vs reference
LENS = [37, 64, 1, 90]
PAD_ROWS = 64


def _ragged_batch(vocab):
    g = torch.Generator(device=DEV).manual_seed(3)
    c = [0]
    for n in LENS + [PAD_ROWS]:
        c.append(c[-1] + n)
    ids = torch.randint(0, vocab, (c[-1],), generator=g, device=DEV)
    labels = ids.clone()
    for s, k in enumerate([9, 5, 0, 17]):
        labels[c[s]:c[s] + k] = -100
    labels[c[4]:] = -100
    pos = torch.cat([torch.arange(b - a, device=DEV) for a, b in zip(c[:-1], c[1:])])
    return dict(input_ids=ids, labels=labels, cu_seqlens=torch.tensor(c, dtype=torch.int32, device=DEV),
                position_ids=pos, max_seqlen=max(LENS))


def _padded_batch(vocab):
    g = torch.Generator(device=DEV).manual_seed(4)
    ids = torch.randint(0, vocab, (4, 64), generator=g, device=DEV)
    labels = ids.clone()
    for r, (skip, n) in enumerate([(9, 37), (5, 64), (0, 2), (17, 50)]):
        labels[r, :skip] = -100
        labels[r, n:] = -100
    return dict(input_ids=ids, labels=labels)


def _distill_run(model, batch, tid, tlp, hip, monkeypatch, tau):
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    out = model.distill_topk_loss(teacher_ids=tid, teacher_logps=tlp, temperature=tau, **batch)
    out.loss.backward()
    torch.cuda.synchronize()
    return out, {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("lora", [False, True])
def test_distill_topk_loss_hip_vs_reference(lora, layout, monkeypatch):
    torch.manual_seed(0)
    cfg = get_config("tiny-gpu")
    m = build_model(cfg, device=DEV, dtype=BF16, seed=1)
    te = build_model(get_config("tiny-gpu-mistral"), device=DEV, dtype=BF16, seed=2).eval().requires_grad_(False)
    if lora:
        from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora
        apply_lora(m, LoRAConfig(r=16, lora_alpha=32.0, lora_dropout=0.0))
        with torch.no_grad():  # B = 0 would make every A gradient zero
            for layer in m.model.layers:
                for fl in (*layer.self_attn.lora.values(), *layer.mlp.lora.values()):
                    for b in fl.B:
                        torch.nn.init.normal_(b, std=0.02)
    m.train()
    batch = (_ragged_batch if layout == "ragged" else _padded_batch)(cfg.vocab_size)
    inputs = {k: v for k, v in batch.items() if k != "labels"}
    tau, k = 0.9, 64
    with torch.no_grad():
        tid, tlp = te.topk_logps_rows(k=k, temperature=tau, **inputs)
        t_logits = te.logits_rows(**inputs)
    assert tid.shape == (256, k) and tid.dtype == torch.int32 and tlp.dtype == torch.float32 and not tlp.requires_grad
    assert torch.equal(tid.long(), torch.sort(t_logits.float(), dim=-1, descending=True, stable=True).indices[:, :k])
    if layout == "padded":  # the collator's [B, T, k] form
        tid, tlp = tid.view(4, 64, k), tlp.view(4, 64, k)
    o_hip, g_hip = _distill_run(m, batch, tid, tlp, True, monkeypatch, tau)
    o_ref, g_ref = _distill_run(m, batch, tid, tlp, False, monkeypatch, tau)
    assert o_hip.stats.shape == (5, 256) and o_hip.metrics.shape == (3,)
    assert o_hip.num_tokens.item() == o_ref.num_tokens.item() == o_hip.metrics[2].item() > 0
    assert 0 < o_hip.teacher_mass.item() <= o_hip.num_tokens.item() * (1 + 1e-5)
    what = f"distill_topk_loss tiny-gpu{' lora' if lora else ''} <- tiny-gpu-mistral {layout}"
    el = abs(o_hip.loss.item() - o_ref.loss.item()) / abs(o_ref.loss.item())
    report(f"{what}: loss", el, 2e-2)
    assert o_ref.loss.item() > 0 and el < 2e-2
    assert g_ref and set(g_ref) == set(g_hip)
    if lora:
        assert all(".lora." in n for n in g_ref)
    worst, name = 0.0, ""
    for n in g_ref:
        e = ((g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)).item()
        if e > worst:
            worst, name = e, n
    report(f"{what}: gradients (worst: {name})", worst, 5e-2)
    assert worst < 5e-2, (name, worst)


def test_topk_methods_refuse_a_reward_model():
    rm = build_model(dataclasses.replace(get_config("tiny-gpu"), num_labels=1), device=DEV, dtype=BF16, seed=1)
    ids = torch.randint(0, 100, (2, 16), device=DEV)
    with pytest.raises(RuntimeError, match="reward model"):
        rm.topk_logps_rows(ids, k=4)
    with pytest.raises(RuntimeError, match="reward model"):
        rm.distill_topk_loss(ids, ids, torch.zeros(32, 4, dtype=torch.int32, device=DEV),
                             torch.zeros(32, 4, device=DEV))


# ------------------------------------------------------------------------------------------------ trainer
def _gkd_trainer(out, teacher=True, save_steps=0, **over):
    from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
    from llm_fine_tune_distributed_amd.train import GKDConfig, GKDTrainer
    kw = dict(output_dir=str(out), per_device_train_batch_size=4, per_device_eval_batch_size=4, max_steps=3,
              learning_rate=1e-3, lr_scheduler_type="constant", logging_steps=1, jsonl_log=False,
              save_strategy="steps" if save_steps else "no", save_steps=save_steps or 500, seed=3,
              dataloader_drop_last=True, beta=0.0, temperature=0.9, teacher_topk=64)
    kw.update(over)
    a = GKDConfig(**kw)
    student = build_model(get_config("tiny-gpu"), device=DEV, dtype=BF16, seed=0)
    te = build_model(get_config("tiny-gpu-mistral"), device=DEV, dtype=BF16, seed=9) if teacher else None
    ds = TokenizedDataset.synthetic(4, 1024, 30, 90, seed=2)  # one batch, seen every step
    return GKDTrainer(model=student, args=a, train_dataset=ds, eval_dataset=ds, teacher_model=te)


def _params(t):
    t.optimizer.synchronize()
    torch.cuda.synchronize()
    return t.engine.param_flat.clone()


def _losses(t):
    return [h["loss"] for h in t.state.log_history if "loss" in h]


@pytest.fixture(scope="module")
def gkd_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("gkd_topk")
    t = _gkd_trainer(out, save_steps=2)
    assert t.teacher is not None and not os.path.exists(t.teacher_topk_path())
    t.precompute_teacher_topk()
    assert t.teacher is None and os.path.exists(t.teacher_topk_path())
    calls = []
    real = CausalLM.logits_rows, CausalLM.topk_logps_rows
    CausalLM.logits_rows = lambda self, *a, **k: (calls.append("logits_rows"), real[0](self, *a, **k))[1]
    CausalLM.topk_logps_rows = lambda self, *a, **k: (calls.append("topk_logps_rows"), real[1](self, *a, **k))[1]
    _ext.ops().dispatch_trace(True)
    try:
        t.train()
        ev = t.evaluate()
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
        CausalLM.logits_rows, CausalLM.topk_logps_rows = real
    trace = {k: int(v) for k, v in (it.split("=") for it in _ext.ops().dispatch_trace_read().split(";") if it)}
    return t, trace, calls, ev, out


def test_gkd_topk_steps_run_from_the_cache(gkd_run):
    t, trace, calls, ev, _ = gkd_run
    assert trace.get("kd_topk_fwd", 0) >= 3 + 1, sorted(trace)  # three steps and the evaluation batch
    assert not [k for k in trace if k.startswith("kd_fwd") or k == "teacher_topk"], sorted(trace)
    assert calls == [] and t.teacher is None                     # no teacher forward in the steps
    losses = _losses(t)
    print(f"\n[distill_topk] GKDTrainer losses {losses}")
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses) and losses[2] < losses[0], losses
    logs = [h for h in t.state.log_history if "loss" in h]
    for k in ("mean_token_accuracy", "teacher_agreement", "teacher_mass", "grad_norm", "learning_rate", "epoch",
              "num_tokens"):
        assert k in logs[-1], k
    assert 0.0 < logs[-1]["teacher_mass"] <= 1.0 + 1e-5
    assert math.isfinite(ev["eval_loss"]) and ev["eval_loss"] > 0 and 0.0 <= ev["eval_teacher_agreement"] <= 1.0


def test_gkd_topk_second_trainer_needs_no_teacher(gkd_run):
    t, _, _, _, out = gkd_run
    t2 = _gkd_trainer(out, teacher=False)
    assert t2.teacher is None
    t2.train()
    assert _losses(t2) == _losses(t)  # bit for bit: the floats of the logs are equal
    assert torch.equal(bits(_params(t2)), bits(_params(t)))


def test_gkd_topk_resume_bit_for_bit(gkd_run):
    t, _, _, _, out = gkd_run
    assert os.path.isdir(os.path.join(str(out), "checkpoint-2"))
    t2 = _gkd_trainer(out, teacher=False)
    torch.manual_seed(12345)
    t2.train(resume_from_checkpoint="auto")
    assert t2.state.global_step == 3
    a, b = _params(t), _params(t2)
    assert torch.equal(bits(a), bits(b)), int((a != b).sum())


def test_gkd_topk_file_refused_when_k_or_temperature_changes(gkd_run, tmp_path):
    t, _, _, _, out = gkd_run
    for over in (dict(teacher_topk=32), dict(temperature=1.0)):
        with pytest.raises(ValueError, match="needs a teacher"):  # another fingerprint: no file, and no teacher
            _gkd_trainer(out, teacher=False, **over)
        # the file under the other run's name: its recorded k / temperature do not match
        other = _gkd_trainer(tmp_path / "x", **over)
        os.makedirs(os.path.dirname(other.teacher_topk_path()), exist_ok=True)
        shutil.copy(t.teacher_topk_path(), other.teacher_topk_path())
        with pytest.raises(ValueError, match="was written for"):
            other.train()
    with pytest.raises(FileNotFoundError):  # a resume needs the file
        tr = _gkd_trainer(tmp_path / "y")
        tr.train(resume_from_checkpoint=os.path.join(str(out), "checkpoint-2"))
