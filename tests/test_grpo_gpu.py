"""GRPO on the GPU: ce_fwd at a temperature, the kernels of csrc/policy.hip (grpo_token_fwd, scale_rows), the
full-vocabulary sampler (sample_tokens_full in csrc/sampler.hip), the policy LM head built on them
(ops.lm_head_policy_loss), CausalLM.policy_loss on the HIP path against the PyTorch reference path, rollout_batch and
GRPOTrainer steps with the kernels' dispatch trace.

Bounds follow tests/test_dpo_gpu.py: each is 2 x the worst error of an fp32 torch emulation with the kernel's rounding
points against the fp64 reference, computed here from the references alone; every test prints its worst measured error
next to the bound (pytest -s); profiles/grpo.md records one run. The cross-entropy statistics use the bounds of
tests/test_kernels_gpu.py::test_cross_entropy, the model tests those of tests/test_dpo_gpu.py."""
import glob
import math
import os

import pytest
import torch

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.inference.generation import rollout_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close, block_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def report(what, worst, bound):
    print(f"\n[grpo] {what}: worst {worst:.3e} bound {bound:.3e}")


def rel_err(got, want64):
    """|got - want| / |want| per element; where the reference is exactly 0 the value must be 0 too."""
    d = (got.double() - want64).abs()
    return torch.where(want64 != 0, d / want64.abs().clamp_min(1e-300),
                       torch.where(d > 0, torch.full_like(d, math.inf), d))


def cu_of(lens, pad=0):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    if pad:
        c.append(c[-1] + pad)
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def raises(*calls):
    for bad in calls:
        with pytest.raises((RuntimeError, NotImplementedError, ValueError)):
            bad()


# ------------------------------------------------------------------------------------------------ ce_fwd at a temperature
def _first_max(x):
    V = x.shape[-1]
    idx = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values


def _ce_case(V):
    M = 3 if V > 100000 else 5
    g = torch.Generator(device=DEV).manual_seed(V)
    logits = (3 * torch.randn(M, V, generator=g, device=DEV)).to(BF16)
    labels = torch.tensor([0, V - 1, V - 3, 17, 8 * (V // 8 - 1) + 2][:M], device=DEV)
    labels[1] = -100
    return logits, labels


@pytest.mark.parametrize("write_grad", [True, False])
@pytest.mark.parametrize("tau", [0.7, 1.5])
@pytest.mark.parametrize("V", [264, 8200, 128256])
def test_ce_temperature(V, tau, write_grad):
    logits, labels = _ce_case(V)
    M = logits.shape[0]
    inv = torch.tensor([1.0 / 7.0], device=DEV)
    lg = logits.clone()
    stats = _ext.ops().ce_fwd(lg, labels, inv, write_grad, 0.0, 0, tau)
    assert stats.shape == (4, M) and stats.dtype == torch.float32 and torch.isfinite(stats).all()
    z = logits.double() / tau
    valid = labels != -100
    logp = torch.log_softmax(z, -1)
    lse = torch.logsumexp(z, -1)
    safe = labels.clamp(min=0)
    loss = torch.where(valid, -logp.gather(-1, safe[:, None]).squeeze(-1), torch.zeros_like(lse))
    ent = -(logp.exp() * logp).sum(-1)
    for name, got, want, atol, rtol in (("loss", stats[0], loss, 2e-3, 1e-3), ("lse", stats[1], lse, 2e-3, 1e-3),
                                        ("entropy", stats[2], ent, 2e-2, 1e-2)):
        err = (got.double() - want).abs()
        print(f"\n[grpo] ce_fwd V={V} tau={tau} grad={write_grad} {name}: worst {err.max().item():.3e}")
        assert bool((err <= atol + rtol * want.abs()).all()), (name, got.tolist(), want.tolist())
    assert torch.equal(stats[3].bool(), (_first_max(logits.double()) == labels) & valid)
    if not write_grad:
        assert torch.equal(bits(lg), bits(logits))  # untouched
        return
    onehot = torch.zeros_like(z)
    onehot[valid, labels[valid]] = 1.0
    want = (logp.exp() - onehot) * inv.double() * valid[:, None]  # no 1 / tau: the caller's row weight carries it
    emul = ref.cross_entropy_grad(logits, labels, inv, temperature=tau).to(BF16)
    bc = 264
    bound = 2 * block_rel_err(emul, want, 1, bc).max().item()
    worst = assert_blocks_close(lg, want, 1, bc, bound, "dlogits")
    report(f"ce_fwd V={V} tau={tau} gradient (1 x {bc} blocks)", worst, bound)
    assert bound > 0
    assert not bits(lg[1]).any()  # the ignored row: +0


@pytest.mark.parametrize("V", [264, 8200])
def test_ce_temperature_one_is_the_plain_call(V):
    logits, labels = _ce_case(V)
    inv = torch.tensor([1.0 / 7.0], device=DEV)
    a, b = logits.clone(), logits.clone()
    sa = _ext.ops().ce_fwd(a, labels, inv, True)
    sb = _ext.ops().ce_fwd(b, labels, inv, True, 0.0, 0, 1.0)
    assert torch.equal(bits(sa), bits(sb)) and torch.equal(bits(a), bits(b))


def test_ce_temperature_refusals():
    logits, labels = _ce_case(264)
    inv = torch.ones(1, device=DEV)
    o = _ext.ops()
    raises(lambda: o.ce_fwd(logits.clone(), labels, inv, False, 0.0, 0, 0.0),
           lambda: o.ce_fwd(logits.clone(), labels, inv, False, 0.0, 0, -1.0),
           lambda: o.ce_fwd(logits.clone(), labels, inv, False, 0.1, 0, 0.7),
           lambda: o.ce_fwd(logits.clone(), labels, inv, False, 0.0, 1, 0.7),
           lambda: ops.lm_head._ce_rows(logits.clone(), labels, inv, False, temperature=0.0),
           lambda: ops.lm_head._ce_rows(logits.clone(), labels, inv, False, label_smoothing=0.1, temperature=0.7))


# ------------------------------------------------------------------------------------------------ grpo_token_fwd
TOK_LENS = [1, 63, 64, 65, 200, 5]          # sequence 5 has no completion row
TOK_PAD = 7
TOK_ADV = [0.7, -1.3, 0.0, 0.4, -0.9, 0.5]  # both signs, one exact 0
EPS_LOW, EPS_HIGH, BETA = 0.2, 0.28, 0.04
RATIOS = [0.6, 0.95, 1.05, 1.5]             # below, inside (twice) and above [0.8, 1.28], off its boundaries


def _tok_case():
    g = torch.Generator(device=DEV).manual_seed(17)
    M = sum(TOK_LENS) + TOK_PAD
    cu = cu_of(TOK_LENS, TOK_PAD)
    c = cu.tolist()
    nll = (2.0 * torch.randn(M, generator=g, device=DEV)).abs() + 0.01
    labels = torch.randint(0, 1000, (M,), generator=g, device=DEV)
    labels[torch.rand(M, generator=g, device=DEV) < 0.3] = -100
    labels[c[0]] = 5                          # the length-1 sequence: a completion row
    labels[c[5]:] = -100                      # sequence 5 and the pad segment
    r = torch.tensor(RATIOS, device=DEV)[torch.randint(0, 4, (M,), generator=g, device=DEV)]
    old = (-nll.double() - r.double().log()).float()
    # the reference policy: |d| = |ref - lp| in [0.05, 0.6], either sign (exp(d) - d - 1 ~ d^2 / 2 cancels as d -> 0:
    # at |d| >= 0.05 the fp32 expression expm1(d) - d keeps 1.2e-7 / 0.05 = 2.4e-6)
    d = (0.05 + 0.55 * torch.rand(M, generator=g, device=DEV)) * (2 * torch.randint(0, 2, (M,), generator=g, device=DEV) - 1)
    rlp = (-nll + d).float()
    adv = torch.tensor(TOK_ADV, dtype=torch.float32, device=DEV)
    return nll, old, rlp, labels, adv, cu


def _tok_fp64(nll, old, rlp, labels, adv, cu, S, inv, per_seq_mean):
    """rows [2, M] and the per-sequence sums by fp64 autograd of the issue's formula."""
    M = nll.numel()
    c = cu.tolist()
    lp = (-nll.double()).requires_grad_(True)
    comp = torch.zeros(M, dtype=torch.bool, device=DEV)
    A = torch.zeros(M, dtype=torch.float64, device=DEV)
    w = torch.zeros(M, dtype=torch.float64, device=DEV)
    for s in range(S):
        a, b = c[s], c[s + 1]
        comp[a:b] = labels[a:b] >= 0
        A[a:b] = adv[s].double()
        n = max(int(comp[a:b].sum()), 1)
        w[a:b] = inv.double() / n if per_seq_mean else inv.double()
    r = torch.exp(lp - old.double().nan_to_num()) if old is not None else torch.exp(lp - lp.detach())
    l = -torch.min(r * A, r.clamp(1 - EPS_LOW, 1 + EPS_HIGH) * A)
    kl = torch.zeros_like(lp)
    if rlp is not None:
        d = rlp.double().nan_to_num() - lp
        kl = torch.exp(d) - d - 1
        l = l + BETA * kl
    rows0 = torch.where(comp, w * l, torch.zeros_like(l))
    (g,) = torch.autograd.grad(rows0.sum(), lp)
    rows1 = torch.where(comp, g, torch.zeros_like(g))
    rd = r.detach()
    low = comp & (rd < 1 - EPS_LOW) & (A < 0)
    high = comp & (rd > 1 + EPS_HIGH) & (A > 0)
    cols = (rows0.detach(), comp.double(), low.double(), high.double(), torch.where(comp, kl.detach(), kl.detach() * 0),
            torch.where(comp, rd, rd * 0))
    seq = torch.stack([torch.stack([v[c[s]:c[s + 1]].sum() for s in range(S)]) for v in cols])
    return torch.stack([rows0.detach(), rows1]), seq


@pytest.mark.parametrize("per_seq_mean", [False, True])
@pytest.mark.parametrize("has_ref", [False, True])
@pytest.mark.parametrize("has_old", [False, True])
def test_grpo_token_fwd_against_fp64(has_old, has_ref, per_seq_mean):
    nll, old, rlp, labels, adv, cu = _tok_case()
    S, M = len(TOK_LENS), nll.numel()
    old = old if has_old else None
    rlp = rlp if has_ref else None
    inv = torch.tensor([1.0 / 37.0], dtype=torch.float32, device=DEV)
    rows, seq = _ext.ops().grpo_token_fwd(nll, old, rlp, labels, adv, cu, S, inv, EPS_LOW, EPS_HIGH, BETA, per_seq_mean)
    assert rows.shape == (2, M) and seq.shape == (6, S) and rows.dtype == seq.dtype == torch.float32
    assert torch.isfinite(rows).all() and torch.isfinite(seq).all()
    want_rows, want_seq = _tok_fp64(nll, old, rlp, labels, adv, cu, S, inv, per_seq_mean)
    twin_rows, twin_seq = ref.grpo_token(nll, old, rlp, labels, adv, cu, S, inv, EPS_LOW, EPS_HIGH, BETA, per_seq_mean)
    for i, name in enumerate(("loss", "coef")):
        bound = 2 * rel_err(twin_rows[i], want_rows[i]).max().item()
        worst = rel_err(rows[i], want_rows[i]).max().item()
        report(f"grpo_token_fwd old={has_old} ref={has_ref} mean={per_seq_mean} rows {name}", worst, bound)
        assert (0 < bound < 1e-3 or (bound == 0 and not has_old and not has_ref)) and worst <= bound
    # the counts are exact; the sums within the twin's bound
    for i in (1, 2, 3):
        assert torch.equal(seq[i].double(), want_seq[i]), (i, seq[i].tolist(), want_seq[i].tolist())
    assert seq[1].tolist()[5] == 0.0 and seq[1].tolist()[0] == 1.0
    if has_old:
        assert seq[2].sum() > 0 and seq[3].sum() > 0
    else:
        assert seq[2].sum() == 0 and seq[3].sum() == 0
    # the sums: at most 200 fp32 terms of one sign per sequence (kl >= 0, r > 0, the loss has its advantage's sign up
    # to a KL term 25 times smaller), each within 1e-6 of fp64 (the rows' bound above), summed in fp32: n eps = 200 x
    # 6e-8 = 1.2e-5 at the very worst, 2e-5 with the terms' own error
    c = cu.tolist()
    for i, name in ((0, "loss"), (4, "kl"), (5, "ratio")):
        worst = rel_err(seq[i], want_seq[i]).max().item()
        report(f"grpo_token_fwd old={has_old} ref={has_ref} mean={per_seq_mean} seq {name}", worst, 2e-5)
        assert worst <= 2e-5
        assert rel_err(twin_seq[i], want_seq[i]).max().item() <= 2e-5  # the twin keeps the same promise
    # rows off the completions: +0 in both outputs
    off = torch.ones(M, dtype=torch.bool, device=DEV)
    off[:c[S]] = labels[:c[S]] < 0
    assert not bits(rows[:, off]).any()
    assert torch.equal(bits(rows), bits(_ext.ops().grpo_token_fwd(nll, old, rlp, labels, adv, cu, S, inv, EPS_LOW,
                                                                  EPS_HIGH, BETA, per_seq_mean)[0]))  # run to run
    if not has_old:
        # r is exactly 1: with beta = 0 the coefficient is (-A_s) w, bit for bit
        r0, s0 = _ext.ops().grpo_token_fwd(nll, None, rlp, labels, adv, cu, S, inv, EPS_LOW, EPS_HIGH, 0.0, per_seq_mean)
        wseq = inv / s0[1].clamp(min=1.0) if per_seq_mean else inv.expand(S)
        for s in range(S):
            comp = labels[c[s]:c[s + 1]] >= 0
            got = r0[1, c[s]:c[s + 1]][comp]
            assert torch.equal(bits(got), bits(((0.0 - adv[s]) * wseq[s]).expand_as(got))), s


@pytest.mark.parametrize("per_seq_mean", [False, True])
def test_grpo_token_fwd_isolation(per_seq_mean):
    """NaN in nll / old / ref on every row that is not a completion row, and past cu[n_seqs]: nothing moves."""
    nll, old, rlp, labels, adv, cu = _tok_case()
    S = len(TOK_LENS)
    inv = torch.tensor([1.0 / 37.0], dtype=torch.float32, device=DEV)
    run = lambda a, b, c_: _ext.ops().grpo_token_fwd(a, b, c_, labels, adv, cu, S, inv, EPS_LOW, EPS_HIGH, BETA,  # noqa: E731
                                                     per_seq_mean)
    base = run(nll, old, rlp)
    off = labels < 0
    off[cu.tolist()[S]:] = True
    nan = torch.full_like(nll, math.nan)
    got = run(torch.where(off, nan, nll), torch.where(off, nan, old), torch.where(off, nan, rlp))
    assert torch.equal(bits(got[0]), bits(base[0])) and torch.equal(bits(got[1]), bits(base[1]))
    # fewer sequences: the later ones are ignored, their rows +0
    r3, s3 = _ext.ops().grpo_token_fwd(nll, old, rlp, labels, adv[:3], cu, 3, inv, EPS_LOW, EPS_HIGH, BETA, per_seq_mean)
    c = cu.tolist()
    assert torch.equal(bits(r3[:, :c[3]]), bits(base[0][:, :c[3]])) and not bits(r3[:, c[3]:]).any()
    assert torch.equal(bits(s3), bits(base[1][:, :3]))


def test_grpo_token_fwd_refusals():
    nll, old, rlp, labels, adv, cu = _tok_case()
    S = len(TOK_LENS)
    inv = torch.ones(1, device=DEV)
    f = _ext.ops().grpo_token_fwd
    raises(lambda: f(nll.double(), old, rlp, labels, adv, cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll.cpu(), old, rlp, labels, adv, cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old[:-1], rlp, labels, adv, cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp.double(), labels, adv, cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels.int(), adv, cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels[:-1], adv, cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv[:-1], cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv.double(), cu, S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv, cu.long(), S, inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv, cu, cu.numel(), inv, 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv, cu, S, inv.cpu(), 0.2, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv, cu, S, inv, 1.0, 0.2, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv, cu, S, inv, 0.2, -0.1, 0.0, False),
           lambda: f(nll, old, rlp, labels, adv, cu, S, inv, 0.2, 0.2, -1.0, False))


# ------------------------------------------------------------------------------------------------ scale_rows
def _check_scale_rows(M, H, gs):
    g = torch.Generator(device=DEV).manual_seed(H + M)
    x = torch.randn(M, H, generator=g, device=DEV).to(BF16)
    x0 = x.clone()
    coef = torch.randn(M, generator=g, device=DEV)
    coef[0], coef[M - 1] = 0.0, 1.0
    gscale = torch.tensor([gs], dtype=torch.float32, device=DEV)
    twin = ref.scale_rows(x, coef, gscale)
    out = _ext.ops().scale_rows(x, coef, gscale)
    assert out.dtype == BF16 and out.shape == x.shape
    assert torch.equal(bits(x), bits(x0))                      # out of place: the input is untouched
    assert torch.equal(bits(out), bits(twin)), (H, gs, (out.float() - twin.float()).abs().max().item())
    y = x.clone()
    _ext.ops().scale_rows_(y, coef, gscale)
    assert torch.equal(bits(y), bits(twin))                    # in place
    assert not (out[0].float() != 0).any()                     # coef 0: zeros (of either sign)
    same = _ext.ops().scale_rows(x, torch.ones(M, device=DEV), torch.ones(1, device=DEV))
    assert torch.equal(bits(same), bits(x))                    # coef 1, gscale 1: the input, bit for bit
    assert torch.equal(bits(ops.scale_rows(x, coef, gscale)), bits(twin))


@pytest.mark.parametrize("gs", [1.0, -1.0 / 0.7])
@pytest.mark.parametrize("H", [8, 520, 2048, 2056])
def test_scale_rows_bit_for_bit(H, gs):
    _check_scale_rows(263, H, gs)


def test_scale_rows_second_grid_pass():
    """65,539 rows: more than the 65,535 row blocks of one pass of the capped grid."""
    _check_scale_rows(65536 + 3, 8, 1.0 / 7.0)


def test_scale_rows_refusals():
    x = torch.randn(8, 16, device=DEV).to(BF16)
    coef = torch.ones(8, device=DEV)
    one = torch.ones(1, device=DEV)
    o = _ext.ops()
    raises(lambda: o.scale_rows(x.float(), coef, one), lambda: o.scale_rows(x, coef[:7], one),
           lambda: o.scale_rows(x, coef.double(), one), lambda: o.scale_rows(x[:, :12], coef, one),
           lambda: o.scale_rows(x, coef, one.cpu()), lambda: o.scale_rows(x, coef.cpu(), one),
           lambda: o.scale_rows_(x[:, :12], coef, one), lambda: o.scale_rows(x.cpu(), coef, one))


# ------------------------------------------------------------------------------------------------ sample_tokens_full
SAMP_V, SAMP_B, SAMP_TAU = 2056, 8192, 0.8
SAMP_TOK = [0, 7, 2047, 2048, 2055]
SAMP_P = [0.4, 0.25, 0.2, 0.1, 0.05]


def _samp_logits(dtype, B=SAMP_B, V=SAMP_V):
    row = torch.full((V,), -30.0, dtype=torch.float64)
    for t, p in zip(SAMP_TOK, SAMP_P):
        row[t] = SAMP_TAU * math.log(p)
    return row.to(dtype).to(DEV).expand(B, V).contiguous()


def _samp_state(B, V, cap=2, present=()):
    words = (V + 31) // 32
    pres = torch.zeros(B, words, dtype=torch.int32, device=DEV)
    for t in present:
        pres[:, t >> 5] |= 1 << (t & 31)
    return dict(presence=pres, state=torch.zeros(B, 4, dtype=torch.long, device=DEV),
                tok=torch.full((B,), -1, dtype=torch.long, device=DEV), pos=torch.zeros(B, dtype=torch.long, device=DEV),
                len=torch.ones(B, dtype=torch.int32, device=DEV),
                log=torch.full((B, cap), -1, dtype=torch.long, device=DEV),
                logp=torch.zeros(B, cap, dtype=torch.float32, device=DEV),
                done=torch.zeros(B, dtype=torch.int32, device=DEV))


def _draw(logits, s, seed, tau=SAMP_TAU, penalty=1.0, eos=-1):
    _ext.ops().sample_tokens_full(logits, s["presence"], s["state"], s["tok"], s["pos"], s["len"], s["log"], s["logp"],
                                  s["done"], eos, tau, penalty, seed)
    torch.cuda.synchronize()
    return s["tok"].clone()


def _penalised(logits, present, penalty, tau):
    z = logits[0].double().clone()
    for t in present:
        z[t] = z[t] * penalty if z[t] < 0 else z[t] / penalty
    return z / tau


def _check_counts(tok, z, what):
    p = torch.softmax(z, -1)
    n = tok.numel()
    counts = torch.bincount(tok, minlength=z.numel()).double()
    other = torch.ones_like(p, dtype=torch.bool)
    for t in SAMP_TOK:
        other[t] = False
        dev = abs(counts[t].item() - n * p[t].item())
        lim = 5 * math.sqrt(n * p[t].item() * (1 - p[t].item()))
        print(f"\n[grpo] sample_tokens_full {what} token {t}: count {int(counts[t])} expected {n * p[t].item():.1f} "
              f"(|dev| {dev:.1f} <= {lim:.1f})")
        assert dev <= lim, (t, counts[t].item(), n * p[t].item())
    assert n * p[other].sum().item() < 1e-5 and counts[other].sum().item() == 0


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_sample_tokens_full_distribution(dtype):
    logits = _samp_logits(dtype)
    s = _samp_state(SAMP_B, SAMP_V)
    tok = _draw(logits, s, 1234)
    z = _penalised(logits, (), 1.0, SAMP_TAU)
    _check_counts(tok, z, str(dtype))
    # the log-probability of the drawn token, the token log, the counters and the presence bits
    want = torch.log_softmax(z, -1)[tok]
    err = (s["logp"][:, 0].double() - want).abs()
    report(f"sample_tokens_full {dtype} logp", err.max().item(), 2e-3)
    assert bool((err <= 2e-3 + 1e-3 * want.abs()).all())
    assert torch.equal(s["log"][:, 0], tok) and bool((s["log"][:, 1] == -1).all())
    assert bool((s["state"][:, 0] == 1).all()) and torch.equal(s["state"][:, 1], tok)
    assert bool((s["pos"] == 1).all()) and bool((s["len"] == 2).all()) and not bool(s["done"].any())
    rows = torch.arange(SAMP_B, device=DEV)
    word = s["presence"][rows, tok >> 5]
    assert bool((((word >> (tok & 31)) & 1) == 1).all()) and int((s["presence"] != 0).sum()) == SAMP_B
    # a second identical call draws the same tokens; row 0 at seed + 1 is row 1 at seed
    assert torch.equal(_draw(logits, _samp_state(SAMP_B, SAMP_V), 1234), tok)
    assert torch.equal(_draw(logits, _samp_state(SAMP_B, SAMP_V), 1235)[:-1], tok[1:])
    # the step counter keys the draw: a second step on the same state draws afresh
    tok2 = _draw(logits, s, 1234)
    assert not torch.equal(tok2, tok) and torch.equal(s["log"][:, 1], tok2) and bool((s["state"][:, 0] == 2).all())


def test_sample_tokens_full_repetition_penalty():
    """Tokens 0 and 2048 marked present: their (negative) logits are multiplied by the penalty before the draw."""
    logits = _samp_logits(torch.float32)
    s = _samp_state(SAMP_B, SAMP_V, present=(0, 2048))
    tok = _draw(logits, s, 99, penalty=1.5)
    z = _penalised(logits, (0, 2048), 1.5, SAMP_TAU)
    _check_counts(tok, z, "penalty 1.5")
    want = torch.log_softmax(z, -1)[tok]
    assert bool(((s["logp"][:, 0].double() - want).abs() <= 2e-3 + 1e-3 * want.abs()).all())
    plain = torch.softmax(_penalised(logits, (), 1.0, SAMP_TAU), -1)
    assert (tok == 0).float().mean().item() < plain[0].item() - 0.05  # visibly rarer than without the penalty


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_sample_tokens_full_done_and_eos_as_sample_tokens(dtype):
    """Rows whose distribution is one token (+40 over -40) against the greedy sample_tokens on the same rows, odd V:
    every output equal, over two calls — EOS logged and flagged, its position not advanced, a finished row skipped."""
    V, eos = 2049, 7
    hot = [7, 5, 2048, 7, 2047]
    B = len(hot)
    logits = torch.full((B, V), -40.0, device=DEV)
    for b, t in enumerate(hot):
        logits[b, t] = 40.0
    logits = logits.to(dtype)
    a, g = _samp_state(B, V), _samp_state(B, V)
    for s in (a, g):
        s["state"][:, 2] = torch.tensor([3, 4, 5, 6, 7], device=DEV)
        s["pos"].fill_(-1)
    for _ in range(2):
        _draw(logits, a, 5, tau=1.0, eos=eos)
        _ext.ops().sample_tokens(logits, g["presence"], g["state"], g["tok"], g["pos"], g["len"], g["log"], g["done"],
                                 eos, 1.0, 1, 1.0, 1.0, False, 5)
    torch.cuda.synchronize()
    for k in ("presence", "state", "tok", "pos", "len", "log", "done"):
        assert torch.equal(a[k], g[k]), (k, a[k].tolist(), g[k].tolist())
    assert a["done"].tolist() == [1, 0, 0, 1, 0] and a["state"][:, 0].tolist() == [1, 2, 2, 1, 2]
    assert a["pos"].tolist() == [-1, 6, 7, -1, 9] and a["log"][0].tolist() == [7, -1]
    assert bool((a["logp"][a["log"] >= 0].abs() < 1e-6).all())


def test_sample_tokens_full_large_vocabulary():
    V, B = 128256, 4
    g = torch.Generator(device=DEV).manual_seed(3)
    logits = (2 * torch.randn(B, V, generator=g, device=DEV)).to(BF16)
    s = _samp_state(B, V)
    tok = _draw(logits, s, 77, tau=0.7)
    assert bool(((tok >= 0) & (tok < V)).all())
    want = torch.log_softmax(logits.double() / 0.7, -1)[torch.arange(B, device=DEV), tok]
    err = (s["logp"][:, 0].double() - want).abs()
    report("sample_tokens_full V=128256 logp", err.max().item(), 2e-3)
    assert bool((err <= 2e-3 + 1e-3 * want.abs()).all())
    assert torch.equal(_draw(logits, _samp_state(B, V), 77, tau=0.7), tok)


def test_sample_tokens_full_refusals():
    V, B = 264, 2
    logits = torch.randn(B, V, device=DEV)
    s = _samp_state(B, V)
    f = _ext.ops().sample_tokens_full
    call = lambda **kw: f(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("logits", logits), ("presence", s["presence"]), ("state", s["state"]), ("tok", s["tok"]), ("pos", s["pos"]),
        ("len", s["len"]), ("log", s["log"]), ("logp", s["logp"]), ("done", s["done"]), ("eos", -1), ("tau", 1.0),
        ("penalty", 1.0), ("seed", 1))])
    call()
    raises(lambda: call(logits=logits.double()), lambda: call(logits=logits[0]), lambda: call(logits=logits.cpu()),
           lambda: call(presence=s["presence"][:, :-1].contiguous()), lambda: call(state=s["state"][:, :3].contiguous()),
           lambda: call(tok=s["tok"][:1]), lambda: call(logp=s["logp"].double()), lambda: call(logp=s["logp"][:1]),
           lambda: call(done=s["done"][:1]), lambda: call(tau=0.0), lambda: call(penalty=0.0),
           lambda: call(log=s["log"].int()))


# ------------------------------------------------------------------------------------------------ lm_head_policy_loss
LENS = [70, 33, 128, 65]
ROWS = 320
HEAD_TAU = 0.8
HEAD_ADV = [0.7, -1.3, 0.0, 0.4]


def _head_case():
    H, V = 256, 8200
    g = torch.Generator(device=DEV).manual_seed(5)
    h = torch.randn(ROWS, H, generator=g, device=DEV).to(BF16)
    w = (0.06 * torch.randn(V, H, generator=g, device=DEV)).to(BF16)
    cu = cu_of(LENS, ROWS - sum(LENS))
    labels = torch.randint(0, V, (ROWS,), generator=g, device=DEV)
    c = cu.tolist()
    for s, k in enumerate([9, 3, 17, 4]):
        labels[c[s]:c[s] + k] = -100          # the prompt
        labels[c[s + 1] - 1] = -100           # the last token of a sequence predicts nothing
    labels[c[4]:] = -100                      # pad rows
    adv = torch.tensor(HEAD_ADV, dtype=torch.float32, device=DEV)
    inv = torch.tensor([1.0 / float((labels >= 0).sum())], dtype=torch.float32, device=DEV)
    # the old and the reference policy: this head's own log-probabilities, moved by known ratios / a little noise
    lp = -ref.cross_entropy((h.float() @ w.float().t()).to(BF16), labels, temperature=HEAD_TAU)[0]
    r = torch.tensor(RATIOS, device=DEV)[torch.randint(0, 4, (ROWS,), generator=g, device=DEV)]
    old = (lp.double() - r.double().log()).float()
    rlp = lp + 0.2 * torch.randn(ROWS, generator=g, device=DEV)
    return h, w, cu, labels, adv, inv, old, rlp


def _head_fp64(h, w, cu, labels, adv, inv, old, rlp):
    """(loss, dh, dW) by fp64 autograd of the objective on the fp64 logits."""
    hh, ww = h.double().requires_grad_(True), w.double().requires_grad_(True)
    z = (hh @ ww.t()) / HEAD_TAU
    safe = labels.clamp(min=0)
    lp = torch.log_softmax(z, -1)[torch.arange(ROWS, device=DEV), safe]
    comp = labels >= 0
    c = cu.tolist()
    A = torch.zeros(ROWS, dtype=torch.float64, device=DEV)
    for s in range(len(LENS)):
        A[c[s]:c[s + 1]] = adv[s].double()
    r = torch.exp(lp - old.double())
    l = -torch.min(r * A, r.clamp(1 - EPS_LOW, 1 + EPS_HIGH) * A)
    d = rlp.double() - lp
    l = l + BETA * (torch.exp(d) - d - 1)
    loss = (torch.where(comp, l, torch.zeros_like(l)) * inv.double()).sum()
    dh, dw = torch.autograd.grad(loss, (hh, ww))
    return loss.detach(), dh, dw


def _head_emul(h, w, cu, labels, adv, inv, old, rlp):
    """The same in fp32 with the HIP path's rounding points: bf16 logits, bf16 G = softmax - onehot, bf16 G W before
    the row weight, the row weight on bf16 h, one bf16 rounding of each result."""
    rnd = lambda t: t.to(BF16).float()  # noqa: E731
    logits = (h.float() @ w.float().t()).to(BF16)
    nll = ref.cross_entropy(logits, labels, temperature=HEAD_TAU)[0]
    rows, _ = ref.grpo_token(nll, old, rlp, labels, adv, cu, len(LENS), inv, EPS_LOW, EPS_HIGH, BETA, False)
    G = rnd(ref.cross_entropy_grad(logits, labels, torch.ones(1, device=DEV), temperature=HEAD_TAU))
    coef = rows[1] * torch.tensor(-1.0 / HEAD_TAU, dtype=torch.float32).item()
    dh = rnd(rnd(G @ w.float()) * coef[:, None])
    dw = rnd(G.t() @ rnd(h.float() * coef[:, None]))
    return rows[0].sum(), dh, dw


def test_lm_head_policy_loss_against_fp64():
    case = _head_case()
    h, w, cu, labels, adv, inv, old, rlp = case
    want = _head_fp64(*case)
    emul = _head_emul(*case)
    hh, ww = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    loss, stats, rows, seq = ops.lm_head_policy_loss(hh, ww, labels, adv, cu, len(LENS), inv, old, rlp, EPS_LOW,
                                                     EPS_HIGH, BETA, HEAD_TAU, False)
    assert stats.shape == (4, ROWS) and rows.shape == (2, ROWS) and seq.shape == (6, len(LENS))
    loss.backward()
    assert torch.equal(bits(hh.detach()), bits(h))  # the saved activation is not scaled in place
    bl = 2 * rel_err(emul[0], want[0]).item()
    el = rel_err(loss.detach(), want[0]).item()
    report("lm_head_policy_loss loss", el, bl)
    assert bl > 0 and el <= bl
    assert seq[2].sum() > 0 and seq[3].sum() > 0   # both clip sides are exercised
    c = cu.tolist()
    bh = 2 * torch.cat([block_rel_err(emul[1][a:b], want[1][a:b], b - a, 64, want[1].pow(2).mean().sqrt())
                        for a, b in zip(c[:-1], c[1:])]).max().item()
    eh = assert_blocks_close(hh.grad, want[1], 0, 64, bh, "dh", row_splits=c)
    report("lm_head_policy_loss dh (per sequence x 64 columns)", eh, bh)
    bw = 2 * block_rel_err(emul[2], want[2], 32, 32).max().item()
    ew = assert_blocks_close(ww.grad, want[2], 32, 32, bw, "dW")
    report("lm_head_policy_loss dW (32 x 32 blocks)", ew, bw)
    assert not (hh.grad[c[4]:] != 0).any()          # pad rows: zeros (of either sign: +0 x the negative gscale)
    with torch.no_grad():                           # no gradient wanted: the same loss, nothing saved
        l2 = ops.lm_head_policy_loss(h, w, labels, adv, cu, len(LENS), inv, old, rlp, EPS_LOW, EPS_HIGH, BETA,
                                     HEAD_TAU, False)[0]
    assert torch.equal(bits(l2), bits(loss.detach()))
    lp = ops.lm_head_token_logps(h, w, labels, HEAD_TAU)
    assert lp.dtype == torch.float32 and torch.equal(bits(lp), bits(0.0 - stats[0]))


# ------------------------------------------------------------------------------------------------ model, HIP vs reference
def _model_batch(vocab):
    g = torch.Generator(device=DEV).manual_seed(3)
    ids = torch.randint(0, vocab, (ROWS,), generator=g, device=DEV)
    cu = cu_of(LENS, ROWS - sum(LENS))
    c = cu.tolist()
    labels = ids.clone()
    for s, k in enumerate([9, 5, 17, 4]):
        labels[c[s]:c[s] + k] = -100
    labels[c[4]:] = -100
    pos = torch.cat([torch.arange(b - a, device=DEV) for a, b in zip(c[:-1], c[1:])])
    return dict(input_ids=ids, labels=labels, cu_seqlens=cu, position_ids=pos, max_seqlen=max(LENS))


def _policy_run(model, batch, extra, hip):
    os.environ["SFTAMD_DISABLE_HIP"] = "0" if hip else "1"  # (conftest restores the environment after the test)
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    out = model.policy_loss(**batch, n_seqs=len(LENS), **extra)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach().double(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()
                                        if p.grad is not None}


@pytest.mark.parametrize("preset,lora", [("tiny-gpu", False), ("tiny-gpu-qwen3", False), ("tiny-gpu-mistral", False),
                                         ("tiny-gpu", True)])
def test_policy_loss_hip_vs_reference(preset, lora):
    torch.manual_seed(0)
    cfg = get_config(preset)
    m = build_model(cfg, device=DEV, dtype=BF16, seed=1)
    if lora:
        from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora
        apply_lora(m, LoRAConfig(r=16, lora_alpha=32.0, lora_dropout=0.0))
        with torch.no_grad():  # B = 0 would make every A gradient zero
            for layer in m.model.layers:
                for fl in (*layer.self_attn.lora.values(), *layer.mlp.lora.values()):
                    for b in fl.B:
                        torch.nn.init.normal_(b, std=0.02)
    m.train()
    batch = _model_batch(cfg.vocab_size)
    # injected rollouts: the old policy's log-probabilities are the reference path's own, moved by known ratios
    os.environ["SFTAMD_DISABLE_HIP"] = "1"
    with torch.no_grad():
        lp = m.token_logps(**batch, temperature=HEAD_TAU)
    g = torch.Generator(device=DEV).manual_seed(9)
    r = torch.tensor(RATIOS, device=DEV)[torch.randint(0, 4, (ROWS,), generator=g, device=DEV)]
    extra = dict(advantages=torch.tensor([0.83, -1.21, 0.37, -0.55], device=DEV), old_logps=lp - r.log(),
                 ref_logps=lp + 0.2 * torch.randn(ROWS, generator=g, device=DEV), eps_low=EPS_LOW, eps_high=EPS_HIGH,
                 beta=BETA, temperature=HEAD_TAU)
    l_hip, g_hip = _policy_run(m, batch, extra, True)
    l_ref, g_ref = _policy_run(m, batch, extra, False)
    el = ((l_hip - l_ref).abs() / l_ref.abs()).item()
    report(f"policy_loss {preset}{' lora' if lora else ''} loss", el, 2e-2)
    assert el < 2e-2
    assert g_ref and set(g_ref) == set(g_hip)
    if lora:
        assert all(".lora." in n for n in g_ref)
    worst, name = 0.0, ""
    for n in g_ref:
        e = ((g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)).item()
        if e > worst:
            worst, name = e, n
    report(f"policy_loss {preset}{' lora' if lora else ''} gradients (worst: {name})", worst, 5e-2)
    assert worst < 5e-2, (name, worst)


def test_policy_loss_and_token_logps_refuse_context_parallel():
    m = build_model(get_config("tiny-gpu"), device=DEV, dtype=BF16, seed=1)
    m.model.layers[0].self_attn.cp_group = object()
    b = _model_batch(1024)
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.policy_loss(**b, advantages=torch.zeros(4, device=DEV), n_seqs=4)
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.token_logps(**b)


# ------------------------------------------------------------------------------------------------ rollout_batch
def test_rollout_batch_graph_and_logps():
    """4 prompts of different lengths, 16 new tokens on tiny-gpu. Graph and no-graph draw the same tokens. The sampler's
    log-probabilities against token_logps of the same sequences on the training path: the two paths run different
    kernels, so the allowance is twice the larger of their distances to the fp32 torch reference model on these
    inputs (all three figures are printed; profiles/grpo.md records one run)."""
    cfg = get_config("tiny-gpu")
    m = build_model(cfg, device=DEV, dtype=BF16, seed=2)
    m.train()
    g = torch.Generator().manual_seed(4)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (3, 9, 17, 6)]
    tau, N = 0.9, 16
    toks, lps = rollout_batch(m, prompts, N, None, temperature=tau, seed=21)
    assert m.training                                   # the flag is restored
    assert [len(t) for t in toks] == [N] * 4 and [len(x) for x in lps] == [N] * 4
    t2, l2 = rollout_batch(m, prompts, N, None, temperature=tau, seed=21, use_graph=False)
    assert t2 == toks and l2 == lps
    tk, lk = rollout_batch(m, prompts, N, None, temperature=tau, top_k=8, seed=21)
    assert lk is None and [len(t) for t in tk] == [N] * 4
    # the same sequences through the training path, and through an fp32 copy of the model on the reference path
    seqs = [p + t for p, t in zip(prompts, toks)]
    ids = torch.tensor([x for s in seqs for x in s], device=DEV)
    cu = cu_of([len(s) for s in seqs])
    labels = torch.tensor([x for p, t in zip(prompts, toks) for x in [-100] * (len(p) - 1) + t + [-100]], device=DEV)
    pos = torch.cat([torch.arange(len(s), device=DEV) for s in seqs])
    kw = dict(cu_seqlens=cu, position_ids=pos, max_seqlen=max(len(s) for s in seqs), shift_labels=False, temperature=tau)
    comp = labels >= 0
    samp = torch.tensor([x for p, lp in zip(prompts, lps) for x in [0.0] * (len(p) - 1) + lp + [0.0]], device=DEV).double()
    m.eval()
    with torch.no_grad():
        train = m.token_logps(ids, labels, **kw).double()
        m32 = build_model(cfg, device=DEV, dtype=torch.float32, seed=2)
        m32.load_hf_state_dict({k: v.float() for k, v in m.hf_state_dict().items()})
        m32.eval()
        os.environ["SFTAMD_DISABLE_HIP"] = "1"          # (conftest restores the environment after the test)
        want = m32.token_logps(ids, labels, **kw).double()
        os.environ["SFTAMD_DISABLE_HIP"] = "0"
    d_s = (samp - want).abs()[comp].max().item()
    d_t = (train - want).abs()[comp].max().item()
    gap = (samp - train).abs()[comp].max().item()
    print(f"\n[grpo] rollout_batch log-probabilities: sampler vs fp32 reference {d_s:.3e}, training path vs fp32 "
          f"reference {d_t:.3e}, sampler vs training path {gap:.3e} (allowed {2 * max(d_s, d_t):.3e})")
    assert max(d_s, d_t) > 0 and gap <= 2 * max(d_s, d_t)


# ------------------------------------------------------------------------------------------------ trainer
LOG_NAMES = ("loss", "reward", "reward_std", "rewards/low_share/mean", "frac_reward_zero_std", "completions/mean_length",
             "completions/clipped_ratio", "clip_ratio/low_mean", "clip_ratio/high_mean", "clip_ratio/region_mean",
             "entropy", "sampling/logp_difference")


@pytest.fixture(scope="module", params=[dict(), dict(num_iterations=2, beta=0.04)], ids=["mu1", "mu2_beta"])
def grpo_run(request, tmp_path_factory):
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer
    out = str(tmp_path_factory.mktemp("grpo"))
    cfg = get_config("tiny-gpu")
    m = build_model(cfg, device=DEV, dtype=BF16, seed=0)
    V = cfg.vocab_size

    def low_share(prompts, completions, completion_ids, **kw):  # a function of the token ids: no tokenizer needed
        return [sum(t < V // 2 for t in c) / max(len(c), 1) for c in completion_ids]

    g = torch.Generator().manual_seed(0)
    ds = [{"prompt_ids": torch.randint(3, V, (int(n),), generator=g).tolist()} for n in (4, 9, 6, 12)]
    a = GRPOConfig(output_dir=out, per_device_train_batch_size=8, num_generations=4, max_completion_length=16,
                   temperature=0.9, max_steps=3, learning_rate=1e-4, lr_scheduler_type="constant", logging_steps=1, jsonl_log=False,
                   save_strategy="steps", save_steps=3, **request.param)
    t = GRPOTrainer(model=m, reward_funcs=low_share, args=a, train_dataset=ds)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    _ext.ops().dispatch_trace(True)
    try:
        t.train()
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
    trace = {k: int(v) for k, v in (it.split("=") for it in _ext.ops().dispatch_trace_read().split(";") if it)}
    moved = any(not torch.equal(before[n], p.detach()) for n, p in m.named_parameters())
    return [h for h in t.state.log_history if "loss" in h], trace, out, request.param, moved, t


def test_grpo_trainer_dispatch_trace(grpo_run):
    trace = grpo_run[1]
    for k in ("ce.temp", "policy.grpo_token", "policy.scale_rows", "samp.full"):
        assert trace.get(k, 0) > 0, (k, sorted(trace))


def test_grpo_trainer_steps(grpo_run):
    logs, _, out, param, moved, t = grpo_run
    assert len(logs) == 3 and moved
    for h in logs:
        assert math.isfinite(h["loss"]) and math.isfinite(h["grad_norm"])
        assert 0.0 <= h["reward"] <= 1.0 and h["completions/mean_length"] > 0
        assert ("kl" in h) == (param.get("beta", 0.0) > 0)
    for name in LOG_NAMES:
        assert any(name in h for h in logs), name
    if param.get("num_iterations", 1) == 1:
        assert all("sampling/logp_difference" in h for h in logs)
        assert all(h[f"clip_ratio/{k}_mean"] == 0.0 for h in logs for k in ("low", "high", "region"))
        assert t.rollouts_generated == 3
    else:
        assert t.rollouts_generated == 2                # steps 1 and 3 generate, step 2 replays step 1's batch
        assert "sampling/logp_difference" not in logs[1]
        assert logs[0]["reward"] == logs[1]["reward"]
    for h in logs:
        if "sampling/logp_difference" in h:
            print(f"\n[grpo] trainer sampling/logp_difference {h['sampling/logp_difference']:.3e}")
            assert h["sampling/logp_difference"] < 0.1


def test_grpo_checkpoint_has_no_reference_copy(grpo_run):
    _, _, out, param, _, t = grpo_run
    assert (t._ref is not None) == (param.get("beta", 0.0) > 0)
    files = [f for f in glob.glob(os.path.join(out, "checkpoint-3", "**", "*"), recursive=True) if os.path.isfile(f)]
    assert files
    from safetensors import safe_open
    names = []
    for f in files:
        assert "ref" not in os.path.basename(f).lower(), f
        if f.endswith(".safetensors"):
            with safe_open(f, "pt") as sf:
                names += list(sf.keys())
    assert names and len(names) == len(set(names)) and not any("ref" in n.lower() for n in names)
    n_model = sum(p.numel() for p in t.model.parameters())
    total = sum(os.path.getsize(f) for f in files if f.endswith(".safetensors"))
    assert total < 2 * n_model * 2 + (1 << 20), (total, n_model)  # one bf16 copy of the weights, not two
