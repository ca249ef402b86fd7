"""Knowledge distillation on the GPU: kd_fwd (csrc/distill.hip) per row against fp64, the LM-head op built on it
(ops.lm_head_distill_loss), CausalLM.distill_loss on the HIP path against the PyTorch reference path, and GKDTrainer
steps with the dispatch trace.

Bounds follow tests/test_objectives_gpu.py: each is 2 x the worst error of an fp32 torch emulation with the kernel's
rounding points against the fp64 reference, computed here from the references alone and pooled over the grid (per
kernel instantiation: forward KL, reverse KL, mixture); every test prints its worst measured error next to the bound
(pytest -s); profiles/distill.md records one run. The model tests use the project's bounds of
tests/test_dpo_gpu.py::test_sequence_logps_hip_vs_reference.

Measured on an MI355X (profiles/distill.md): every case below passes its bound."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext, lm_head
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close, block_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SCALE = 1.0 / 7.0
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

SMALL_V = [8 * n for n in (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2049)]
BIG_V = [128256, 151936]
BETAS = [0.0, 0.5, 0.3, 1.0]
TAUS = [1.0, 0.9, 2.0]
# the two training vocabularies: every instantiation and every temperature once
BIG_GRID = [(0.0, 1.0), (0.5, 0.9), (0.3, 2.0), (1.0, 0.9)]
GRID = [(V, b, t) for V in SMALL_V for b in BETAS for t in TAUS] + [(V, b, t) for V in BIG_V for b, t in BIG_GRID]


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def report(what, worst, bound):
    print(f"\n[distill] {what}: worst {worst:.3e} bound {bound:.3e}")


def mode_of(beta):
    return "fkl" if beta == 0.0 else ("rkl" if beta == 1.0 else "mix")


def first_argmax(x):
    """argmax over the last dimension, ties resolved to the first index."""
    V = x.shape[-1]
    cols = torch.arange(V, device=x.device).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, cols, torch.full_like(cols, V)).min(-1).values


# ------------------------------------------------------------------------------------------------ kd_fwd rows
ROW_KINDS = ["random, teacher's argmax at column 0", "teacher == student", "label -100",
             "near-one-hot teacher at column V - 1 where the student is near its minimum",
             "near-one-hot student where the teacher is near its minimum", "gaps past 100"]
BIG_KINDS = [0, 5, 2]  # the three rows of the training vocabularies


def _kd_rows(V):
    """bf16 student / teacher logits [M, V] and labels, one row per kind of ROW_KINDS (BIG_KINDS for the two training
    vocabularies)."""
    g = torch.Generator(device=DEV).manual_seed(V)
    s = (3 * torch.randn(6, V, device=DEV, generator=g)).to(BF16)
    t = (3 * torch.randn(6, V, device=DEV, generator=g)).to(BF16)
    labels = torch.randint(0, V, (6,), device=DEV, generator=g)
    t[0, 0] = t[0].float().max() + 1.0                     # the teacher's argmax at column 0
    labels[0] = int(s[0].float().argmax())                 # a row the student gets right
    t[1] = s[1]
    labels[2] = -100
    t[3, V - 1] = t[3].float().max() + 30.0                # the teacher's argmax at column V - 1
    s[3, V - 1] = s[3].float().min()
    c = int(torch.randint(0, V, (1,), device=DEV, generator=g))
    s[4, c] = s[4].float().max() + 30.0
    t[4, c] = t[4].float().min()
    k = max(1, V // 16)
    s[5, :k] += 150.0                                      # the student far above the teacher in the first columns,
    t[5, V - k:] += 150.0                                  # the teacher far above the student in the last ones
    if V > 100000:
        keep = torch.tensor(BIG_KINDS, device=DEV)
        s, t, labels = s[keep], t[keep], labels[keep]
    return s.contiguous(), t.contiguous(), labels.contiguous()


def _kd_refs(s, t, labels, beta, tau):
    """fp64 (loss, grad, lse_s, lse_t) of the definition on the bf16 logits, and the fp32 emulation (loss, bf16 grad,
    lse_s, lse_t). The emulation rounds where the kernel does: logits times fp32(1 / tau), exp as exp2(fp32(x log2 e))
    and log as fp32(log2(s) ln 2) (the hardware transcendentals behind __expf / __logf), lse = m + log s, the two KL
    losses as numerator / sum + (lse - lse'), the mixture's log as max + log(1 + e^-|u - w|), the gradient element in
    the kernel's association, one rounding to bf16."""
    sc = torch.tensor([SCALE], dtype=torch.float64, device=s.device)
    loss, lse_s, lse_t, _, _ = ref.generalized_jsd(s.double(), t.double(), labels, beta, tau)
    grad = ref.generalized_jsd_grad(s.double(), t.double(), labels, sc, beta, tau)

    def f(v):
        return torch.tensor(v, dtype=torch.float32, device=s.device)

    def exp(x):
        return torch.exp2(x * f(LOG2E))

    def log(x):
        return torch.log2(x) * f(LN2)
    valid = (labels != -100).float()
    it = f(1.0 / tau)
    a, b = s.float() * it, t.float() * it
    ms, mt = a.max(-1, keepdim=True).values, b.max(-1, keepdim=True).values
    es, et = exp(a - ms), exp(b - mt)
    Ss, St = es.sum(-1), et.sum(-1)
    ls, lt = ms[:, 0] + log(Ss), mt[:, 0] + log(St)
    lp, lq = a - ls[:, None], b - lt[:, None]
    scale = f(SCALE) * it
    if beta == 0.0:
        loss32 = (et * (b - a)).sum(-1) / St + (ls - lt)
        grad32 = (exp(lp) - exp(lq)) * scale
    elif beta == 1.0:
        loss32 = (es * (a - b)).sum(-1) / Ss + (lt - ls)
        grad32 = (exp(lp) * ((lp - lq) - loss32[:, None])) * scale
    else:
        u, w = lp + f(math.log1p(-float(f(beta)))), lq + f(math.log(float(f(beta))))
        lm = torch.maximum(u, w) + log(f(1.0) + exp(-(u - w).abs()))
        kp, kq = (exp(lp) * (lp - lm)).sum(-1), (exp(lq) * (lq - lm)).sum(-1)
        loss32 = f(beta) * kq + (f(1.0) - f(beta)) * kp
        grad32 = (exp(lp) * ((lp - lm) - kp[:, None])) * (scale * (f(1.0) - f(beta)))
    return (loss, grad, lse_s, lse_t), (loss32 * valid, (grad32 * valid[:, None]).to(BF16), ls, lt)


def _ulps(err, *mags):
    """An absolute error in fp32 ulps of the largest of ``mags`` (at least 1): the loss is a sum of the two lse and a
    mean of logit differences, so one ulp of the largest of them (and of the loss itself, which bounds the mean) is the
    unit a rounding of any term moves it by."""
    top = torch.stack([m.abs() for m in mags]).max(0).values.clamp(min=1.0)
    return err / torch.exp2(torch.floor(torch.log2(top)) - 23)


@pytest.fixture(scope="module")
def kd_cases():
    """Per (V, beta, tau): the inputs and the fp64 references, computed once and left unchanged; plus the bounds pooled
    over the grid per instantiation: (loss, lse, gradient)."""
    cases = {}
    bound = {m: [0.0, 0.0, 0.0] for m in ("fkl", "rkl", "mix")}
    rows = {V: _kd_rows(V) for V in SMALL_V + BIG_V}
    for V, beta, tau in GRID:
        s, t, labels = rows[V]
        want, emul = _kd_refs(s, t, labels, beta, tau)
        cases[V, beta, tau] = (s, t, labels, want)
        b = bound[mode_of(beta)]
        b[0] = max(b[0], _ulps((emul[0].double() - want[0]).abs(), want[2], want[3], want[0]).max().item())
        b[1] = max(b[1], _ulps((emul[2].double() - want[2]).abs(), want[2]).max().item(),
                   _ulps((emul[3].double() - want[3]).abs(), want[3]).max().item())
        b[2] = max(b[2], block_rel_err(emul[1], want[1], 1, V).max().item())
    return cases, {m: [2 * v for v in b] for m, b in bound.items()}


def _call(s, t, labels, write_grad, beta, tau):
    lg, tc = s.clone(), t.clone()
    stats = _ext.ops().kd_fwd(lg, tc, labels, torch.tensor([SCALE], device=DEV), write_grad, beta, tau)
    assert torch.equal(bits(tc), bits(t))  # the teacher's logits are only read
    return lg, stats


@pytest.mark.parametrize("V,beta,tau", GRID)
def test_kd_fwd_rows(V, beta, tau, kd_cases):
    cases, bounds = kd_cases
    s, t, labels, (loss, grad, lse_s, lse_t) = cases[V, beta, tau]
    bl, be, bg = bounds[mode_of(beta)]
    M = s.shape[0]
    valid = labels != -100
    lg, stats = _call(s, t, labels, True, beta, tau)
    torch.cuda.synchronize()
    assert stats.shape == (5, M) and stats.dtype == torch.float32
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(lg.float()).all())
    e_loss = _ulps((stats[0].double() - loss).abs(), lse_s, lse_t, loss).max().item()
    report(f"kd_fwd V={V} beta={beta} tau={tau}: loss (fp32 ulps of the row's largest term)", e_loss, bl)
    e_lse = max(_ulps((stats[1].double() - lse_s).abs(), lse_s).max().item(),
                _ulps((stats[2].double() - lse_t).abs(), lse_t).max().item())
    report(f"kd_fwd V={V} beta={beta} tau={tau}: the two lse (fp32 ulps)", e_lse, be)
    e_grad = block_rel_err(lg, grad, 1, V).max().item()
    report(f"kd_fwd V={V} beta={beta} tau={tau}: gradient rows", e_grad, bg)
    assert 0 < bl and 0 < be and 0 < bg < 1e-2
    assert e_loss <= bl
    assert e_lse <= be
    assert e_grad <= bg
    assert bool((stats[0][~valid] == 0).all())
    assert not bits(lg[~valid]).any()           # a label of -100: every gradient element has zero bits
    top_s, top_t = first_argmax(s.float()), first_argmax(t.float())
    assert torch.equal(stats[3], ((top_s == labels) & valid).float())
    assert torch.equal(stats[4], ((top_s == top_t) & valid).float())
    if M == 6:
        assert stats[3][0].item() == 1.0        # the row the student gets right
        assert stats[4][1].item() == 1.0        # teacher == student agrees with itself
        assert int(top_t[0]) == 0 and int(top_t[3]) == V - 1


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_kd_fwd_argmax_rows_with_ties(beta):
    """Stats rows 3 and 4 against argmax comparisons in torch, ties resolved to the first index: the maximum twice in
    one row (in two vectors of the unrolled loop, in two threads, in the tail), in the student and in the teacher."""
    V = 8 * 1025
    g = torch.Generator(device=DEV).manual_seed(7)
    s = torch.randn(6, V, device=DEV, generator=g).to(BF16)
    t = torch.randn(6, V, device=DEV, generator=g).to(BF16)
    hi = 8.0
    s[0, 5], s[0, 8 * 300 + 1] = hi, hi              # student tie: first at 5
    t[0, 5] = hi                                     # agrees with the first
    s[1, 8 * 1024 + 3], s[1, 17] = hi, hi            # tie between the tail and the unrolled part: first at 17
    t[1, 8 * 1024 + 3] = hi                          # the teacher picks the later one: no agreement
    s[2, 40] = hi
    t[2, 40], t[2, 33] = hi, hi                      # teacher tie: first at 33, the student is at 40
    s[3, V - 1] = hi
    t[3, V - 1], t[3, V - 2] = hi, hi                # teacher tie at the last two columns: V - 2
    s[4, 0], s[4, V - 1] = hi, hi                    # student tie first / last column: 0
    t[4, 0] = hi
    labels = torch.tensor([5, 17, 40, V - 1, V - 1, 3], device=DEV)
    labels[5] = int(s[5].float().argmax())
    _, stats = _call(s, t, labels, False, beta, 0.9)
    top_s, top_t = first_argmax(s.float()), first_argmax(t.float())
    assert top_s.tolist()[:5] == [5, 17, 40, V - 1, 0] and top_t.tolist()[:5] == [5, 8 * 1024 + 3, 33, V - 2, 0]
    assert stats[3].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0, 1.0]
    assert torch.equal(stats[4], (top_s == top_t).float()) and stats[4].tolist()[:5] == [1.0, 0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("V", [8 * 257, 8 * 2049])
def test_kd_fwd_row_isolation(V, beta):
    """One row's teacher logits replaced by large values: that row's stats and gradient move, every other row's bits
    stay."""
    s, t, labels = _kd_rows(V)
    lg0, st0 = _call(s, t, labels, True, beta, 0.9)
    for r in (0, 3):
        tp = t.clone()
        tp[r] = (1e4 * torch.randn(V, device=DEV)).to(BF16)
        lg1, st1 = _call(s, tp, labels, True, beta, 0.9)
        assert bool(torch.isfinite(st1).all()) and bool(torch.isfinite(lg1.float()).all())
        others = torch.arange(6, device=DEV) != r
        assert torch.equal(bits(st1[:, others]), bits(st0[:, others]))
        assert torch.equal(bits(lg1[others]), bits(lg0[others]))
        assert st1[0, r].item() != st0[0, r].item() and not torch.equal(bits(lg1[r]), bits(lg0[r]))


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("V", [8, 8 * 1025, 128256])
def test_kd_fwd_stats_only(V, beta):
    """write_grad=False: the student's logits stay untouched, bit for bit, and the stats equal those of a
    write_grad=True call on a clone."""
    s, t, labels = _kd_rows(V)
    lg, st = _call(s, t, labels, False, beta, 0.9)
    assert torch.equal(bits(lg), bits(s))
    lg1, st1 = _call(s, t, labels, True, beta, 0.9)
    assert torch.equal(bits(st), bits(st1)) and not torch.equal(bits(lg1), bits(s))


def test_kd_fwd_refusals():
    s, t, labels = _kd_rows(64)
    inv = torch.tensor([SCALE], device=DEV)
    o = _ext.ops()
    bad = [lambda: o.kd_fwd(s.clone(), t[:, :56].contiguous(), labels, inv, True, 0.5, 1.0),  # shape mismatch
           lambda: o.kd_fwd(s.clone(), t[:5], labels, inv, True, 0.5, 1.0),
           lambda: o.kd_fwd(s.clone(), t.float(), labels, inv, True, 0.5, 1.0),               # dtype mismatch
           lambda: o.kd_fwd(s.float(), t.float(), labels, inv, True, 0.5, 1.0),               # fp32 logits
           lambda: o.kd_fwd(s[:, :60].contiguous(), t[:, :60].contiguous(), labels, inv, True, 0.5, 1.0),  # V % 8
           lambda: o.kd_fwd(s.clone(), t, labels, inv, True, 1.5, 1.0),
           lambda: o.kd_fwd(s.clone(), t, labels, inv, True, -0.1, 1.0),
           lambda: o.kd_fwd(s.clone(), t, labels, inv, True, 0.5, 0.0),
           lambda: o.kd_fwd(s.clone(), t, labels, inv.cpu(), True, 0.5, 1.0),                 # CPU inv_count
           lambda: o.kd_fwd(s.clone(), t, labels.int(), inv, True, 0.5, 1.0),
           lambda: o.kd_fwd(s.clone(), t, labels[:5], inv, True, 0.5, 1.0),
           lambda: o.kd_fwd(s.clone(), t[:, ::2], labels, inv, True, 0.5, 1.0)]               # not contiguous
    for fn in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
    x = s.clone()
    with pytest.raises(RuntimeError, match="alias"):
        o.kd_fwd(x, x, labels, inv, True, 0.5, 1.0)
    assert torch.equal(bits(x), bits(s))
    empty = o.kd_fwd(s[:0], t[:0], labels[:0], inv, True, 0.5, 1.0)
    assert empty.shape == (5, 0) and empty.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ lm_head_distill_loss
T_ROWS, HID, VOC = 70, 256, 1024


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


def _head_refs(h, w, teacher, labels, beta, tau, gl, dt):
    """(loss, dh, dW) of gl * loss in ``dt``; dt fp32 rounds where the HIP path does: bf16 logits, the bf16 gradient
    over them, the loss gradient rounded to bf16 on the bf16 G W and on h, one bf16 rounding of each result."""
    emul = dt == torch.float32
    rnd = (lambda x: x.to(BF16).to(dt)) if emul else (lambda x: x)
    n = (labels != -100).sum().to(dt)
    inv = (1.0 / n).reshape(1)
    logits = rnd(h.to(dt) @ w.to(dt).t())
    loss = ref.generalized_jsd(logits, teacher.to(dt), labels, beta, tau)[0].sum() * inv[0]
    G = rnd(ref.generalized_jsd_grad(logits, teacher.to(dt), labels, inv, beta, tau))
    g = rnd(torch.tensor(gl, dtype=dt, device=DEV))
    dh = rnd(rnd(G @ w.to(dt)) * g)
    dw = rnd(G.t() @ rnd(h.to(dt) * g))
    return loss, dh, dw


@pytest.mark.parametrize("gl", [1.0, 1.0 / 7.0])
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_lm_head_distill_loss_against_fp64(beta, gl):
    tau = 0.9
    h, w, teacher, labels = _head_case()
    want = _head_refs(h, w, teacher, labels, beta, tau, gl, torch.float64)
    emul = _head_refs(h, w, teacher, labels, beta, tau, gl, torch.float32)
    inv = (1.0 / (labels != -100).sum().float()).reshape(1)
    hh, ww = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    t0 = teacher.clone()
    loss, stats = ops.lm_head_distill_loss(hh, ww, teacher, labels, inv, beta, tau)
    assert stats.shape == (5, T_ROWS) and loss.dtype == torch.float32
    (loss * gl).backward()
    assert torch.equal(bits(teacher), bits(t0))
    bl = 2 * abs(emul[0].item() - want[0].item()) / abs(want[0].item())
    el = abs(loss.item() - want[0].item()) / abs(want[0].item())
    report(f"lm_head_distill_loss beta={beta} dloss={gl:.3f}: loss", el, bl)
    assert bl > 0 and el <= bl
    bh = 2 * block_rel_err(emul[1], want[1], 1, HID).max().item()
    eh = assert_blocks_close(hh.grad, want[1], 1, HID, bh, "dh")
    report(f"lm_head_distill_loss beta={beta} dloss={gl:.3f}: dh rows", eh, bh)
    bw = 2 * block_rel_err(emul[2], want[2], 32, 32).max().item()
    ew = assert_blocks_close(ww.grad, want[2], 32, 32, bw, "dW")
    report(f"lm_head_distill_loss beta={beta} dloss={gl:.3f}: dW (32 x 32 blocks)", ew, bw)
    assert not (hh.grad[labels == -100] != 0).any()
    # a frozen weight: no dW, the same dh
    h2, wf = h.clone().requires_grad_(True), w.clone()
    loss2, _ = ops.lm_head_distill_loss(h2, wf, teacher, labels, inv, beta, tau)
    (loss2 * gl).backward()
    assert wf.grad is None and torch.equal(bits(h2.grad), bits(hh.grad)) and loss2.item() == loss.item()


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


def _distill_run(model, batch, t_logits, hip, monkeypatch, beta, tau):
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    out = model.distill_loss(teacher_logits=t_logits, beta=beta, temperature=tau, **batch)
    out.loss.backward()
    torch.cuda.synchronize()
    return out, {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("student,teacher,lora", [("tiny-gpu", "tiny-gpu", False),
                                                  ("tiny-gpu-qwen3", "tiny-gpu-mistral", False),
                                                  ("tiny-gpu", "tiny-gpu-mistral", True)])
def test_distill_loss_hip_vs_reference(student, teacher, lora, layout, monkeypatch):
    torch.manual_seed(0)
    cfg = get_config(student)
    m = build_model(cfg, device=DEV, dtype=BF16, seed=1)
    te = build_model(get_config(teacher), device=DEV, dtype=BF16, seed=2).eval().requires_grad_(False)
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
    with torch.no_grad():
        t_logits = te.logits_rows(**inputs)
    assert t_logits.shape == (256, cfg.vocab_size) and t_logits.dtype == BF16 and not t_logits.requires_grad
    beta, tau = 0.5, 0.9
    o_hip, g_hip = _distill_run(m, batch, t_logits, True, monkeypatch, beta, tau)
    o_ref, g_ref = _distill_run(m, batch, t_logits, False, monkeypatch, beta, tau)
    assert o_hip.stats.shape == (5, 256) and o_hip.metrics.shape == (3,)
    assert o_hip.num_tokens.item() == o_ref.num_tokens.item() == o_hip.metrics[2].item() > 0
    what = f"distill_loss {student}{' lora' if lora else ''} <- {teacher} {layout}"
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


# ------------------------------------------------------------------------------------------------ trainer
def _gkd_trainer(out, steps=3, save_steps=0):
    from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
    from llm_fine_tune_distributed_amd.train import GKDConfig, GKDTrainer
    a = GKDConfig(output_dir=str(out), per_device_train_batch_size=4, per_device_eval_batch_size=4, max_steps=steps,
                  learning_rate=1e-3, lr_scheduler_type="constant", logging_steps=1, jsonl_log=False,
                  save_strategy="steps" if save_steps else "no", save_steps=save_steps or 500, seed=3,
                  dataloader_drop_last=True, beta=0.5, temperature=0.9)
    student = build_model(get_config("tiny-gpu"), device=DEV, dtype=BF16, seed=0)
    teacher = build_model(get_config("tiny-gpu-mistral"), device=DEV, dtype=BF16, seed=9)
    ds = TokenizedDataset.synthetic(4, 1024, 30, 90, seed=2)  # one batch, seen every step
    return GKDTrainer(model=student, args=a, train_dataset=ds, eval_dataset=ds, teacher_model=teacher)


def _params(t):
    t.optimizer.synchronize()
    torch.cuda.synchronize()
    return t.engine.param_flat.clone()


@pytest.fixture(scope="module")
def gkd_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("gkd")
    t = _gkd_trainer(out, save_steps=2)
    before = {n: p.detach().clone() for n, p in t.teacher.named_parameters()}
    ce_calls = []
    real = lm_head._ce_rows
    lm_head._ce_rows = lambda *a, **k: (ce_calls.append(1), real(*a, **k))[1]
    _ext.ops().dispatch_trace(True)
    try:
        t.train()
        ev = t.evaluate()
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
        lm_head._ce_rows = real
    trace = {k: int(v) for k, v in (it.split("=") for it in _ext.ops().dispatch_trace_read().split(";") if it)}
    return t, before, trace, len(ce_calls), ev, out


def test_gkd_trainer_runs_kd_fwd_and_no_cross_entropy(gkd_run):
    _, _, trace, ce_calls, _, _ = gkd_run
    assert trace.get("kd_fwd.mix", 0) >= 3 + 1, sorted(trace)  # three steps and the evaluation batch
    assert ce_calls == 0                                        # the fused cross-entropy is never called


def test_gkd_trainer_steps_and_teacher(gkd_run):
    t, before, _, _, ev, _ = gkd_run
    logs = [h for h in t.state.log_history if "loss" in h]
    assert len(logs) == 3
    losses = [h["loss"] for h in logs]
    print(f"\n[distill] GKDTrainer losses {losses}")
    assert all(math.isfinite(v) for v in losses) and losses[2] < losses[0], losses
    for k in ("mean_token_accuracy", "teacher_agreement", "grad_norm", "learning_rate", "epoch", "num_tokens"):
        assert k in logs[-1], k
    assert math.isfinite(ev["eval_loss"]) and ev["eval_loss"] > 0 and 0.0 <= ev["eval_teacher_agreement"] <= 1.0
    assert "eval_mean_token_accuracy" in ev and ev["eval_num_tokens"] > 0
    for n, p in t.teacher.named_parameters():
        assert torch.equal(p, before[n]) and not p.requires_grad, n
    assert not t.teacher.training


def test_gkd_trainer_resume_bit_for_bit(gkd_run):
    """A checkpoint written at step 2, resumed by a fresh trainer with the same teacher, reaches the straight run's
    parameters at step 3 bit for bit."""
    import os
    t, _, _, _, _, out = gkd_run
    assert os.path.isdir(os.path.join(str(out), "checkpoint-2"))
    files = os.listdir(os.path.join(str(out), "checkpoint-2"))
    t2 = _gkd_trainer(out, save_steps=0)
    torch.manual_seed(12345)  # the generators disturbed: the checkpoint restores what the step needs
    t2.train(resume_from_checkpoint="auto")
    assert t2.state.global_step == 3
    a, b = _params(t), _params(t2)
    d = (a.float() - b.float()).abs()
    assert torch.equal(bits(a), bits(b)), (int((d > 0).sum()), d.max().item(), files)
