"""The SFT objectives' kernels on the GPU: the noisy embedding gather (csrc/elementwise.hip embedding_noise_fwd) bit for
bit against its torch twin, the label-smoothing and dft instantiations of the fused cross-entropy
(csrc/cross_entropy.hip) per row against fp64, and a model step per objective against the PyTorch reference path.

Bounds follow tests/test_rowwise_gpu.py: each is 2 x the worst error of an fp32 torch emulation with the kernel's
rounding points against the fp64 reference, computed here from the references alone and pooled over the grid; every test prints
its worst measured error next to the bound (pytest -s); profiles/sft_objectives.md records one run."""

import pytest
import torch

from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import block_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SCALE = 1.0 / 7.0
EPS = 0.1


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16)


def report(what, worst, bound):
    print(f"\n[objectives] {what}: worst {worst:.3e} bound {bound:.3e}")


# ------------------------------------------------------------------------------------------------ noisy embedding
VOCAB = 97


def _emb_case(M, H, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(VOCAB, H, generator=g, device=DEV).to(BF16)
    ids = torch.randint(0, VOCAB, (M,), generator=g, device=DEV)
    ids[0] = VOCAB - 1
    if M > 1:
        ids[-1] = 0
    if M > 4:
        ids[2] = ids[3] = ids[1]  # repeats: the same row at three positions
    mag = 0.05 + 0.5 * torch.rand(M, generator=g, device=DEV)
    if M > 1:
        mag[M // 2] = 0.0
    return w, ids, mag


def _check_noisy_embedding(M, H):
    w, ids, mag = _emb_case(M, H, 100 + 7 * M + H)
    ops = _ext.ops()
    plain = ops.embedding_fwd(ids, w)
    outs = {}
    for seed in (1, 2 ** 31 - 2):
        out = ops.embedding_noise_fwd(ids, w, mag, seed)
        assert out.shape == (M, H) and out.dtype == BF16
        twin = ref.embedding_noise(ids, w, mag, seed)
        assert torch.equal(bits(out), bits(twin)), (M, H, seed, (out.float() - twin.float()).abs().max().item())
        assert torch.equal(bits(out), bits(ops.embedding_noise_fwd(ids, w, mag, seed)))  # same seed: identical
        outs[seed] = out
    assert not torch.equal(bits(outs[1]), bits(outs[2 ** 31 - 2]))                    # two seeds: different
    if M > 1:
        z = M // 2
        assert torch.equal(bits(outs[1][z]), bits(plain[z]))                            # mag 0: the plain gather
        live = torch.ones(M, dtype=torch.bool, device=DEV)
        live[z] = False
        assert bool((bits(outs[1])[live] != bits(plain)[live]).any(-1).all())           # every other row moved
    zero = ops.embedding_noise_fwd(ids, w, torch.zeros(M, device=DEV), 1)
    assert torch.equal(bits(zero), bits(plain))


@pytest.mark.parametrize("M", [1, 5, 67])
@pytest.mark.parametrize("H", [8, 520, 2048, 2056])
def test_noisy_embedding_bit_for_bit(M, H):
    _check_noisy_embedding(M, H)


def test_noisy_embedding_second_grid_stride_pass():
    """2049 x 2056 / 8 = 526,593 vectors, more than the 524,288 of one pass of the capped grid: the second pass, with a
    ragged tail, and element indices m H + c past 2^22."""
    _check_noisy_embedding(2049, 2056)


def test_noisy_embedding_shapes_and_refusals():
    w, ids, mag = _emb_case(6, 64, 5)
    ops = _ext.ops()
    out = ops.embedding_noise_fwd(ids.view(2, 3), w, mag, 3)
    assert out.shape == (2, 3, 64) and torch.equal(bits(out.view(6, 64)), bits(ops.embedding_noise_fwd(ids, w, mag, 3)))
    assert ops.embedding_noise_fwd(ids[:0], w, mag[:0], 3).shape == (0, 64)
    for bad in (mag[:5], mag.double(), mag.cpu()):
        with pytest.raises(RuntimeError):
            ops.embedding_noise_fwd(ids, w, bad, 3)


# ------------------------------------------------------------------------------------------------ cross-entropy modes
CE_V = [8 * n for n in (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2049)] + [128256, 151936]
MODES = {"smooth": (EPS, 0), "dft": (0.0, 1)}
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def _ce_rows(V):
    """bf16 logits [M, V] and labels: the first and the last column, the argmax, a column of the unrolled part of the
    row loop (1024 vectors per pass), a column of its tail, and -100; three of them (argmax, tail, -100) for the two
    training vocabularies."""
    big = V > 100000
    M = 3 if big else 6
    g = torch.Generator(device=DEV).manual_seed(V)
    x = (3 * torch.randn(M, V, device=DEV, generator=g)).to(BF16)
    nvec = V // 8
    unrolled = 8 * min(5, nvec - 1) + 3          # the first pass (the tail loop where the row has no whole pass)
    tail = 8 * (nvec - 1 - min(2, nvec - 1)) + 1  # the last vectors: the remainder loop unless nvec % 1024 == 0
    if big:
        labels = [int(x[0].float().argmax()), tail, -100]
    else:
        labels = [0, V - 1, int(x[2].float().argmax()), unrolled, tail, -100]
    return x.contiguous(), torch.tensor(labels, device=DEV, dtype=torch.int64)


def _ce_refs(x, labels, mode):
    """fp64 (loss, grad, lse) and the fp32 emulation (loss, bf16 grad) of one objective on bf16 logits. The emulation
    rounds where the kernel does: exp as exp2(fp32(x log2 e)) and log as fp32(log2(s) ln 2) (the hardware
    transcendentals behind __expf / __logf), lse = m + log s, the loss and the gradient element in the kernel's
    association, one rounding to bf16."""
    eps, lm = MODES[mode]
    M, V = x.shape
    valid = labels != -100
    safe = labels.clamp(min=0)
    rows = torch.arange(M, device=x.device)
    x64 = x.double()
    lse = torch.logsumexp(x64, -1)
    p = torch.softmax(x64, -1)
    xl = x64[rows, safe]
    onehot = torch.zeros_like(p)
    onehot[rows, safe] = 1.0
    if lm == 1:
        w = torch.exp(xl - lse)
        loss, grad = w * (lse - xl), w[:, None] * (p - onehot) * SCALE
    else:
        loss = lse - (1 - eps) * xl - eps * x64.sum(-1) / V
        grad = (p - (1 - eps) * onehot - eps / V) * SCALE
    loss, grad = loss * valid, grad * valid[:, None]

    def f(v):
        return torch.tensor(v, dtype=torch.float32, device=x.device)
    xf = x.float()
    m = xf.max(-1, keepdim=True).values
    s = torch.exp2((xf - m) * f(LOG2E)).sum(-1)
    lse32 = m[:, 0] + torch.log2(s) * f(LN2)
    xl32 = xf[rows, safe]
    p32 = torch.exp2((xf - lse32[:, None]) * f(LOG2E))
    hot = onehot.float()
    sc = f(SCALE) * valid.float()
    if lm == 1:
        w32 = torch.exp2((xl32 - lse32) * f(LOG2E))
        loss32 = w32 * (lse32 - xl32)
        grad32 = (p32 - hot) * (sc * w32)[:, None]
    else:
        loss32 = lse32 - (f(1.0) - f(eps)) * xl32 - f(eps) * (xf.sum(-1) / float(V))
        grad32 = ((p32 - hot * (f(1.0) - f(eps))) - f(eps) / float(V)) * sc[:, None]
    return loss, grad, lse, loss32 * valid, grad32.to(BF16)


def _ulps(err, lse64, sens=None):
    """An absolute loss error in units of what one fp32 ulp of the row's logsumexp (the largest term of every formula
    here, and the one both transcendentals feed) does to the loss: 1 for the smoothed loss lse - ..., and
    w max(1, nll) for dft's w (lse - x_y), whose rows differ by orders of magnitude in w = p_y (``sens``)."""
    unit = torch.exp2(torch.floor(torch.log2(lse64.abs().clamp(min=1.0))) - 23)
    return err / (unit if sens is None else unit * sens)


def _sens(x, labels, lse64, mode):
    if MODES[mode][1] != 1:
        return None
    nll = lse64 - x.double()[torch.arange(x.shape[0], device=x.device), labels.clamp(min=0)]
    return (torch.exp(-nll) * nll.clamp(min=1.0)).clamp(min=1e-300)


@pytest.fixture(scope="module")
def ce_cases():
    """Per (V, mode): the inputs and references, computed once and left unchanged; plus the pooled bounds."""
    cases, loss_b, grad_b, sum_ref = {}, {m: 0.0 for m in MODES}, {m: 0.0 for m in MODES}, 0.0
    for V in CE_V:
        x, labels = _ce_rows(V)
        for mode in MODES:
            loss, grad, lse, loss_em, grad_em = _ce_refs(x, labels, mode)
            cases[V, mode] = (x, labels, loss, grad, lse)
            loss_b[mode] = max(loss_b[mode],
                               _ulps((loss_em.double() - loss).abs(), lse, _sens(x, labels, lse, mode)).max().item())
            grad_b[mode] = max(grad_b[mode], block_rel_err(grad_em, grad, 1, V).max().item())
            if mode == "smooth":  # the yardstick of the row-sum test: the bf16-rounded fp64 gradient's own row sums
                sum_ref = max(sum_ref, grad.to(BF16).double().sum(-1).abs().max().item())
    return cases, {m: 2 * v for m, v in loss_b.items()}, {m: 2 * v for m, v in grad_b.items()}, sum_ref


def _call(x, labels, write_grad, eps, lm):
    lg = x.clone()
    stats = _ext.ops().ce_fwd(lg, labels, torch.tensor([SCALE], device=DEV), write_grad, eps, lm)
    return lg, stats


@pytest.mark.parametrize("write_grad", [True, False])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("V", CE_V)
def test_ce_modes(V, mode, write_grad, ce_cases):
    cases, loss_bound, grad_bound, _ = ce_cases
    x, labels, loss, grad, lse = cases[V, mode]
    eps, lm = MODES[mode]
    M = x.shape[0]
    valid = labels != -100
    lg, stats = _call(x, labels, write_grad, eps, lm)
    plain_lg = x.clone()
    plain = _ext.ops().ce_fwd(plain_lg, labels, torch.tensor([SCALE], device=DEV), write_grad)
    torch.cuda.synchronize()
    assert stats.shape == (4, M) and bool(torch.isfinite(stats).all())
    # lse, entropy, correct: the plain call's, bit for bit (the TRL metrics do not move)
    assert torch.equal(stats[1:].view(torch.int32), plain[1:].view(torch.int32))
    e_loss = _ulps((stats[0].double() - loss).abs(), lse, _sens(x, labels, lse, mode)).max().item()
    report(f"ce {mode} V={V} grad={write_grad}: loss (in fp32 ulps of lse)", e_loss, loss_bound[mode])
    assert e_loss <= loss_bound[mode]
    assert bool((stats[0][~valid] == 0).all())
    assert bool((stats[0][valid] != plain[0][valid]).all())  # and it is another objective than the plain one
    if not write_grad:
        assert torch.equal(bits(lg), bits(x))  # untouched
        return
    e_grad = block_rel_err(lg, grad, 1, V).max().item()
    report(f"ce {mode} V={V}: gradient rows", e_grad, grad_bound[mode])
    assert e_grad <= grad_bound[mode]
    assert bool((lg[~valid] == 0).all())       # ignored rows: exactly zero


@pytest.mark.parametrize("write_grad", [True, False])
@pytest.mark.parametrize("V", CE_V)
def test_ce_default_arguments_are_the_plain_call(V, write_grad):
    x, labels = _ce_rows(V)
    a_lg, a = _call(x, labels, write_grad, 0.0, 0)
    b_lg = x.clone()
    b = _ext.ops().ce_fwd(b_lg, labels, torch.tensor([SCALE], device=DEV), write_grad)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(bits(a_lg), bits(b_lg))


def test_ce_smoothed_gradient_rows_sum_to_zero(ce_cases):
    """Each valid row of (p - (1 - e) onehot - e / V) s sums to zero; what is left after the bf16 store is rounding.
    Yardstick: the row sums of the bf16-rounded fp64 gradient, pooled over the grid; the kernel's stay within 2 x."""
    cases, _, _, sum_ref = ce_cases
    worst = 0.0
    for V in CE_V:
        x, labels = cases[V, "smooth"][:2]
        lg, _ = _call(x, labels, True, EPS, 0)
        worst = max(worst, lg.double().sum(-1).abs().max().item())
    report("ce smooth: |row sum| of the gradient", worst, 2 * sum_ref)
    assert 0 < sum_ref and worst <= 2 * sum_ref


def test_ce_mode_refusals():
    x, labels = _ce_rows(64)
    for eps, lm in ((1.0, 0), (-0.1, 0), (0.1, 1), (0.0, 2)):
        with pytest.raises(RuntimeError):
            _call(x, labels, True, eps, lm)


# ------------------------------------------------------------------------------------------------ model step
def _step(model, ids, labels, hip, monkeypatch, seed, **kw):
    monkeypatch.setenv("SFTAMD_DISABLE_HIP", "0" if hip else "1")
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    torch.manual_seed(seed)  # both paths draw the same noise seed
    out = model(ids, labels=labels, **kw)
    out.loss.backward()
    return out.loss.detach().float(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("what", ["smooth", "dft", "neftune"])
def test_tiny_gpu_step_hip_vs_reference(what, monkeypatch):
    """2 x 128 tokens on tiny-gpu, the HIP path against SFTAMD_DISABLE_HIP=1 on the same bf16 weights, with the bounds
    of test_model_gpu.test_model_hip_vs_reference; and the objective differs from the plain step's."""
    cfg = get_config("tiny-gpu")
    m = build_model(cfg, device=DEV, dtype=BF16, seed=1)
    m.train()
    g = torch.Generator(device=DEV).manual_seed(0)
    ids = torch.randint(0, cfg.vocab_size, (2, 128), device=DEV, generator=g)
    labels = ids.clone()
    labels[:, 100:] = -100
    kw = {"smooth": {"label_smoothing": EPS}, "dft": {"loss_type": "dft"}, "neftune": {}}[what]
    l_plain, _ = _step(m, ids, labels, True, monkeypatch, 3)
    if what == "neftune":
        m.neftune_noise_alpha = 5.0
    l_hip, g_hip = _step(m, ids, labels, True, monkeypatch, 3, **kw)
    l_ref, g_ref = _step(m, ids, labels, False, monkeypatch, 3, **kw)
    assert l_hip.item() != l_plain.item()
    print(f"\n[objectives] tiny-gpu {what}: loss hip {l_hip.item():.6f} ref {l_ref.item():.6f} plain {l_plain.item():.6f}")
    assert abs(l_hip.item() - l_ref.item()) < 2e-2 * abs(l_ref.item())
    worst = 0.0
    for n in g_ref:
        e = ((g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)).item()
        worst = max(worst, e)
        assert e < 5e-2, (n, e)
    report(f"tiny-gpu {what}: gradient, worst parameter", worst, 5e-2)
