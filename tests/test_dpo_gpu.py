"""DPO on the GPU: the three kernels of csrc/preference.hip (seq_logp_sum, scale_rows_by_seq, dpo_pair_fwd), the
sequence-level LM head built on them (ops.lm_head_seq_logps), CausalLM.sequence_logps on the HIP path against the
PyTorch reference path, and DPOTrainer steps with the kernels' dispatch trace.

Bounds follow tests/test_objectives_gpu.py and tests/test_rowwise_gpu.py: each is 2 x the worst error of an fp32 torch
emulation with the kernel's rounding points against the fp64 reference, computed here from the references alone; every
test prints its worst measured error next to the bound (pytest -s); profiles/dpo.md records one run. The model tests
use the project's bounds of tests/test_model_gpu.py::test_model_hip_vs_reference."""
import glob
import math
import os

import pytest
import torch

from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close, block_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
LN2 = math.log(2.0)


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def report(what, worst, bound):
    print(f"\n[dpo] {what}: worst {worst:.3e} bound {bound:.3e}")


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


# ------------------------------------------------------------------------------------------------ seq_logp_sum
SEQ_LENS = [1, 63, 64, 65, 129, 0, 1000]
SEQ_PAD = 7


def _nll_case():
    g = torch.Generator(device=DEV).manual_seed(11)
    M = sum(SEQ_LENS) + SEQ_PAD
    nll = (3.0 * torch.randn(M, generator=g, device=DEV)).abs()
    nll[torch.rand(M, generator=g, device=DEV) < 0.2] = 0.0  # ignored rows carry an exact 0
    nll[0] = 2.5
    return nll


def _emul_seq_sum(x):
    """fp32 twin of one wave: lane l adds rows l, l + 64, ... in order, then the xor butterfly 32, 16, ..., 1."""
    n = x.numel()
    k = -(-n // 64)
    rows = torch.zeros(max(k, 1) * 64, dtype=torch.float32, device=x.device)
    rows[:n] = x
    rows = rows.view(-1, 64)
    acc = torch.zeros(64, dtype=torch.float32, device=x.device)
    for r in rows:
        acc = acc + r
    lane = torch.arange(64, device=x.device)
    o = 32
    while o:
        acc = acc + acc[lane ^ o]
        o >>= 1
    return 0.0 - acc[0]


def test_seq_logp_sum_against_fp64():
    nll, cu = _nll_case(), cu_of(SEQ_LENS, SEQ_PAD)
    S = len(SEQ_LENS)
    got = _ext.ops().seq_logp_sum(nll, cu, S)
    assert got.shape == (S,) and got.dtype == torch.float32
    c = cu.tolist()
    want = torch.stack([-nll[c[s]:c[s + 1]].double().sum() for s in range(S)])
    emul = torch.stack([_emul_seq_sum(nll[c[s]:c[s + 1]]) for s in range(S)])
    bound = 2 * rel_err(emul, want).max().item()
    worst = rel_err(got, want).max().item()
    report("seq_logp_sum", worst, bound)
    assert bound > 0 and worst <= bound
    assert bits(got[5]).item() == 0                                                 # the empty segment: +0
    assert torch.equal(bits(got), bits(_ext.ops().seq_logp_sum(nll, cu, S)))      # two calls: identical bits
    assert torch.equal(bits(got[:3]), bits(_ext.ops().seq_logp_sum(nll, cu, 3)))  # later segments are ignored


@pytest.mark.parametrize("poison", [0, 1])
def test_seq_logp_sum_isolation(poison):
    """The sequences in reversed order, every other one (and the pad segment) replaced by 1e30: the untouched
    sequences' bits do not move."""
    nll, cu = _nll_case(), cu_of(SEQ_LENS, SEQ_PAD)
    S = len(SEQ_LENS)
    base = _ext.ops().seq_logp_sum(nll, cu, S)
    c = cu.tolist()
    order = list(reversed(range(S)))
    parts = []
    for j, s in enumerate(order):
        seg = nll[c[s]:c[s + 1]].clone()
        if j % 2 == poison:
            seg.fill_(1e30)
        parts.append(seg)
    parts.append(torch.full((SEQ_PAD,), 1e30, device=DEV))
    got = _ext.ops().seq_logp_sum(torch.cat(parts), cu_of([SEQ_LENS[s] for s in order], SEQ_PAD), S)
    assert torch.isfinite(got).all()
    for j, s in enumerate(order):
        if j % 2 != poison:
            assert bits(got[j]).item() == bits(base[s]).item(), (s, got[j].item(), base[s].item())


def test_seq_logp_sum_refusals():
    nll, cu = _nll_case(), cu_of(SEQ_LENS, SEQ_PAD)
    o = _ext.ops()
    for bad in (lambda: o.seq_logp_sum(nll.double(), cu, 3), lambda: o.seq_logp_sum(nll, cu.long(), 3),
                lambda: o.seq_logp_sum(nll.to(BF16), cu, 3), lambda: o.seq_logp_sum(nll, cu, cu.numel()),
                lambda: o.seq_logp_sum(nll.cpu(), cu, 3)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            bad()


# ------------------------------------------------------------------------------------------------ scale_rows_by_seq
ROW_LENS = [1, 63, 65, 129]
ROW_TAIL = 5


def _check_scale_rows(lens, tail, H, gs, coef):
    M = sum(lens) + tail
    g = torch.Generator(device=DEV).manual_seed(H + M)
    x = torch.randn(M, H, generator=g, device=DEV).to(BF16)
    x0 = x.clone()
    cu = cu_of(lens, tail)
    n = len(lens)
    coef = torch.tensor(coef, dtype=torch.float32, device=DEV)
    gscale = torch.tensor([gs], dtype=torch.float32, device=DEV)
    twin = ref.scale_rows_by_seq(x, coef, cu, n, gscale)
    out = _ext.ops().scale_rows_by_seq(x, coef, cu, n, gscale)
    assert out.dtype == BF16 and out.shape == x.shape
    assert torch.equal(bits(x), bits(x0))                      # out of place: the input is untouched
    assert torch.equal(bits(out), bits(twin)), (H, gs, (out.float() - twin.float()).abs().max().item())
    assert not bits(out[M - tail:]).any()                      # tail rows: +0
    y = x.clone()
    _ext.ops().scale_rows_by_seq_(y, coef, cu, n, gscale)
    assert torch.equal(bits(y), bits(twin))                    # in place
    ones = torch.ones(n, dtype=torch.float32, device=DEV)
    same = _ext.ops().scale_rows_by_seq(x, ones, cu, n, torch.ones(1, device=DEV))
    assert torch.equal(bits(same[:M - tail]), bits(x[:M - tail]))  # coef 1, gscale 1: the input, bit for bit
    return out


@pytest.mark.parametrize("gs", [1.0, 1.0 / 7.0])
@pytest.mark.parametrize("H", [8, 520, 2048, 2056])
def test_scale_rows_bit_for_bit(H, gs):
    out = _check_scale_rows(ROW_LENS, ROW_TAIL, H, gs, [0.0, -1.5, 1.0, 0.37])
    assert not (out[:1].float() != 0).any()  # coef 0: zeros (of either sign)


def test_scale_rows_second_grid_pass_and_empty_segment():
    """65,835 rows: more than the 65,535 row blocks of one pass of the capped grid, with an empty segment inside."""
    _check_scale_rows([3, 0, 65535 + 290, 2], 5, 8, 1.0 / 7.0, [2.0, 5.0, -0.25, 1.0])


def test_scale_rows_refusals():
    x = torch.randn(8, 16, device=DEV).to(BF16)
    cu = cu_of([3, 5])
    coef = torch.ones(2, device=DEV)
    one = torch.ones(1, device=DEV)
    o = _ext.ops()
    for bad in (lambda: o.scale_rows_by_seq(x.float(), coef, cu, 2, one), lambda: o.scale_rows_by_seq(x, coef, cu, 3, one),
                lambda: o.scale_rows_by_seq(x, coef[:1], cu, 2, one), lambda: o.scale_rows_by_seq(x, coef, cu.long(), 2, one),
                lambda: o.scale_rows_by_seq(x[:, :12], coef, cu, 2, one), lambda: o.scale_rows_by_seq(x, coef, cu, 2, one.cpu()),
                lambda: o.scale_rows_by_seq(x, coef.double(), cu, 2, one)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            bad()


# ------------------------------------------------------------------------------------------------ dpo_pair_fwd
BETA = torch.tensor(0.1, dtype=torch.float32).item()  # 0.1 as the fp32 the kernel receives, for every reference
BETA32 = BETA
DPO_P = [1, 3, 64, 65, 257]
DELTAS = [0.0, 1e-3, -1e-3, 5.0, -5.0, 1e4 / BETA, -1e4 / BETA]


def _dpo_case(P):
    """(logps, ref_logps) fp32 [2 P]: pair p has delta DELTAS[p % 7] up to the rounding of the four log-probabilities
    (delta 0 exactly: policy == reference), the pairs past the seven a random delta of a few units."""
    g = torch.Generator(device=DEV).manual_seed(P)
    rc = -60.0 * torch.rand(P, generator=g, device=DEV, dtype=torch.float64) - 5.0
    rr = -60.0 * torch.rand(P, generator=g, device=DEV, dtype=torch.float64) - 5.0
    pr = -60.0 * torch.rand(P, generator=g, device=DEV, dtype=torch.float64) - 5.0
    d = 20.0 * torch.randn(P, generator=g, device=DEV, dtype=torch.float64)
    fixed = torch.tensor(DELTAS, dtype=torch.float64, device=DEV)
    k = min(P, len(DELTAS))
    sel = torch.arange(k, device=DEV) if P >= len(DELTAS) else torch.tensor([0, 5, 6][:k], device=DEV)
    d[:k] = fixed[sel]
    pc = pr + (rc - rr) + d
    zero = d == 0
    pc = torch.where(zero, rc, pc)
    pr = torch.where(zero, rr, pr)
    lp = torch.stack([pc, pr], 1).reshape(-1).float()
    rl = torch.stack([rc, rr], 1).reshape(-1).float()
    return lp, rl, zero


def _dpo_bound():
    """2 x the worst relative error, over every P, of the fp32 twin (the kernel's expression and rounding points)
    against the same expression in fp64 on the same fp32 inputs: (loss bound, coef bound)."""
    wl = wc = 0.0
    for P in DPO_P:
        lp, rl, _ = _dpo_case(P)
        inv = torch.tensor([1.0 / P], dtype=torch.float32, device=DEV)
        e = ref.dpo_pair(lp, rl, inv, BETA)
        w = ref.dpo_pair(lp.double(), rl.double(), inv.double(), BETA)
        wl = max(wl, rel_err(e[0], w[0]).max().item())
        wc = max(wc, rel_err(e[1], w[1]).max().item())
    return 2 * wl, 2 * wc


@pytest.mark.parametrize("P", DPO_P)
def test_dpo_pair_fwd(P):
    bl, bc = _dpo_bound()
    lp, rl, zero = _dpo_case(P)
    inv = torch.tensor([1.0 / P], dtype=torch.float32, device=DEV)
    st = _ext.ops().dpo_pair_fwd(lp, rl, inv, BETA)
    assert st.shape == (5, P) and st.dtype == torch.float32
    assert torch.isfinite(st).all()
    w = ref.dpo_pair(lp.double(), rl.double(), inv.double(), BETA)
    el, ec = rel_err(st[0], w[0]).max().item(), rel_err(st[1], w[1]).max().item()
    report(f"dpo_pair_fwd P={P} loss", el, bl)
    report(f"dpo_pair_fwd P={P} coef", ec, bc)
    assert 0 < bl < 1e-3 and 0 < bc < 1e-3 and el <= bl and ec <= bc
    # rewards and delta: single fp32 operations, exact
    assert torch.equal(bits(st[2]), bits(BETA32 * (lp[0::2] - rl[0::2])))
    assert torch.equal(bits(st[3]), bits(BETA32 * (lp[1::2] - rl[1::2])))
    assert torch.equal(bits(st[4]), bits((lp[0::2] - lp[1::2]) - (rl[0::2] - rl[1::2])))
    assert bool(zero.any())
    ln2 = torch.tensor(LN2, dtype=torch.float32, device=DEV)
    l0 = st[0][zero]
    assert ((l0 >= torch.nextafter(ln2, ln2 - 1)) & (l0 <= torch.nextafter(ln2, ln2 + 1))).all(), l0  # 1 ulp of ln 2
    half = (-BETA32 * 0.5) * inv[0]
    c0 = st[1][zero]
    assert ((c0 >= torch.nextafter(half, half - 1)) & (c0 <= torch.nextafter(half, half + 1))).all(), (c0, half)


def test_dpo_loss_backward_signs_and_refusals():
    P = 65
    lp, rl, _ = _dpo_case(P)
    inv = torch.tensor([1.0 / P], dtype=torch.float32, device=DEV)
    x = lp.clone().requires_grad_(True)
    loss, st = ops.dpo_loss(x, rl, inv, BETA)
    assert abs(loss.item() - st[0].double().sum().item() / P) <= 1e-6 * abs(loss.item())
    loss.backward()
    g = x.grad
    assert torch.equal(bits(g[0::2]), bits(st[1]))        # chosen: coef (dloss = 1)
    assert torch.equal(bits(g[1::2]), bits(-g[0::2]))     # rejected: its exact negative
    o = _ext.ops()
    for bad in (lambda: o.dpo_pair_fwd(lp.double(), rl, inv, BETA), lambda: o.dpo_pair_fwd(lp, rl[:-2], inv, BETA),
                lambda: o.dpo_pair_fwd(lp[:-1], rl[:-1], inv, BETA), lambda: o.dpo_pair_fwd(lp, rl, inv.cpu(), BETA),
                lambda: o.dpo_pair_fwd(lp, rl.double(), inv, BETA)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            bad()


# ------------------------------------------------------------------------------------------------ lm_head_seq_logps
LENS = [70, 33, 128, 65]
ROWS = 320


def _head_case():
    H, V = 256, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    h = torch.randn(ROWS, H, generator=g, device=DEV).to(BF16)
    w = (0.06 * torch.randn(V, H, generator=g, device=DEV)).to(BF16)
    cu = cu_of(LENS, ROWS - sum(LENS))
    labels = torch.randint(0, V, (ROWS,), generator=g, device=DEV)
    c = cu.tolist()
    for s, k in enumerate([9, 0, 17, 4]):
        labels[c[s]:c[s] + k] = -100          # masked prompt
        labels[c[s + 1] - 1] = -100           # the last token of a sequence predicts nothing
    labels[c[1]:c[2]] = -100                  # sequence 1: every label ignored
    labels[c[4]:] = -100                      # pad rows
    dlogps = torch.tensor([0.7, -1.3, 0.0, 0.4], dtype=torch.float32, device=DEV)  # both signs, one exact 0 (sequence 2)
    return h, w, cu, labels, dlogps


def _head_refs(h, w, cu, labels, dlogps, dt):
    """(logps, dh, dW) of sum_s dlogps[s] logp_s in ``dt``; dt fp32 rounds where the HIP path does: bf16 logits, bf16
    G = softmax - onehot, bf16 G W before the row weight, the row weight on bf16 h, one bf16 rounding of each result."""
    emul = dt == torch.float32
    rnd = (lambda t: t.to(BF16).to(dt)) if emul else (lambda t: t)
    n = len(LENS)
    valid = labels != -100
    safe = labels.clamp(min=0)
    rows = torch.arange(ROWS, device=DEV)
    logits = rnd(h.to(dt) @ w.to(dt).t())
    lse = torch.logsumexp(logits, -1)
    nll = torch.where(valid, lse - logits[rows, safe], torch.zeros((), dtype=dt, device=DEV))
    c = cu.tolist()
    logps = torch.stack([-nll[c[s]:c[s + 1]].sum() for s in range(n)])
    G = torch.softmax(logits, -1)
    G[rows, safe] -= 1.0
    G = rnd(G * valid[:, None].to(dt))
    r = torch.zeros(ROWS, dtype=dt, device=DEV)
    for s in range(n):
        r[c[s]:c[s + 1]] = -dlogps[s].to(dt)
    dh = rnd(rnd(G @ w.to(dt)) * r[:, None])
    dw = rnd(G.t() @ rnd(h.to(dt) * r[:, None]))
    return logps, dh, dw


def test_lm_head_seq_logps_against_fp64():
    h, w, cu, labels, dlogps = _head_case()
    n = len(LENS)
    want = _head_refs(h, w, cu, labels, dlogps, torch.float64)
    emul = _head_refs(h, w, cu, labels, dlogps, torch.float32)
    hh, ww = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    logps, stats = ops.lm_head_seq_logps(hh, ww, labels, cu, n)
    assert logps.dtype == torch.float32 and logps.shape == (n,) and stats.shape == (4, ROWS)
    (logps * dlogps).sum().backward()
    assert torch.equal(bits(hh.detach()), bits(h))  # the saved activation is not scaled in place
    bl = 2 * rel_err(emul[0], want[0]).max().item()
    el = rel_err(logps.detach(), want[0]).max().item()
    report("lm_head_seq_logps logps", el, bl)
    assert bl > 0 and el <= bl
    assert logps[1].item() == 0.0                   # every label ignored
    c = cu.tolist()
    splits = c                                      # one row block per sequence, and the pad rows
    bh = 2 * torch.cat([block_rel_err(emul[1][a:b], want[1][a:b], b - a, 64, want[1].pow(2).mean().sqrt())
                        for a, b in zip(c[:-1], c[1:])]).max().item()
    eh = assert_blocks_close(hh.grad, want[1], 0, 64, bh, "dh", row_splits=splits)
    report("lm_head_seq_logps dh (per sequence x 64 columns)", eh, bh)
    bw = 2 * block_rel_err(emul[2], want[2], 32, 32).max().item()
    ew = assert_blocks_close(ww.grad, want[2], 32, 32, bw, "dW")
    report("lm_head_seq_logps dW (32 x 32 blocks)", ew, bw)
    assert not (hh.grad[c[2]:c[3]] != 0).any()      # dlogps == 0
    assert not (hh.grad[c[1]:c[2]] != 0).any()      # all labels ignored
    assert not bits(hh.grad[c[4]:]).any()           # pad rows: +0
    with torch.no_grad():                           # no gradient wanted: the same log-probs, nothing saved
        lp2, _ = ops.lm_head_seq_logps(h, w, labels, cu, n)
    assert torch.equal(bits(lp2), bits(logps.detach()))


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
    return dict(input_ids=ids, labels=labels, cu_seqlens=cu, position_ids=pos, max_seqlen=max(LENS), n_seqs=len(LENS))


COEF = [0.83, -1.21, 0.37, -0.55]  # fixed weights of the linear objective sum_s c_s logp_s


def _seq_run(model, batch, hip):
    os.environ["SFTAMD_DISABLE_HIP"] = "0" if hip else "1"  # (conftest restores the environment after the test)
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    logps, _ = model.sequence_logps(**batch)
    (logps * torch.tensor(COEF, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return logps.detach().double(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()
                                     if p.grad is not None}


@pytest.mark.parametrize("preset,lora", [("tiny-gpu", False), ("tiny-gpu-qwen3", False), ("tiny-gpu-mistral", False),
                                         ("tiny-gpu", True)])
def test_sequence_logps_hip_vs_reference(preset, lora):
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
    lp_hip, g_hip = _seq_run(m, batch, True)
    lp_ref, g_ref = _seq_run(m, batch, False)
    el = ((lp_hip - lp_ref).abs() / lp_ref.abs()).max().item()
    report(f"sequence_logps {preset}{' lora' if lora else ''} logps", el, 2e-2)
    assert el < 2e-2
    assert g_ref and set(g_ref) == set(g_hip)
    if lora:
        assert all(".lora." in n for n in g_ref)
    worst, name = 0.0, ""
    for n in g_ref:
        e = ((g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)).item()
        if e > worst:
            worst, name = e, n
    report(f"sequence_logps {preset}{' lora' if lora else ''} gradients (worst: {name})", worst, 5e-2)
    assert worst < 5e-2, (name, worst)


def test_sequence_logps_refuses_context_parallel():
    m = build_model(get_config("tiny-gpu"), device=DEV, dtype=BF16, seed=1)
    m.model.layers[0].self_attn.cp_group = object()
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.sequence_logps(**_model_batch(1024))


# ------------------------------------------------------------------------------------------------ trainer
def _token_pairs(n, vocab, seed=0):
    from llm_fine_tune_distributed_amd.data.dataset import TokenizedDataset
    g = torch.Generator().manual_seed(seed)
    seqs, starts = [], []
    for _ in range(n):
        p = torch.randint(3, vocab, (int(torch.randint(3, 9, (1,), generator=g)),), generator=g).tolist()
        for _ in range(2):
            seqs.append(p + torch.randint(3, vocab, (int(torch.randint(2, 12, (1,), generator=g)),), generator=g).tolist())
            starts.append(len(p))
    return TokenizedDataset.from_token_lists(seqs, starts)


@pytest.fixture(scope="module")
def dpo_run(tmp_path_factory):
    from llm_fine_tune_distributed_amd.train import DPOConfig, DPOTrainer
    out = str(tmp_path_factory.mktemp("dpo"))
    cfg = get_config("tiny-gpu")
    m = build_model(cfg, device=DEV, dtype=BF16, seed=0)
    ds = _token_pairs(8, cfg.vocab_size)
    a = DPOConfig(output_dir=out, per_device_train_batch_size=4, max_steps=6, learning_rate=1e-4, beta=BETA,
                  lr_scheduler_type="constant", logging_steps=1, jsonl_log=False, save_strategy="no")
    t = DPOTrainer(model=m, args=a, train_dataset=ds)
    _ext.ops().dispatch_trace(True)
    try:
        t.train()
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
    trace = {k: int(v) for k, v in (it.split("=") for it in _ext.ops().dispatch_trace_read().split(";") if it)}
    return [h for h in t.state.log_history if "loss" in h], trace, out


def test_dpo_trainer_dispatch_trace(dpo_run):
    _, trace, _ = dpo_run
    for k in ("pref.seq_logp", "pref.dpo_pair", "pref.scale_rows"):
        assert trace.get(k, 0) > 0, (k, sorted(trace))


def test_dpo_trainer_steps(dpo_run):
    logs, _, out = dpo_run
    assert len(logs) == 6
    losses = [h["loss"] for h in logs]
    assert all(math.isfinite(v) for v in losses), losses
    gap = abs(losses[0] - LN2)
    report("DPOTrainer first loss - ln 2", gap, 1e-2)
    assert gap < 1e-2
    for k in ("rewards/chosen", "rewards/rejected", "rewards/accuracies", "rewards/margins", "logps/chosen",
              "logps/rejected", "grad_norm", "learning_rate", "epoch", "num_tokens"):
        assert k in logs[-1], k
    assert len(glob.glob(os.path.join(out, "ref_logps-*.pt"))) == 1
