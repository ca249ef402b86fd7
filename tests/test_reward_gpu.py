"""Reward modelling on the GPU: the three kernels of csrc/reward.hip (seq_score_fwd, seq_score_bwd, reward_pair_fwd),
CausalLM.sequence_scores on the HIP path against the PyTorch reference path, RewardTrainer steps with the kernels'
dispatch trace and a reward model as a GRPO reward function.

Bounds follow tests/test_dpo_gpu.py: each is 2 x the worst error of the fp32 twin (ops/reference.py, the kernel's
expression and rounding points) against the same expression in fp64 on the same inputs, computed here from the
references alone; every test prints its worst measured error next to the bound (pytest -s); profiles/reward.md records
one run. dh and dw are promised bit-equal to their twins. The model test's gradient bound is the project's 5e-2 of
tests/test_dpo_gpu.py::test_sequence_logps_hip_vs_reference; its score bound is measured in the test."""
import dataclasses
import math
import os

import pytest
import torch

from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

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
    print(f"\n[reward] {what}: worst {worst:.3e} bound {bound:.3e}")


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


def trace_of(fn):
    _ext.ops().dispatch_trace(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _ext.ops().dispatch_trace(False)
    return out, {k: int(v) for k, v in (it.split("=") for it in _ext.ops().dispatch_trace_read().split(";") if it)}


# ------------------------------------------------------------------------------------------------ seq_score
SEQ_LENS = [1, 63, 64, 65, 129, 0, 1000]
SEQ_PAD = 7
# one active lane; 32 lanes; a lane with two chunks; the real width (four passes); a ragged last pass
WIDTHS = [8, 256, 520, 2048, 2056]
S = len(SEQ_LENS)


def _score_case(H, lens=SEQ_LENS, pad=SEQ_PAD):
    """h, w bf16 and cu. The elements of h carry a random power of two in 2^-6 .. 2^6: a product of two bf16 values
    has 16 significant bits, so sums of eight equal-sized ones would be exact in fp32 and the H = 8 bound vacuous.
    Drawn on the host, so the values (and whether the twin rounds) do not depend on the device's generator."""
    g = torch.Generator().manual_seed(H)
    M = sum(lens) + pad
    h = (torch.randn(M, H, generator=g) * torch.exp2(torch.randint(-6, 7, (M, H), generator=g).float())).to(BF16)
    w = (0.05 * torch.randn(H, generator=g)).to(BF16)
    return h.to(DEV), w.to(DEV), cu_of(lens, pad)


def _last_rows(lens):
    out, o = [], 0
    for n in lens:
        o += n
        if n:
            out.append(o - 1)
    return out


def _score_err(got, h, w, cu, n):
    """Per sequence |got - fp64| / sum_j |h_j w_j| over the last row (0 for an empty segment, which must score 0)."""
    want = ref.seq_score(h.double(), w.double(), cu, n)
    last, nonempty = ref._last_rows(h.shape[0], cu, n)
    scale = (h[last].double() * w.double()[None]).abs().sum(1)
    d = (got.double() - want).abs()
    return torch.where(nonempty, d / scale.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), d))


@pytest.mark.parametrize("H", WIDTHS)
def test_seq_score_fwd_against_fp64(H):
    h, w, cu = _score_case(H)
    got = _ext.ops().seq_score_fwd(h, w, cu, S)
    assert got.shape == (S,) and got.dtype == torch.float32 and torch.isfinite(got).all()
    twin = ref.seq_score(h, w, cu, S)
    bound = 2 * _score_err(twin, h, w, cu, S).max().item()
    worst = _score_err(got, h, w, cu, S).max().item()
    report(f"seq_score_fwd H={H}", worst, bound)
    assert bound > 0 and worst <= bound
    assert bits(got[5]).item() == 0                                                  # the empty segment: +0
    assert torch.equal(bits(got), bits(_ext.ops().seq_score_fwd(h, w, cu, S)))     # two calls: identical bits
    assert torch.equal(bits(got[:3]), bits(_ext.ops().seq_score_fwd(h, w, cu, 3)))  # later segments are ignored
    assert torch.equal(bits(ops.seq_score(h, w[None], cu, S)), bits(got))            # the op, with the [1, H] parameter


@pytest.mark.parametrize("H", [8, 520, 2056])
def test_seq_score_fwd_isolation(H):
    """Every row that is not a scored last row (the pad segment included) overwritten with 1e30, then NaN: the
    scores' bits do not move."""
    h, w, cu = _score_case(H)
    base = _ext.ops().seq_score_fwd(h, w, cu, S)
    keep = torch.zeros(h.shape[0], dtype=torch.bool, device=DEV)
    keep[_last_rows(SEQ_LENS)] = True
    for poison in (1e30, float("nan")):
        hp = torch.where(keep[:, None], h, torch.full_like(h, poison))
        got = _ext.ops().seq_score_fwd(hp, w, cu, S)
        assert torch.equal(bits(got), bits(base)), (poison, got, base)


def _g_case(n, seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    return torch.randn(n, generator=g, device=DEV) * 1.5  # mixed signs


@pytest.mark.parametrize("H", WIDTHS)
def test_seq_score_bwd_bits_and_bound(H):
    h, w, cu = _score_case(H)
    g = _g_case(S)
    g[5] = 1e30  # the empty segment's gradient must go nowhere
    (dh, dw), trace = trace_of(lambda: _ext.ops().seq_score_bwd(g, h, w, cu, S, True, True))
    assert trace == {"reward.seq_score_bwd": 1, "reward.seq_score_bwd.dh": 1, "reward.seq_score_bwd.dw": 1}, trace
    tdh, tdw = ref.seq_score_bwd(g, h, w, cu, S)
    assert dh.dtype == BF16 and dh.shape == h.shape and dw.dtype == torch.float32 and dw.shape == (H,)
    assert torch.equal(bits(dh), bits(tdh))      # every row: bit-equal to the twin
    last = _last_rows(SEQ_LENS)
    keep = torch.zeros(h.shape[0], dtype=torch.bool, device=DEV)
    keep[last] = True
    assert len(last) == 6 and not bits(dh[~keep]).any()   # exact +0 everywhere but the six last rows, pad rows included
    c = cu.tolist()
    assert torch.equal(bits(dh[c[5] - 1]), bits((g[4] * w.float()).to(BF16)))   # segment 4's last row: g_4 w, untouched
    assert torch.isfinite(dh.float()).all() and torch.isfinite(dw).all()
    assert torch.equal(bits(dw), bits(tdw))      # bit-equal to the twin
    _, want = ref.seq_score_bwd(g.double(), h.double(), w.double(), cu, S, need_dh=False)
    gs = g.double().clone()
    gs[5] = 0.0
    scale = (gs[[0, 1, 2, 3, 4, 6], None] * h[last].double()).abs().sum(0).clamp_min(1e-300)
    bound = 2 * ((tdw.double() - want).abs() / scale).max().item()
    worst = ((dw.double() - want).abs() / scale).max().item()
    report(f"seq_score_bwd dw H={H}", worst, bound)
    assert bound > 0 and worst <= bound
    dh2, dw2 = _ext.ops().seq_score_bwd(g, h, w, cu, S, True, True)
    assert torch.equal(bits(dh2), bits(dh)) and torch.equal(bits(dw2), bits(dw))   # two calls: identical bits
    # n_seqs = 3: segments past it receive nothing
    dh3, dw3 = _ext.ops().seq_score_bwd(g[:3].contiguous(), h, w, cu, 3, True, True)
    t3h, t3w = ref.seq_score_bwd(g[:3], h, w, cu, 3)
    assert torch.equal(bits(dh3), bits(t3h)) and torch.equal(bits(dw3), bits(t3w)) and not bits(dh3[c[3]:]).any()


def test_seq_score_bwd_halves_and_autograd():
    h, w, cu = _score_case(256)
    g = _g_case(S)
    (dh, dw), trace = trace_of(lambda: _ext.ops().seq_score_bwd(g, h, w, cu, S, False, True))
    assert dh is None and dw is not None and "reward.seq_score_bwd.dh" not in trace and trace["reward.seq_score_bwd.dw"] == 1
    (dh, dw), trace = trace_of(lambda: _ext.ops().seq_score_bwd(g, h, w, cu, S, True, False))
    assert dw is None and dh is not None and "reward.seq_score_bwd.dw" not in trace and trace["reward.seq_score_bwd.dh"] == 1
    (dh, dw), trace = trace_of(lambda: _ext.ops().seq_score_bwd(g, h, w, cu, S, False, False))
    assert dh is None and dw is None and not trace
    # the autograd Function honours needs_input_grad: a frozen head launches no dw half, a frozen trunk no dh half
    hh = h.clone().requires_grad_(True)
    _, trace = trace_of(lambda: (ops.seq_score(hh, w[None], cu, S) * g).sum().backward())
    assert "reward.seq_score_bwd.dw" not in trace and trace["reward.seq_score_bwd.dh"] == 1
    tdh, tdw = ref.seq_score_bwd(g, h, w, cu, S)
    assert torch.equal(bits(hh.grad), bits(tdh))
    ww = w[None].clone().requires_grad_(True)
    _, trace = trace_of(lambda: (ops.seq_score(h, ww, cu, S) * g).sum().backward())
    assert "reward.seq_score_bwd.dh" not in trace and trace["reward.seq_score_bwd.dw"] == 1
    assert ww.grad.shape == (1, 256) and torch.equal(bits(ww.grad), bits(tdw.to(BF16)[None]))
    # a main_grad slice receives dw directly and the use counter is decremented
    p = torch.nn.Parameter(w[None].clone())
    p.main_grad, p._sftamd_fresh, p._sftamd_remaining = torch.zeros_like(p), True, 1
    (ops.seq_score(h, p, cu, S) * g).sum().backward()
    assert p.grad is None and p._sftamd_remaining == 0 and torch.equal(bits(p.main_grad), bits(tdw.to(BF16)[None]))


@pytest.mark.parametrize("H", [8, 520])
def test_seq_score_many_short_sequences(H):
    """130 sequences of 1..3 rows: the wave-per-sequence grids end in a ragged block (130 = 32 x 4 + 2)."""
    lens = [1 + (i * 7) % 3 for i in range(130)]
    h, w, cu = _score_case(H, lens, 5)
    n = len(lens)
    got = _ext.ops().seq_score_fwd(h, w, cu, n)
    twin = ref.seq_score(h, w, cu, n)
    bound = 2 * _score_err(twin, h, w, cu, n).max().item()
    worst = _score_err(got, h, w, cu, n).max().item()
    report(f"seq_score_fwd S=130 H={H}", worst, bound)
    assert bound > 0 and worst <= bound
    g = _g_case(n, 1)
    dh, dw = _ext.ops().seq_score_bwd(g, h, w, cu, n, True, True)
    tdh, tdw = ref.seq_score_bwd(g, h, w, cu, n)
    assert torch.equal(bits(dh), bits(tdh)) and torch.equal(bits(dw), bits(tdw))


def test_seq_score_refusals():
    h, w, cu = _score_case(256)
    g = _g_case(S)
    o = _ext.ops()
    bad = (lambda: o.seq_score_fwd(h.float(), w, cu, S), lambda: o.seq_score_fwd(h, w.float(), cu, S),
           lambda: o.seq_score_fwd(h.cpu(), w, cu, S), lambda: o.seq_score_fwd(h, w, cu.cpu(), S),
           lambda: o.seq_score_fwd(h, w, cu.long(), S), lambda: o.seq_score_fwd(h[None], w, cu, S),
           lambda: o.seq_score_fwd(h.t(), w, cu, S), lambda: o.seq_score_fwd(h, w[:-8], cu, S),
           lambda: o.seq_score_fwd(h, w, cu, S + 2), lambda: o.seq_score_fwd(h, w, cu, -1),
           lambda: o.seq_score_fwd(h[:, :12].contiguous(), w[:12].contiguous(), cu, S),   # H % 8
           lambda: o.seq_score_bwd(g.double(), h, w, cu, S, True, True),
           lambda: o.seq_score_bwd(g[:-1].contiguous(), h, w, cu, S, True, True),
           lambda: o.seq_score_bwd(g.cpu(), h, w, cu, S, True, True),
           lambda: o.seq_score_bwd(g, h.float(), w, cu, S, True, True))
    for f in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            f()
    assert o.seq_score_fwd(h, w, cu, 0).shape == (0,)


# ------------------------------------------------------------------------------------------------ reward_pair_fwd
PAIR_P = [1, 3, 64, 65, 257]  # tests/test_dpo_gpu.py DPO_P
ZS = [0.0, 1e-3, -1e-3, 5.0, -5.0, 1e4, -1e4]
COEFS = [0.0, torch.tensor(0.01, dtype=torch.float32).item()]  # 0.01 as the fp32 the kernel receives


def _pair_case(P, with_margin):
    """(scores fp32 [2 P], margins fp32 [P] or None, the pairs whose z is exactly 0): pair p has r_c - r_r = ZS[p % 7]
    up to the rounding of the two scores (0 exactly: r_c == r_r), the pairs past the seven a random gap of a few
    units."""
    g = torch.Generator(device=DEV).manual_seed(P)
    rr = 3.0 * torch.randn(P, generator=g, device=DEV, dtype=torch.float64)
    d = 4.0 * torch.randn(P, generator=g, device=DEV, dtype=torch.float64)
    fixed = torch.tensor(ZS, dtype=torch.float64, device=DEV)
    k = min(P, len(ZS))
    sel = torch.arange(k, device=DEV) if P >= len(ZS) else torch.tensor([0, 5, 6][:k], device=DEV)
    d[:k] = fixed[sel]
    scores = torch.stack([rr + d, rr], 1).reshape(-1).float()
    margins = (2.0 * torch.rand(P, generator=g, device=DEV)) if with_margin else None
    zero = (d == 0) if not with_margin else torch.zeros(P, dtype=torch.bool, device=DEV)
    return scores, margins, zero


def _pair_bound():
    """2 x the worst relative error, over every case, of the fp32 twin against the same expression in fp64 on the same
    fp32 inputs: (loss bound, bound of both coefficients)."""
    wl = wc = 0.0
    for P in PAIR_P:
        for with_margin in (False, True):
            for c in COEFS:
                s, m, _ = _pair_case(P, with_margin)
                inv = torch.tensor([1.0 / P], dtype=torch.float32, device=DEV)
                e = ref.reward_pair(s, m, inv, c)
                w = ref.reward_pair(s.double(), None if m is None else m.double(), inv.double(), c)
                wl = max(wl, rel_err(e[0], w[0]).max().item())
                wc = max(wc, rel_err(e[1], w[1]).max().item(), rel_err(e[2], w[2]).max().item())
    return 2 * wl, 2 * wc


@pytest.fixture(scope="module")
def pair_bound():
    return _pair_bound()


@pytest.mark.parametrize("c", COEFS, ids=["c0", "c0.01"])
@pytest.mark.parametrize("with_margin", [False, True], ids=["plain", "margins"])
@pytest.mark.parametrize("P", PAIR_P)
def test_reward_pair_fwd(P, with_margin, c, pair_bound):
    bl, bc = pair_bound
    s, m, zero = _pair_case(P, with_margin)
    inv = torch.tensor([1.0 / P], dtype=torch.float32, device=DEV)
    st = _ext.ops().reward_pair_fwd(s, m, inv, c)
    assert st.shape == (4, P) and st.dtype == torch.float32
    assert torch.isfinite(st).all()
    w = ref.reward_pair(s.double(), None if m is None else m.double(), inv.double(), c)
    el = rel_err(st[0], w[0]).max().item()
    ec = max(rel_err(st[1], w[1]).max().item(), rel_err(st[2], w[2]).max().item())
    report(f"reward_pair_fwd P={P} margins={with_margin} c={c:g} loss", el, bl)
    report(f"reward_pair_fwd P={P} margins={with_margin} c={c:g} coefficients", ec, bc)
    assert 0 < bl < 1e-3 and 0 < bc < 1e-3 and el <= bl and ec <= bc
    z = s[0::2] - s[1::2]
    assert torch.equal(bits(st[3]), bits(z - m if with_margin else z))   # z: fp32 subtractions, exact
    assert torch.equal(bits(st), bits(_ext.ops().reward_pair_fwd(s, m, inv, c)))   # two calls: identical bits
    if c == 0.0:
        assert torch.equal(bits(st[2]), bits(-st[1]))                    # the exact negation, signed zeros included
        if not with_margin:
            assert bool(zero.any())
            ln2 = torch.tensor(LN2, dtype=torch.float32, device=DEV)
            l0 = st[0][zero]
            assert ((l0 >= torch.nextafter(ln2, ln2 - 1)) & (l0 <= torch.nextafter(ln2, ln2 + 1))).all(), l0
            half = -0.5 * inv[0]
            c0 = st[1][zero]
            assert ((c0 >= torch.nextafter(half, half - 1)) & (c0 <= torch.nextafter(half, half + 1))).all(), (c0, half)


def test_reward_pair_loss_backward_and_refusals():
    P = 65
    s, m, _ = _pair_case(P, True)
    inv = torch.tensor([1.0 / P], dtype=torch.float32, device=DEV)
    for c in COEFS:
        x = s.clone().requires_grad_(True)
        (loss, st), trace = trace_of(lambda: ops.reward_pair_loss(x, m, inv, c))
        assert trace == {"reward.pair": 1}
        assert abs(loss.item() - st[0].double().sum().item() / P) <= 1e-6 * abs(loss.item())
        loss.backward()
        assert torch.equal(bits(x.grad[0::2]), bits(st[1])) and torch.equal(bits(x.grad[1::2]), bits(st[2]))  # dloss = 1
    o = _ext.ops()
    for bad in (lambda: o.reward_pair_fwd(s.double(), m, inv, 0.0), lambda: o.reward_pair_fwd(s[:-1], m, inv, 0.0),
                lambda: o.reward_pair_fwd(s, m[:-1], inv, 0.0), lambda: o.reward_pair_fwd(s, m.double(), inv, 0.0),
                lambda: o.reward_pair_fwd(s, m.cpu(), inv, 0.0), lambda: o.reward_pair_fwd(s, m, inv.cpu(), 0.0),
                lambda: o.reward_pair_fwd(s.cpu(), m, inv, 0.0), lambda: o.reward_pair_fwd(s.view(-1, 2), m, inv, 0.0)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            bad()
    assert o.reward_pair_fwd(s[:0], None, inv, 0.0).shape == (4, 0)


# ------------------------------------------------------------------------------------------------ model, HIP vs reference
# 32 sequences of 1 .. 129 tokens (1, 63, 66 and 129 among them) and a pad segment. The score bound below compares two
# maxima of bf16 rounding noise over the sequences. For two paths of EQUAL (normal) noise the ratio of two such maxima
# passes 2 with probability 0.12 over the 4 sequences of the DPO test's batch, so one of four cases would fail every
# other run for no reason; over 32 sequences the probability is 0.005
LENS = [1 + (37 * i) % 131 for i in range(32)]
ROWS = -(-(sum(LENS) + 1) // 256) * 256
COEF = [(-1.0) ** i * (0.3 + 0.11 * (i % 9)) for i in range(32)]  # fixed weights of the objective sum_s c_s score_s


def _model_batch(vocab):
    g = torch.Generator(device=DEV).manual_seed(3)
    ids = torch.randint(0, vocab, (ROWS,), generator=g, device=DEV)
    cu = cu_of(LENS, ROWS - sum(LENS))
    c = cu.tolist()
    pos = torch.cat([torch.arange(b - a, device=DEV) for a, b in zip(c[:-1], c[1:])])
    return dict(input_ids=ids, cu_seqlens=cu, position_ids=pos, max_seqlen=max(LENS), n_seqs=len(LENS))


def _score_run(model, batch, hip):
    os.environ["SFTAMD_DISABLE_HIP"] = "0" if hip else "1"  # (conftest restores the environment after the test)
    for p in model.parameters():
        p.grad = None
    model.reset_grad_use_counters()
    s = model.sequence_scores(**batch)
    (s * torch.tensor(COEF, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return s.detach().double(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()
                                 if p.grad is not None}


def _with_lora(m):
    from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora
    apply_lora(m, LoRAConfig(r=16, lora_alpha=32.0, lora_dropout=0.0))
    return m


@pytest.mark.parametrize("preset,lora", [("tiny-gpu", False), ("tiny-gpu-qwen3", False), ("tiny-gpu-mistral", False),
                                         ("tiny-gpu", True)])
def test_sequence_scores_hip_vs_reference(preset, lora):
    torch.manual_seed(0)
    cfg = dataclasses.replace(get_config(preset), num_labels=1)
    m = build_model(cfg, device=DEV, dtype=BF16, seed=1)
    f32 = build_model(cfg, device=DEV, dtype=torch.float32, seed=1)
    if lora:
        _with_lora(m)
        with torch.no_grad():  # B = 0 would make every A gradient zero
            for layer in m.model.layers:
                for fl in (*layer.self_attn.lora.values(), *layer.mlp.lora.values()):
                    for b in fl.B:
                        torch.nn.init.normal_(b, std=0.02)
    with torch.no_grad():  # the fp32 copy: the bf16 model's values, upcast
        f32.load_hf_state_dict({k: v.float() for k, v in m.hf_state_dict().items()})
        if lora:
            _with_lora(f32)
            src = {n: p for n, p in m.named_parameters() if ".lora." in n}
            for n, p in f32.named_parameters():
                if ".lora." in n:
                    p.copy_(src[n].float())
    m.train()
    f32.train()
    batch = _model_batch(cfg.vocab_size)
    s_hip, g_hip = _score_run(m, batch, True)
    s_ref, g_ref = _score_run(m, batch, False)
    s_f32, _ = _score_run(f32, batch, False)
    tag = f"sequence_scores {preset}{' lora' if lora else ''}"
    bound = 2 * (s_ref - s_f32).abs().max().item()  # the bf16 reference path's own distance from fp32
    worst = (s_hip - s_f32).abs().max().item()
    report(f"{tag} scores (|s - s_f32|)", worst, bound)
    assert bound > 0 and worst <= bound
    assert g_ref and set(g_ref) == set(g_hip)
    if lora:
        assert all(".lora." in n or n == "score" for n in g_ref) and "score" in g_ref
    bad, name = 0.0, ""
    for n in g_ref:
        e = ((g_hip[n] - g_ref[n]).norm() / (g_ref[n].norm() + 1e-12)).item()
        if e > bad:
            bad, name = e, n
    report(f"{tag} gradients (worst: {name})", bad, 5e-2)
    assert bad < 5e-2, (name, bad)
    # sequence_scores is ops.seq_score over the model's own trunk
    os.environ["SFTAMD_DISABLE_HIP"] = "0"
    m.eval()
    with torch.no_grad():
        (s, trace) = trace_of(lambda: m.sequence_scores(**batch))
        h, _, cu = m._hidden(batch["input_ids"], None, batch["cu_seqlens"], batch["max_seqlen"], batch["position_ids"],
                             False)
        assert trace.get("reward.seq_score") == 1
        assert torch.equal(bits(s), bits(ops.seq_score(h, m.score, cu, len(LENS))))


def test_reward_model_refusals_on_gpu():
    m = build_model(dataclasses.replace(get_config("tiny-gpu"), num_labels=1), device=DEV, dtype=BF16, seed=1)
    b = _model_batch(1024)
    with pytest.raises(RuntimeError, match="reward model"):
        m(b["input_ids"][None], labels=b["input_ids"][None])
    lm = build_model(get_config("tiny-gpu"), device=DEV, dtype=BF16, seed=1)
    with pytest.raises(RuntimeError, match="reward model"):
        lm.sequence_scores(**b)
    m.model.layers[0].self_attn.cp_group = object()
    with pytest.raises(NotImplementedError, match="context parallel"):
        m.sequence_scores(**b)


# ------------------------------------------------------------------------------------------------ trainers
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
def reward_run(tmp_path_factory):
    from llm_fine_tune_distributed_amd.train import RewardConfig, RewardTrainer
    out = str(tmp_path_factory.mktemp("reward"))
    cfg = dataclasses.replace(get_config("tiny-gpu"), num_labels=1)
    m = build_model(cfg, device=DEV, dtype=BF16, seed=0)
    ds = _token_pairs(8, cfg.vocab_size)
    a = RewardConfig(output_dir=out, per_device_train_batch_size=4, max_steps=6, learning_rate=1e-4,
                     center_rewards_coefficient=0.01, lr_scheduler_type="constant", logging_steps=1, jsonl_log=False,
                     save_strategy="no")
    t = RewardTrainer(model=m, args=a, train_dataset=ds, eval_dataset=ds)
    _, trace = trace_of(t.train)
    ev = t.evaluate()
    saved = os.path.join(out, "saved")
    t.save_model(saved)
    return [h for h in t.state.log_history if "loss" in h], trace, ev, saved, m


def test_reward_trainer_dispatch_trace(reward_run):
    _, trace, _, _, _ = reward_run
    for k in ("reward.seq_score", "reward.seq_score_bwd", "reward.seq_score_bwd.dh", "reward.seq_score_bwd.dw",
              "reward.pair"):
        assert trace.get(k, 0) >= 6, (k, sorted(trace))
    assert not any(k.startswith("ce.") or k.startswith("pref.") for k in trace), sorted(trace)  # no LM head, no CE


def test_reward_trainer_steps(reward_run):
    logs, _, ev, saved, m = reward_run
    assert len(logs) == 6
    assert all(math.isfinite(h["loss"]) for h in logs), [h["loss"] for h in logs]
    for k in ("loss", "accuracy", "margin", "mean_reward", "min_reward", "max_reward", "num_tokens", "grad_norm",
              "learning_rate", "epoch"):
        assert k in logs[-1] and math.isfinite(logs[-1][k]), k
    assert logs[-1]["min_reward"] <= logs[-1]["mean_reward"] <= logs[-1]["max_reward"]
    for k in ("eval_loss", "eval_accuracy", "eval_margin", "eval_mean_reward", "eval_min_reward", "eval_max_reward"):
        assert k in ev and math.isfinite(ev[k]), k
    from llm_fine_tune_distributed_amd.train import checkpoint as ckpt
    again = ckpt.from_pretrained(saved, device=DEV, dtype=BF16).eval()
    assert again.is_reward_model and torch.equal(bits(again.score), bits(m.score))
    b = _model_batch(1024)
    m.eval()
    with torch.no_grad():
        assert torch.equal(bits(again.sequence_scores(**b)), bits(m.sequence_scores(**b)))


def test_grpo_scores_completions_with_a_reward_model(tmp_path):
    from llm_fine_tune_distributed_amd.train import GRPOConfig, GRPOTrainer
    cfg = get_config("tiny-gpu")
    policy = build_model(cfg, device=DEV, dtype=BF16, seed=0)
    rm = build_model(dataclasses.replace(cfg, num_labels=1), device=DEV, dtype=BF16, seed=5)
    g = torch.Generator().manual_seed(0)
    ds = [{"prompt_ids": torch.randint(3, cfg.vocab_size, (int(n),), generator=g).tolist()} for n in (4, 9, 6, 12)]
    a = GRPOConfig(output_dir=str(tmp_path), per_device_train_batch_size=8, num_generations=4, max_completion_length=8,
                   temperature=0.9, max_steps=2, learning_rate=1e-4, lr_scheduler_type="constant", logging_steps=1,
                   jsonl_log=False, save_strategy="no")
    t = GRPOTrainer(model=policy, reward_funcs=[rm], args=a, train_dataset=ds)
    assert t.reward_names == ["CausalLM"] and not any(p.requires_grad for p in rm.parameters())
    assert not {id(p) for p in rm.parameters()} & set(t.engine.param_names)
    b = t._make_batch(0, 0, torch.tensor([0, 1]))
    rows = [ds[i] for i in (0, 1) for _ in range(4)]
    (per_fn, trace) = trace_of(lambda: t._rewards(rows, b["completion_ids"]))
    assert trace.get("reward.seq_score") == 1 and per_fn.dtype == torch.float64 and per_fn.shape == (1, 8)
    with torch.no_grad():  # the policy batch is the same padding-free layout: prompt + completion, pad segment last
        want = rm.sequence_scores(b["input_ids"], cu_seqlens=b["cu_seqlens"], position_ids=b["position_ids"],
                                  max_seqlen=b["max_seqlen"], n_seqs=8)
    assert torch.equal(per_fn[0], want.double().cpu())   # bit for bit
    assert torch.equal(b["rewards"].double(), per_fn[0].float().double())
    t.train()
    torch.cuda.synchronize()
    logs = [h for h in t.state.log_history if "loss" in h]
    assert len(logs) == 2 and all(math.isfinite(h["loss"]) and "rewards/CausalLM/mean" in h for h in logs)
