"""Common-mode attention inputs, the fp64 reference, a torch emulation of the flash kernels' arithmetic and the metrics
of the common-mode tests (a helper module, not a conftest).

Every attention test before these drew q, k and v i.i.d. N(0, 1): nothing is common to all tokens, and an attention
backward whose delta is off stays far below the per-block bounds. ``common_mode_inputs`` adds one fixed direction per
head to every token's q and k (what a large q / k bias does), ``emulate`` computes what the kernels of
csrc/attention.hip compute with their rounding points, from the inputs alone, so that a test's bound is 2 x the
emulation's own value of the same metric against fp64 (the convention of _rowwise.py), and ``metrics`` judges a result
four ways: per (sequence, head) block, as token-reduced products X^T dq / X^T dk per head (what a weight or bias
gradient sees: an error with the same direction in every row adds up coherently there, the signal does not), and by the
exact invariant sum_j dk_j = 0 per (sequence, kv head) (the rows of dS sum to zero). Everything runs on the tensors'
device, so tests/test_attn_emul_cpu.py uses the same functions as the GPU tests."""
import math

import torch

from _blockwise import block_rel_err
from llm_fine_tune_distributed_amd.ops import reference as ref

D = 128
BF16 = torch.bfloat16
INPUTS = [(1.0, 0.0), (1.0, 4.0), (0.25, 2.0), (1.0, 16.0)]  # (noise, common)
# (noise, common, v_common): the four above, and a common part of v (a v bias) with only a mild one in q and k. delta
# cancels dO . (the common part of v) out of dP, so the rounding of O, which is relative to ALL of O, is large against
# what is left: the case a bias layer of a model is in (tests/test_qwen2_gpu.py), which the four do not reach
INPUTS_V = [(n, c, 0.0) for n, c in INPUTS] + [(1.0, 1.0, 4.0)]


def cu_of(lens, device):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=device)


def common_mode_inputs(lens, nq, nkv, noise, common, seed, device, v_common=0.0):
    """(qkv [M, (nq + 2 nkv) * 128], dout [M, nq * 128]) in bf16: q_h = noise N(0, 1) + common c_h with one fixed
    c_h ~ N(0, 1)^128 per q head, k the same per kv head, v = N(0, 1) + v_common c_v per kv head and dout N(0, 1).
    Drawn from a CPU generator, so the CPU and the GPU tests see the same numbers."""
    g = torch.Generator().manual_seed(seed)
    M = sum(lens)
    x = torch.randn(M, nq + 2 * nkv, D, generator=g)
    c = torch.randn(nq + nkv, D, generator=g)
    x[:, :nq + nkv] = noise * x[:, :nq + nkv] + common * c[None]
    dout = torch.randn(M, nq * D, generator=g)
    if v_common:
        x[:, nq + nkv:] += v_common * torch.randn(nkv, D, generator=g)[None]
    return x.reshape(M, -1).to(BF16).to(device), dout.to(BF16).to(device)


def reference64(qkv, dout, cu, nq, nkv, scale, causal):
    """(out, dqkv) in fp64: ops.reference.attention on the bf16 inputs taken to fp64, and autograd."""
    q64 = qkv.double().requires_grad_(True)
    o64 = ref.attention(q64, nq, nkv, D, cu, scale, causal)
    (g64,) = torch.autograd.grad(o64, q64, dout.double())
    return o64.detach(), g64


def exact_delta(dout, o64, nq):
    """fp32 [nq, M] rowsum(dO . O) per head with the fp64 attention output: the delta flash_bwd takes as an argument."""
    M = dout.shape[0]
    return (dout.double() * o64).view(M, nq, D).sum(-1).t().contiguous().float()


THR = 8.0  # csrc/attention.hip THR (l. 120): the forward's deferred rescale threshold, log2 domain


def _deferred_max_p(raw, scale):
    """The forward's unnormalised P as fwd32_step forms it (csrc/attention.hip l. 322-349), for masked raw scores
    [heads, T, T] (-inf where invisible): per 64-key tile, P = exp2(s sl2 - m) with the wave's DEFERRED running max m
    (log2 domain, sl2 = scale log2 e): a wave is 32 consecutive queries of one head, m starts at -1e30 and every lane
    takes m = max(m, tile max) only on a tile where some lane of the wave has tile max > m + THR (l. 329-337). P is
    rounded to bf16 at that scale, so which m a tile was exponentiated with decides the rounding. Returns (P, w, m):
    w = exp2(m_tile - m_final) per element, the factor the later rescales put on the tile's contribution to O and l
    (l. 332-335), and the final m [heads, T, 1]."""
    H, T, _ = raw.shape
    sl2 = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)).item()
    nt, nb = -(-T // 64), -(-T // 32)
    tm = torch.nn.functional.pad(raw, (0, nt * 64 - T, 0, nb * 32 - T), value=float("-inf"))
    tm = tm.view(H, nb, 32, nt, 64).amax(-1) * sl2                      # [H, wave, lane, tile]
    m = torch.full((H, nb, 32), -1e30, dtype=raw.dtype, device=raw.device)
    used = []
    for kt in range(nt):
        trig = (tm[..., kt] > m + THR).any(-1, keepdim=True)
        m = torch.where(trig, torch.maximum(m, tm[..., kt]), m)
        used.append(m)
    used = torch.stack(used, -1).view(H, nb * 32, nt)[:, :T]             # m at the time of each tile
    mfin = m.view(H, nb * 32, 1)[:, :T]
    tile = torch.arange(T, device=raw.device) // 64
    mk = used[:, :, tile]                                               # [H, T, T]: the m of each key's tile
    p = torch.exp2(raw * sl2 - mk)                                      # masked: exp2(-inf) = 0
    return p, torch.exp2(mk - mfin), mfin


def emulate(qkv, dout, cu, nq, nkv, scale, causal, delta="kernel", o64=None, rounding=True, ds_fault=None):
    """(out, lse, dqkv, delta) as flash_fwd / flash_bwd of csrc/attention.hip compute them, in torch fp32 with the
    kernels' rounding points (line numbers of csrc/attention.hip):

    * scores: bf16 q . k with fp32 accumulation, unscaled; ``scale`` enters the forward only inside the exponent
      (sl2 = scale log2 e, l. 931, 343-344) and the backward inside the exponent of P (l. 980, 506, 706) and as one fp32
      factor on the dq / dk accumulators at their store (dq32 l. 637-643, dq3 l. 530 with store4 l. 76-81, dK l. 878-884;
      dV is stored unscaled, l. 885);
    * forward: p = exp2(s sl2 - m) and the row sum l stay fp32 (l. 343-350); P is rounded to bf16 only as the operand
      of O += P V (pack8, l. 354); O / l is rounded once to bf16 at the store (l. 422-423, store_t21 l. 273-276); lse =
      m + log l is fp32 (l. 424);
    * delta = fp32 rowsum(bf16 dO . bf16 O) (delta_kernel l. 94-98, 105), or what the caller hands over;
    * dK / dV (dkdv32_step): P = exp(s scale - lse) in fp32 from the fp32 lse (l. 706), dS = P (dP - delta) in fp32
      (l. 707); dS is rounded to bf16 ONCE (pack8w, l. 726) and those bits are both the dK operand (l. 734, 739) and the
      materialised dS^T that bwd_dq32 reads (l. 727-732; dq32 l. 578-581); P is rounded to bf16 for dV (pack8, l. 734,
      738); dK, dV accumulate in fp32 and round once at the store;
    * the bwd_dq3 recompute path forms the same fp32 P and dS (l. 506, 511) and rounds dS to bf16 (pack_acc, l. 515,
      66-69): the two dQ routes round the same quantity, so one emulation serves both.

    The forward's P is rounded at the scale of the wave's deferred running max, not of the row max (_deferred_max_p:
    with another m the same P rounds to other bf16 values, O's error changes, and with it delta's); the emulation sums
    in torch's order and takes exp / log from torch: the 2 x of the bounds covers those.

    ``delta``: "kernel" (from the emulated bf16 O), "exact" (from ``o64``, the fp64 output) or an fp32 [nq, M] tensor.
    ``rounding=False`` switches every rounding off (the structure check against fp64; run it on fp64 inputs to take
    the fp32 arithmetic out as well). ``ds_fault(b, dS, P, dP, delta_b)`` -> dS replaces dS of sequence b ([nq, T, T],
    query x key): only for planting faults in tests of the metrics. Uses the inputs and ``o64`` alone."""
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    r = (lambda t: t.to(BF16).to(ct)) if rounding else (lambda t: t)
    M, rep = qkv.shape[0], nq // nkv
    x = qkv.to(ct).view(M, nq + 2 * nkv, D)
    do = dout.to(ct).view(M, nq, D)
    out = torch.zeros(M, nq, D, dtype=ct, device=qkv.device)
    lse = torch.zeros(nq, M, dtype=ct, device=qkv.device)
    dqkv = torch.zeros(M, nq + 2 * nkv, D, dtype=ct, device=qkv.device)
    cul = [int(v) for v in cu.tolist()]
    seqs = []
    for b in range(len(cul) - 1):
        s, e = cul[b], cul[b + 1]
        if e <= s:
            continue
        T = e - s
        q = x[s:e, :nq].transpose(0, 1)                                       # [nq, T, D]
        k = x[s:e, nq:nq + nkv].transpose(0, 1).repeat_interleave(rep, 0)
        v = x[s:e, nq + nkv:].transpose(0, 1).repeat_interleave(rep, 0)
        raw = q @ k.transpose(-1, -2)
        vis = torch.ones(T, T, dtype=torch.bool, device=qkv.device)
        sc = (raw * scale).masked_fill(~(vis.tril() if causal else vis), float("-inf"))
        if rounding:
            p, w, m = _deferred_max_p(raw.masked_fill(torch.isinf(sc), float("-inf")), scale)
            l = (p * w).sum(-1, keepdim=True)
            out[s:e] = r(((r(p) * w) @ v) / l).transpose(0, 1)
            lse[:, s:e] = ((m + torch.log2(l)) * math.log(2.0)).squeeze(-1)
        else:
            m = sc.amax(-1, keepdim=True)
            p = torch.exp(sc - m)
            l = p.sum(-1, keepdim=True)
            out[s:e] = ((p @ v) / l).transpose(0, 1)
            lse[:, s:e] = (m + torch.log(l)).squeeze(-1)
        seqs.append((s, e, q, k, v, sc))
    if isinstance(delta, str):
        if delta == "kernel":
            dl = (do * out).sum(-1).t()
        else:
            assert delta == "exact" and o64 is not None
            dl = exact_delta(dout, o64, nq).to(ct)
    else:
        assert delta.shape == (nq, M), delta.shape
        dl = delta.to(ct)
    for b, (s, e, q, k, v, sc) in enumerate(seqs):
        g = do[s:e].transpose(0, 1)
        P = torch.exp(sc - lse[:, s:e, None])
        dP = g @ v.transpose(-1, -2)
        dS = P * (dP - dl[:, s:e, None])
        if ds_fault is not None:
            dS = ds_fault(b, dS, P, dP, dl[:, s:e])
        dSb, Pb = r(dS), r(P)
        T = e - s
        dqkv[s:e, :nq] = ((dSb @ k) * scale).transpose(0, 1)
        dqkv[s:e, nq:nq + nkv] = ((dSb.transpose(-1, -2) @ q) * scale).view(nkv, rep, T, D).sum(1).transpose(0, 1)
        dqkv[s:e, nq + nkv:] = (Pb.transpose(-1, -2) @ g).view(nkv, rep, T, D).sum(1).transpose(0, 1)
    o2, g2 = out.reshape(M, nq * D), dqkv.reshape(M, -1)
    if rounding:
        o2, g2 = o2.to(BF16), g2.to(BF16)
    return o2, lse.float() if rounding else lse, g2, dl.float() if rounding else dl


# ------------------------------------------------------------------------------------------------ metrics
def token_matrix(M, device, seed=77):
    """The fixed fp64 X [M, 32] of the token-reduced metric: column 0 is ones (X^T dq is then the bias gradient), the
    rest N(0, 1)."""
    X = torch.randn(M, 32, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    X[:, 0] = 1.0
    return X.to(device)


def _per_seq(got, want, cu):
    """Worst (sequence, head) block error of [M, heads * 128] (the blocks of _blockwise.assert_blocks_close with
    row_splits: the floor is the rms of the whole reference)."""
    rms = want.double().pow(2).mean().sqrt()
    rs = [int(v) for v in cu.tolist()]
    assert rs[0] == 0 and rs[-1] == got.shape[0]
    return torch.cat([block_rel_err(got[s:t], want[s:t], t - s, D, rms) for s, t in zip(rs[:-1], rs[1:]) if t > s])


def metrics(out, dqkv, o64, g64, cu, nq, nkv, X):
    """Every metric of the common-mode tests as {name: fp64 tensor of per-block values}, no sequence or head left out:

    * ``out``, ``dq``, ``dk``, ``dv``: per (sequence, head) block error [sequences, heads];
    * ``wq``, ``wk``: per head, the error of X^T dq_h / X^T dk_h [32, 128] against the same product of the fp64
      gradient (block_rel_err with 32 x 128 blocks) [1, heads];
    * ``bq``, ``bk``: the same for column 0 of X alone, the bias gradient sum_m dq[m] (1 x 128 blocks, against the
      floor of the whole product's rms: the exact sum_m dk[m] is zero) [1, heads];
    * ``inv``: per (sequence, kv head), rms over the 128 columns of sum_j dk_j divided by rms(dk64) sqrt(len) — the
      exact value is zero, so this is an error already [sequences, kv heads]."""
    cul = [int(v) for v in cu.tolist()]
    sl = {"dq": slice(0, nq * D), "dk": slice(nq * D, (nq + nkv) * D), "dv": slice((nq + nkv) * D, None)}
    res = {"out": _per_seq(out, o64, cu)}
    for name, s in sl.items():
        res[name] = _per_seq(dqkv[:, s], g64[:, s], cu)
    for name, s in (("q", sl["dq"]), ("k", sl["dk"])):
        got, want = X.t() @ dqkv[:, s].double(), X.t() @ g64[:, s]
        res["w" + name] = block_rel_err(got, want, 32, D)
        res["b" + name] = block_rel_err(got[:1], want[:1], 1, D, want.pow(2).mean().sqrt())
    dk, rms = dqkv[:, sl["dk"]].double(), g64[:, sl["dk"]].pow(2).mean().sqrt()
    inv = [dk[s:e].sum(0).view(nkv, D).pow(2).mean(-1).sqrt() / (rms * math.sqrt(e - s))
           for s, e in zip(cul[:-1], cul[1:]) if e > s]
    res["inv"] = torch.stack(inv)
    return res


BLOCKWISE = ("out", "dq", "dk", "dv", "wq", "wk", "bq", "bk")  # bounded by 2 x the emulation's worst block


def bounds_from(em: dict) -> dict:
    """2 x the emulation's own value of every metric: its worst block for the block metrics, per (sequence, kv head)
    for the invariant (a norm over 128 columns of a sum over the sequence's rows is concentrated, so the emulation's
    value of the same block is the yardstick; a sequence of one token is held to 1e-4 instead: its exact dk is zero
    and the emulation's may be exactly zero too)."""
    b = {k: 2 * em[k].max().item() for k in BLOCKWISE}
    b["inv"] = 2 * em["inv"]
    return b


def check(got: dict, bounds: dict, lens, what=None, floors=None) -> list:
    """The metrics of ``got`` over their bound, as [(name, value, bound)] (empty: all hold); with ``what`` every measured
    value is printed next to its bound. ``floors`` {name: bound} are fixed bounds that must ALSO hold (the suite's
    2e-2 / 3e-2 on i.i.d. inputs)."""
    lens = [l for l in lens if l > 0]
    one = torch.tensor([l == 1 for l in lens], device=got["inv"].device)[:, None]
    inv_bound = torch.where(one, torch.full_like(bounds["inv"], 1e-4), bounds["inv"])
    bad = []
    for k in BLOCKWISE:
        v = got[k].max().item()
        if what is not None:
            print(f"{what} {k}: {v:.3e} (bound {bounds[k]:.3e})")
        if not v <= bounds[k]:
            bad.append((k, v, bounds[k]))
        if floors and k in floors and not v <= floors[k]:
            bad.append((k + " fixed", v, floors[k]))
    if what is not None:
        for b in range(got["inv"].shape[0]):
            print(f"{what} inv seq {b} (len {lens[b]}): " + ", ".join(
                f"{v:.3e} (bound {w:.3e})" for v, w in zip(got["inv"][b].tolist(), inv_bound[b].tolist())))
    for b, h in torch.nonzero(~(got["inv"] <= inv_bound)).tolist():
        bad.append((f"inv seq {b} kv head {h}", got["inv"][b, h].item(), inv_bound[b, h].item()))
    return bad
