"""References for the per-row kernel tests (a helper module, not a conftest): for every op an fp64 reference and a
torch fp32 emulation that rounds where the kernel rounds, so that a test's bound is 2 x the emulation's own worst
per-row error against fp64 (the convention of _blockwise.swiglu_bwd_reference) and never a number read off the kernel.
Also the exact torch twin of the fused sampler's draw (csrc/sampler.hip). Everything runs on the tensors' device, so
the CPU tests (tests/test_rowwise_cpu.py) use the same functions as the GPU tests."""
import math

import torch

from _blockwise import block_rel_err
from llm_fine_tune_distributed_amd.ops import reference as ref

BF16 = torch.bfloat16


def row_bound(emul: torch.Tensor, want64: torch.Tensor, rms=None) -> float:
    """2 x the emulation's worst per-row error: the bound of a per-row check of [R, C] against ``want64``."""
    return 2 * block_rel_err(emul, want64, 1, want64.shape[1], rms).max().item()


def rel_elem_err(got: torch.Tensor, want64: torch.Tensor) -> float:
    """Worst element error relative to max(|want|, rms(want)): the 1 x 1 block metric, for short fp32 vectors."""
    flat = want64.reshape(1, -1)
    return block_rel_err(got.reshape(1, -1), flat, 1, 1).max().item() if flat.numel() else 0.0


# ------------------------------------------------------------------------------------------------ RMSNorm
def wave_sum_emul(sq: torch.Tensor) -> torch.Tensor:
    """fp32 sum over the last dimension of [M, H] (H % 8 == 0) in the order of a 64-lane wave that owns 16-byte
    vectors: lane l adds elements (l + 64 j) * 8 .. + 7 for j = 0, 1, .. one after another, then a butterfly over the
    lanes (xor 32, 16, .. 1)."""
    M, H = sq.shape
    nv = -(-H // 512)
    v = torch.nn.functional.pad(sq.float(), (0, nv * 512 - H)).view(M, nv, 64, 8)
    acc = torch.zeros(M, 64, dtype=torch.float32, device=sq.device)
    for j in range(nv):
        for i in range(8):
            acc = acc + v[:, j, :, i]
    lanes = torch.arange(64, device=sq.device)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def rmsnorm_fwd_refs(x, res, w, eps):
    """(h, y64, rstd64, y_emul, rstd_emul) of the fused residual add + RMSNorm forward on bf16 x / res / w.
    h = bf16(x + res) is exactly determined (one fp32 add of two bf16 values, one rounding) and is the input of the
    norm; the emulation is bf16(bf16(h * rstd) * w) with an fp32 rstd summed in wave order."""
    h = x if res is None else (x.float() + res.float()).to(BF16)
    h64 = h.double()
    rstd64 = torch.rsqrt(h64.pow(2).mean(-1) + eps)
    y64 = h64 * rstd64[:, None] * w.double()
    hf = h.float()
    H = h.shape[-1]
    rstd32 = torch.rsqrt(wave_sum_emul(hf * hf) / float(H) + torch.tensor(eps, dtype=torch.float32, device=x.device))
    y_emul = ((hf * rstd32[:, None]).to(BF16).float() * w.float()).to(BF16)
    return h, y64, rstd64, y_emul, rstd32


def rmsnorm_bwd_refs(dy, h, w, rstd, dres):
    """(dx64, dw64, dx_emul, dw_emul) of the RMSNorm backward given the forward's fp32 rstd: dx = rstd (dy w - n
    mean(dy w n)) + dres with n = h rstd, dW = sum over rows of dy n. The emulation does the same in fp32 and rounds dx
    once to bf16; its dW is the fp32 column sum of the fp32 products."""
    def run(ct):
        g, n, wf, r = dy.to(ct), h.to(ct), w.to(ct), rstd.to(ct)[:, None]
        nn = n * r
        dot = (g * wf * nn).sum(-1, keepdim=True) / h.shape[-1]
        dx = r * (g * wf - nn * dot)
        if dres is not None:
            dx = dx + dres.to(ct)
        return dx, (g * nn).sum(0)
    dx64, dw64 = run(torch.float64)
    dx32, dw32 = run(torch.float32)
    return dx64, dw64, dx32.to(BF16), dw32


# ------------------------------------------------------------------------------------------------ elementwise
def swiglu_fwd_refs(gu):
    """(want64, emul) of silu(gate) * up on the bf16 [M, 2 I] gate | up: fp32 g / (1 + exp(-g)) * u, one rounding."""
    g, u = gu.double().chunk(2, dim=-1)
    want = g / (1.0 + torch.exp(-g)) * u
    gf, uf = gu.float().chunk(2, dim=-1)
    return want, (gf / (1.0 + torch.exp(-gf)) * uf).to(BF16)


def rope_refs(qk, cos, sin, inverse):
    """(want64, emul) of rotate-half RoPE on bf16 qk [M, nh, D] with fp32 cos / sin [M, D / 2]: fp32 products and one
    rounding to bf16 in the emulation."""
    want = ref.apply_rope(qk.double(), cos.double(), sin.double(), inverse=inverse)
    return want, ref.apply_rope(qk.float(), cos, sin, inverse=inverse).to(BF16)


def embedding_bwd_refs(g, ids, dy):
    """(want64, emul) of g[id] += sum of the dy rows with that id, for a bf16 gradient g [V, H]: the emulation sums
    each id's rows one after another in fp32, adds the old row and rounds once."""
    want = g.double().index_add_(0, ids, dy.double())
    acc = torch.zeros(g.shape, dtype=torch.float32, device=g.device)
    for m in range(ids.numel()):  # sequential, as the kernel's run loop (the tests' M is below 100)
        acc[ids[m]] += dy[m].float()
    return want, (g.float() + acc).to(BF16)


def dropout_add_refs(a, b, p, seed):
    """(keep, want64, emul) of (a or 0) + keep * b / (1 - p) for bf16 [T, K] views: the mask is ref.dropout_keep of
    the element index t K + k, the emulation scales by fp32(1 / (1 - p)) in fp32 and rounds once."""
    T, K = b.shape
    p = min(max(float(p), 0.0), 0.999)
    idx = torch.arange(T * K, device=b.device, dtype=torch.int64).view(T, K)
    keep = ref.dropout_keep(idx, seed, p)
    want = torch.where(keep, b.double() / (1.0 - p), torch.zeros((), dtype=torch.float64, device=b.device))
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32, device=b.device)
    em = torch.where(keep, b.float() * scale, torch.zeros((), device=b.device))
    if a is not None:
        want, em = want + a.double(), em + a.float()
    return keep, want, em.to(BF16)


# ------------------------------------------------------------------------------------------------ optimizer
def strided_sum_emul(sq: torch.Tensor, lanes: int = 256) -> torch.Tensor:
    """fp32 sum of a flat fp32 tensor as ``lanes`` threads would take it: element i goes to lane i % lanes, every lane
    adds its elements one after another, then a pairwise tree over the lanes."""
    n = sq.numel()
    if n == 0:
        return torch.zeros((), dtype=torch.float32, device=sq.device)
    rows = -(-n // lanes)
    v = torch.nn.functional.pad(sq.float().reshape(-1), (0, rows * lanes - n)).view(rows, lanes)
    acc = torch.zeros(lanes, dtype=torch.float32, device=sq.device)
    for r in range(rows):
        acc = acc + v[r]
    while acc.numel() > 1:
        acc = acc[: acc.numel() // 2] + acc[acc.numel() // 2:]
    return acc[0]


def adamw_kernel_order(w, g, m, v, lr, b1, b2, eps, wd, bc1, bc2):
    """One AdamW step in fp32 torch, associated as csrc/optim.hip adam_elem writes it (and so differently from
    ref.adamw_: sqrt(v) * (1 / sqrt(bc2)) for sqrt(v / bc2), lr * (1 / bc1) * m / denom for (lr / bc1) * (m / denom),
    (omb2 * g) * g for omb2 * (g * g)). Returns (w, m, v) in fp32; no storage rounding."""
    def f(x):
        return torch.tensor(x, dtype=torch.float32, device=w.device)
    m = f(b1) * m + f(1.0 - b1) * g
    v = f(b2) * v + f(1.0 - b2) * g * g
    denom = v.sqrt() * f(1.0 / math.sqrt(bc2)) + f(eps)
    w = w * (1.0 - f(lr) * f(wd)) - f(lr) * f(1.0 / bc1) * m / denom
    return w, m, v


def fp32_tolerance(alt: torch.Tensor, want: torch.Tensor):
    """(rel, abs) such that |x - want| <= rel |want| + abs holds for an fp32 evaluation x in another association
    order: abs = 2^-22 max|want| (four half-ulps of the largest value: what the handful of roundings of a cancelling
    sum can leave behind), rel = 2 x what ``alt`` needs on top of abs, and never below 2^-21: two evaluations of an
    expression with at most four roundings on the way to each state (half an ulp each) can differ by four ulps."""
    a = 2.0 ** -22 * want.abs().max().item()
    need = ((alt.double() - want.double()).abs() - a).clamp_min(0) / want.double().abs().clamp_min(1e-300)
    return max(2 * need.max().item(), 2.0 ** -21), a


# ------------------------------------------------------------------------------------------------ decode attention
def decode_refs(q, K, V, scale):
    """(want64, emul) [nq, D] of one decode step: q bf16 [nq, D], K / V bf16 [L, nkv, D] (live rows only). The emulation
    takes scores, softmax and P.V in fp32 and rounds the output once to bf16."""
    nq, D = q.shape
    nkv = K.shape[1]

    def run(ct):
        qf = q.to(ct).view(nkv, nq // nkv, D)
        att = torch.einsum("grd,sgd->grs", qf, K.to(ct)) * scale
        return torch.einsum("grs,sgd->grd", att.softmax(-1), V.to(ct)).reshape(nq, D)
    return run(torch.float64), run(torch.float32).to(BF16)


# ------------------------------------------------------------------------------------------------ LoRA adapter gradients
def lora_adapter_grad_refs(x, dy, As, Bs, meta, s, ct=torch.float64, rounding=False):
    """(dAs, dBs) of the wide LoRA backward (ops.fused._lora_wide_bwd, dropout 0) for bf16 x [T, K], dy [T, n], adapters
    A_i [r, K], B_i [rows_i, r] of the sub-projection at dy's columns [o_i, o_i + rows_i) (``meta`` [(o, rows, c)]) and
    the scale s: dB_i = dy_i^T (s x A_i^T), dA_i = (s dy_i B_i)^T x. ``ct`` fp64 without rounding is the reference;
    fp32 with ``rounding`` rounds where the kernels of csrc/lora.hip (and their torch twins on the shapes the kernels
    do not take) round: the adapter columns s x A^T of the widened activation are bf16 (fwd_kernel's store, l. 205;
    ops.reference.lora_fwd), dxa = s dy B is bf16 (dxa_kernel l. 719, dxa_finish_kernel l. 829; torch.addmm in bf16),
    the two token reductions are fp32 sums of bf16 products (tsum_kernel) and each gradient is rounded once to the
    parameter's bf16 (grad_out_kernel l. 472; ops.fused._accumulate_small_grad)."""
    r = (lambda t: t.to(BF16).to(ct)) if rounding else (lambda t: t)
    xc, dyc = x.to(ct), dy.to(ct)
    dAs, dBs = [], []
    for A, B, (o, rows, _) in zip(As, Bs, meta):
        xa = r((xc @ A.to(ct).t()) * s)
        dxa = r((dyc[:, o:o + rows] @ B.to(ct)) * s)
        dBs.append(r(dyc[:, o:o + rows].t() @ xa))
        dAs.append(r(dxa.t() @ xc))
    return dAs, dBs


# ------------------------------------------------------------------------------------------------ sampler twin
SKIP_EPS = 1e-4  # ~30 x the fp32 error of a <= 64-term softmax with native exp at |x| <= 20


def penalised_scaled(logits: torch.Tensor, present: torch.Tensor, temperature: float, penalty: float,
                     do_sample: bool = True) -> torch.Tensor:
    """The fp32 keys the sampler sorts: x * penalty (x < 0) or x / penalty for the tokens of the history, then
    x * fp32(1 / T) when sampling, with the kernel's single fp32 operations (a true division: the divisor is a tensor)."""
    x = logits.float()
    if penalty != 1.0:
        pen = torch.full_like(x, penalty)
        x = torch.where(present, torch.where(x < 0, x * pen, x / pen), x)
    if do_sample:
        x = x * torch.full_like(x, 1.0 / max(temperature, 1e-5))
    return x


def sampler_twin(logits: torch.Tensor, present: torch.Tensor, step: int, seed: int, temperature: float, top_k: int,
                 top_p: float, penalty: float):
    """The token csrc/sampler.hip draws at ``step`` from one row of logits (fp32 or bf16) whose history is the bool mask
    ``present`` [V], and whether the step is too close to call: (token, ambiguous, support). Keys in fp32 as the kernel
    forms them, top K by a stable descending sort (ties: lowest index first), softmax over the K in fp64, final_body's
    top-p rule (rank r is kept while the mass ranked above it is <= top_p), u = ((hash >> 8) + 0.5) / 2^24 * kept and
    the first rank whose cumulative mass reaches u. ``ambiguous``: u within SKIP_EPS * kept of a cumulative boundary
    or a rank's mass-above within SKIP_EPS of top_p, where the kernel's fp32 native exp may decide otherwise.
    ``support`` is the list of kept tokens."""
    x = penalised_scaled(logits, present, temperature, penalty)
    # the first K of a stable descending sort of the whole row, without sorting it: everything >= the K-th largest
    # value, in index order, sorted stably
    cand = (x >= torch.topk(x, top_k).values[-1]).nonzero().squeeze(1)
    sv, order = torch.sort(x[cand], descending=True, stable=True)
    sv, si = sv[:top_k].double(), cand[order[:top_k]]
    p = torch.exp(sv - sv[0])
    p = p / p.sum()
    above = torch.cumsum(p, 0) - p  # mass ranked above rank r
    keep = above <= top_p
    keep[0] = True
    n = int(keep.to(torch.int64).cumprod(0).sum())  # the kernel stops at the first rank that fails
    ambiguous = bool(((above[1:] - top_p).abs() < SKIP_EPS).any())
    cum = torch.cumsum(p[:n], 0)
    kept = cum[-1].item()
    h = int(ref.hash_u32(torch.tensor(int(step), dtype=torch.int64), seed))
    u = ((h >> 8) + 0.5) / 16777216.0 * kept
    hit = (cum >= u).nonzero()
    r = int(hit[0]) if hit.numel() else n - 1
    ambiguous = ambiguous or bool(((cum - u).abs() < SKIP_EPS * kept).any())
    return int(si[r]), ambiguous, si[:n].tolist()


def history_mask(V: int, history) -> torch.Tensor:
    m = torch.zeros(V, dtype=torch.bool)
    m[torch.as_tensor(list(history), dtype=torch.long)] = True
    return m


def sampler_logits(steps: int, V: int, history, seed: int = 1234, rows: int = 0) -> torch.Tensor:
    """Fresh fp32 logits for every step from a CPU generator: randn * 2, the history tokens raised by 3 (so that the
    penalised tokens compete). [steps, V], or [steps, rows, V] with ``history`` a list per row."""
    g = torch.Generator().manual_seed(seed)
    if rows:
        lg = torch.randn(steps, rows, V, generator=g) * 2
        for b, h in enumerate(history):
            lg[:, b, list(h)] += 3.0
    else:
        lg = torch.randn(steps, V, generator=g) * 2
        lg[:, list(history)] += 3.0
    return lg


def twin_run(logits: torch.Tensor, history, seed: int, temperature, top_k, top_p, penalty, forced=None):
    """The twin over logits [steps, V] on the CPU: (tokens, ambiguous flags). The history grows by the drawn token
    each step, or by ``forced[t]`` (the kernel's own log) when given, so that one close call does not change the
    steps after it."""
    V = logits.shape[1]
    present = history_mask(V, history)
    toks, amb = [], []
    for t in range(logits.shape[0]):
        tok, a, _ = sampler_twin(logits[t], present, t, seed, temperature, top_k, top_p, penalty)
        toks.append(tok)
        amb.append(a)
        present[forced[t] if forced is not None else tok] = True
    return toks, amb
