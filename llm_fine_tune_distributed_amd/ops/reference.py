"""Pure-PyTorch reference implementations of every fused op.

These run on CPU (tests, the gloo plumbing config of BASELINE.json) and serve as the fp32
numerics oracle for the HIP kernels. Semantics follow the HF modules the reference runs
(transformers ``modeling_smollm3.py``: RMSNorm, rotate_half RoPE, SwiGLU, causal GQA SDPA,
``loss_utils.py`` ForCausalLMLoss with ignore_index=-100 and sum/num_items normalisation).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

IGNORE_INDEX = -100


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (y, rstd). y = weight * x / sqrt(mean(x^2) + eps), computed in fp32."""
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    y = (xf * rstd).to(x.dtype) * weight
    return y, rstd.squeeze(-1)


def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    g, u = gate_up.chunk(2, dim=-1)
    return (F.silu(g.float()) * u.float()).to(gate_up.dtype)


def rope_cos_sin(positions: torch.Tensor, head_dim: int, theta: float,
                 scaling: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin tables [n, head_dim/2] in fp32 for the given integer positions."""
    inv_freq = rope_inv_freq(head_dim, theta, scaling, positions.device)
    freqs = positions.float()[:, None] * inv_freq[None, :]
    return freqs.cos(), freqs.sin()


def rope_inv_freq(head_dim: int, theta: float, scaling: Optional[dict], device=None) -> torch.Tensor:
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64, device=device) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo, hi = scaling.get("low_freq_factor", 1.0), scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        lo_wl, hi_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        scaled = torch.where(wl > lo_wl, inv / factor, inv)
        smooth = (old / wl - lo) / (hi - lo)
        mid = (1 - smooth) * scaled / factor + smooth * scaled
        is_mid = (wl <= lo_wl) & (wl >= hi_wl)
        inv = torch.where(is_mid, mid, scaled)
    return inv.float()


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """x [M, H, D]; cos/sin [M, D/2]. rotate_half convention (HF Llama/SmolLM3)."""
    d2 = x.shape[-1] // 2
    xf = x if x.dtype == torch.float64 else x.float()  # (fp64 stays fp64: gradient checks)
    x1, x2 = xf[..., :d2], xf[..., d2:]
    c, s = cos[:, None, :], sin[:, None, :]
    if inverse:
        s = -s
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    return torch.cat([o1, o2], dim=-1).to(x.dtype)


def _qk_weights(qw: torch.Tensor, kw: torch.Tensor, n_q: int, n_kv: int, dtype) -> torch.Tensor:
    """[n_q + n_kv, D]: the q_norm weight for the query heads, the k_norm weight for the key heads."""
    return torch.cat([qw.to(dtype).expand(n_q, -1), kw.to(dtype).expand(n_kv, -1)], 0)


def qk_norm_rope(qkv: torch.Tensor, qw: torch.Tensor, kw: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                 n_q: int, n_kv: int, head_dim: int, eps: float) -> torch.Tensor:
    """Per-head QK RMSNorm + RoPE on the packed qkv [M, (n_q + 2 n_kv) * D] (Qwen3): every q and k head row becomes
    rope(w * x * rsqrt(mean(x^2) + eps)) with w = qw [D] for the query heads and kw [D] for the key heads; the V
    columns pass through. Math in fp32 (fp64 for fp64 inputs), one rounding to the input dtype. Out of place and
    differentiable by autograd in qkv, qw and kw."""
    M, nh, D = qkv.shape[0], n_q + n_kv, head_dim
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    x = qkv[:, : nh * D].to(ct).view(M, nh, D)
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    n = x * rstd * _qk_weights(qw, kw, n_q, n_kv, ct)[None]
    y = apply_rope(n, cos.to(ct), sin.to(ct))
    return torch.cat([y.reshape(M, nh * D).to(qkv.dtype), qkv[:, nh * D:]], dim=-1)


def qk_norm_rope_bwd(dqkv: torch.Tensor, qk_raw: torch.Tensor, qw: torch.Tensor, kw: torch.Tensor, cos: torch.Tensor,
                     sin: torch.Tensor, n_q: int, n_kv: int, head_dim: int, eps: float):
    """Backward of qk_norm_rope in closed form (the math of csrc/qk_norm.hip): dqkv is the gradient w.r.t. the output,
    qk_raw [M, (n_q + n_kv) * D] the un-normalised q|k input. Returns (dx [M, (n_q + n_kv) * D] in dqkv's dtype,
    dq_weight [D], dk_weight [D]); the weight gradients are fp32 (fp64 for fp64 inputs)."""
    M, nh, D = dqkv.shape[0], n_q + n_kv, head_dim
    ct = torch.float64 if dqkv.dtype == torch.float64 else torch.float32
    x = qk_raw.to(ct).view(M, nh, D)
    g = apply_rope(dqkv[:, : nh * D].to(ct).view(M, nh, D), cos.to(ct), sin.to(ct), inverse=True)
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh = x * rstd
    gw = g * _qk_weights(qw, kw, n_q, n_kv, ct)[None]
    dx = rstd * (gw - xh * (gw * xh).mean(-1, keepdim=True))
    gx = g * xh
    return (dx.reshape(M, nh * D).to(dqkv.dtype), gx[:, :n_q].sum((0, 1)), gx[:, n_q:].sum((0, 1)))


def qkv_bias_rope(qkv: torch.Tensor, bias: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_q: int, n_kv: int,
                  head_dim: int) -> torch.Tensor:
    """q / k / v projection bias + RoPE on the packed qkv [M, (n_q + 2 n_kv) * D] (Qwen2): every q and k head row
    becomes rope(row + bias[head cols]), every v head row becomes row + bias[head cols]; bias [(n_q + 2 n_kv) * D].
    Math in fp32 (fp64 for fp64 inputs), one rounding to the input dtype. Out of place and differentiable by autograd
    in qkv and bias."""
    M, nh, D = qkv.shape[0], n_q + n_kv, head_dim
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    x = qkv.to(ct) + bias.to(ct)[None]
    y = apply_rope(x[:, : nh * D].view(M, nh, D), cos.to(ct), sin.to(ct))
    return torch.cat([y.reshape(M, nh * D), x[:, nh * D:]], dim=-1).to(qkv.dtype)


def attention(qkv: torch.Tensor, n_q: int, n_kv: int, head_dim: int, cu_seqlens: torch.Tensor,
              scale: Optional[float] = None, causal: bool = True, window: int = 0) -> torch.Tensor:
    """Varlen causal GQA attention on the packed qkv layout [M, (n_q+2n_kv)*D] -> [M, n_q*D]. Math in fp32 (fp64 for
    fp64 inputs: the tests' reference), one rounding to the input dtype. ``window`` W > 0 is a sliding window: the
    query at position i of its sequence sees the keys j with i - W < j <= i (W keys, itself included; transformers'
    ``sliding_window_overlay``); 0 is no window. A window requires ``causal``."""
    window = int(window or 0)
    if window < 0 or (window > 0 and not causal):
        raise ValueError(f"attention: window={window} needs window >= 0 and causal=True")
    scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    M = qkv.shape[0]
    q = qkv[:, : n_q * head_dim].view(M, n_q, head_dim)
    k = qkv[:, n_q * head_dim: (n_q + n_kv) * head_dim].view(M, n_kv, head_dim)
    v = qkv[:, (n_q + n_kv) * head_dim:].view(M, n_kv, head_dim)
    out = torch.empty(M, n_q, head_dim, dtype=qkv.dtype, device=qkv.device)
    rep = n_q // n_kv
    cu = cu_seqlens.tolist()
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        if e <= s:
            continue
        qi = q[s:e].to(ct).transpose(0, 1)  # [H, T, D]
        ki = k[s:e].to(ct).transpose(0, 1).repeat_interleave(rep, 0)
        vi = v[s:e].to(ct).transpose(0, 1).repeat_interleave(rep, 0)
        att = (qi @ ki.transpose(-1, -2)) * scale
        if causal:
            T = e - s
            mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
            if window > 0:
                mask &= ~torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril(-window)
            att = att.masked_fill(~mask, float("-inf"))
        p = att.softmax(-1)
        out[s:e] = (p @ vi).transpose(0, 1).to(qkv.dtype)
    if cu[-1] < M:  # tokens outside any sequence (should not happen) -> zeros
        out[cu[-1]:] = 0
    return out.view(M, n_q * head_dim)


def _at_temperature(lf: torch.Tensor, temperature: float) -> torch.Tensor:
    """x / tau as the kernel forms it: one fp32 product with the fp32 value of 1 / tau (tau 1: x itself)."""
    if float(temperature) == 1.0:
        return lf
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    return lf * torch.tensor(1.0 / float(temperature), dtype=torch.float32).item()


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, label_smoothing: float = 0.0, loss_mode: int = 0,
                  temperature: float = 1.0):
    """Per-token CE in fp32 (ignore_index=-100). Returns (loss_per_token, lse, argmax_correct, entropy).

    The per-token loss is the objective's (twin of csrc/cross_entropy.hip): ``lse - x_y`` by default,
    ``lse - (1 - e) x_y - e sum(x) / V`` with ``label_smoothing`` e (HF ``LabelSmoother``), ``p_y (lse - x_y)`` with
    ``loss_mode`` 1 (TRL ``dft_loss``; p_y is a constant of the gradient: see ``cross_entropy_grad``). A
    ``temperature`` tau != 1 makes every quantity that of softmax(x / tau) (plain NLL only)."""
    if float(temperature) != 1.0 and (label_smoothing > 0 or loss_mode != 0):
        raise ValueError("a temperature takes neither label smoothing nor dft")
    lf = _at_temperature(logits.float(), temperature)
    lse = torch.logsumexp(lf, dim=-1)
    valid = labels != IGNORE_INDEX
    safe = labels.clamp(min=0)
    tgt = lf.gather(-1, safe[:, None]).squeeze(-1)
    if loss_mode == 1:
        nll = lse - tgt
        loss = torch.where(valid, torch.exp(-nll) * nll, torch.zeros_like(lse))
    elif label_smoothing > 0:
        e = float(label_smoothing)
        loss = torch.where(valid, lse - (1.0 - e) * tgt - e * lf.mean(-1), torch.zeros_like(lse))
    else:
        loss = torch.where(valid, lse - tgt, torch.zeros_like(lse))
    p = torch.softmax(lf, -1)
    entropy = lse - (p * lf).sum(-1)
    correct = (lf.argmax(-1) == labels) & valid
    return loss, lse, correct, entropy


def cross_entropy_grad(logits: torch.Tensor, labels: torch.Tensor, scale: torch.Tensor, label_smoothing: float = 0.0,
                       loss_mode: int = 0, temperature: float = 1.0) -> torch.Tensor:
    """d(sum of the per-token objective of ``cross_entropy`` * scale) / dlogits in fp32, zero on ignored rows:
    (p - onehot) scale, (p - (1 - e) onehot - e / V) scale when smoothed, p_y (p - onehot) scale for dft. With a
    ``temperature`` tau, p = softmax(x / tau) and the chain rule's 1 / tau is NOT applied (the caller's row weight
    carries it, as csrc/cross_entropy.hip CE_TEMP leaves it)."""
    valid = labels != IGNORE_INDEX
    rows = torch.arange(logits.shape[0], device=logits.device)
    safe = labels.clamp(min=0)
    g = torch.softmax(_at_temperature(logits.float(), temperature), -1)
    rs = valid.float() * scale.float()
    if loss_mode == 1:
        rs = rs * g[rows, safe]
        g[rows, safe] -= 1.0
    elif label_smoothing > 0:
        e = float(label_smoothing)
        g[rows, safe] -= 1.0 - e
        g -= e / logits.shape[-1]
    else:
        g[rows, safe] -= 1.0
    g *= rs[:, None]
    return g


def _jsd_terms(student_logits: torch.Tensor, teacher_logits: torch.Tensor, beta: float, temperature: float):
    """(lp, lq, lm) of the generalized JSD: the two log-softmaxes at ``temperature`` and, for 0 < beta < 1, the
    mixture's log-probabilities logsumexp(lp + log(1 - beta), lq + log beta) (None at beta 0 or 1). fp64 for fp64
    student logits, fp32 otherwise."""
    dt = torch.float64 if student_logits.dtype == torch.float64 else torch.float32
    a = student_logits.to(dt) / float(temperature)
    b = teacher_logits.to(dt) / float(temperature)
    lp = a - torch.logsumexp(a, -1, keepdim=True)
    lq = b - torch.logsumexp(b, -1, keepdim=True)
    lm = None
    if 0.0 < beta < 1.0:
        lm = torch.logaddexp(lp + math.log1p(-beta), lq + math.log(beta))
    return lp, lq, lm


def generalized_jsd(student_logits: torch.Tensor, teacher_logits: torch.Tensor, labels: torch.Tensor,
                    beta: float = 0.5, temperature: float = 1.0):
    """Per-token generalized Jensen-Shannon divergence of TRL's ``GKDTrainer.generalized_jsd_loss`` (twin of
    csrc/distill.hip). ``labels`` are the rows' already shifted labels; a -100 row costs 0. With lp / lq the student's /
    teacher's log-softmax of logits / temperature and p, q their exponentials, per row:
    beta 0: sum q (lq - lp) = KL(teacher || student); beta 1: sum p (lp - lq) = KL(student || teacher); otherwise
    beta sum q (lq - lm) + (1 - beta) sum p (lp - lm) with lm = logsumexp(lp + log(1 - beta), lq + log beta). No tau^2
    factor (TRL has none). Returns (loss_per_token, student lse, teacher lse, student argmax == label, student argmax
    == teacher argmax), the last two False on ignored rows."""
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must be in [0, 1], got {beta}")
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    lp, lq, lm = _jsd_terms(student_logits, teacher_logits, beta, temperature)
    if beta == 0.0:
        loss = (lq.exp() * (lq - lp)).sum(-1)
    elif beta == 1.0:
        loss = (lp.exp() * (lp - lq)).sum(-1)
    else:
        loss = beta * (lq.exp() * (lq - lm)).sum(-1) + (1.0 - beta) * (lp.exp() * (lp - lm)).sum(-1)
    valid = labels != IGNORE_INDEX
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    dt = lp.dtype
    lse_s = torch.logsumexp(student_logits.to(dt) / float(temperature), -1)
    lse_t = torch.logsumexp(teacher_logits.to(dt) / float(temperature), -1)
    top = student_logits.argmax(-1)
    return loss, lse_s, lse_t, (top == labels) & valid, (top == teacher_logits.argmax(-1)) & valid


def generalized_jsd_grad(student_logits: torch.Tensor, teacher_logits: torch.Tensor, labels: torch.Tensor,
                         scale: torch.Tensor, beta: float = 0.5, temperature: float = 1.0) -> torch.Tensor:
    """d(sum of ``generalized_jsd``'s per-token loss * scale) / d student_logits, zero on ignored rows: with the names
    of ``generalized_jsd``, times scale / temperature, p - q at beta 0, p ((lp - lq) - L) at beta 1 and otherwise
    (1 - beta) p ((lp - lm) - K), K = sum p (lp - lm)."""
    beta = float(beta)
    lp, lq, lm = _jsd_terms(student_logits, teacher_logits, beta, temperature)
    p = lp.exp()
    if beta == 0.0:
        g = p - lq.exp()
    elif beta == 1.0:
        d = lp - lq
        g = p * (d - (p * d).sum(-1, keepdim=True))
    else:
        d = lp - lm
        g = (1.0 - beta) * p * (d - (p * d).sum(-1, keepdim=True))
    rs = (labels != IGNORE_INDEX).to(g.dtype) * (scale.to(g.dtype) / float(temperature))
    return g * rs[:, None]


def teacher_topk(logits: torch.Tensor, k: int, temperature: float = 1.0):
    """The k largest logits of every row as (int32 ids [M, k], log softmax(logits / temperature) at them [M, k], the
    lse taken over the whole row): value descending, equal values by column ascending (a stable descending sort; -0 = +0).
    Twin of csrc/distill_topk.hip teacher_topk; the log-probabilities are fp32 for logits below fp32, else the
    logits' dtype."""
    V = logits.shape[-1]
    if not 1 <= int(k) <= min(256, V):
        raise ValueError(f"k must be in 1 .. min(256, vocab={V}), got {k}")
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    x = logits.reshape(-1, V)
    x = x if x.dtype in (torch.float32, torch.float64) else x.float()
    vals, ids = torch.sort(x, dim=-1, descending=True, stable=True)
    a = x / float(temperature)
    lse = torch.logsumexp(a, -1, keepdim=True)
    ids = ids[:, :int(k)]
    return ids.to(torch.int32), a.gather(1, ids) - lse


def _topk_terms(student_logits, ids, logps, temperature):
    dt = student_logits.dtype if student_logits.dtype in (torch.float32, torch.float64) else torch.float32
    a = student_logits.to(dt) / float(temperature)
    lse = torch.logsumexp(a, -1)
    return a - lse[:, None], lse, ids.to(torch.int64), logps.to(dt)


def distill_topk(student_logits: torch.Tensor, ids: torch.Tensor, logps: torch.Tensor, labels: torch.Tensor,
                 temperature: float = 1.0):
    """Per-token forward KL of the student against a teacher truncated to its top-k support (twin of
    csrc/distill_topk.hip kd_topk_fwd): with lp the student's log-softmax of logits / temperature, the cached
    (id_k, tlp_k) of ``teacher_topk`` and p_k = e^tlp_k, L = sum_k p_k (tlp_k - lp[id_k]), not renormalised; at k = vocab
    it is ``generalized_jsd`` at beta 0. A -100 row costs 0. The ids of a row must be distinct and in [0, vocab).
    Returns (loss_per_token, student lse, the teacher mass kept m = sum_k p_k, student argmax == label, student argmax
    == ids[:, 0]), the last two False on ignored rows."""
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    lp, lse, idx, tlp = _topk_terms(student_logits, ids, logps, temperature)
    p = tlp.exp()
    loss = (p * (tlp - lp.gather(1, idx))).sum(-1)
    valid = labels != IGNORE_INDEX
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    top = student_logits.argmax(-1)
    return loss, lse, p.sum(-1), (top == labels) & valid, (top == idx[:, 0]) & valid


def distill_topk_grad(student_logits: torch.Tensor, ids: torch.Tensor, logps: torch.Tensor, labels: torch.Tensor,
                      scale: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """d(sum of ``distill_topk``'s per-token loss * scale) / d student_logits, zero on ignored rows:
    (m softmax_j - sum_k [id_k = j] p_k) * scale / temperature."""
    lp, _, idx, tlp = _topk_terms(student_logits, ids, logps, temperature)
    p = tlp.exp()
    g = p.sum(-1, keepdim=True) * lp.exp()
    g = g.scatter_add(1, idx, -p)
    rs = (labels != IGNORE_INDEX).to(g.dtype) * (scale.to(g.dtype) / float(temperature))
    return g * rs[:, None]


def embedding_noise_u(idx: torch.Tensor, seed: int) -> torch.Tensor:
    """The NEFTune uniform of element index ``idx`` (int64): (2 (hash_u32 >> 9) + 1 - 2^23) 2^-23 in fp32 — the odd
    integers of (-2^23, 2^23) scaled by 2^-23: exact, symmetric about 0, never 0 or +-1 (twin of
    csrc/elementwise.hip embedding_noise_fwd_kernel)."""
    k = 2 * (hash_u32(idx, seed) >> 9) + 1 - (1 << 23)
    return k.to(torch.float32) * (2.0 ** -23)


def embedding_noise(ids: torch.Tensor, weight: torch.Tensor, mag: torch.Tensor, seed: int) -> torch.Tensor:
    """weight[ids] + mag[m] * u(m * H + c, seed), bit-equal to the HIP kernel on bf16 weights: one fp32 product, one
    fp32 sum, one rounding to the weight's dtype. ``mag`` is fp32 with one value per token."""
    H = weight.shape[1]
    flat = ids.reshape(-1)
    M = flat.numel()
    idx = torch.arange(M * H, dtype=torch.int64, device=weight.device).view(M, H)
    noise = mag.reshape(M, 1).to(torch.float32) * embedding_noise_u(idx, seed)
    out = (weight[flat].float() + noise).to(weight.dtype)
    return out.view(*ids.shape, H)


def adamw_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
           master: Optional[torch.Tensor], lr: float, beta1: float, beta2: float, eps: float,
           weight_decay: float, step: int, grad_scale: float = 1.0, sr_seed: int = 0, sr_offset: int = 0) -> None:
    """Decoupled-weight-decay Adam (torch.optim.AdamW semantics) on flat tensors, in place.

    Math in fp32 whatever the storage dtypes (twin of csrc/optim.hip adamw_kernel). bf16 storage
    (parameters without a master copy, and bf16 moments) is written with stochastic rounding when
    ``sr_seed`` is set — the same hash streams as the kernel, so CPU and GPU agree bit for bit on
    the rounding — and round-to-nearest otherwise."""
    w = master if master is not None else param.float()
    g = grad.float() * grad_scale
    m = exp_avg.float().mul_(beta1).add_(g, alpha=1 - beta1)
    v = exp_avg_sq.float().mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v / bc2).sqrt().add_(eps)
    w.mul_(1 - lr * weight_decay)
    w.addcdiv_(m, denom, value=-lr / bc1)
    sr = bool(sr_seed) and master is None
    for dst, src, s in ((exp_avg, m, _SEED_M), (exp_avg_sq, v, _SEED_V)):
        if dst.dtype == torch.bfloat16 and sr:
            dst.copy_(bf16_stochastic_round(src, (int(sr_seed) ^ s) & _M32, sr_offset))
        else:
            dst.copy_(src)
    if master is not None:
        param.copy_(master)
    elif sr and param.dtype == torch.bfloat16:
        param.copy_(bf16_stochastic_round(w, int(sr_seed), sr_offset))
    else:
        param.copy_(w)


_M32 = 0xFFFFFFFF
_SEED_M, _SEED_V = 0x68E31DA4, 0xB5297A4D  # csrc/optim.hip SEED_M / SEED_V


def hash_u32(idx: torch.Tensor, seed: int) -> torch.Tensor:
    """Bit-exact torch twin of csrc/common.h hash_u32 (int64 tensors holding uint32 values)."""
    lo, hi = idx & _M32, (idx >> 32) & _M32
    x = ((lo * 0x9E3779B9) & _M32) ^ ((hi * 0x85EBCA6B) & _M32) ^ ((int(seed) * 0xC2B2AE35) & _M32)
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def bf16_stochastic_round(x: torch.Tensor, seed: int, offset: int = 0) -> torch.Tensor:
    """fp32 -> bf16 with stochastic rounding: bits + noise(offset + i), truncated, where elements 2q / 2q + 1 take the
    low / high 16 bits of hash(q, seed). Twin of csrc/optim.hip f2bf_sr / sr_hash over a flat tensor (E[result] = x)."""
    xf = x.float().contiguous().reshape(-1)
    idx = torch.arange(xf.numel(), dtype=torch.int64, device=xf.device) + int(offset)
    bits = xf.view(torch.int32).to(torch.int64) & _M32
    finite = (bits & 0x7F800000) != 0x7F800000
    h = hash_u32(idx >> 1, seed)
    noise = torch.where((idx & 1) == 1, h >> 16, h & 0xFFFF)
    rounded = ((bits + noise) >> 16) << 16
    out = torch.where(finite, rounded, bits)
    out = torch.where(out >= 1 << 31, out - (1 << 32), out).to(torch.int32).view(torch.float32)
    res = out.to(torch.bfloat16)  # exact: low 16 bits are zero (non-finite: round-to-nearest, as f2bf)
    return torch.where(finite, res, xf.to(torch.bfloat16)).view(x.shape)


def dropout_keep(idx: torch.Tensor, seed: int, p: float) -> torch.Tensor:
    """Twin of csrc/common.h drop_keep: elements 2q and 2q + 1 share hash(q, seed), whose low / high 16 bits are
    compared with int(p * 65536)."""
    h = hash_u32(idx >> 1, seed)
    half = torch.where((idx & 1) == 1, h >> 16, h & 0xFFFF)
    return half >= int(min(max(float(p), 0.0), 0.999) * 65536.0)


def dropout_add(a: Optional[torch.Tensor], b: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """(a or 0) + b * keep / (1-p), keep = dropout_keep(t*K + k) (same mask as the HIP kernels)."""
    T, K = b.shape
    p = min(max(float(p), 0.0), 0.999)
    idx = torch.arange(T * K, device=b.device, dtype=torch.int64).view(T, K)
    keep = dropout_keep(idx, seed, p)
    out = torch.where(keep, b.float() * (1.0 / (1.0 - p)), torch.zeros((), device=b.device))
    if a is not None:
        out = out + a.float()
    return out.to(b.dtype)


def lora_fwd(x: torch.Tensor, A: torch.Tensor, s: float, p: float, seed: int, ldX: int = 0):
    """(X' = [x | s * dropout(x) A^T | 0], xd = dropout(x) or None) — twin of csrc/lora.hip lora_fwd; ``ldX`` (0 =
    K + R) is the padded width of X'."""
    xd = dropout_add(None, x, p, seed) if p > 0 else None
    xa = (xd if xd is not None else x).float() @ A.float().t()
    parts = [x, (xa * s).to(x.dtype)]
    pad = (ldX or x.shape[1] + A.shape[0]) - x.shape[1] - A.shape[0]
    if pad > 0:
        parts.append(x.new_zeros(x.shape[0], pad))
    return torch.cat(parts, dim=1), xd


def lora_bwd_dx(base: torch.Tensor, dxa: torch.Tensor, A: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """dx = base + dropout(dxa @ A) (same mask as the forward) — twin of csrc/lora.hip lora_bwd_dx."""
    dxd = (dxa.float() @ A.float()).to(base.dtype)
    if p > 0:
        return dropout_add(base, dxd, p, seed)
    return (base.float() + dxd.float()).to(base.dtype)


# ----------------------------------------------------------------------------- sequence-level objectives (DPO)
def _row_segments(M: int, cu_seqlens: torch.Tensor, n_seqs: int) -> torch.Tensor:
    """int64 [M]: the segment of ``cu_seqlens`` each row lies in; ``n_seqs`` for rows at or past ``cu[n_seqs]``."""
    t = torch.arange(M, dtype=torch.int64, device=cu_seqlens.device)
    return torch.searchsorted(cu_seqlens[1:n_seqs + 1].to(torch.int64).contiguous(), t, right=True)


def seq_logp_sum(nll: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int) -> torch.Tensor:
    """logps[s] = -sum nll[cu[s] : cu[s + 1]] for the first ``n_seqs`` segments (an empty one gives 0; later segments,
    the collator's pad, are ignored) — twin of csrc/preference.hip seq_logp_sum, in nll's dtype."""
    seg = _row_segments(nll.numel(), cu_seqlens.to(nll.device), n_seqs)
    keep = seg < n_seqs
    out = torch.zeros(n_seqs, dtype=nll.dtype, device=nll.device)
    return out.index_add_(0, seg[keep], -nll[keep])


def scale_rows_by_seq(x: torch.Tensor, coef: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int,
                      gscale: torch.Tensor) -> torch.Tensor:
    """out[t, :] = x[t, :] * (coef[s(t)] * gscale) with s(t) the segment of row t, +0 on rows at or past ``cu[n_seqs]``.
    Bit-equal to csrc/scale_rows.hip scale_rows_by_seq on bf16: the two scalars are multiplied first, in fp32, then
    one fp32 product per element and one rounding to x's dtype (fp64 stays fp64)."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    M = x.shape[0]
    if n_seqs == 0 or M == 0:
        return torch.zeros_like(x)
    seg = _row_segments(M, cu_seqlens.to(x.device), n_seqs)
    c = coef.to(ct) * gscale.to(ct).reshape(())
    rows = c[seg.clamp(max=n_seqs - 1)]
    out = (x.to(ct) * rows[:, None]).to(x.dtype)
    return torch.where((seg >= n_seqs)[:, None], torch.zeros((), dtype=x.dtype, device=x.device), out)


def dpo_pair(logps: torch.Tensor, ref_logps: torch.Tensor, inv_pairs: torch.Tensor, beta: float) -> torch.Tensor:
    """DPO (sigmoid loss) per pair, sequence 2p chosen and 2p + 1 rejected — twin of csrc/preference.hip dpo_pair_fwd.
    stats [5, P] in logps' dtype: loss = softplus(-beta delta) as max(-z, 0) + log1p(exp(-|z|)), coef = d(inv_pairs
    sum loss) / d logp_chosen = -beta sigmoid(-z) inv_pairs (the rejected sequence's is its negative), reward_chosen,
    reward_rejected, delta = (pi_c - pi_r) - (ref_c - ref_r)."""
    ref_logps = ref_logps.to(logps.dtype)
    pc, pr, rc, rr = logps[0::2], logps[1::2], ref_logps[0::2], ref_logps[1::2]
    delta = (pc - pr) - (rc - rr)
    z = beta * delta
    e = torch.exp(-z.abs())
    loss = (-z).clamp(min=0) + torch.log1p(e)
    sig = torch.where(z >= 0, e, torch.ones_like(e)) / (1 + e)
    coef = (-beta * sig) * inv_pairs.to(logps.dtype).reshape(())
    return torch.stack([loss, coef, beta * (pc - rc), beta * (pr - rr), delta])


# ----------------------------------------------------------------------------- per-token policy objective (GRPO)
def grpo_token(nll: torch.Tensor, old_logps: Optional[torch.Tensor], ref_logps: Optional[torch.Tensor],
               labels: torch.Tensor, adv: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int, inv_norm: torch.Tensor,
               eps_low: float, eps_high: float, beta: float, per_seq_mean: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """Twin of csrc/policy.hip grpo_token_fwd, in nll's dtype (fp64 stays fp64), with its expressions in its order. A
    completion row is a row with ``labels >= 0`` inside one of the first ``n_seqs`` segments; for it, with lp = -nll,
    A the sequence's advantage, r = exp(lp - old) (exactly 1 without ``old_logps``), d = ref - lp:
        l = -min(r A, clamp(r, 1 - eps_low, 1 + eps_high) A) + beta (exp(d) - d - 1)      (no KL term without ref)
        c = dl / dlp = -A r [r A <= clamp(r) A] + beta (1 - exp(d))
    rows [2, M] = (w l, w c), w = inv_norm, divided by the sequence's completion rows (at least 1) with
    ``per_seq_mean``; every other row is +0. seq [6, n_seqs] = the sequences' sums of (w l, 1, [r < 1 - eps_low and
    A < 0], [r > 1 + eps_high and A > 0], exp(d) - d - 1, r) over their completion rows."""
    dt = nll.dtype
    M = nll.numel()
    rows = torch.zeros(2, M, dtype=dt, device=nll.device)
    seq = torch.zeros(6, n_seqs, dtype=dt, device=nll.device)
    if n_seqs == 0 or M == 0:
        return rows, seq
    seg = _row_segments(M, cu_seqlens.to(nll.device), n_seqs)
    first = int(cu_seqlens[0])
    comp = (seg < n_seqs) & (labels.to(nll.device) >= 0) & (torch.arange(M, device=nll.device) >= first)
    sc = seg.clamp(max=n_seqs - 1)
    cnt = torch.zeros(n_seqs, dtype=dt, device=nll.device).index_add_(0, sc[comp], comp[comp].to(dt))
    w = inv_norm.to(dt).reshape(()).expand(n_seqs)
    if per_seq_mean:
        w = w / cnt.clamp(min=1.0)
    w, A = w[sc], adv.to(dt)[sc]
    one = torch.ones((), dtype=dt, device=nll.device)
    lo = one - torch.tensor(float(eps_low), dtype=dt, device=nll.device)
    hi = one + torch.tensor(float(eps_high), dtype=dt, device=nll.device)
    lp = 0.0 - torch.where(comp, nll, torch.zeros_like(nll))
    r = torch.exp(lp - torch.where(comp, old_logps.to(dt), torch.zeros_like(nll))) if old_logps is not None \
        else torch.ones_like(nll)
    r = torch.where(comp, r, torch.ones_like(r))
    t1 = r * A
    t2 = torch.minimum(torch.maximum(r, lo), hi) * A
    l = 0.0 - torch.minimum(t1, t2)
    c = torch.where(t1 <= t2, 0.0 - t1, torch.zeros_like(t1))
    kl = torch.zeros_like(nll)
    if ref_logps is not None:
        d = torch.where(comp, ref_logps.to(dt), torch.zeros_like(nll)) - lp
        em = torch.expm1(d)  # exp(d) - 1 without the cancellation at small d
        kl = em - d
        l = l + beta * kl
        c = c - beta * em
    zero = torch.zeros_like(nll)
    rows[0] = torch.where(comp, w * l, zero)
    rows[1] = torch.where(comp, w * c, zero)
    cols = (rows[0], comp.to(dt), (comp & (r < lo) & (A < 0)).to(dt), (comp & (r > hi) & (A > 0)).to(dt),
            torch.where(comp, kl, zero), torch.where(comp, r, zero))
    for i, v in enumerate(cols):
        seq[i].index_add_(0, sc[comp], v[comp])
    return rows, seq


def scale_rows(x: torch.Tensor, coef: torch.Tensor, gscale: torch.Tensor) -> torch.Tensor:
    """out[t, :] = x[t, :] * (coef[t] * gscale). Bit-equal to csrc/scale_rows.hip scale_rows on bf16: the two scalars are
    multiplied first, in fp32, then one fp32 product per element and one rounding to x's dtype (fp64 stays fp64)."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    c = coef.to(ct) * gscale.to(ct).reshape(())
    return (x.to(ct) * c[:, None]).to(x.dtype)


# ----------------------------------------------------------------------------- reward modelling (csrc/reward.hip)
def _last_rows(M: int, cu_seqlens: torch.Tensor, n_seqs: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(last int64 [n_seqs], nonempty bool [n_seqs]): segment s is [a, b) with a = clamp(cu[s], 0, M), b =
    clamp(cu[s + 1], a, M); its last row is b - 1 (0 where the segment is empty)."""
    cu = cu_seqlens[:n_seqs + 1].to(torch.int64)
    a = cu[:-1].clamp(0, M)
    b = torch.minimum(torch.maximum(cu[1:], a), torch.tensor(M, dtype=torch.int64, device=cu.device))
    nonempty = b > a
    return torch.where(nonempty, b - 1, torch.zeros_like(b)), nonempty


def _lane_dot(prod: torch.Tensor) -> torch.Tensor:
    """The row sums of ``prod`` [S, H] (H a multiple of 8) in seq_score_fwd's order: lane l of 64 adds the elements of
    the 8-wide chunks l, l + 64, ... in element order, then the xor butterfly 32, 16, ..., 1 over the lanes."""
    S, H = prod.shape
    nc = H // 8
    passes = (nc + 63) // 64
    p = torch.zeros(S, passes * 64 * 8, dtype=prod.dtype, device=prod.device)
    p[:, :H] = prod
    p = p.view(S, passes, 64, 8)
    acc = torch.zeros(S, 64, dtype=prod.dtype, device=prod.device)
    for k in range(passes):
        for i in range(8):
            acc = acc + p[:, k, :, i]
    lanes = torch.arange(64, device=prod.device)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def seq_score(h: torch.Tensor, w: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int) -> torch.Tensor:
    """scores[s] = h[last row of segment s] . w for the first ``n_seqs`` segments of ``cu_seqlens`` (an empty one
    gives +0; later segments, the collators' pad, are ignored) — twin of csrc/reward.hip seq_score_fwd with its
    summation order, in fp32 (fp64 operands stay fp64)."""
    ct = torch.float64 if h.dtype == torch.float64 else torch.float32
    M, H = h.shape
    if H % 8:
        raise ValueError(f"seq_score: H must be a multiple of 8, got {H}")
    if n_seqs == 0:
        return torch.zeros(0, dtype=ct, device=h.device)
    last, nonempty = _last_rows(M, cu_seqlens.to(h.device), n_seqs)
    if M == 0:
        return torch.zeros(n_seqs, dtype=ct, device=h.device)
    dots = _lane_dot(h[last].to(ct) * w.reshape(1, -1).to(ct))
    return torch.where(nonempty, dots, torch.zeros_like(dots))


def seq_score_bwd(g: torch.Tensor, h: torch.Tensor, w: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int,
                  need_dh: bool = True, need_dw: bool = True):
    """(dh in h's dtype [M, H], dw fp32 [H]; None for the half not needed) — twin of csrc/reward.hip seq_score_bwd,
    bit-equal on bf16. dh is +0 except the last row of each non-empty segment, g_s * w in one product and one
    rounding; dw[j] = sum over the non-empty segments in increasing s of g_s * h[last_s, j]."""
    ct = torch.float64 if h.dtype == torch.float64 else torch.float32
    M, H = h.shape
    last, nonempty = _last_rows(M, cu_seqlens.to(h.device), n_seqs)
    gs, wf = g.to(ct), w.reshape(-1).to(ct)
    dh = dw = None
    if need_dh:
        dh = torch.zeros_like(h)
        if M:
            dh[last[nonempty]] = (gs[nonempty, None] * wf[None, :]).to(h.dtype)
    if need_dw:
        dw = torch.zeros(H, dtype=ct, device=h.device)
        for s in torch.nonzero(nonempty).reshape(-1).tolist() if M else []:
            dw = dw + gs[s] * h[last[s]].to(ct)
    return dh, dw


def reward_pair(scores: torch.Tensor, margins: Optional[torch.Tensor], inv_pairs: torch.Tensor,
                center_coef: float = 0.0) -> torch.Tensor:
    """The pairwise reward-model loss (TRL ``RewardTrainer``), score 2p chosen and 2p + 1 rejected — twin of
    csrc/reward.hip reward_pair_fwd. With z = (r_c - r_r) - margin and c = ``center_coef``, stats [4, P] in the scores'
    dtype: softplus(-z) + c (r_c + r_r)^2 with softplus as max(-z, 0) + log1p(exp(-|z|)); d(inv_pairs sum loss) / d
    r_c = (-sigmoid(-z) + 2 c (r_c + r_r)) inv_pairs; the same / d r_r = (sigmoid(-z) + 2 c (r_c + r_r)) inv_pairs; z.
    With c == 0 the centring terms are not formed: row 2 is the exact negation of row 1."""
    dt = scores.dtype
    rc, rr = scores[0::2], scores[1::2]
    z = rc - rr
    z = z - (margins.to(dt) if margins is not None else torch.zeros_like(z))
    e = torch.exp(-z.abs())
    loss = (-z).clamp(min=0) + torch.log1p(e)
    sig = torch.where(z >= 0, e, torch.ones_like(e)) / (1 + e)
    gc, gr = -sig, sig
    c = torch.tensor(float(center_coef), dtype=torch.float32).to(dt)  # the kernel's fp32 coefficient
    if float(center_coef) != 0.0:
        total = rc + rr
        tc = (2 * c) * total
        loss = loss + c * (total * total)
        gc, gr = gc + tc, gr + tc
    inv = inv_pairs.to(dt).reshape(())
    return torch.stack([loss, gc * inv, gr * inv, z])
