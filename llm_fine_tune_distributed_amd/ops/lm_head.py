"""Training objectives on the LM head: cross-entropy, distillation, sequence log-probs + DPO, the GRPO policy loss.

One skeleton (the kernels' side of it: csrc/vocab_rows.h). The forward GEMM writes the bf16 logits (``_logits``); a row
kernel over the vocabulary (``_ce_rows`` / ``_kd_rows``) returns per-row stats and, when a gradient is needed, leaves
the gradient over the logits in their buffer, so fp32 logits are never materialised; the backward puts
the rest of the chain rule, a scalar (``_scalar_backward``) or a row weight (``_row_backward``), onto the two
[T, hidden] operands of its GEMMs, never onto the [T, vocab] one. HIP on GPU tensors, ``ops.reference`` on CPU ones.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch.autograd import Function

from . import _ext
from . import reference as ref
from .fused import _accumulate_weight_grad, dgrad_mm, fwd_gemm

LOSS_MODES = {"nll": 0, "dft": 1}
_CONSTS: dict = {}


def _const(value: float, device) -> torch.Tensor:
    """A cached fp32 device scalar (the unit inv_count / the -1 of the sequence-level LM head)."""
    key = (float(value), str(device))
    t = _CONSTS.get(key)
    if t is None:
        t = _CONSTS[key] = torch.full((1,), float(value), dtype=torch.float32, device=device)
    return t


# ----------------------------------------------------------------------------- the shared skeleton
def _logits(h: torch.Tensor, weight: torch.Tensor):
    """(h2d [M, hidden], logits [M, vocab] in h's dtype): the HIP forward GEMM on the GPU."""
    h2d = h.reshape(-1, h.shape[-1])
    return h2d, fwd_gemm(h2d, weight) if _ext.use_hip(h2d) else torch.nn.functional.linear(h2d, weight)


def _forward(ctx, h, weight):
    """The forward's common opening: (h2d, logits, need_grad) — need_grad tells the row kernel to write the gradient."""
    return (*_logits(h, weight), ctx.needs_input_grad[0] or ctx.needs_input_grad[1])


def _save(ctx, h, weight, need_grad, saved, non_differentiable):
    """The forward's ctx bookkeeping: ``saved`` = (h2d, the gradient over the logits, ...) for the two backwards."""
    if need_grad:
        ctx.save_for_backward(*saved)
    ctx.weight = weight
    ctx.h_shape = h.shape
    ctx.mark_non_differentiable(*non_differentiable)


def _scalar_backward(ctx, dloss):
    """(dh, dW) where the forward left dloss-free dlogits over the logits (LMHeadCEFn, LMHeadDistillFn)."""
    h2d, dlogits = ctx.saved_tensors
    w = ctx.weight
    # the loss gradient (a device scalar: 1 for the trainer's loss.backward(), no host sync to find out) scales the
    # two [T, hidden] operands below — ~26 us per step at 16 x 512, bitwise a no-op at 1 — rather than the
    # [T, vocab] dlogits
    g = dloss.float()
    dh = dw = None
    if ctx.needs_input_grad[0]:
        dh = (dgrad_mm(dlogits, w) * g.to(dlogits.dtype)).view(ctx.h_shape)
    if ctx.needs_input_grad[1]:
        dw = _accumulate_weight_grad(w, dlogits, h2d, scale=g)
    return dh, dw


def _row_backward(ctx, h2d, G, scale, *args):
    """(dh, dW) where the forward left G = softmax - onehot over the logits and the rows carry a weight:
    dh = diag(.) (G W), dW = G^T (diag(.) h), with ``scale(x, *args, inplace=)`` one of the two scale_rows*."""
    w = ctx.weight
    dh = dw = None
    if ctx.needs_input_grad[0]:
        dh = scale(dgrad_mm(G, w), *args, inplace=True).view(ctx.h_shape)
    if ctx.needs_input_grad[1]:
        # (out of place: h2d is a saved activation)
        dw = _accumulate_weight_grad(w, G, scale(h2d, *args))
    return dh, dw


def _scale_rows(name: str, x: torch.Tensor, args, inplace: bool) -> torch.Tensor:
    """The body of scale_rows / scale_rows_by_seq: the HIP op ``name`` (``name_`` in place) or its bit-equal twin."""
    if _ext.use_hip(x) and x.dtype == torch.bfloat16:
        if inplace:
            getattr(_ext.ops(), name + "_")(x, *args)
            return x
        return getattr(_ext.ops(), name)(x.contiguous(), *args)
    out = getattr(ref, name)(x, *args)
    return x.copy_(out) if inplace else out


# ----------------------------------------------------------------------------- LM head + CE
def _ce_rows(logits: torch.Tensor, labels: torch.Tensor, inv_count: torch.Tensor, write_grad: bool,
             label_smoothing: float = 0.0, loss_mode: int = 0, temperature: float = 1.0):
    """Per-row CE over the vocab. Returns stats [4, M] fp32 = (loss, lse, entropy, correct); ``loss`` is the
    objective's per-row value (label smoothing e, or loss_mode 1 = dft: ref.cross_entropy).
    If write_grad, logits is overwritten in place by d(sum(loss)*inv_count)/dlogits. A ``temperature`` tau != 1 gives
    the stats of softmax(x / tau) and, with write_grad, (softmax(x / tau) - onehot) * inv_count: the chain rule's
    1 / tau is the caller's (LMHeadPolicyFn puts it onto its row weight)."""
    if float(temperature) != 1.0:
        if not float(temperature) > 0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        if label_smoothing != 0 or loss_mode != 0:
            raise ValueError("a temperature takes neither label smoothing nor dft")
        if _ext.use_hip(logits):
            return _ext.ops().ce_fwd(logits, labels, inv_count, write_grad, 0.0, 0, float(temperature))
        loss, lse, correct, ent = ref.cross_entropy(logits, labels, temperature=temperature)
        if write_grad:
            logits.copy_(ref.cross_entropy_grad(logits, labels, inv_count, temperature=temperature))
        return torch.stack([loss, lse, ent, correct.float()])
    if _ext.use_hip(logits):
        if label_smoothing == 0 and loss_mode == 0:  # four arguments: also what an older build (SFTAMD_LIB) takes
            return _ext.ops().ce_fwd(logits, labels, inv_count, write_grad)
        return _ext.ops().ce_fwd(logits, labels, inv_count, write_grad, float(label_smoothing), int(loss_mode))
    loss, lse, correct, ent = ref.cross_entropy(logits, labels, label_smoothing, loss_mode)
    if write_grad:
        logits.copy_(ref.cross_entropy_grad(logits, labels, inv_count, label_smoothing, loss_mode))
    return torch.stack([loss, lse, ent, correct.float()])


class LMHeadCEFn(Function):
    """loss = sum_t CE(h_t W^T, y_t) * inv_count, with dlogits computed in the forward pass, over the logits."""

    @staticmethod
    def forward(ctx, h, weight, labels, inv_count, label_smoothing=0.0, loss_mode=0):
        h2d, logits, need_grad = _forward(ctx, h, weight)
        stats = _ce_rows(logits, labels.reshape(-1), inv_count, need_grad, label_smoothing, loss_mode)
        loss = (stats[0].sum() * inv_count.float()).reshape(())
        _save(ctx, h, weight, need_grad, (h2d, logits), (stats,))
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        return (*_scalar_backward(ctx, dloss), None, None, None, None)


def lm_head_cross_entropy(h, weight, labels, inv_count, label_smoothing: float = 0.0,
                          loss_type: str = "nll") -> Tuple[torch.Tensor, torch.Tensor]:
    """``label_smoothing`` e in [0, 1): HF LabelSmoother; ``loss_type`` "dft": TRL dft_loss (not with smoothing)."""
    if loss_type not in LOSS_MODES:
        raise ValueError(f"loss_type must be one of {sorted(LOSS_MODES)}, got {loss_type!r}")
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
    if loss_type == "dft" and label_smoothing > 0:
        raise ValueError("loss_type='dft' takes no label smoothing")
    return LMHeadCEFn.apply(h, weight, labels, inv_count, float(label_smoothing), LOSS_MODES[loss_type])


# ----------------------------------------------------------------------------- LM head + distillation
def lm_head_logits(h: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """[M, vocab] logits of the LM head in h's dtype, no autograd graph (a teacher's side of a distillation step)."""
    return _logits(h.detach(), weight.detach())[1]


def _kd_rows(logits: torch.Tensor, teacher_logits: torch.Tensor, labels: torch.Tensor, inv_count: torch.Tensor,
             write_grad: bool, beta: float, temperature: float):
    """Per-row generalized JSD against a teacher over the vocab (csrc/distill.hip; ref.generalized_jsd). Returns stats
    [5, M] fp32 = (loss, student lse, teacher lse, correct, agrees with the teacher's argmax). If write_grad, logits is
    overwritten in place by d(sum(loss) * inv_count) / dlogits; teacher_logits is only read."""
    if _ext.use_hip(logits):
        return _ext.ops().kd_fwd(logits, teacher_logits.contiguous(), labels, inv_count, write_grad, float(beta),
                                 float(temperature))
    loss, lse_s, lse_t, correct, agree = ref.generalized_jsd(logits, teacher_logits, labels, beta, temperature)
    if write_grad:
        logits.copy_(ref.generalized_jsd_grad(logits, teacher_logits, labels, inv_count, beta, temperature))
    return torch.stack([loss, lse_s, lse_t, correct.to(loss.dtype), agree.to(loss.dtype)]).float()


class LMHeadDistillFn(Function):
    """loss = sum_t JSD_beta(h_t W^T / tau, teacher_t / tau) * inv_count: LMHeadCEFn with _kd_rows in place of
    _ce_rows. The teacher's logits are read in the forward only and not saved."""

    @staticmethod
    def forward(ctx, h, weight, teacher_logits, labels, inv_count, beta, temperature):
        h2d, logits, need_grad = _forward(ctx, h, weight)
        stats = _kd_rows(logits, teacher_logits, labels.reshape(-1), inv_count, need_grad, beta, temperature)
        loss = (stats[0].sum() * inv_count.float()).reshape(())
        _save(ctx, h, weight, need_grad, (h2d, logits), (stats,))
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        return (*_scalar_backward(ctx, dloss), None, None, None, None, None)


def lm_head_distill_loss(h, weight, teacher_logits, labels, inv_count, beta: float = 0.5,
                         temperature: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Knowledge distillation through the LM head (TRL ``GKDTrainer.generalized_jsd_loss``): ``teacher_logits``
    [M, vocab] in h's dtype, ``labels`` already shifted (-100: the row costs nothing), ``beta`` in [0, 1] (0: forward
    KL(teacher || student), 1: reverse KL), ``temperature`` > 0. Returns (loss, stats [5, M])."""
    if not 0.0 <= float(beta) <= 1.0:
        raise ValueError(f"beta must be in [0, 1], got {beta}")
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    M = h.numel() // h.shape[-1]
    if teacher_logits.dim() < 1 or teacher_logits.numel() != M * weight.shape[0] or \
            teacher_logits.shape[-1] != weight.shape[0]:
        raise ValueError(f"teacher_logits must be [{M}, {weight.shape[0]}] (the student's rows and vocabulary), got "
                         f"{tuple(teacher_logits.shape)}")
    if teacher_logits.requires_grad:
        teacher_logits = teacher_logits.detach()
    return LMHeadDistillFn.apply(h, weight, teacher_logits.reshape(M, -1), labels, inv_count, float(beta),
                                 float(temperature))


# ----------------------------------------------------------------------------- LM head + offline distillation
def teacher_topk(logits: torch.Tensor, k: int, temperature: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(int32 ids [M, k], fp32 log softmax(logits / temperature) at them [M, k]) of the k <= 256 largest logits of every
    row, value descending and equal values by column ascending; the lse is the whole row's (csrc/distill_topk.hip;
    ref.teacher_topk). ``logits`` [M, vocab] are only read."""
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    x = logits.reshape(-1, logits.shape[-1])
    if _ext.use_hip(x):
        ids, lps = _ext.ops().teacher_topk(x.contiguous(), int(k), float(temperature))
        return ids, lps
    ids, lps = ref.teacher_topk(x, int(k), temperature)
    return ids, lps.float()


def _kd_topk_rows(logits: torch.Tensor, ids: torch.Tensor, logps: torch.Tensor, labels: torch.Tensor,
                  inv_count: torch.Tensor, write_grad: bool, temperature: float):
    """Per-row forward KL against a teacher's cached top-k log-probabilities (csrc/distill_topk.hip kd_topk_fwd;
    ref.distill_topk). Returns stats [5, M] fp32 = (loss, student lse, teacher mass kept, correct, agrees with
    ids[:, 0]). If write_grad, logits is overwritten in place by d(sum(loss) * inv_count) / dlogits. The ids of a row
    must be distinct and in [0, vocab): anything else is a caller error (the debug build asserts it)."""
    if _ext.use_hip(logits):
        return _ext.ops().kd_topk_fwd(logits, ids.contiguous(), logps.contiguous(), labels, inv_count, write_grad,
                                      float(temperature))
    loss, lse, mass, correct, agree = ref.distill_topk(logits, ids, logps, labels, temperature)
    if write_grad:
        logits.copy_(ref.distill_topk_grad(logits, ids, logps, labels, inv_count, temperature))
    return torch.stack([loss, lse, mass, correct.to(loss.dtype), agree.to(loss.dtype)]).float()


class LMHeadDistillTopKFn(Function):
    """loss = sum_t sum_k p_tk (tlp_tk - log softmax(h_t W^T / tau)[id_tk]) * inv_count: LMHeadDistillFn with
    _kd_topk_rows in place of _kd_rows. The cached tensors are read in the forward only and not saved."""

    @staticmethod
    def forward(ctx, h, weight, ids, logps, labels, inv_count, temperature):
        h2d, logits, need_grad = _forward(ctx, h, weight)
        stats = _kd_topk_rows(logits, ids, logps, labels.reshape(-1), inv_count, need_grad, temperature)
        loss = (stats[0].sum() * inv_count.float()).reshape(())
        _save(ctx, h, weight, need_grad, (h2d, logits), (stats,))
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        return (*_scalar_backward(ctx, dloss), None, None, None, None, None)


def lm_head_distill_topk_loss(h, weight, ids, logps, labels, inv_count,
                              temperature: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Offline distillation through the LM head: the forward KL(teacher || student) over the teacher's top-k support,
    not renormalised, from cached ``ids`` int32 [M, k] and ``logps`` fp32 [M, k] (``teacher_topk`` /
    ``lm_head_topk_logps`` of the same rows at the same ``temperature``). ``labels`` are already shifted (-100: the
    row costs nothing and its cached values are never used). Returns (loss, stats [5, M])."""
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    M = h.numel() // h.shape[-1]
    if ids.dim() >= 2 and ids.shape == logps.shape:  # [M, k], or a padded batch's [B, T, k]
        ids, logps = ids.reshape(-1, ids.shape[-1]), logps.reshape(-1, ids.shape[-1])
    if ids.dim() != 2 or ids.shape != logps.shape or ids.shape[0] != M or \
            not 1 <= ids.shape[1] <= min(256, weight.shape[0]):
        raise ValueError(f"ids / logps must both be [{M}, k] with 1 <= k <= min(256, vocab), got {tuple(ids.shape)} / "
                         f"{tuple(logps.shape)}")
    if ids.dtype != torch.int32 or logps.dtype != torch.float32:
        raise ValueError(f"ids must be int32 and logps fp32, got {ids.dtype} / {logps.dtype}")
    return LMHeadDistillTopKFn.apply(h, weight, ids, logps.detach(), labels, inv_count, float(temperature))


def lm_head_topk_logps(h: torch.Tensor, weight: torch.Tensor, k: int,
                       temperature: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The teacher's side of offline distillation, no autograd graph: the forward GEMM, then ``teacher_topk`` of its
    logits. Returns (ids int32 [M, k], logps fp32 [M, k])."""
    return teacher_topk(_logits(h.detach(), weight.detach())[1], k, temperature)


# ----------------------------------------------------------------------------- sequence log-probs + DPO
def seq_logp_sum(nll: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int) -> torch.Tensor:
    """logps[s] = -sum nll[cu[s] : cu[s + 1]], s < n_seqs (csrc/preference.hip; ref.seq_logp_sum)."""
    if _ext.use_hip(nll):
        return _ext.ops().seq_logp_sum(nll.contiguous(), cu_seqlens, int(n_seqs))
    return ref.seq_logp_sum(nll, cu_seqlens, int(n_seqs))


def scale_rows_by_seq(x: torch.Tensor, coef: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int,
                      gscale: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """Row t of sequence s times coef[s] * gscale, rows past the last sequence zeroed (csrc/scale_rows.hip; the twin
    ref.scale_rows_by_seq is bit-equal). ``inplace`` overwrites x."""
    return _scale_rows("scale_rows_by_seq", x, (coef, cu_seqlens, int(n_seqs), gscale), inplace)


class LMHeadSeqLogpsFn(Function):
    """logps[s] = sum over the rows t of sequence s of log softmax(h_t W^T)[y_t] (ignored rows add 0). The forward
    leaves G = softmax - onehot over the logits; the backward's row weight is the per-sequence r_s = -dlogps[s]."""

    @staticmethod
    def forward(ctx, h, weight, labels, cu_seqlens, n_seqs):
        h2d, logits, need_grad = _forward(ctx, h, weight)
        stats = _ce_rows(logits, labels.reshape(-1), _const(1.0, h.device), need_grad)
        logps = seq_logp_sum(stats[0], cu_seqlens, n_seqs)
        _save(ctx, h, weight, need_grad, (h2d, logits, cu_seqlens), (stats,))
        ctx.n_seqs = int(n_seqs)
        return logps, stats

    @staticmethod
    def backward(ctx, dlogps, _dstats):
        h2d, G, cu = ctx.saved_tensors
        # r = -dlogps: coef * gscale, one product
        return (*_row_backward(ctx, h2d, G, scale_rows_by_seq, dlogps.float().contiguous(), cu, ctx.n_seqs,
                               _const(-1.0, h2d.device)), None, None, None)


def lm_head_seq_logps(h, weight, labels, cu_seqlens, n_seqs: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-sequence log-probabilities of ``labels`` (already shifted, -100 ignored) under the LM head: differentiable
    ``logps`` [n_seqs] (fp32 on the bf16 path) and the fused cross-entropy's stats [4, M]."""
    if cu_seqlens.numel() < int(n_seqs) + 1:
        raise ValueError(f"n_seqs {n_seqs} over the {cu_seqlens.numel() - 1} segments of cu_seqlens")
    return LMHeadSeqLogpsFn.apply(h, weight, labels, cu_seqlens, int(n_seqs))


def dpo_pair_stats(logps, ref_logps, inv_pairs, beta: float) -> torch.Tensor:
    """stats [5, P] = (loss, coef, reward_chosen, reward_rejected, delta) of P pairs (csrc/preference.hip)."""
    if _ext.use_hip(logps) and logps.dtype == torch.float32:
        return _ext.ops().dpo_pair_fwd(logps.contiguous(), ref_logps.float().contiguous(), inv_pairs, float(beta))
    return ref.dpo_pair(logps, ref_logps, inv_pairs, float(beta))


class DPOLossFn(Function):
    @staticmethod
    def forward(ctx, logps, ref_logps, inv_pairs, beta):
        stats = dpo_pair_stats(logps, ref_logps, inv_pairs, beta)
        ctx.save_for_backward(stats[1])
        ctx.mark_non_differentiable(stats)
        return (stats[0].sum() * inv_pairs.to(stats.dtype).reshape(())).reshape(()), stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        coef, = ctx.saved_tensors
        return torch.stack([coef, -coef], dim=1).reshape(-1) * dloss, None, None, None


def dpo_loss(logps, ref_logps, inv_pairs, beta: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """DPO sigmoid loss of P pairs (sequence 2p chosen, 2p + 1 rejected): loss = inv_pairs * sum softplus(-beta
    delta_p), and the per-pair stats [5, P]. ``inv_pairs`` is a fp32 scalar tensor on logps' device."""
    if logps.dim() != 1 or logps.numel() % 2 or ref_logps.shape != logps.shape:
        raise ValueError(f"dpo_loss: logps / ref_logps must be [2 P], got {tuple(logps.shape)} / {tuple(ref_logps.shape)}")
    return DPOLossFn.apply(logps, ref_logps, inv_pairs, float(beta))


# ----------------------------------------------------------------------------- per-token policy objective (GRPO)
def grpo_token_stats(nll, old_logps, ref_logps, labels, adv, cu_seqlens, n_seqs: int, inv_norm, eps_low: float = 0.2,
                     eps_high: float = 0.2, beta: float = 0.0, per_seq_mean: bool = False):
    """(rows [2, M] = per-row (w l, w dl/dlogp), seq [6, S] = per-sequence sums of loss, completion tokens, low-clipped,
    high-clipped, KL, ratio) of the clipped policy objective (csrc/policy.hip grpo_token_fwd; ref.grpo_token)."""
    if not (0.0 <= float(eps_low) < 1.0 and float(eps_high) >= 0.0 and float(beta) >= 0.0):
        raise ValueError(f"eps_low in [0, 1), eps_high >= 0 and beta >= 0 expected, got {eps_low}, {eps_high}, {beta}")
    if _ext.use_hip(nll) and nll.dtype == torch.float32:
        f32 = lambda t: None if t is None else t.float().contiguous()  # noqa: E731
        return _ext.ops().grpo_token_fwd(nll.contiguous(), f32(old_logps), f32(ref_logps), labels.contiguous(),
                                         adv.float().contiguous(), cu_seqlens, int(n_seqs), inv_norm, float(eps_low),
                                         float(eps_high), float(beta), bool(per_seq_mean))
    return ref.grpo_token(nll, old_logps, ref_logps, labels, adv, cu_seqlens, int(n_seqs), inv_norm, float(eps_low),
                          float(eps_high), float(beta), bool(per_seq_mean))


def scale_rows(x: torch.Tensor, coef: torch.Tensor, gscale: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """Row t times coef[t] * gscale (csrc/scale_rows.hip; the twin ref.scale_rows is bit-equal), ``inplace`` over x."""
    return _scale_rows("scale_rows", x, (coef, gscale), inplace)


class LMHeadPolicyFn(Function):
    """loss = sum over the completion rows of w_t l_t, l_t the clipped-ratio objective (+ beta k3 KL) of the row's
    log-probability under softmax(h_t W^T / tau) (grpo_token_stats). The forward leaves G = softmax - onehot over the
    logits (ce_fwd at tau) and the per-row derivative c_t = w_t dl_t / dlogp_t in rows[1]; since dlogp_t / dlogits =
    -G_t / tau, the backward's row weight is c_t * gscale with gscale = -dloss / tau."""

    @staticmethod
    def forward(ctx, h, weight, labels, adv, cu_seqlens, n_seqs, inv_norm, old_logps, ref_logps, eps_low, eps_high,
                beta, temperature, per_seq_mean):
        h2d, logits, need_grad = _forward(ctx, h, weight)
        labels = labels.reshape(-1)
        stats = _ce_rows(logits, labels, _const(1.0, h.device), need_grad, temperature=temperature)
        rows, seq = grpo_token_stats(stats[0], old_logps, ref_logps, labels, adv, cu_seqlens, n_seqs, inv_norm,
                                     eps_low, eps_high, beta, per_seq_mean)
        _save(ctx, h, weight, need_grad, (h2d, logits, rows), (stats, rows, seq))
        ctx.tau = float(temperature)
        return rows[0].sum(), stats, rows, seq

    @staticmethod
    def backward(ctx, dloss, _dstats, _drows, _dseq):
        h2d, G, rows = ctx.saved_tensors
        gscale = (dloss.float() * (-1.0 / ctx.tau)).reshape(1)
        return _row_backward(ctx, h2d, G, scale_rows, rows[1].float().contiguous(), gscale) + (None,) * 12


def lm_head_policy_loss(h, weight, labels, adv, cu_seqlens, n_seqs: int, inv_norm, old_logps=None, ref_logps=None,
                        eps_low: float = 0.2, eps_high: float = 0.2, beta: float = 0.0, temperature: float = 1.0,
                        per_seq_mean: bool = False):
    """The GRPO family's per-token objective through the LM head (TRL ``GRPOTrainer._compute_loss`` at token-level
    importance sampling). ``labels`` are already shifted, -100 off the completions; ``adv`` fp32 [n_seqs] the
    sequences' advantages; ``inv_norm`` a fp32 scalar tensor (1 / what the loss type normalises by); ``old_logps`` /
    ``ref_logps`` fp32 [M] or None (None: ratio exactly 1 / no KL term). Returns (loss, the cross-entropy's stats
    [4, M] at ``temperature``, rows [2, M], seq [6, n_seqs])."""
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    if cu_seqlens.numel() < int(n_seqs) + 1:
        raise ValueError(f"n_seqs {n_seqs} over the {cu_seqlens.numel() - 1} segments of cu_seqlens")
    M = h.numel() // h.shape[-1]
    for name, t in (("old_logps", old_logps), ("ref_logps", ref_logps)):
        if t is not None and t.numel() != M:
            raise ValueError(f"{name} must hold one value per row ({M}), got {tuple(t.shape)}")
    det = lambda t: None if t is None else t.detach().reshape(-1)  # noqa: E731
    return LMHeadPolicyFn.apply(h, weight, labels, adv.detach(), cu_seqlens, int(n_seqs), inv_norm, det(old_logps),
                                det(ref_logps), float(eps_low), float(eps_high), float(beta), float(temperature),
                                bool(per_seq_mean))


def lm_head_token_logps(h: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor,
                        temperature: float = 1.0) -> torch.Tensor:
    """fp32 [M]: log softmax(h_t W^T / temperature)[labels_t] per row (0 where the label is -100), no autograd graph:
    the forward GEMM and the fused cross-entropy's stats pass (write_grad off)."""
    if not float(temperature) > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    logits = _logits(h.detach(), weight.detach())[1]
    stats = _ce_rows(logits, labels.reshape(-1), _const(1.0, h.device), False, temperature=temperature)
    return (0.0 - stats[0]).float()
