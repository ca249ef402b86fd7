"""Reward modelling: the score head on the trunk's hidden states and the pairwise loss (csrc/reward.hip).

A reward model's score is the dot product of each sequence's LAST hidden row with the ``score`` parameter, so the head
is row work, not a GEMM: ``seq_score`` reads one row per sequence, its backward writes one row per sequence of dh and
sums the same rows into dw. ``reward_pair_loss`` is ``dpo_loss``'s shape over scores. HIP on GPU tensors,
``ops.reference`` on CPU ones (and under SFTAMD_DISABLE_HIP=1).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd import Function

from . import _ext
from . import reference as ref
from .fused import _accumulate_small_grad


def _hip_rows(h: torch.Tensor) -> bool:
    return _ext.use_hip(h) and h.dtype == torch.bfloat16


class SeqScoreFn(Function):
    """scores[s] = h[last row of segment s] . w (fp32 on the bf16 path). dh goes to autograd; dw goes through
    ``_accumulate_small_grad`` (a DDP ``main_grad`` slice takes it directly and the use counter is decremented)."""

    @staticmethod
    def forward(ctx, h, weight, cu_seqlens, n_seqs):
        h2d = h.reshape(-1, h.shape[-1])
        w = weight.detach().reshape(-1)
        if _hip_rows(h2d):
            scores = _ext.ops().seq_score_fwd(h2d.contiguous(), w.contiguous(), cu_seqlens, int(n_seqs))
        else:
            scores = ref.seq_score(h2d, w, cu_seqlens, int(n_seqs))
        ctx.save_for_backward(h2d, cu_seqlens)
        ctx.weight = weight
        ctx.h_shape = h.shape
        ctx.n_seqs = int(n_seqs)
        return scores

    @staticmethod
    def backward(ctx, g):
        h2d, cu = ctx.saved_tensors
        weight = ctx.weight
        need_dh, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        w = weight.detach().reshape(-1)
        if _hip_rows(h2d):
            dh, dw = _ext.ops().seq_score_bwd(g.float().contiguous(), h2d.contiguous(), w.contiguous(), cu, ctx.n_seqs,
                                              bool(need_dh), bool(need_dw))
        else:
            dh, dw = ref.seq_score_bwd(g, h2d, w, cu, ctx.n_seqs, need_dh, need_dw)
        if dh is not None:
            dh = dh.view(ctx.h_shape)
        if dw is not None:
            dw = _accumulate_small_grad(weight, dw.view(weight.shape))
        return dh, dw, None, None


def seq_score(h: torch.Tensor, w: torch.Tensor, cu_seqlens: torch.Tensor, n_seqs: int) -> torch.Tensor:
    """Per-sequence scores of the first ``n_seqs`` segments of ``cu_seqlens`` (non-decreasing): the last row of each
    segment of ``h`` [M, H] times ``w`` ([H] or the [1, H] score parameter), differentiable in both; an empty segment
    scores +0 and passes no gradient."""
    if cu_seqlens.numel() < int(n_seqs) + 1:
        raise ValueError(f"n_seqs {n_seqs} over the {cu_seqlens.numel() - 1} segments of cu_seqlens")
    if w.numel() != h.shape[-1]:
        raise ValueError(f"seq_score: w must hold {h.shape[-1]} values (one label), got {tuple(w.shape)}")
    return SeqScoreFn.apply(h, w, cu_seqlens, int(n_seqs))


def reward_pair_stats(scores, margins, inv_pairs, center_coef: float = 0.0) -> torch.Tensor:
    """stats [4, P] = (loss, d / d r_chosen, d / d r_rejected, z) of P pairs (csrc/reward.hip; ref.reward_pair)."""
    if _ext.use_hip(scores) and scores.dtype == torch.float32:
        m = None if margins is None else margins.float().contiguous()
        return _ext.ops().reward_pair_fwd(scores.contiguous(), m, inv_pairs, float(center_coef))
    return ref.reward_pair(scores, margins, inv_pairs, float(center_coef))


class RewardPairLossFn(Function):
    @staticmethod
    def forward(ctx, scores, margins, inv_pairs, center_coef):
        stats = reward_pair_stats(scores, margins, inv_pairs, center_coef)
        ctx.save_for_backward(stats[1], stats[2])
        ctx.mark_non_differentiable(stats)
        return (stats[0].sum() * inv_pairs.to(stats.dtype).reshape(())).reshape(()), stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        gc, gr = ctx.saved_tensors
        return torch.stack([gc, gr], dim=1).reshape(-1) * dloss, None, None, None


def reward_pair_loss(scores, margins: Optional[torch.Tensor], inv_pairs,
                     center_coef: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The pairwise reward-model loss of P pairs (score 2p chosen, 2p + 1 rejected; TRL ``RewardTrainer``): loss =
    inv_pairs * sum (softplus(-(r_c - r_r - margin_p)) + center_coef (r_c + r_r)^2), and the per-pair stats [4, P].
    ``margins`` is [P] or None; ``inv_pairs`` a fp32 scalar tensor on the scores' device."""
    if scores.dim() != 1 or scores.numel() % 2:
        raise ValueError(f"reward_pair_loss: scores must be [2 P], got {tuple(scores.shape)}")
    if margins is not None and tuple(margins.shape) != (scores.numel() // 2,):
        raise ValueError(f"reward_pair_loss: margins must be [{scores.numel() // 2}], got {tuple(margins.shape)}")
    if not float(center_coef) >= 0.0:
        raise ValueError(f"center_coef must be >= 0, got {center_coef}")
    if margins is not None and margins.requires_grad:
        margins = margins.detach()
    return RewardPairLossFn.apply(scores, margins, inv_pairs, float(center_coef))
