"""Decoder-only causal LM (SmolLM3 / Llama / Qwen3 / Qwen2 families) built on the fused ops.

Replaces ``AutoModelForCausalLM.from_pretrained(...)`` of the reference
(``training.py:97-105``) and the transformers modules it runs
(``transformers/models/smollm3/modeling_smollm3.py``).

MI355X-first layout decisions:
* tokens are packed as a flat [M = sum(len), hidden] stream; attention is varlen over
  ``cu_seqlens`` so padded batches and padding-free packing share one code path;
* q/k/v and gate/up are fused weights (one GEMM each); HF key names are restored on
  save/load (``hf_state_dict`` / ``load_hf_state_dict``);
* RoPE is applied in place on the packed qkv GEMM output, NoPE layers skip it;
* the LM head and cross-entropy are one op that never materialises fp32 logits.
"""
from __future__ import annotations

import math
import os
import zlib
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from .. import ops
from ..ops import reference as ref
from .config import ModelConfig


@dataclass
class CausalLMOutput:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    stats: Optional[torch.Tensor] = None  # [4, M]: loss, lse, entropy, correct (per token)
    num_tokens: Optional[torch.Tensor] = None
    metrics: Optional[torch.Tensor] = None
    rows: Optional[torch.Tensor] = None   # policy_loss: [2, M] per-row loss and coefficient
    seq: Optional[torch.Tensor] = None    # policy_loss: [6, S] per-sequence sums
    teacher_mass: Optional[torch.Tensor] = None  # distill_topk_loss: the kept teacher mass summed over the valid rows


class RMSNorm(nn.Module):
    def __init__(self, hidden: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.eps = eps


class Attention(nn.Module):
    def __init__(self, cfg: ModelConfig, layer_idx: int):
        super().__init__()
        self.cfg = cfg
        self.layer_idx = layer_idx
        self.use_rope = cfg.uses_rope(layer_idx)
        self.qkv_proj = nn.Parameter(torch.empty(cfg.qkv_size, cfg.hidden_size))
        self.o_proj = nn.Parameter(torch.empty(cfg.hidden_size, cfg.q_size))
        self.qk_norm = bool(cfg.qk_norm)
        if self.qk_norm:  # Qwen3: RMSNorm over each query / key head (one weight [head_dim] per layer), before RoPE
            self.q_norm = RMSNorm(cfg.head_dim, cfg.rms_norm_eps)
            self.k_norm = RMSNorm(cfg.head_dim, cfg.rms_norm_eps)
        self.has_qkv_bias = bool(cfg.qkv_bias)
        assert not (self.qk_norm and self.has_qkv_bias), "qk_norm and qkv_bias are not implemented together"
        if self.has_qkv_bias:  # Qwen2: q_proj / k_proj / v_proj biases as one vector in the fused weight's row order
            self.qkv_bias = nn.Parameter(torch.zeros(cfg.qkv_size))
        # sliding window of THIS layer (0: full causal attention), read per module: a per-layer schedule
        # (Qwen's max_window_layers) would only change this line
        self.window = int(cfg.sliding_window or 0)
        self.lora = None  # set by apply_lora
        self.cp_group = None  # context-parallel process group (CausalLM.enable_context_parallel)
        self.cp_layout = "zigzag"

    def rotate_qk_(self, qkv, cos, sin):
        """What this layer does to the packed qkv between the projection and attention, in place; returns qkv.
        Nothing on a NoPE layer. On a RoPE layer the rotation of the q|k columns: behind the per-head RMSNorm for a
        qk-norm layer (Qwen3: ops.qk_norm_rope_), behind the q / k / v bias for a bias layer (Qwen2:
        ops.qkv_bias_rope_, which also adds the bias to the v columns), each as one kernel. Under no_grad
        (generation) the ops keep no copy for a backward and make no autograd node; they are shape-static, so the
        graph decoders capture them."""
        c = self.cfg
        nq, nkv, D = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        if not self.use_rope:
            return qkv
        if self.qk_norm:
            return ops.qk_norm_rope_(qkv, self.q_norm.weight, self.k_norm.weight, cos, sin, nq, nkv, D,
                                     self.q_norm.eps)
        if self.has_qkv_bias:
            return ops.qkv_bias_rope_(qkv, self.qkv_bias, cos, sin, nq, nkv, D)
        return ops.rope_(qkv, cos, sin, nq, nkv, D)

    def forward(self, h, rope_cs, cu_seqlens, max_seqlen):
        c = self.cfg
        nq, nkv, D = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        mid = self.qk_norm or self.has_qkv_bias  # a node between the projection and the rotation
        win = {"window": self.window} if self.window else {}  # (a layer without a window makes the calls it made)
        assert self.use_rope or not mid, "qk-norm and qkv-bias layers rotate on every layer"
        if self.use_rope and not mid and self.cp_group is None:
            if self.lora is None:
                # projection + RoPE (GEMM epilogue) + attention as one autograd node: the backward applies the
                # inverse rotation inside the attention kernels' dq / dK epilogues
                # the o_proj backward computes the attention backward's delta in its dgrad epilogue (link: the hand-off)
                link = ops.AttnLink()
                a = ops.qkv_rope_attention(h, self.qkv_proj, rope_cs[0], rope_cs[1], cu_seqlens, max_seqlen, nq, nkv, D,
                                           link=link, **win)
                return ops.attn_out_linear(a, self.o_proj, link)
            # the LoRA-widened qkv GEMM with the RoPE epilogue + attention as one node (inverse RoPE in the backward's
            # dq / dK epilogues), the plain composition where the HIP path does not apply
            a = ops.lora_qkv_rope_attention(h, self.qkv_proj, self.lora["qkv"], rope_cs[0], rope_cs[1], cu_seqlens,
                                            max_seqlen, nq, nkv, D, **win)
            return ops.lora_linear(a, self.o_proj, self.lora["o"])
        # The unfused composition: a NoPE layer, a layer with a mid node (the fused qkv + RoPE epilogue does not
        # apply), a context-parallel layer. With a link (no LoRA, no context-parallel group) the qkv node also issues
        # o_proj's weight gradient, as one launch with its own and carried into the previous MLP's, and the attention
        # delta comes from the o_proj dgrad epilogue. The projection node saves its input, not its output, so the
        # in-place rotate_qk_ modifies nothing another node has saved.
        link = ops.AttnLink() if (self.lora is None and self.cp_group is None) else None
        if self.lora is None and self.use_rope and not mid:
            # (context parallel) projection + RoPE in one HIP GEMM (epilogue rotation) where the shapes allow
            qkv = ops.linear_rope(h, self.qkv_proj, rope_cs[0], rope_cs[1], nq, nkv, D)
        else:
            qkv = (ops.qkv_in_linear(h, self.qkv_proj, link) if self.lora is None
                   else ops.lora_linear(h, self.qkv_proj, self.lora["qkv"]))
            qkv = self.rotate_qk_(qkv, rope_cs[0], rope_cs[1])
        if self.cp_group is not None:
            from ..parallel.context_parallel import ring_attention
            assert self.window == 0, "ring attention has no sliding window (CausalLM.enable_context_parallel)"
            a = ring_attention(qkv, cu_seqlens, max_seqlen, nq, nkv, D, self.cp_group, layout=self.cp_layout)
        else:
            a = ops.flash_attention(qkv, cu_seqlens, max_seqlen, nq, nkv, D, link=link, **win)
        if link is not None:
            return ops.attn_out_linear(a, self.o_proj, link)
        return ops.linear(a, self.o_proj) if self.lora is None else ops.lora_linear(a, self.o_proj, self.lora["o"])


class MLP(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        self.gate_up_proj = nn.Parameter(torch.empty(2 * cfg.intermediate_size, cfg.hidden_size))
        self.down_proj = nn.Parameter(torch.empty(cfg.hidden_size, cfg.intermediate_size))
        self.lora = None

    def forward(self, h):
        L = self.lora
        if L is None:  # SwiGLU fused into the GEMM epilogues where the kernels apply (ops.swiglu_mlp)
            return ops.swiglu_mlp(h, self.gate_up_proj, self.down_proj)
        return ops.lora_swiglu_mlp(h, self.gate_up_proj, self.down_proj, L["gate_up"], L["down"])


def _wide_ld(lora, key: str, weight) -> int:
    """Row width of the LoRA wide weight W' that consumes this norm's output (0: none), so the norm writes its output
    straight into the left block of the consumer's widened activation X' (ops.add_rms_norm y_ld)."""
    fl = None if lora is None else lora[key]
    wide = getattr(fl, "wide", None)
    if wide is None or not any(fl.active) or weight.data_ptr() != wide.data_ptr():
        return 0
    # only where the consumer's in-place widening kernel takes the shape (else the norm writes a plain y and the
    # consumer copies it into X')
    if not ops.lora_inplace_ok(fl.in_features, fl.r * sum(1 for a in fl.active if a)):
        return 0
    return wide.shape[1]


class DecoderLayer(nn.Module):
    def __init__(self, cfg: ModelConfig, layer_idx: int):
        super().__init__()
        self.input_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)
        self.self_attn = Attention(cfg, layer_idx)
        self.post_attention_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)
        self.mlp = MLP(cfg)

    def forward(self, x, residual, rope_cs, cu_seqlens, max_seqlen):
        """Pre-norm block with the residual add fused into the norms:
        (x: previous sublayer output, residual: residual stream before adding x)."""
        ln = self.input_layernorm
        at, ml = self.self_attn, self.mlp
        h, residual = ops.add_rms_norm(x, residual, ln.weight, ln.eps, _wide_ld(at.lora, "qkv", at.qkv_proj))
        a = at(h, rope_cs, cu_seqlens, max_seqlen)
        ln2 = self.post_attention_layernorm
        h, residual = ops.add_rms_norm(a, residual, ln2.weight, ln2.eps, _wide_ld(ml.lora, "gate_up", ml.gate_up_proj))
        return ml(h), residual


class Model(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        self.embed_tokens = nn.Parameter(torch.empty(cfg.vocab_size, cfg.hidden_size))
        self.layers = nn.ModuleList([DecoderLayer(cfg, i) for i in range(cfg.num_hidden_layers)])
        self.norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)


class CausalLM(nn.Module):
    """SmolLM3ForCausalLM / LlamaForCausalLM / Qwen3ForCausalLM / Qwen2ForCausalLM equivalent."""

    def __init__(self, cfg: ModelConfig):
        super().__init__()
        self.config = cfg
        self.model = Model(cfg)
        # a reward model (cfg.num_labels == 1; HF ...ForSequenceClassification): the trunk plus score [1, hidden], no
        # LM head at all, tied or not — sequence_scores is its one output
        self.score = None
        if cfg.num_labels is not None:
            self.score = nn.Parameter(torch.empty(1, cfg.hidden_size))
        if cfg.tie_word_embeddings or cfg.num_labels is not None:
            self.lm_head = None
        else:
            self.lm_head = nn.Parameter(torch.empty(cfg.vocab_size, cfg.hidden_size))
        self.gradient_checkpointing = False
        # NEFTune (SFTTrainer.train sets it from SFTConfig.neftune_noise_alpha and restores 0 when it ends): uniform
        # noise on the embedding output in training forwards only; neftune_rank is mixed into the per-forward seed
        self.neftune_noise_alpha = 0.0
        self.neftune_rank = 0
        inv = ref.rope_inv_freq(cfg.head_dim, cfg.rope_theta, cfg.rope_scaling)
        self.register_buffer("inv_freq", inv, persistent=False)
        self._declare_uses()

    # ------------------------------------------------------------------ params
    @property
    def lm_head_weight(self) -> torch.Tensor:
        self._refuse_reward_model("the LM head")
        return self.model.embed_tokens if self.lm_head is None else self.lm_head

    @property
    def is_reward_model(self) -> bool:
        return self.score is not None

    def _refuse_reward_model(self, what: str) -> None:
        if self.score is not None:
            raise RuntimeError(f"{what} on a reward model (num_labels=1): it has a score head and no LM head; use "
                               "sequence_scores")

    def _declare_uses(self):
        for p in self.parameters():
            p._sftamd_uses = 1
        if self.lm_head is None and self.score is None:
            self.model.embed_tokens._sftamd_uses = 2

    def reset_grad_use_counters(self):
        for p in self.parameters():
            if p.requires_grad:
                p._sftamd_remaining = getattr(p, "_sftamd_uses", 1)

    def gradient_checkpointing_enable(self, **_):
        self.gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        self.gradient_checkpointing = False

    def enable_context_parallel(self, group, layout: str = "zigzag") -> None:
        """Attention over sequence chunks spread across ``group`` (ring attention, parallel/context_parallel.py).
        Inputs must then be this rank's chunk with explicit global ``position_ids`` and pre-shifted labels
        (``context_parallel.shard_batch`` with the same ``layout``). Ring attention has no sliding window: a
        windowed model is rejected here."""
        if self.config.sliding_window:
            raise NotImplementedError(
                f"sliding_window={self.config.sliding_window} with context parallelism is not supported: ring "
                "attention implements full causal attention only (use context_parallel_size=1)")
        for layer in self.model.layers:
            layer.self_attn.cp_group = group
            layer.self_attn.cp_layout = layout

    @torch.no_grad()
    def init_weights(self, seed: int = 0):
        """Random init (HF-style normal(0, initializer_range), norms = 1). Deterministic per seed
        so every DDP rank builds identical weights without a 6 GB broadcast."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        std = self.config.initializer_range
        for name, p in self.named_parameters():
            if name.endswith("layernorm.weight") or name.endswith("norm.weight"):
                p.fill_(1.0)
            elif name.endswith("qkv_bias"):
                p.zero_()  # as in HF
            elif p.device.type == "cpu":
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float32).mul_(std).to(p.dtype))
            else:
                gg = torch.Generator(device=p.device).manual_seed(seed * 1000003 + zlib.crc32(name.encode()))
                p.normal_(0.0, std, generator=gg)
        return self

    def num_parameters(self, trainable_only: bool = False) -> int:
        seen, n = set(), 0
        for p in self.parameters():
            if id(p) in seen or (trainable_only and not p.requires_grad):
                continue
            seen.add(id(p))
            n += p.numel()
        return n

    # ------------------------------------------------------------------ forward
    def _padded_meta(self, B: int, T: int, dev):
        cache = self.__dict__.setdefault("_meta_cache", {})
        key = (B, T, str(dev), self.inv_freq.data_ptr())
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 8:
                cache.clear()
            cu = torch.arange(0, (B + 1) * T, T, dtype=torch.int32, device=dev)
            hit = cache[key] = (cu, T, self.rope_tables(torch.arange(T, device=dev).expand(B, T)))
        return hit

    def _neftune_mag(self, cu_seqlens: torch.Tensor, M: int, padded) -> torch.Tensor:
        """fp32 [M]: alpha / sqrt(L_m * hidden), L_m the length of token m's sequence as attention sees it (its
        ``cu_seqlens`` segment): T for every row of a padded [B, T] batch, pads included (HF's alpha / sqrt(seq_len *
        hidden)); the sample's own length in a packed / padding-free batch (the paper's definition; HF on a flattened
        [1, total] batch would use the total, an artefact of that layout); the global length, local length x group
        size, under context parallelism. Built on the device, no host sync; a cached constant for the padded shapes
        of ``_padded_meta``. ``padded`` is (B, T) for such a batch, else None."""
        alpha, H = float(self.neftune_noise_alpha), self.config.hidden_size
        group = self.model.layers[0].self_attn.cp_group if len(self.model.layers) else None
        cp = torch.distributed.get_world_size(group) if group is not None else 1
        dev = cu_seqlens.device
        if padded is not None:
            cache = self.__dict__.setdefault("_neftune_cache", {})
            key = (padded, str(dev), alpha, cp)
            hit = cache.get(key)
            if hit is None:
                if len(cache) >= 8:
                    cache.clear()
                hit = cache[key] = torch.full((M,), alpha / math.sqrt(padded[1] * cp * H), dtype=torch.float32,
                                              device=dev)
            return hit
        cu = cu_seqlens.to(torch.int64)
        # (rows past the last boundary, if any, form a segment of their own, so the lengths always sum to M)
        lens = torch.cat([cu[1:] - cu[:-1], (M - cu[-1:]).clamp(min=0)])
        per_seq = alpha * torch.rsqrt(lens.clamp(min=1).to(torch.float32) * float(cp * H))
        return torch.repeat_interleave(per_seq, lens, output_size=int(M))

    def rope_tables(self, position_ids: torch.Tensor):
        freqs = position_ids.reshape(-1).float()[:, None] * self.inv_freq[None, :].to(position_ids.device)
        return freqs.cos().contiguous(), freqs.sin().contiguous()

    def forward(self, input_ids: torch.Tensor, labels: Optional[torch.Tensor] = None,
                cu_seqlens: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None,
                position_ids: Optional[torch.Tensor] = None, num_items_in_batch=None,
                return_logits: bool = False, shift_labels: bool = True, label_smoothing: float = 0.0,
                loss_type: str = "nll", **_) -> CausalLMOutput:
        """input_ids [B, T] (padded, right) or [M] (packed with cu_seqlens).

        ``labels`` are unshifted HF-style labels (-100 ignored) unless ``shift_labels=False``.
        Loss = sum of token CE / num_items_in_batch (HF ``num_items_in_batch`` semantics), or the
        mean over valid tokens when ``num_items_in_batch`` is None. ``label_smoothing`` (HF ``LabelSmoother``) and
        ``loss_type="dft"`` (TRL ``dft_loss``) change the per-token objective inside the fused cross-entropy.
        """
        self._refuse_reward_model("forward (a language-model loss or logits)")
        dev = input_ids.device
        h, labels, _ = self._hidden(input_ids, labels, cu_seqlens, max_seqlen, position_ids, shift_labels)

        out = CausalLMOutput()
        if labels is not None:
            valid = labels != -100
            inv = _inv_count(num_items_in_batch, valid, dev)
            out.loss, out.stats = ops.lm_head_cross_entropy(h, self.lm_head_weight, labels, inv, label_smoothing,
                                                            loss_type)
            vf = valid.float()
            out.num_tokens = vf.sum()
            # TRL-style training metrics from the same fused CE pass: [correct, entropy_sum, valid]
            out.metrics = torch.stack([out.stats[3].sum(), (out.stats[2] * vf).sum(), out.num_tokens])
        if return_logits or labels is None:
            out.logits = torch.nn.functional.linear(h, self.lm_head_weight)
        return out

    def sequence_logps(self, input_ids: torch.Tensor, labels: torch.Tensor, cu_seqlens: Optional[torch.Tensor] = None,
                       position_ids: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None,
                       n_seqs: Optional[int] = None, shift_labels: bool = True):
        """Per-sequence log-probabilities log pi(y | x) = sum of the label tokens' log-probabilities (-100 ignored) of
        the first ``n_seqs`` segments of ``cu_seqlens`` (default: all of them; every row of a padded [B, T] batch).
        Returns (logps fp32 [n_seqs], differentiable; the fused cross-entropy's stats [4, M]). The trunk is
        ``forward``'s. Sequence-level objectives (DPO) build on this."""
        self._refuse_cp("sequence_logps")
        h, labels, cu_seqlens = self._hidden(input_ids, labels, cu_seqlens, max_seqlen, position_ids, shift_labels)
        if n_seqs is None:
            n_seqs = cu_seqlens.numel() - 1
        return ops.lm_head_seq_logps(h, self.lm_head_weight, labels, cu_seqlens, int(n_seqs))

    def _refuse_cp(self, what: str) -> None:
        self._refuse_reward_model(what)
        if len(self.model.layers) and self.model.layers[0].self_attn.cp_group is not None:
            raise NotImplementedError(f"{what} under context parallelism: a sequence's label rows are spread over "
                                      "the group's ranks and the per-sequence sum is not reduced across them")

    def sequence_scores(self, input_ids: torch.Tensor, cu_seqlens: Optional[torch.Tensor] = None,
                        position_ids: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None,
                        n_seqs: Optional[int] = None, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A reward model's scores, fp32 [n_seqs], differentiable: the final hidden state of each sequence's LAST token
        times the ``score`` head (``ops.seq_score``; HF ``...ForSequenceClassification`` logits[:, 0]). Padding-free
        ``input_ids`` [M] with ``cu_seqlens`` score the first ``n_seqs`` segments (default: all of them). A padded
        (right) [B, T] batch scores column ``lengths[b] - 1`` of row b (default T - 1): the same op over a cu_seqlens
        built from the lengths, attention still running over the whole rows. The trunk is ``forward``'s."""
        if self.score is None:
            raise RuntimeError("sequence_scores needs a reward model: build it with num_labels=1 (it has a score head "
                               "in place of the LM head)")
        if len(self.model.layers) and self.model.layers[0].self_attn.cp_group is not None:
            raise NotImplementedError("sequence_scores under context parallelism: a sequence's last row lives on one "
                                      "rank of the group and the score is not shared across them")
        padded = input_ids.dim() == 2 and cu_seqlens is None
        if lengths is not None and not padded:
            raise ValueError("lengths go with a padded [B, T] batch; a padding-free batch has cu_seqlens")
        h, _, cu = self._hidden(input_ids, None, cu_seqlens, max_seqlen, position_ids, False)
        if padded and lengths is not None:
            B, T = input_ids.shape
            # a non-decreasing cu over the B T rows: segment 2b = row b's tokens [b T, b T + len_b), segment 2b + 1 =
            # its padding; the even segments are the scores (a zero length scores +0)
            ln = lengths.to(device=h.device, dtype=torch.int64).clamp(0, T)
            start = torch.arange(B, device=h.device, dtype=torch.int64) * T
            cu2 = torch.stack([start, start + ln], dim=1).reshape(-1)
            cu2 = torch.cat([cu2, cu2.new_full((1,), B * T)]).to(torch.int32)
            return ops.seq_score(h, self.score, cu2, 2 * B)[0::2]
        if n_seqs is None:
            n_seqs = cu.numel() - 1
        return ops.seq_score(h, self.score, cu, int(n_seqs))

    def policy_loss(self, input_ids: torch.Tensor, labels: torch.Tensor, advantages: torch.Tensor,
                    cu_seqlens: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
                    max_seqlen: Optional[int] = None, n_seqs: Optional[int] = None, shift_labels: bool = True,
                    num_items_in_batch=None, old_logps: Optional[torch.Tensor] = None,
                    ref_logps: Optional[torch.Tensor] = None, eps_low: float = 0.2, eps_high: float = 0.2,
                    beta: float = 0.0, temperature: float = 1.0, per_seq_mean: bool = False) -> CausalLMOutput:
        """The GRPO family's clipped policy objective over the completion rows (label not -100) of the first
        ``n_seqs`` segments, each sequence weighted by its entry of ``advantages`` [n_seqs], normalised by
        ``num_items_in_batch`` (and, with ``per_seq_mean``, by each sequence's completion length first).
        ``old_logps`` / ``ref_logps`` are fp32 per row [M] as ``token_logps`` returns them, or None (ratio exactly 1 /
        no KL term). ``stats`` is the cross-entropy's [4, M] at ``temperature``; ``rows`` [2, M] and ``seq`` [6, n_seqs]
        are ``ops.lm_head_policy_loss``'s. The trunk is ``forward``'s."""
        self._refuse_cp("policy_loss")
        dev = input_ids.device
        h, labels, cu_seqlens = self._hidden(input_ids, labels, cu_seqlens, max_seqlen, position_ids, shift_labels)
        if n_seqs is None:
            n_seqs = cu_seqlens.numel() - 1
        inv = _inv_count(num_items_in_batch, labels != -100, dev)
        out = CausalLMOutput()
        out.loss, out.stats, out.rows, out.seq = ops.lm_head_policy_loss(
            h, self.lm_head_weight, labels, advantages, cu_seqlens, int(n_seqs), inv, old_logps, ref_logps, eps_low,
            eps_high, beta, temperature, per_seq_mean)
        out.num_tokens = out.seq[1].sum()
        return out

    def token_logps(self, input_ids: torch.Tensor, labels: torch.Tensor, cu_seqlens: Optional[torch.Tensor] = None,
                    position_ids: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None,
                    shift_labels: bool = True, temperature: float = 1.0) -> torch.Tensor:
        """fp32 [M]: every row's log softmax(logits / temperature) at its (shifted) label, 0 where the label is -100;
        no autograd graph through the LM head (call it under ``torch.no_grad()``). The trunk is ``forward``'s."""
        self._refuse_cp("token_logps")
        h, labels, _ = self._hidden(input_ids, labels, cu_seqlens, max_seqlen, position_ids, shift_labels)
        return ops.lm_head_token_logps(h, self.lm_head_weight, labels, temperature)

    def logits_rows(self, input_ids: torch.Tensor, cu_seqlens: Optional[torch.Tensor] = None,
                    position_ids: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None) -> torch.Tensor:
        """The logits of every token row, [M, vocab] in the model's dtype (M = B x T of a padded batch, pads included),
        without an autograd graph through the LM head: what a distillation teacher hands to the student's
        ``distill_loss`` (call it under ``torch.no_grad()``). The trunk is ``forward``'s."""
        self._refuse_reward_model("logits_rows")
        h, _, _ = self._hidden(input_ids, None, cu_seqlens, max_seqlen, position_ids, False)
        return ops.lm_head_logits(h, self.lm_head_weight)

    def distill_loss(self, input_ids: torch.Tensor, labels: torch.Tensor, teacher_logits: torch.Tensor,
                     cu_seqlens: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None,
                     position_ids: Optional[torch.Tensor] = None, num_items_in_batch=None, shift_labels: bool = True,
                     beta: float = 0.5, temperature: float = 1.0, **_) -> CausalLMOutput:
        """Knowledge distillation (TRL ``GKDTrainer.generalized_jsd_loss``): the generalized JSD between this model's
        and a teacher's token distributions over the rows whose shifted label is not -100, summed and divided by
        ``num_items_in_batch`` (the mean over those rows when None), exactly as ``forward`` normalises the
        cross-entropy. ``teacher_logits`` [M, vocab] are a teacher's ``logits_rows`` of the same batch. ``stats`` is
        [5, M] (loss, student lse, teacher lse, correct, agrees with the teacher's argmax) and ``metrics`` =
        [correct, teacher-agreement count, valid]."""
        self._refuse_reward_model("distill_loss")
        dev = input_ids.device
        h, labels, _ = self._hidden(input_ids, labels, cu_seqlens, max_seqlen, position_ids, shift_labels)
        valid = labels != -100
        inv = _inv_count(num_items_in_batch, valid, dev)
        out = CausalLMOutput()
        out.loss, out.stats = ops.lm_head_distill_loss(h, self.lm_head_weight, teacher_logits, labels, inv, beta,
                                                       temperature)
        out.num_tokens = valid.float().sum()
        out.metrics = torch.stack([out.stats[3].sum(), out.stats[4].sum(), out.num_tokens])
        return out

    def topk_logps_rows(self, input_ids: torch.Tensor, cu_seqlens: Optional[torch.Tensor] = None,
                        position_ids: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None, k: int = 64,
                        temperature: float = 1.0):
        """A teacher's top-``k`` token log-probabilities of every token row, (ids int32 [M, k], logps fp32 [M, k])
        with M as in ``logits_rows``: the k largest logits (value descending, equal values by column ascending) and
        log softmax(logits / temperature) there. What offline distillation caches and the student's
        ``distill_topk_loss`` consumes (call it under ``torch.no_grad()``). The trunk is ``forward``'s."""
        self._refuse_cp("topk_logps_rows")
        h, _, _ = self._hidden(input_ids, None, cu_seqlens, max_seqlen, position_ids, False)
        return ops.lm_head_topk_logps(h, self.lm_head_weight, int(k), temperature)

    def distill_topk_loss(self, input_ids: torch.Tensor, labels: torch.Tensor, teacher_ids: torch.Tensor,
                          teacher_logps: torch.Tensor, cu_seqlens: Optional[torch.Tensor] = None,
                          max_seqlen: Optional[int] = None, position_ids: Optional[torch.Tensor] = None,
                          num_items_in_batch=None, shift_labels: bool = True, temperature: float = 1.0,
                          **_) -> CausalLMOutput:
        """Offline knowledge distillation: the forward KL(teacher || student) over the teacher's top-k support, not
        renormalised, from a teacher's cached ``topk_logps_rows`` of the same batch (``teacher_ids`` int32 and
        ``teacher_logps`` fp32, [M, k] or [B, T, k]) at the same ``temperature``. Rows, normalisation, ``stats`` layout
        and ``metrics`` are ``distill_loss``'s, with the teacher mass kept in ``stats[2]`` and the teacher's first
        cached id in the agreement count."""
        self._refuse_cp("distill_topk_loss")
        dev = input_ids.device
        h, labels, _ = self._hidden(input_ids, labels, cu_seqlens, max_seqlen, position_ids, shift_labels)
        valid = labels != -100
        inv = _inv_count(num_items_in_batch, valid, dev)
        out = CausalLMOutput()
        k = teacher_ids.shape[-1]
        out.loss, out.stats = ops.lm_head_distill_topk_loss(h, self.lm_head_weight, teacher_ids.reshape(-1, k),
                                                            teacher_logps.reshape(-1, k), labels, inv, temperature)
        vf = valid.float()
        out.num_tokens = vf.sum()
        out.metrics = torch.stack([out.stats[3].sum(), out.stats[4].sum(), out.num_tokens])
        out.teacher_mass = (out.stats[2] * vf).sum()
        return out

    def _hidden(self, input_ids, labels, cu_seqlens, max_seqlen, position_ids, shift_labels):
        """The trunk shared by ``forward``, ``sequence_logps``, ``policy_loss``, ``token_logps``, ``logits_rows``,
        ``distill_loss``, ``topk_logps_rows`` and ``distill_topk_loss``: batch metadata, embedding (NEFTune in training),
        the decoder layers and the final norm.
        Returns (h [M, hidden], the shifted flat labels or None, cu_seqlens)."""
        dev = input_ids.device
        rope_cs = None
        padded = tuple(input_ids.shape) if input_ids.dim() == 2 and cu_seqlens is None else None
        if input_ids.dim() == 2 and cu_seqlens is None and position_ids is None:
            # padded batches of one shape repeat every step: cu_seqlens / RoPE tables are built once
            cu_seqlens, max_seqlen, rope_cs = self._padded_meta(input_ids.shape[0], input_ids.shape[1], dev)
        if input_ids.dim() == 2:
            B, T = input_ids.shape
            if cu_seqlens is None:
                cu_seqlens = torch.arange(0, (B + 1) * T, T, dtype=torch.int32, device=dev)
                max_seqlen = T
            if position_ids is None:
                position_ids = torch.arange(T, device=dev).expand(B, T)
            if labels is not None and shift_labels:
                labels = torch.cat([labels[:, 1:], torch.full_like(labels[:, :1], -100)], dim=1)
                shift_labels = False
        ids = input_ids.reshape(-1)
        M = ids.numel()
        if cu_seqlens is None:
            cu_seqlens = torch.tensor([0, M], dtype=torch.int32, device=dev)
            max_seqlen = M
        if max_seqlen is None:
            max_seqlen = int((cu_seqlens[1:] - cu_seqlens[:-1]).max().item())
        if position_ids is None:
            position_ids = _positions_from_cu(cu_seqlens, M)
        if labels is not None:
            labels = labels.reshape(-1)
            if shift_labels:
                labels = _shift_packed(labels, cu_seqlens)
        if rope_cs is None:
            rope_cs = self.rope_tables(position_ids)

        if self.training and torch.is_grad_enabled() and (self.neftune_noise_alpha or 0) > 0:
            x = ops.noisy_embedding(ids, self.model.embed_tokens, self._neftune_mag(cu_seqlens, M, padded),
                                    ops.neftune_seed(self.neftune_rank))
        else:
            x = ops.embedding(ids, self.model.embed_tokens)
        residual = None
        ckpt = self.gradient_checkpointing and self.training and torch.is_grad_enabled()
        # (a layer's o_proj + qkv weight gradients join the previous layer's MLP launch: ops.wgrad_carry_scope)
        with ops.wgrad_carry_scope(enabled=not ckpt):
            for layer in self.model.layers:
                if ckpt:
                    x, residual = checkpoint(layer, x, residual, rope_cs, cu_seqlens, max_seqlen, use_reentrant=False)
                else:
                    x, residual = layer(x, residual, rope_cs, cu_seqlens, max_seqlen)
        n = self.model.norm
        h, _ = ops.add_rms_norm(x, residual, n.weight, n.eps)
        return h, labels, cu_seqlens

    # ------------------------------------------------------------------ HF state dict
    def hf_state_dict(self) -> Dict[str, torch.Tensor]:
        """State dict with HF key names (q/k/v and gate/up split, tied lm_head omitted)."""
        cfg = self.config
        sd = {"model.embed_tokens.weight": self.model.embed_tokens.detach()}
        for i, l in enumerate(self.model.layers):
            p = f"model.layers.{i}."
            q, k, v = l.self_attn.qkv_proj.detach().split([cfg.q_size, cfg.kv_size, cfg.kv_size], 0)
            sd[p + "self_attn.q_proj.weight"] = q
            sd[p + "self_attn.k_proj.weight"] = k
            sd[p + "self_attn.v_proj.weight"] = v
            sd[p + "self_attn.o_proj.weight"] = l.self_attn.o_proj.detach()
            if l.self_attn.qk_norm:
                sd[p + "self_attn.q_norm.weight"] = l.self_attn.q_norm.weight.detach()
                sd[p + "self_attn.k_norm.weight"] = l.self_attn.k_norm.weight.detach()
            if l.self_attn.has_qkv_bias:
                bq, bk, bv = l.self_attn.qkv_bias.detach().split([cfg.q_size, cfg.kv_size, cfg.kv_size], 0)
                sd[p + "self_attn.q_proj.bias"] = bq
                sd[p + "self_attn.k_proj.bias"] = bk
                sd[p + "self_attn.v_proj.bias"] = bv
            g, u = l.mlp.gate_up_proj.detach().split([cfg.intermediate_size] * 2, 0)
            sd[p + "mlp.gate_proj.weight"] = g
            sd[p + "mlp.up_proj.weight"] = u
            sd[p + "mlp.down_proj.weight"] = l.mlp.down_proj.detach()
            sd[p + "input_layernorm.weight"] = l.input_layernorm.weight.detach()
            sd[p + "post_attention_layernorm.weight"] = l.post_attention_layernorm.weight.detach()
        sd["model.norm.weight"] = self.model.norm.weight.detach()
        if self.lm_head is not None:
            sd["lm_head.weight"] = self.lm_head.detach()
        if self.score is not None:
            sd["score.weight"] = self.score.detach()
        return sd

    @torch.no_grad()
    def load_hf_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        cfg = self.config
        used = set()

        def take(key):
            used.add(key)
            return sd[key]

        self.model.embed_tokens.copy_(take("model.embed_tokens.weight"))
        for i, l in enumerate(self.model.layers):
            p = f"model.layers.{i}."
            l.self_attn.qkv_proj.copy_(torch.cat([take(p + "self_attn.q_proj.weight"),
                                                  take(p + "self_attn.k_proj.weight"),
                                                  take(p + "self_attn.v_proj.weight")], 0))
            l.self_attn.o_proj.copy_(take(p + "self_attn.o_proj.weight"))
            if l.self_attn.qk_norm:
                l.self_attn.q_norm.weight.copy_(take(p + "self_attn.q_norm.weight"))
                l.self_attn.k_norm.weight.copy_(take(p + "self_attn.k_norm.weight"))
            if l.self_attn.has_qkv_bias:
                l.self_attn.qkv_bias.copy_(torch.cat([take(p + "self_attn.q_proj.bias"),
                                                      take(p + "self_attn.k_proj.bias"),
                                                      take(p + "self_attn.v_proj.bias")], 0))
            l.mlp.gate_up_proj.copy_(torch.cat([take(p + "mlp.gate_proj.weight"), take(p + "mlp.up_proj.weight")], 0))
            l.mlp.down_proj.copy_(take(p + "mlp.down_proj.weight"))
            l.input_layernorm.weight.copy_(take(p + "input_layernorm.weight"))
            l.post_attention_layernorm.weight.copy_(take(p + "post_attention_layernorm.weight"))
        self.model.norm.weight.copy_(take("model.norm.weight"))
        if self.lm_head is not None:
            self.lm_head.copy_(take("lm_head.weight"))
        if self.score is not None and "score.weight" in sd:
            # (a causal-LM state dict has none: the head keeps its initialisation, the LM head is dropped below)
            self.score.copy_(take("score.weight"))
        extra = set(sd) - used - {"lm_head.weight"}
        if strict and extra:
            raise KeyError(f"unexpected keys: {sorted(extra)[:8]}")
        return self


def _positions_from_cu(cu: torch.Tensor, M: int) -> torch.Tensor:
    idx = torch.arange(M, device=cu.device)
    seq = torch.searchsorted(cu[1:].to(torch.int64), idx, right=True)
    return idx - cu.to(torch.int64)[seq.clamp(max=cu.numel() - 2)]


def _shift_packed(labels: torch.Tensor, cu: torch.Tensor) -> torch.Tensor:
    out = torch.cat([labels[1:], labels.new_full((1,), -100)])
    ends = cu[1:].to(torch.int64) - 1
    ends = ends[ends >= 0]
    out[ends] = -100
    return out


def _inv_count(num_items_in_batch, valid: torch.Tensor, dev) -> torch.Tensor:
    """fp32 [1] on ``dev``: 1 / num_items_in_batch (HF semantics: a number, a tensor, or the trainer's in-flight global
    count, PendingCount), or 1 / the number of ``valid`` rows (at least 1) when it is None."""
    if hasattr(num_items_in_batch, "resolve"):
        num_items_in_batch = num_items_in_batch.resolve()
    if num_items_in_batch is None:
        cnt = valid.sum().clamp(min=1)
    elif torch.is_tensor(num_items_in_batch):
        cnt = num_items_in_batch
    else:
        cnt = torch.tensor(float(num_items_in_batch))
    return (1.0 / cnt.to(device=dev, dtype=torch.float32)).reshape(1)


def build_model(cfg: ModelConfig, device="cpu", dtype=torch.bfloat16, seed: int = 0) -> CausalLM:
    with torch.device("meta"):
        m = CausalLM(cfg)
    m = m.to_empty(device=device)
    m.inv_freq = ref.rope_inv_freq(cfg.head_dim, cfg.rope_theta, cfg.rope_scaling, device=device)
    for p in m.parameters():
        p.data = p.data.to(dtype)
    m._declare_uses()
    m.init_weights(seed)
    return m
