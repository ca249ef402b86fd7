"""``RewardTrainer``: reward modelling on preference pairs (TRL ``RewardTrainer``) on the ``SFTTrainer`` engine.

The step is ``SFTTrainer``'s — DDP engine, ``no_sync`` gradient accumulation, clipping, flat AdamW, ZeRO-1, heartbeat,
checkpoints — with ``CausalLM.sequence_scores`` -> ``ops.reward_pair_loss`` -> ``backward`` in place of
``model(...).loss``. The model is a reward model (``num_labels=1``: the trunk plus a score head, no LM head); a preset
name or a causal-LM directory given as ``model=`` is read as one, with a fresh head. The loss, per pair
``-logsigmoid(r_chosen - r_rejected - margin) + center_rewards_coefficient (r_chosen + r_rejected)^2``, is normalised
by the GLOBAL number of pairs of the optimizer step (``global_num_items`` with ``num_items`` = pairs).

Rows are ``{"chosen", "rejected"}`` with an optional ``"prompt"`` (``data.preference``: with a prompt exactly
``DPOTrainer``'s tokenisation; without one TRL's implicit-prompt format) and an optional numeric ``"margin"``, which
travels on the collator indexed by pair. An already tokenised ``TokenizedDataset`` of 2N sequences is taken as it is.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Any, Dict, List, Optional

import torch

from .. import ops
from ..data.collator import DataLoader, DistributedBatchSampler
from ..data.dataset import TokenizedDataset
from ..data.preference import PreferenceCollator, cached_tokenize_preferences, preference_margins
from ..models import CausalLM, build_model, get_config
from ..parallel.process_group import barrier, setup_distributed
from . import checkpoint as ckpt
from .config import RewardConfig
from .trainer import SFTTrainer

# the accumulator after the loss: pairs with r_c > r_r, sum of r_c - r_r, sum of all rewards, pairs
_ACC, _MARGIN, _REWARD, _PAIRS = range(1, 5)


def load_reward_model(model, device, seed: int = 0) -> CausalLM:
    """``model`` as a reward model on ``device``: a preset name (built with ``num_labels=1``), a local HF directory (a
    ``...ForSequenceClassification`` one as saved; a causal-LM one keeps its trunk, drops ``lm_head.weight`` and gets a
    fresh head from ``seed``), or a model object that already has a score head."""
    if isinstance(model, str):
        if os.path.isdir(model) and any(f.endswith(".safetensors") for f in os.listdir(model)):
            model = ckpt.from_pretrained(model, device=device, dtype=torch.bfloat16, num_labels=1, seed=seed)
        else:
            cfg = dataclasses.replace(get_config(model), num_labels=1)
            model = build_model(cfg, device=device, dtype=torch.bfloat16, seed=seed)
    if not isinstance(model, CausalLM) or model.score is None:
        raise TypeError("a reward model is expected: a preset name, a local HF directory, or a model built with "
                        f"num_labels=1 (got {type(model).__name__} without a score head)")
    return model


class RewardTrainer(SFTTrainer):
    _acc_size = 5

    def __init__(self, model=None, args: Optional[RewardConfig] = None, train_dataset=None, eval_dataset=None, **kw):
        args = args or RewardConfig()
        if not isinstance(args, RewardConfig):
            raise TypeError("RewardTrainer expects a RewardConfig")
        if int(getattr(args, "context_parallel_size", 1) or 1) > 1:
            raise NotImplementedError("RewardTrainer under context parallelism: a sequence's last row lives on one "
                                      "rank of a context-parallel group")
        if kw.get("data_collator") is not None:
            raise ValueError("RewardTrainer builds its own PreferenceCollator")
        args.validate_objective()
        dist = setup_distributed(timeout_s=args.ddp_timeout, verbose=False)
        model = load_reward_model(model, dist.device, seed=kw.get("model_init_seed", 0))
        self._margins: Dict[str, Optional[torch.Tensor]] = {}
        self._prepare_slot = "train"
        super().__init__(model, args, train_dataset, eval_dataset, **kw)
        for ds in (self.train_dataset, self.eval_dataset):
            if ds is not None and len(ds) % 2:
                raise ValueError("a preference dataset holds 2N sequences (chosen at 2i, rejected at 2i + 1)")
        pad_mult = args.pad_to_multiple_of
        if pad_mult is None and self.dist.device.type == "cuda":
            pad_mult = 256
        self.packed = True
        self.collator = PreferenceCollator(self._pad_id, pad_mult, margins=self._margins.get("train"))
        self.eval_collator = PreferenceCollator(self._pad_id, pad_mult, margins=self._margins.get("eval"))
        self._center = float(args.center_rewards_coefficient or 0.0)
        self._extremes = {"train": None, "eval": None}  # running (max reward, max of -reward) of a log window / an eval

    # ------------------------------------------------------------------ data
    def _sparse_cap(self) -> int:
        return 0  # (a batch holds 2 x batch-size sequences: every rank measures its pass)

    def _prepare(self, ds, limit):
        # (called for the train set, then the eval set, by the base constructor; by evaluate() for a new eval set)
        slot, self._prepare_slot = self._prepare_slot, "eval"
        if ds is None or isinstance(ds, TokenizedDataset):
            self._margins[slot] = None
            return ds
        rows = list(ds) if not isinstance(ds, list) else ds
        if limit:
            rows = rows[:limit]
        self._margins[slot] = preference_margins(rows)
        return cached_tokenize_preferences(rows, self.tokenizer, self._cache_dir(), is_main=self.dist.is_main,
                                           barrier=barrier if self.dist.world_size > 1 else None,
                                           max_length=self.args.max_length, max_prompt_length=None)

    def _loader(self, ds, collator, batch_size, **sampler_kw) -> DataLoader:
        a = self.args
        s = DistributedBatchSampler(len(ds) // 2, batch_size, self.dp_size, self.dp_rank,
                                    drop_last=a.dataloader_drop_last, **sampler_kw)
        return DataLoader(ds, collator, s, self.dist.device, a.dataloader_pin_memory, a.prefetch_batches)

    def get_train_dataloader(self) -> DataLoader:
        a = self.args
        return self._loader(self.train_dataset, self.collator, a.per_device_train_batch_size, shuffle=True,
                            seed=a.data_seed or a.seed)

    def get_eval_dataloader(self) -> DataLoader:
        return self._loader(self.eval_dataset, self.eval_collator, self.args.per_device_eval_batch_size, shuffle=False)

    def _merge_micro(self, micro: List[Dict]) -> List[Dict]:
        # GA micro-batches stay separate passes: a merged varlen batch would interleave each micro-batch's pad segment
        # with the sequences, and sequence_scores takes the first n_seqs segments
        return micro

    # ------------------------------------------------------------------ objective
    def _pair_loss(self, b: Dict, inv_pairs, slot: str):
        scores = self.model.sequence_scores(b["input_ids"], cu_seqlens=b["cu_seqlens"], position_ids=b["position_ids"],
                                            max_seqlen=b["max_seqlen"], n_seqs=b["n_seqs"])
        if hasattr(inv_pairs, "resolve"):  # the in-flight global pair count: awaited after the trunk
            inv_pairs = inv_pairs.resolve()
        if not torch.is_tensor(inv_pairs):
            inv_pairs = torch.tensor(float(inv_pairs))
        inv = (1.0 / inv_pairs.to(device=scores.device, dtype=torch.float32)).reshape(1)
        loss, st = ops.reward_pair_loss(scores, b.get("margins"), inv, self._center)
        r = scores.detach().float().view(-1, 2)
        metrics = torch.stack([(r[:, 0] > r[:, 1]).float().sum(), (r[:, 0] - r[:, 1]).sum(), r.sum(),
                               r.new_full((), float(r.shape[0]))])
        ext = torch.stack([r.max(), (-r).max()])
        prev = self._extremes[slot]
        self._extremes[slot] = ext if prev is None else torch.maximum(prev, ext)
        return loss, metrics

    def _micro_loss(self, b: Dict, n_items):
        return self._pair_loss(b, n_items, "train")

    def _eval_loss(self, b: Dict):
        return self._pair_loss(b, 1.0, "eval")

    def _take_extremes(self, slot: str):
        """(min, max) reward since the last call, over every rank (a MAX all-reduce of (max, -min))."""
        ext, self._extremes[slot] = self._extremes[slot], None
        if ext is None:
            ext = torch.full((2,), float("-inf"), device=self.dist.device)
        if self.dist.world_size > 1:
            torch.distributed.all_reduce(ext, op=torch.distributed.ReduceOp.MAX)
        mx, neg_mn = ext.tolist()
        return -neg_mn, mx

    def _reward_entries(self, v: List[float], slot: str, prefix: str = "") -> Dict[str, float]:
        p = max(v[_PAIRS], 1.0)
        mn, mx = self._take_extremes(slot)
        return {f"{prefix}accuracy": v[_ACC] / p, f"{prefix}margin": v[_MARGIN] / p,
                f"{prefix}mean_reward": v[_REWARD] / (2.0 * p), f"{prefix}min_reward": mn, f"{prefix}max_reward": mx}

    def _train_logs(self, v: List[float], steps: int, common: Dict[str, Any]) -> Dict[str, Any]:
        return {"loss": v[0] / steps, **self._reward_entries(v, "train"), **common}

    def _eval_logs(self, v: List[float], prefix: str, common: Dict[str, Any]) -> Dict[str, Any]:
        return {f"{prefix}_loss": v[0] / max(v[_PAIRS], 1.0), **common, **self._reward_entries(v, "eval", f"{prefix}_")}

    def evaluate(self, eval_dataset=None, metric_key_prefix: str = "eval") -> Dict[str, float]:
        if eval_dataset is not None:
            self._prepare_slot = "eval"
            self.eval_dataset = self._prepare(eval_dataset, self.args.max_eval_samples)
            self.eval_collator.margins = self._margins.get("eval")
        if self.eval_dataset is None:
            return {}
        self._extremes["eval"] = None
        return super().evaluate(None, metric_key_prefix)
