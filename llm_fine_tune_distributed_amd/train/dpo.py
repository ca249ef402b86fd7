"""``DPOTrainer``: Direct Preference Optimization (sigmoid loss) on the ``SFTTrainer`` engine.

The step is ``SFTTrainer``'s — DDP engine, ``no_sync`` gradient accumulation, clipping, flat AdamW, ZeRO-1, heartbeat —
with ``CausalLM.sequence_logps`` -> ``ops.dpo_loss`` -> ``backward`` in place of ``model(...).loss``. The loss is
normalised by the GLOBAL number of pairs of the optimizer step (``global_num_items`` with ``num_items`` = pairs).

Reference log-probabilities are always precomputed (TRL ``precompute_ref_log_probs=True``): one no-grad, eval-mode
pass over the train and eval sets at the start of ``train()``, with the model as it then stands (fresh LoRA adapters
have B = 0, so that is the base model) or with ``ref_model=``, written to ``output_dir/ref_logps-<fingerprint>.pt``.
A resume loads that file and fails if it is missing: the resumed weights are not the reference.
"""
from __future__ import annotations

import hashlib
import os
from typing import Any, Dict, List, Optional

import torch

from .. import ops
from ..data.collator import DataLoader, DistributedBatchSampler
from ..data.dataset import TokenizedDataset
from ..data.preference import PreferenceCollator, cached_tokenize_preferences
from ..models import CausalLM, build_model, get_config
from ..parallel.process_group import all_reduce_sum_, barrier
from . import checkpoint as ckpt
from .config import DPOConfig
from .trainer import SFTTrainer, TrainOutput


class DPOTrainer(SFTTrainer):
    # loss, reward_chosen, reward_rejected, accurate pairs, margin, logp_chosen, logp_rejected, pairs
    _acc_size = 8

    def __init__(self, model=None, args: Optional[DPOConfig] = None, train_dataset=None, eval_dataset=None,
                 ref_model=None, **kw):
        args = args or DPOConfig()
        if not isinstance(args, DPOConfig):
            raise TypeError("DPOTrainer expects a DPOConfig")
        if int(getattr(args, "context_parallel_size", 1) or 1) > 1:
            raise NotImplementedError("DPOTrainer under context parallelism: per-sequence log-probabilities are not "
                                      "reduced across a context-parallel group")
        if kw.get("data_collator") is not None:
            raise ValueError("DPOTrainer builds its own PreferenceCollator")
        self._ref_model = ref_model
        self._ref_ready = False
        super().__init__(model, args, train_dataset, eval_dataset, **kw)
        for ds in (self.train_dataset, self.eval_dataset):
            if ds is not None and (len(ds) % 2 or ds.loss_start is None):
                raise ValueError("a preference dataset holds 2N sequences (chosen at 2i, rejected at 2i + 1) with "
                                 "loss_start = the prompt length")
        pad_mult = args.pad_to_multiple_of
        if pad_mult is None and self.dist.device.type == "cuda":
            pad_mult = 256
        self.packed = True
        self.collator = PreferenceCollator(self._pad_id, pad_mult)       # carries the train set's ref_logps
        self.eval_collator = PreferenceCollator(self._pad_id, pad_mult)  # the eval set's

    # ------------------------------------------------------------------ data
    def _sparse_cap(self) -> int:
        return 0  # (a batch holds 2 x batch-size sequences: every rank measures its pass)

    def _prepare(self, ds, limit):
        if ds is None or isinstance(ds, TokenizedDataset):
            return ds
        rows = list(ds) if not isinstance(ds, list) else ds
        if limit:
            rows = rows[:limit]
        return cached_tokenize_preferences(rows, self.tokenizer, self._cache_dir(), is_main=self.dist.is_main,
                                           barrier=barrier if self.dist.world_size > 1 else None,
                                           max_length=self.args.max_length,
                                           max_prompt_length=self.args.max_prompt_length)

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
        # with the sequences, and sequence_logps takes the first n_seqs segments
        return micro

    # ------------------------------------------------------------------ reference log-probs
    def _ref_fingerprint(self) -> str:
        h = hashlib.sha256()
        for ds in (self.train_dataset, self.eval_dataset):
            if ds is None:
                h.update(b"none")
                continue
            for t in (ds.tokens, ds.offsets, ds.loss_start):
                h.update(t.contiguous().cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    def ref_logps_path(self) -> str:
        return os.path.join(self.args.output_dir, f"ref_logps-{self._ref_fingerprint()}.pt")

    @staticmethod
    def _seq_inputs(b: Dict) -> Dict:
        return dict(input_ids=b["input_ids"], labels=b["labels"], cu_seqlens=b["cu_seqlens"],
                    position_ids=b["position_ids"], max_seqlen=b["max_seqlen"], n_seqs=b["n_seqs"],
                    shift_labels=not b.get("shifted", False))

    @torch.no_grad()
    def _compute_ref(self, model: CausalLM, ds: Optional[TokenizedDataset]) -> Optional[torch.Tensor]:
        """fp32 [2N]: every rank scores pairs rank, rank + world, ... into a zero vector; one all-reduce completes it."""
        if ds is None:
            return None
        dev = self.dist.device
        out = torch.zeros(len(ds), dtype=torch.float32, device=dev)
        mine = torch.arange(self.dp_rank, len(ds) // 2, self.dp_size)
        coll = PreferenceCollator(self._pad_id, self.collator.pad_to_multiple_of)
        for chunk in mine.split(max(1, int(self.args.per_device_eval_batch_size))):
            b = coll(ds, chunk)
            b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
            logps, _ = model.sequence_logps(**self._seq_inputs(b))
            out[torch.stack([2 * chunk, 2 * chunk + 1], dim=1).reshape(-1).to(dev)] = logps.float()
        all_reduce_sum_(out)
        return out.cpu()

    def _ensure_ref_logps(self, resume: bool = False) -> None:
        if self._ref_ready:
            return
        path = self.ref_logps_path()
        if resume:
            if not os.path.exists(path):
                raise FileNotFoundError(f"resuming DPO needs the reference log-probabilities written at the start of "
                                        f"the run ({path}): the resumed weights are not the reference")
            d = torch.load(path, weights_only=True)
        else:
            self.optimizer.synchronize()
            ref = self._ref_model if self._ref_model is not None else self.model
            if isinstance(ref, str):
                dev = self.dist.device
                if os.path.isdir(ref) and any(f.endswith(".safetensors") for f in os.listdir(ref)):
                    ref = ckpt.from_pretrained(ref, device=dev, dtype=torch.bfloat16)
                else:
                    ref = build_model(get_config(ref), device=dev, dtype=torch.bfloat16)
            elif next(ref.parameters()).device != self.dist.device:
                ref.to(self.dist.device)
                ref.inv_freq = ref.inv_freq.to(self.dist.device)
            was_training = ref.training
            ref.eval()
            d = {"train": self._compute_ref(ref, self.train_dataset), "eval": self._compute_ref(ref, self.eval_dataset)}
            ref.train(was_training)
            self._ref_model = ref = None  # evaluated once, then released
            if self.dist.is_main:
                os.makedirs(self.args.output_dir, exist_ok=True)
                tmp = f"{path}.tmp{os.getpid()}"
                torch.save(d, tmp)
                os.replace(tmp, path)
            barrier()
        if self.train_dataset is not None and (d.get("train") is None or d["train"].numel() != len(self.train_dataset)):
            raise ValueError(f"{path} does not match the training set")
        self.collator.ref_logps = d.get("train")
        self.eval_collator.ref_logps = d.get("eval")
        self._ref_ready = True

    def precompute_ref_logps(self) -> None:
        """The reference pass on its own (``train()`` runs it when it has not happened yet)."""
        self._ensure_ref_logps()

    # ------------------------------------------------------------------ objective
    def _dpo(self, b: Dict, inv_pairs):
        logps, _ = self.model.sequence_logps(**self._seq_inputs(b))
        if hasattr(inv_pairs, "resolve"):  # the in-flight global pair count: awaited after the trunk
            inv_pairs = inv_pairs.resolve()
        if not torch.is_tensor(inv_pairs):
            inv_pairs = torch.tensor(float(inv_pairs))
        inv = (1.0 / inv_pairs.to(device=logps.device, dtype=torch.float32)).reshape(1)
        loss, st = ops.dpo_loss(logps, b["ref_logps"], inv, float(self.args.beta))
        lp = logps.detach().view(-1, 2).sum(0)
        metrics = torch.stack([st[2].sum(), st[3].sum(), (st[2] > st[3]).float().sum(), (st[2] - st[3]).sum(),
                               lp[0], lp[1], st.new_full((), float(st.shape[1]))])
        return loss, metrics

    def _micro_loss(self, b: Dict, n_items):
        return self._dpo(b, n_items)

    def _eval_loss(self, b: Dict):
        return self._dpo(b, 1.0)

    @staticmethod
    def _reward_entries(v: List[float], prefix: str = "") -> Dict[str, float]:
        p = max(v[7], 1.0)
        return {f"{prefix}rewards/chosen": v[1] / p, f"{prefix}rewards/rejected": v[2] / p,
                f"{prefix}rewards/accuracies": v[3] / p, f"{prefix}rewards/margins": v[4] / p,
                f"{prefix}logps/chosen": v[5] / p, f"{prefix}logps/rejected": v[6] / p}

    def _train_logs(self, v: List[float], steps: int, common: Dict[str, Any]) -> Dict[str, Any]:
        return {"loss": v[0] / steps, **self._reward_entries(v), **common}

    def _eval_logs(self, v: List[float], prefix: str, common: Dict[str, Any]) -> Dict[str, Any]:
        return {f"{prefix}_loss": v[0] / max(v[7], 1.0), **common, **self._reward_entries(v, f"{prefix}_")}

    def evaluate(self, eval_dataset=None, metric_key_prefix: str = "eval") -> Dict[str, float]:
        if eval_dataset is not None:
            self.eval_dataset = self._prepare(eval_dataset, self.args.max_eval_samples)
            self._ref_ready = False
        if self.eval_dataset is None:
            return {}
        self._ensure_ref_logps()
        return super().evaluate(None, metric_key_prefix)

    def train(self, resume_from_checkpoint: Optional[str] = None) -> TrainOutput:
        resume = resume_from_checkpoint or self.args.resume_from_checkpoint
        if resume is True or resume == "auto":
            resume = ckpt.latest_checkpoint(self.args.output_dir)
        self._ensure_ref_logps(resume=bool(resume))
        return super().train(resume_from_checkpoint)
