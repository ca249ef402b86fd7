"""``GKDTrainer``: knowledge distillation from a frozen teacher (TRL ``GKDTrainer``, off-policy) on the ``SFTTrainer``
engine.

The step is ``SFTTrainer``'s — DDP engine, gradient accumulation and its merging, clipping, flat AdamW, ZeRO-1, LoRA and
partial-freeze students, gradient checkpointing, packing, ``assistant_only_loss`` — with the teacher's
``CausalLM.logits_rows`` (no grad) -> the student's ``CausalLM.distill_loss`` -> ``backward`` in place of
``model(...).loss``. The objective is TRL's ``generalized_jsd_loss`` over the rows whose shifted label is not -100,
normalised by the GLOBAL number of such rows of the optimizer step, exactly as the SFT cross-entropy is.

The teacher is a bf16 ``CausalLM`` in ``eval()`` with every parameter frozen. It belongs to this object only: the DDP
engine, the optimizer, checkpoints and ``save_model`` never see it, so a resumed run is given the same teacher again
(``args.teacher_model_name_or_path`` records where it came from). Its vocabulary must be the student's.
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional

import torch

from ..models import CausalLM, build_model, get_config
from . import checkpoint as ckpt
from .config import GKDConfig
from .trainer import SFTTrainer


class GKDTrainer(SFTTrainer):
    # loss, correct, rows where the student's argmax is the teacher's, valid
    _acc_size = 4

    def __init__(self, model=None, args: Optional[GKDConfig] = None, train_dataset=None, eval_dataset=None,
                 teacher_model=None, **kw):
        args = args or GKDConfig()
        if not isinstance(args, GKDConfig):
            raise TypeError("GKDTrainer expects a GKDConfig")
        if teacher_model is None:
            teacher_model = args.teacher_model_name_or_path
        if teacher_model is None:
            raise ValueError("GKDTrainer needs a teacher: teacher_model= (a preset name, a local HF directory or a "
                             "CausalLM) or args.teacher_model_name_or_path")
        if isinstance(teacher_model, str):
            args.teacher_model_name_or_path = teacher_model  # the resolved config records the teacher
        super().__init__(model, args, train_dataset, eval_dataset, **kw)
        self.teacher = self._load_teacher(teacher_model)
        vs, vt = self.model.config.vocab_size, self.teacher.config.vocab_size
        if vs != vt:
            raise ValueError(f"the teacher's vocab_size ({vt}) differs from the student's ({vs}): distillation compares "
                             "the two token distributions column by column, so both models need one tokenizer")

    def _load_teacher(self, teacher) -> CausalLM:
        dev = self.dist.device
        if isinstance(teacher, str):
            if os.path.isdir(teacher) and any(f.endswith(".safetensors") for f in os.listdir(teacher)):
                teacher = ckpt.from_pretrained(teacher, device=dev, dtype=torch.bfloat16)
            else:
                teacher = build_model(get_config(teacher), device=dev, dtype=torch.bfloat16)
        if not isinstance(teacher, CausalLM):
            raise TypeError("teacher_model must be a preset name, a local HF directory or a CausalLM")
        if teacher is self.model:
            raise ValueError("the teacher must not be the student object: it is frozen and never updated")
        if next(teacher.parameters()).device != dev:
            teacher.to(dev)
            teacher.inv_freq = teacher.inv_freq.to(dev)
        for p in teacher.parameters():  # (the parameters only: inv_freq stays fp32)
            if p.dtype != torch.bfloat16:
                p.data = p.data.to(torch.bfloat16)
        teacher.eval()
        teacher.requires_grad_(False)
        return teacher

    # ------------------------------------------------------------------ objective
    def _distill(self, b: Dict, n_items):
        kw = self._model_inputs(b)
        labels = kw.pop("labels")
        shift = kw.pop("shift_labels", True)
        with torch.no_grad():
            self.teacher.eval()
            t_logits = self.teacher.logits_rows(**kw)
        out = self.model.distill_loss(labels=labels, teacher_logits=t_logits, shift_labels=shift,
                                      num_items_in_batch=n_items, beta=float(self.args.beta),
                                      temperature=float(self.args.temperature), **kw)
        return out.loss, out.metrics

    def _micro_loss(self, b: Dict, n_items):
        return self._distill(b, n_items)

    def _eval_loss(self, b: Dict):
        return self._distill(b, 1.0)

    def _train_logs(self, v: List[float], steps: int, common: Dict[str, Any]) -> Dict[str, Any]:
        valid = max(v[3], 1.0)
        return {"loss": v[0] / steps, "grad_norm": common["grad_norm"], "learning_rate": common["learning_rate"],
                "epoch": common["epoch"], "mean_token_accuracy": v[1] / valid, "teacher_agreement": v[2] / valid,
                "num_tokens": common["num_tokens"]}

    def _eval_logs(self, v: List[float], prefix: str, common: Dict[str, Any]) -> Dict[str, Any]:
        valid = max(v[3], 1.0)
        return {f"{prefix}_loss": v[0] / valid, **common, f"{prefix}_mean_token_accuracy": v[1] / valid,
                f"{prefix}_teacher_agreement": v[2] / valid, f"{prefix}_num_tokens": v[3]}
