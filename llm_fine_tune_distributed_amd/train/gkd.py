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

Offline distillation (``args.teacher_topk = K``, forward KL only). The teacher is frozen and the data fixed, so its
forward is taken out of the step as ``DPOTrainer`` takes the reference model's out: one no-grad pass over the train and
eval sets stores the teacher's K largest token log-probabilities of every token row in
``output_dir/teacher_topk-<fingerprint>.pt`` (``precompute_teacher_topk()``; ``train()`` runs it when needed), the
teacher is released, and the step becomes ``CausalLM.distill_topk_loss`` on rows the collator attaches to each batch.
With a matching file present no teacher is needed at all; a resume needs the file.
"""
from __future__ import annotations

import hashlib
import os
from typing import Any, Dict, List, Optional

import torch

from ..data.collator import DataLoader, DistillTopKCollator, SFTCollator
from ..data.dataset import TokenizedDataset
from ..models import CausalLM, build_model, get_config
from ..parallel.process_group import all_reduce_sum_, barrier
from . import checkpoint as ckpt
from .config import GKDConfig
from .trainer import SFTTrainer, TrainOutput


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
        self.topk = int(args.teacher_topk) if args.teacher_topk is not None else None
        no_teacher = ValueError("GKDTrainer needs a teacher: teacher_model= (a preset name, a local HF directory or a "
                                "CausalLM) or args.teacher_model_name_or_path")
        if teacher_model is None and self.topk is None:
            raise no_teacher
        if isinstance(teacher_model, str):
            args.teacher_model_name_or_path = teacher_model  # the resolved config records the teacher
        if self.topk is not None and kw.get("data_collator") is not None:
            raise ValueError("GKDTrainer with teacher_topk builds its own DistillTopKCollator")
        super().__init__(model, args, train_dataset, eval_dataset, **kw)
        self._topk_ready = False
        if self.topk is not None:
            self._acc_size = 5  # ... and the teacher mass kept, summed over the valid rows
            c = self.collator
            mk = lambda: DistillTopKCollator(c.pad_token_id, c.pad_to_multiple_of, c.max_length, c.packing,  # noqa: E731
                                             c.max_tokens)
            self.collator, self.eval_collator = mk(), mk()  # carry the train set's / the eval set's cached rows
            if os.path.exists(self.teacher_topk_path()):
                teacher_model = None  # the cache stands in for the teacher
            elif teacher_model is None:
                raise no_teacher
        self.teacher = self._load_teacher(teacher_model) if teacher_model is not None else None
        if self.teacher is not None:
            vs, vt = self.model.config.vocab_size, self.teacher.config.vocab_size
            if vs != vt:
                raise ValueError(f"the teacher's vocab_size ({vt}) differs from the student's ({vs}): distillation "
                                 "compares the two token distributions column by column, so both models need one "
                                 "tokenizer")

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

    # ------------------------------------------------------------------ the teacher's cached top-k log-probabilities
    def _topk_fingerprint(self) -> str:
        """DPOTrainer._ref_fingerprint's data hash, plus what the cached values depend on besides the teacher. Hashed
        once: the datasets, k and the temperature are fixed when the trainer is built (evaluate() takes no other set)."""
        if getattr(self, "_topk_fp", None) is not None:
            return self._topk_fp
        h = hashlib.sha256()
        for ds in (self.train_dataset, self.eval_dataset):
            if ds is None:
                h.update(b"none")
                continue
            for t in (ds.tokens, ds.offsets, ds.loss_start):
                h.update(b"none" if t is None else t.contiguous().cpu().numpy().tobytes())
        h.update(repr((self.topk, float(self.args.temperature), int(self.model.config.vocab_size))).encode())
        self._topk_fp = h.hexdigest()[:16]
        return self._topk_fp

    def teacher_topk_path(self) -> str:
        return os.path.join(self.args.output_dir, f"teacher_topk-{self._topk_fingerprint()}.pt")

    def _topk_meta(self) -> Dict[str, Any]:
        return {"k": self.topk, "temperature": float(self.args.temperature),
                "vocab_size": int(self.model.config.vocab_size)}

    @torch.no_grad()
    def _compute_topk(self, ds: Optional[TokenizedDataset]):
        """(int32 ids, fp32 logps), each [N_tokens, k] with the row of sample i at position j at offsets[i] + j: every
        rank runs the teacher on samples rank, rank + world, ... in padding-free batches and fills their rows of two
        zero tensors; one all-reduce each completes them (as DPOTrainer._compute_ref)."""
        if ds is None:
            return None
        dev = self.dist.device
        n_tok = int(ds.offsets[-1])
        ids = torch.zeros(n_tok, self.topk, dtype=torch.int32)
        lps = torch.zeros(n_tok, self.topk, dtype=torch.float32)
        coll = SFTCollator(self._pad_id, self.collator.pad_to_multiple_of, None, True, None)
        mine = torch.arange(self.dp_rank, len(ds), self.dp_size)
        for chunk in mine.split(max(1, int(self.args.per_device_eval_batch_size))):
            b = coll(ds, chunk)
            cu = b["cu_seqlens"].to(torch.int64)
            tid, tlp = self.teacher.topk_logps_rows(
                b["input_ids"].to(dev), cu_seqlens=b["cu_seqlens"].to(dev), position_ids=b["position_ids"].to(dev),
                max_seqlen=b["max_seqlen"], k=self.topk, temperature=float(self.args.temperature))
            tid, tlp = tid.cpu(), tlp.float().cpu()
            for s, i in enumerate(chunk.tolist()):
                a, e, o = int(cu[s]), int(cu[s + 1]), int(ds.offsets[i])
                ids[o:o + e - a] = tid[a:e]
                lps[o:o + e - a] = tlp[a:e]
        if self.dist.world_size > 1:
            ids, lps = ids.to(dev), lps.to(dev)
            all_reduce_sum_(ids)
            all_reduce_sum_(lps)
            ids, lps = ids.cpu(), lps.cpu()
        return ids, lps

    def _ensure_teacher_topk(self, resume: bool = False) -> None:
        if self.topk is None or self._topk_ready:
            return
        path = self.teacher_topk_path()
        if os.path.exists(path):
            d = torch.load(path, weights_only=True)
        elif resume:
            raise FileNotFoundError(f"resuming offline distillation needs the teacher's top-k cache written at the "
                                    f"start of the run ({path})")
        elif self.teacher is None:
            raise FileNotFoundError(f"no teacher and no teacher top-k cache at {path}")
        else:
            self.teacher.eval()
            d = {"meta": self._topk_meta()}
            for name, ds in (("train", self.train_dataset), ("eval", self.eval_dataset)):
                r = self._compute_topk(ds)
                if r is not None:
                    d[f"{name}_ids"], d[f"{name}_logps"] = r
            if self.dist.is_main:
                os.makedirs(self.args.output_dir, exist_ok=True)
                tmp = f"{path}.tmp{os.getpid()}"
                torch.save(d, tmp)
                os.replace(tmp, path)
            barrier()
        if d.get("meta") != self._topk_meta():
            raise ValueError(f"{path} was written for {d.get('meta')}, this run asks for {self._topk_meta()}")
        for name, ds, coll in (("train", self.train_dataset, self.collator), ("eval", self.eval_dataset,
                                                                              self.eval_collator)):
            if ds is None:
                continue
            ti, tl = d.get(f"{name}_ids"), d.get(f"{name}_logps")
            want = (int(ds.offsets[-1]), self.topk)
            if ti is None or tl is None or tuple(ti.shape) != want or tuple(tl.shape) != want:
                raise ValueError(f"{path} does not match the {name} set")
            coll.teacher_ids, coll.teacher_logps = ti, tl
        # the teacher has done its work: released, and its memory returned before the first step
        self.teacher = None
        if self.dist.device.type == "cuda":
            torch.cuda.empty_cache()
        self._topk_ready = True

    def precompute_teacher_topk(self) -> None:
        """The teacher's caching pass on its own (``train()`` and ``evaluate()`` run it when it has not happened)."""
        if self.topk is None:
            raise ValueError("precompute_teacher_topk needs args.teacher_topk")
        self._ensure_teacher_topk()

    def get_eval_dataloader(self) -> DataLoader:
        if self.topk is None:
            return super().get_eval_dataloader()
        train_collator, self.collator = self.collator, self.eval_collator  # the inherited loader, the eval set's rows
        try:
            return super().get_eval_dataloader()
        finally:
            self.collator = train_collator

    def _merge_micro(self, micro: List[Dict]) -> List[Dict]:
        out = super()._merge_micro(micro)
        if out is micro or "teacher_ids" not in micro[0]:
            return out
        # the inherited merge knows nothing of the cached rows: concatenated like the tokens they belong to
        if "cu_seqlens" in micro[0]:
            rows = lambda key: torch.cat([b[key] for b in micro])  # noqa: E731
        else:
            T = out[0]["input_ids"].shape[1]
            F = torch.nn.functional
            rows = lambda key: torch.cat([F.pad(b[key], (0, 0, 0, T - b[key].shape[1])) for b in micro])  # noqa: E731
        out[0]["teacher_ids"], out[0]["teacher_logps"] = rows("teacher_ids"), rows("teacher_logps")
        return out

    def evaluate(self, eval_dataset=None, metric_key_prefix: str = "eval") -> Dict[str, float]:
        if self.topk is not None:
            if eval_dataset is not None:
                raise ValueError("GKDTrainer with teacher_topk evaluates the eval_dataset it cached the teacher for")
            if self.eval_dataset is not None:
                self._ensure_teacher_topk()
        return super().evaluate(eval_dataset, metric_key_prefix)

    def train(self, resume_from_checkpoint: Optional[str] = None) -> TrainOutput:
        if self.topk is not None:
            resume = resume_from_checkpoint or self.args.resume_from_checkpoint
            if resume is True or resume == "auto":
                resume = ckpt.latest_checkpoint(self.args.output_dir)
            self._ensure_teacher_topk(resume=bool(resume))
        return super().train(resume_from_checkpoint)

    # ------------------------------------------------------------------ objective
    def _distill(self, b: Dict, n_items):
        kw = self._model_inputs(b)
        labels = kw.pop("labels")
        shift = kw.pop("shift_labels", True)
        if self.topk is not None:
            out = self.model.distill_topk_loss(labels=labels, teacher_ids=b["teacher_ids"],
                                               teacher_logps=b["teacher_logps"], shift_labels=shift,
                                               num_items_in_batch=n_items, temperature=float(self.args.temperature),
                                               **kw)
            return out.loss, torch.cat([out.metrics, out.teacher_mass.reshape(1)])
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
                "num_tokens": common["num_tokens"], **({"teacher_mass": v[4] / valid} if len(v) > 4 else {})}

    def _eval_logs(self, v: List[float], prefix: str, common: Dict[str, Any]) -> Dict[str, Any]:
        valid = max(v[3], 1.0)
        return {f"{prefix}_loss": v[0] / valid, **common, f"{prefix}_mean_token_accuracy": v[1] / valid,
                f"{prefix}_teacher_agreement": v[2] / valid, f"{prefix}_num_tokens": v[3],
                **({f"{prefix}_teacher_mass": v[4] / valid} if self.topk is not None else {})}
