"""What the trainers on ``SFTTrainer`` share off the step: a model argument resolved to a model, an auxiliary model
held frozen next to the trained one, and the pieces of caching a frozen model's pass over the data under
``output_dir`` (``DPOTrainer``'s reference log-probabilities, ``GKDTrainer``'s top-k teacher rows). When a cache is
computed, loaded or refused is each trainer's own policy."""
from __future__ import annotations

import dataclasses
import hashlib
import os
from typing import Optional

import torch

from ..models import CausalLM, build_model, get_config
from ..parallel.process_group import barrier
from . import checkpoint as ckpt

# hold_frozen's refusals by ``what``: (not a model, the trained object itself)
_REFUSALS = {
    "teacher": ("teacher_model must be a preset name, a local HF directory or a CausalLM",
                "the teacher must not be the student object: it is frozen and never updated"),
    "reference": ("ref_model must be a preset name, a local HF directory or a CausalLM",
                  "the reference must not be the policy object: it is frozen and never updated"),
    "reward model": ("a reward model must be a CausalLM with a score head",
                     "a reward model must not be the policy object: it is frozen and never updated"),
}


def resolve_model(spec, device, *, seed: int = 0, **from_pretrained_kw):
    """``spec`` as a bf16 model on ``device``: a local HF directory holding ``.safetensors`` is loaded, any other
    string is a preset built from ``seed``, anything else (a model object) is returned as it is. The keywords
    (``num_labels=1``) override the preset's config, or go to ``checkpoint.from_pretrained`` together with the seed,
    from which it draws what they add to the directory's weights; without them a directory is loaded without the seed."""
    if not isinstance(spec, str):
        return spec
    if os.path.isdir(spec) and any(f.endswith(".safetensors") for f in os.listdir(spec)):
        if from_pretrained_kw:
            from_pretrained_kw["seed"] = seed
        return ckpt.from_pretrained(spec, device=device, dtype=torch.bfloat16, **from_pretrained_kw)
    cfg = get_config(spec)
    if from_pretrained_kw:
        cfg = dataclasses.replace(cfg, **from_pretrained_kw)
    return build_model(cfg, device=device, dtype=torch.bfloat16, seed=seed)


def to_device(model: CausalLM, device) -> CausalLM:
    if next(model.parameters()).device != device:
        model.to(device)
        model.inv_freq = model.inv_freq.to(device)  # (a plain attribute: Module.to leaves it behind)
    return model


def hold_frozen(model, device, *, trained, what: str, cast_bf16: bool = False) -> CausalLM:
    """``model`` as the frozen ``what`` ("teacher", "reference", "reward model") of a run that trains ``trained``: on
    the device, in eval mode, no parameter requiring a gradient; ``cast_bf16`` also makes every parameter bf16."""
    not_a_model, is_trained = _REFUSALS[what]
    if not isinstance(model, CausalLM):
        raise TypeError(not_a_model)
    if model is trained:
        raise ValueError(is_trained)
    to_device(model, device)
    if cast_bf16:
        for p in model.parameters():  # (the parameters only: inv_freq stays fp32)
            if p.dtype != torch.bfloat16:
                p.data = p.data.to(torch.bfloat16)
    model.eval()
    return model.requires_grad_(False)


def dataset_fingerprint(datasets, extra=None) -> str:
    """16 hex digits over the stored tensors of the given sets (None: a set that is not there) and ``repr(extra)``,
    what the cached values depend on besides the frozen model and the data."""
    h = hashlib.sha256()
    for ds in datasets:
        if ds is None:
            h.update(b"none")
            continue
        for t in (ds.tokens, ds.offsets, ds.loss_start):
            h.update(b"none" if t is None else t.contiguous().cpu().numpy().tobytes())
    if extra is not None:
        h.update(repr(extra).encode())
    return h.hexdigest()[:16]


def tmp_sibling(path: str) -> str:
    """Where this process writes what ``os.replace`` then puts at ``path``."""
    return f"{path}.tmp{os.getpid()}"


def save_on_main(obj, path: str, is_main: bool) -> None:
    """Rank 0 writes ``obj`` to ``path`` (whole or not at all); every rank returns once the file is there."""
    if is_main:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(obj, tmp_sibling(path))
        os.replace(tmp_sibling(path), path)
    barrier()


def resolve_resume(args, resume_from_checkpoint=None) -> Optional[str]:
    """The checkpoint ``train(resume_from_checkpoint)`` resumes from (True / "auto": the latest under ``output_dir``),
    or a false value for a fresh run."""
    resume = resume_from_checkpoint or args.resume_from_checkpoint
    if resume is True or resume == "auto":
        resume = ckpt.latest_checkpoint(args.output_dir)
    return resume
