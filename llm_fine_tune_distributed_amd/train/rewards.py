"""Built-in reward functions for ``GRPOTrainer`` (``cli/train.py --trainer grpo --reward
llm_fine_tune_distributed_amd.train.rewards:answer_match``).

A reward function is called as ``f(prompts=, completions=, completion_ids=, **columns) -> list[float]``: one float per
completion; ``columns`` are the dataset's other columns, repeated per completion. ``completions`` are the decoded
texts (the token-id lists when the trainer has no tokenizer).
"""
from __future__ import annotations

import importlib
import re
from typing import Callable, List, Optional, Sequence


def length_band(prompts=None, completions=None, completion_ids=None, min_tokens: int = 16, max_tokens: int = 192,
                **_) -> List[float]:
    """1 inside ``[min_tokens, max_tokens]`` completion tokens, falling linearly to 0 at 0 tokens and at twice
    ``max_tokens``: neither one-word answers nor run-on text."""
    out = []
    for ids in completion_ids:
        n = len(ids)
        if n < min_tokens:
            out.append(n / float(min_tokens))
        elif n <= max_tokens:
            out.append(1.0)
        else:
            out.append(max(0.0, 1.0 - (n - max_tokens) / float(max_tokens)))
    return out


def _norm(text) -> str:
    return re.sub(r"\s+", " ", str(text).strip().lower())


def answer_match(prompts=None, completions=None, completion_ids=None, answer: Optional[Sequence] = None,
                 **_) -> List[float]:
    """Against the dataset's ``answer`` column, case- and whitespace-insensitive: 1 for an exact match, 0.5 when the
    answer appears inside the completion, 0 otherwise (and 0 for a row without an answer)."""
    if answer is None:
        raise ValueError("answer_match needs an 'answer' column in the dataset")
    out = []
    for c, a in zip(completions, answer):
        if a is None or not isinstance(c, str):
            out.append(0.0)
            continue
        c, a = _norm(c), _norm(a)
        out.append(1.0 if c == a else (0.5 if a and a in c else 0.0))
    return out


def resolve(spec: str) -> Callable:
    """``pkg.module:function`` -> the callable (the CLI's ``--reward``)."""
    if ":" not in spec:
        raise ValueError(f"--reward expects pkg.module:function, got {spec!r}")
    mod, name = spec.split(":", 1)
    fn = getattr(importlib.import_module(mod), name, None)
    if not callable(fn):
        raise ValueError(f"{spec!r} does not name a callable")
    return fn
