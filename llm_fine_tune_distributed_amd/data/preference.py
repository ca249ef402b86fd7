"""Preference data for DPO: rows ``{"prompt", "chosen", "rejected"}`` -> a ``TokenizedDataset`` of 2N sequences
(chosen at 2i, rejected at 2i + 1) and the collator that turns B pairs into one varlen batch of 2B sequences.

Two row formats, as in TRL: plain strings (the prompt is a user turn) and message lists (the conversational
preference format: ``prompt`` a list of messages, ``chosen`` / ``rejected`` the assistant's messages). The prompt is
rendered through the chat template with the generation prompt; prompt and completion are tokenised SEPARATELY and the
ids concatenated (TRL ``tokenize_row``), EOS appended when the completion does not end with it — so both sequences
of a pair start with the same prompt ids and ``loss_start = len(prompt_ids)``.

Reward modelling (train/reward.py) reads the same rows, and also rows without ``"prompt"`` (TRL's implicit-prompt
format: ``chosen`` / ``rejected`` are whole texts or whole conversations) and a numeric ``"margin"`` column, which the
collator carries per pair (``preference_margins``).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import torch

from .collator import SFTCollator
from .dataset import TokenizedDataset, cached_tokenize


def _prompt_messages(prompt) -> List[Dict[str, str]]:
    return [{"role": "user", "content": prompt}] if isinstance(prompt, str) else list(prompt)


def _completion_text(tokenizer, prompt_msgs, prompt_text: str, completion) -> str:
    if isinstance(completion, str):
        return completion
    msgs = list(completion)
    full = tokenizer.apply_chat_template(prompt_msgs + msgs, tokenize=False)
    if full.startswith(prompt_text):  # the template's own rendering of the assistant turn(s)
        return full[len(prompt_text):]
    return "".join(m["content"] for m in msgs)


def tokenize_preference_rows(rows: Sequence[Dict], tokenizer, max_length: Optional[int] = None,
                             max_prompt_length: Optional[int] = None) -> TokenizedDataset:
    """2N sequences prompt + chosen, prompt + rejected. ``max_prompt_length`` keeps the prompt's last tokens,
    ``max_length`` cuts the completion's tail."""
    eos = tokenizer.eos_token_id
    seqs, starts = [], []
    for r in rows:
        if "prompt" not in r:
            # TRL's implicit-prompt format (reward modelling): each side is a whole conversation. A string is tokenised
            # as it stands plus EOS, a message list through the chat template without the generation prompt; there
            # is no prompt to mask (loss_start 0)
            for key in ("chosen", "rejected"):
                v = r[key]
                ids = tokenizer.encode(v if isinstance(v, str) else tokenizer.apply_chat_template(list(v), tokenize=False))
                if isinstance(v, str) and eos is not None and (not ids or ids[-1] != eos):
                    ids = ids + [eos]
                if max_length:
                    ids = ids[:int(max_length)]
                seqs.append(ids)
                starts.append(0)
            continue
        pm = _prompt_messages(r["prompt"])
        ptext = tokenizer.apply_chat_template(pm, tokenize=False, add_generation_prompt=True)
        pids = tokenizer.encode(ptext)
        if max_prompt_length:
            pids = pids[-int(max_prompt_length):]
        for key in ("chosen", "rejected"):
            cids = tokenizer.encode(_completion_text(tokenizer, pm, ptext, r[key]))
            if eos is not None and (not cids or cids[-1] != eos):
                cids = cids + [eos]
            ids = pids + cids
            if max_length:
                ids = ids[:int(max_length)]
            seqs.append(ids)
            starts.append(min(len(pids), len(ids)))
    return TokenizedDataset.from_token_lists(seqs, starts)


def cached_tokenize_preferences(rows: Sequence[Dict], tokenizer, cache_dir: Optional[str], is_main: bool = True,
                                barrier: Optional[Callable[[], None]] = None, max_length: Optional[int] = None,
                                max_prompt_length: Optional[int] = None) -> TokenizedDataset:
    """``tokenize_preference_rows`` through ``cached_tokenize``'s main-process-first cache, under its own fingerprint."""
    kw = dict(max_length=max_length, max_prompt_length=max_prompt_length)
    return cached_tokenize(rows, tokenizer, cache_dir, is_main=is_main, barrier=barrier,
                           tokenize=lambda r, t: tokenize_preference_rows(r, t, **kw),
                           fingerprint=dict(kind="preference", **kw))


class PreferenceCollator(SFTCollator):
    """B pair indices -> one padding-free batch of the 2B sequences (chosen, rejected, chosen, ...): ``cu_seqlens``,
    ``position_ids``, shifted labels with the prompt masked (``SFTCollator._pack`` on the expanded indices), plus
    ``n_seqs`` = 2B, ``num_items`` = ``num_samples`` = B (the pairs) and, when ``ref_logps`` [2N] is set, the batch's
    reference log-probabilities. ``num_tokens`` counts both sequences. Always padding-free, on CPU too."""

    def __init__(self, pad_token_id: int, pad_to_multiple_of: Optional[int] = None,
                 ref_logps: Optional[torch.Tensor] = None, margins: Optional[torch.Tensor] = None):
        super().__init__(pad_token_id, pad_to_multiple_of, None, packing=True, max_tokens=None)
        self.ref_logps = ref_logps
        self.margins = margins  # [N], one per pair (reward modelling): the batch's are b["margins"]

    def __call__(self, ds: TokenizedDataset, indices: torch.Tensor) -> Dict:
        pairs = indices.to(torch.int64).reshape(-1)
        idx = torch.stack([2 * pairs, 2 * pairs + 1], dim=1).reshape(-1)
        b = self._pack(ds, idx)
        B = int(pairs.numel())
        assert b["num_samples"] == 2 * B, "a pair's sequence was left out of the batch"
        b.update(n_seqs=2 * B, num_items=B, num_samples=B)
        if self.ref_logps is not None:
            b["ref_logps"] = self.ref_logps[idx].to(torch.float32)
        if self.margins is not None:
            b["margins"] = self.margins[pairs].to(torch.float32)
        return b


def preference_margins(rows: Sequence[Dict]) -> Optional[torch.Tensor]:
    """fp32 [N]: the rows' numeric ``"margin"`` column (TRL ``RewardTrainer``; a row without one counts 0), or None
    when no row has it."""
    if not any("margin" in r and r["margin"] is not None for r in rows):
        return None
    return torch.tensor([float(r.get("margin") or 0.0) for r in rows], dtype=torch.float32)
