"""Inference CLI (reference ``ask_tuned_model.py`` / ``ask_original_model.py``).

    python -m llm_fine_tune_distributed_amd.cli.ask "How do I tie a bowline?" [--model outputs/best_model]

Loads an HF-layout directory (safetensors + config + tokenizer) in bf16 on the GPU (CPU fallback),
applies the chat template with the wilderness system prompt and ``add_generation_prompt=True``,
samples with the reference's settings (T=0.6, top_p=0.95, top_k=40, repetition_penalty=1.1) and
prints the assistant span.

    python -m llm_fine_tune_distributed_amd.cli.ask --questions-file questions.txt --batch-size 16 --output answers.jsonl

answers a whole list (one question per line, or a parquet / JSONL with a ``question`` column) with batched
generation: ``--batch-size`` prompts are decoded per step.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import List, Optional

import torch


def load_model(path: str, device=None):
    from ..data.tokenizer import load_tokenizer
    from ..models import build_model, get_config
    from ..train.checkpoint import from_pretrained
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    if os.path.isdir(path):
        model = from_pretrained(path, device=device, dtype=torch.bfloat16 if device != "cpu" else torch.float32)
        tok = load_tokenizer(path)
    else:  # preset (random init) — the base hub model is not downloadable offline
        tok = load_tokenizer(None)
        cfg = get_config(path)
        cfg.vocab_size = max(cfg.vocab_size, tok.vocab_size)  # every id the tokenizer can emit has an embedding row
        model = build_model(cfg, device=device, dtype=torch.bfloat16 if device != "cpu" else torch.float32)
    return model, tok


def _chat_prompt(tokenizer, question: str, enable_thinking: bool) -> str:
    from ..data.prompts import WILDERNESS_EXPERT_SYSTEM_PROMPT
    msgs = [{"role": "system", "content": WILDERNESS_EXPERT_SYSTEM_PROMPT}, {"role": "user", "content": question}]
    return tokenizer.apply_chat_template(msgs, tokenize=False, add_generation_prompt=True,
                                         enable_thinking=enable_thinking)


def _sampling(overrides) -> dict:
    kw = dict(temperature=0.6, top_p=0.95, top_k=40, repetition_penalty=1.1, do_sample=True)
    kw.update(overrides)
    return kw


def ask_question(model, tokenizer, question: str, max_new_tokens: int = 3768, enable_thinking: bool = False,
                 seed=None, **sampling) -> str:
    from ..data.chat_template import assistant_span
    from ..inference.generation import generate
    prompt = _chat_prompt(tokenizer, question, enable_thinking)
    ids = tokenizer.encode(prompt)
    out = generate(model, ids, max_new_tokens=max_new_tokens, eos_token_id=tokenizer.eos_token_id, seed=seed,
                   **_sampling(sampling))
    return assistant_span(prompt + tokenizer.decode(out))


def ask_questions(model, tokenizer, questions: List[str], batch_size: int = 16, max_new_tokens: int = 3768,
                  enable_thinking: bool = False, seed: Optional[int] = None, **sampling) -> List[str]:
    """``ask_question`` for a list: same template, system prompt and sampling defaults, ``batch_size`` questions
    decoded per step (inference.generation.generate_batch). Question i draws with ``seed + i``."""
    from ..data.chat_template import assistant_span
    from ..inference.generation import generate_batch
    answers: List[str] = []
    for i in range(0, len(questions), max(1, batch_size)):
        prompts = [_chat_prompt(tokenizer, q, enable_thinking) for q in questions[i:i + max(1, batch_size)]]
        outs = generate_batch(model, [tokenizer.encode(p) for p in prompts], max_new_tokens=max_new_tokens,
                              eos_token_id=tokenizer.eos_token_id, seed=None if seed is None else seed + i,
                              **_sampling(sampling))
        answers += [assistant_span(p + tokenizer.decode(o)) for p, o in zip(prompts, outs)]
    return answers


def load_questions(path: str) -> List[str]:
    """One question per line, or the ``question`` column of a parquet / JSONL file."""
    from ..data.dataset import load_jsonl, load_qa_parquet
    if path.endswith(".parquet"):
        return [str(r["question"]) for r in load_qa_parquet(path)]
    if path.endswith((".jsonl", ".json")):
        return [str(r["question"]) for r in load_jsonl(path)]
    with open(path) as f:
        return [l.strip() for l in f if l.strip()]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("question", nargs="*")
    ap.add_argument("--model", default="outputs/best_model")
    ap.add_argument("--max-new-tokens", type=int, default=3768)
    ap.add_argument("--enable-thinking", action="store_true")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--questions-file", default=None,
                    help="one question per line, or a parquet / JSONL with a 'question' column")
    ap.add_argument("--batch-size", type=int, default=16, help="questions decoded per step with --questions-file")
    ap.add_argument("--output", default=None, help='with --questions-file: write JSONL rows {"question", "answer"}')
    a = ap.parse_args(argv)
    if a.questions_file:
        questions = load_questions(a.questions_file)
        model, tok = load_model(a.model)
        answers = ask_questions(model, tok, questions, a.batch_size, a.max_new_tokens, a.enable_thinking, seed=a.seed)
        if a.output:
            with open(a.output, "w") as f:
                for q, ans in zip(questions, answers):
                    f.write(json.dumps({"question": q, "answer": ans}) + "\n")
        for q, ans in zip(questions, answers):
            print(f"Question: {q}\n\nAnswer:\n{ans}\n")
        return
    if not a.question:
        print('Usage: python -m llm_fine_tune_distributed_amd.cli.ask "Your question here"')
        sys.exit(1)
    q = " ".join(a.question)
    print(f"Question: {q}\n")
    model, tok = load_model(a.model)
    print("Answer:")
    print(ask_question(model, tok, q, a.max_new_tokens, a.enable_thinking, seed=a.seed))


if __name__ == "__main__":
    main()
