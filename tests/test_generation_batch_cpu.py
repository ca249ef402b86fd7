"""Batched generation on CPU: element b of ``generate_batch`` is ``generate`` on prompt b, per-sequence EOS, and
the batched ask CLI (questions file in, JSONL out)."""
import json

import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import generate, generate_batch
from llm_fine_tune_distributed_amd.models import build_model, tiny

NEW = 10


@pytest.fixture(scope="module")
def model():
    return build_model(tiny(), dtype=torch.float32, seed=2)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(0, 512, (n,), generator=g).tolist() for n in (9, 3, 14)]


@pytest.mark.parametrize("rp", [1.0, 1.3, 2.0])  # 2.0: the random model stops repeating one token
def test_greedy_batch_equals_per_prompt(model, prompts, rp):
    ref = [generate(model, p, max_new_tokens=NEW, do_sample=False, repetition_penalty=rp) for p in prompts]
    out = generate_batch(model, prompts, max_new_tokens=NEW, do_sample=False, repetition_penalty=rp)
    assert out == ref
    assert all(len(o) == NEW for o in out)


def test_eos_stops_each_sequence_on_its_own(model, prompts):
    # penalty 2.0: the random model emits distinct tokens, so a token first seen at step 3 exists
    free = generate_batch(model, prompts, max_new_tokens=NEW, do_sample=False, repetition_penalty=2.0)
    eos = free[0][3]
    assert eos not in free[0][:3], "sequence 0 must emit the EOS at step 3 for the first time"
    out = generate_batch(model, prompts, max_new_tokens=NEW, do_sample=False, repetition_penalty=2.0,
                         eos_token_id=eos)
    assert out[0] == free[0][:4] and out[0][-1] == eos
    for o, f in zip(out, free):
        want = f[:f.index(eos) + 1] if eos in f else f
        assert o == want
    assert any(len(o) == NEW for o in out[1:]), "no sequence ran to its cap: the case checks nothing"
    single = [generate(model, p, max_new_tokens=NEW, do_sample=False, repetition_penalty=2.0, eos_token_id=eos)
              for p in prompts]
    assert out == single


def test_sampled_batch_uses_seed_plus_row(model, prompts):
    ref = [generate(model, p, max_new_tokens=NEW, seed=11 + b) for b, p in enumerate(prompts)]
    assert generate_batch(model, prompts, max_new_tokens=NEW, seed=11) == ref


class _Tok:
    """Word-level stand-in for the SFT tokenizer: enough for the chat template / decode round trip."""
    eos_token_id = 2

    def apply_chat_template(self, msgs, tokenize=False, add_generation_prompt=True, enable_thinking=False):
        return "".join(f"<|im_start|>{m['role']}\n{m['content']}<|im_end|>\n" for m in msgs) + "<|im_start|>assistant\n"

    def encode(self, text):
        return [3 + sum(map(ord, w)) % 500 for w in text.split()][-24:]

    def decode(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_ask_questions_returns_one_answer_per_question(model):
    from llm_fine_tune_distributed_amd.cli.ask import ask_questions
    ans = ask_questions(model, _Tok(), ["How do I tie a bowline?", "What is a bivouac?"], batch_size=2,
                        max_new_tokens=5, seed=0)
    assert len(ans) == 2 and all(isinstance(a, str) for a in ans)
    # a batch size that does not divide the list answers every question too
    assert len(ask_questions(model, _Tok(), ["a b", "c d e", "f"], batch_size=2, max_new_tokens=3, seed=0)) == 3


def test_main_questions_file_writes_jsonl(tmp_path, capsys):
    from llm_fine_tune_distributed_amd.cli.ask import main
    f, o = tmp_path / "q.txt", tmp_path / "answers.jsonl"
    f.write_text("How do I purify water?\n\nHow do I build a debris hut?\n")
    main(["--questions-file", str(f), "--output", str(o), "--model", "tiny", "--max-new-tokens", "4",
          "--batch-size", "2", "--seed", "0"])
    rows = [json.loads(l) for l in open(o)]
    assert [r["question"] for r in rows] == ["How do I purify water?", "How do I build a debris hut?"]
    assert all(set(r) == {"question", "answer"} and isinstance(r["answer"], str) for r in rows)
    assert "How do I purify water?" in capsys.readouterr().out
