"""Every generation path against the full forward, on the CPU: after the prefill and after each of four forced
tokens, the last-token logits of ``forward_cached`` (prefill, then decode), ``GraphDecoder.step`` and
``prefill_batch`` + ``BatchGraphDecoder.step`` equal ``m(ids[None], return_logits=True)`` of the same sequence.
All four tiny families, plain and LoRA, with the qkv biases, the q / k norm weights and the adapters randomised so
that none of them is a no-op.

Bound: 1e-5 absolute on fp32 logits of magnitude about 1. The paths differ from the full forward only in the order
of fp32 sums (attention over a cache, one row at a time); measured at most 6.6e-7 over the eight cases, the bound
leaves about 15x over that for other BLAS builds."""
import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import (BatchGraphDecoder, BatchKVCache, GraphDecoder,
                                                                KVCache, forward_cached, prefill_batch)
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.models.lora import LoRAConfig, apply_lora

PRESETS = ["tiny", "tiny-llama", "tiny-qwen3", "tiny-qwen2"]
LENS = (9, 3, 14)
FORCED = 4
TOL = 1e-5


class _Case:
    def __init__(self, preset: str, lora: bool):
        g = torch.Generator().manual_seed(7)
        m = build_model(get_config(preset), dtype=torch.float32, seed=3)
        if lora:
            apply_lora(m, LoRAConfig())
        with torch.no_grad():
            for n, p in m.named_parameters():
                if p.numel() == 0:
                    continue
                if n.endswith("qkv_bias"):
                    p.copy_(0.5 * torch.randn(p.shape, generator=g))
                elif n.endswith("q_norm.weight") or n.endswith("k_norm.weight"):
                    p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
                elif ".lora." in n:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
        self.model = m.eval()
        V = m.config.vocab_size
        self.prompts = [torch.randint(0, V, (n,), generator=g).tolist() for n in LENS]
        self.forced = [torch.randint(0, V, (FORCED,), generator=g).tolist() for _ in LENS]
        # want[b][t]: the full forward's last-token logits of prompt b followed by its first t forced tokens
        self.want = []
        with torch.no_grad():
            for p, f in zip(self.prompts, self.forced):
                rows = []
                for t in range(FORCED + 1):
                    ids = torch.tensor(p + f[:t])
                    rows.append(m(ids[None], return_logits=True).logits.reshape(-1, V)[-1].float())
                self.want.append(rows)

    def check(self, got: torch.Tensor, b: int, t: int, path: str) -> None:
        err = (got.float() - self.want[b][t]).abs().max().item()
        assert err <= TOL, f"{path}: prompt {b}, {t} forced tokens: max |dlogit| = {err:.3g}"

    def prefilled(self, b: int):
        m = self.model
        cache = KVCache(m.config, LENS[b] + FORCED + 1, "cpu", torch.float32)
        logits = forward_cached(m, torch.tensor(self.prompts[b]), cache, prefill=True)
        return cache, logits


@pytest.fixture(scope="module", params=[(p, l) for p in PRESETS for l in (False, True)],
                ids=lambda pl: f"{pl[0]}-{'lora' if pl[1] else 'plain'}")
def case(request):
    return _Case(*request.param)


def test_tiny_has_both_kinds_of_layer():
    cfg = get_config("tiny")
    rope = [cfg.uses_rope(i) for i in range(cfg.num_hidden_layers)]
    assert any(rope) and not all(rope), "tiny must run both arms of Attention.rotate_qk_"


def test_reference_is_not_degenerate(case):
    w = torch.stack([r for rows in case.want for r in rows])
    assert torch.isfinite(w).all() and 0.1 < w.abs().max().item() < 100


def test_forward_cached_prefill_then_decode(case):
    for b in range(len(LENS)):
        cache, logits = case.prefilled(b)
        case.check(logits, b, 0, "forward_cached prefill")
        for t in range(FORCED):
            logits = forward_cached(case.model, torch.tensor(case.forced[b][t:t + 1]), cache, prefill=False)
            case.check(logits, b, t + 1, "forward_cached decode")
        assert cache.len == LENS[b] + FORCED


def test_graph_decoder_step(case):
    for b in range(len(LENS)):
        cache, _ = case.prefilled(b)
        dec = GraphDecoder(case.model, cache)
        for t in range(FORCED):
            logits = dec.step(case.forced[b][t], cache.len, use_graph=False)
            cache.len += 1
            case.check(logits, b, t + 1, "GraphDecoder.step")


def test_prefill_batch_then_batch_decoder_step(case):
    m = case.model
    cache = BatchKVCache(m.config, len(LENS), max(LENS) + FORCED + 1, "cpu", torch.float32)
    logits = prefill_batch(m, case.prompts, cache)
    for b in range(len(LENS)):
        case.check(logits[b], b, 0, "prefill_batch")
    dec = BatchGraphDecoder(m, cache)
    for t in range(FORCED):
        logits = dec.step([f[t] for f in case.forced], use_graph=False)
        for b in range(len(LENS)):
            case.check(logits[b], b, t + 1, "BatchGraphDecoder.step")
    assert cache.lens == [n + FORCED for n in LENS]
