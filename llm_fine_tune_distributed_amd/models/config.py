"""Model configuration for the decoder-only LMs this framework trains.

The reference loads ``HuggingFaceTB/SmolLM3-3B`` from the Hub (``training.py:54,97-102``).
There is no network here, so models are built from a config (HF ``config.json`` keys are
accepted) and either random-initialised or loaded from local safetensors.

SmolLM3 facts: GQA 16q/4kv, head_dim 128, 36 layers, SwiGLU 11008,
vocab 128256, tied embeddings, NoPE on every 4th layer (``no_rope_layers``), eps 1e-6.
"""
from __future__ import annotations

import dataclasses
import json
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional


@dataclass
class ModelConfig:
    model_type: str = "smollm3"
    vocab_size: int = 128256
    hidden_size: int = 2048
    intermediate_size: int = 11008
    num_hidden_layers: int = 36
    num_attention_heads: int = 16
    num_key_value_heads: int = 4
    head_dim: Optional[int] = None
    rms_norm_eps: float = 1e-6
    rope_theta: float = 2_000_000.0
    rope_scaling: Optional[Dict[str, Any]] = None
    max_position_embeddings: int = 32768
    tie_word_embeddings: bool = True
    # 1 = layer uses RoPE, 0 = NoPE layer (SmolLM3 convention).
    no_rope_layers: Optional[List[int]] = None
    no_rope_layer_interval: int = 4
    initializer_range: float = 0.02
    bos_token_id: Optional[int] = 128000
    eos_token_id: Optional[int] = 128001
    pad_token_id: Optional[int] = 128004
    torch_dtype: str = "bfloat16"
    # RMSNorm over every query and key head after the projection, before RoPE (Qwen3: self_attn.q_norm / k_norm).
    # None: decided by the model type.
    qk_norm: Optional[bool] = None
    # Learned bias on the q, k and v projections (not on o_proj), added before RoPE (Qwen2 / Qwen2.5:
    # self_attn.{q,k,v}_proj.bias). None: decided by the model type.
    qkv_bias: Optional[bool] = None
    # Sliding-window attention (Mistral): the query at position i sees the keys j with i - W < j <= i, W keys with
    # itself (transformers' sliding_window_overlay). None: full causal attention. Every layer has the same window;
    # each Attention module reads its own (Attention.window), so a per-layer list would only change that one read.
    sliding_window: Optional[int] = None
    # Sequence classification: None is the causal LM; 1 is a reward model, the trunk plus a ``score`` head [1, hidden]
    # and no LM head (HF ``...ForSequenceClassification`` with one label). No other value is accepted.
    num_labels: Optional[int] = None
    extra: Dict[str, Any] = field(default_factory=dict)

    def __post_init__(self):
        if self.qk_norm is None:
            self.qk_norm = self.model_type == "qwen3"
        if self.qkv_bias is None:
            self.qkv_bias = self.model_type == "qwen2"
        if self.head_dim is None:
            self.head_dim = self.hidden_size // self.num_attention_heads
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads
        if self.no_rope_layers is None:
            if self.model_type == "smollm3":
                iv = self.no_rope_layer_interval
                self.no_rope_layers = [int((i + 1) % iv != 0) for i in range(self.num_hidden_layers)]
            else:
                self.no_rope_layers = [1] * self.num_hidden_layers
        assert len(self.no_rope_layers) >= self.num_hidden_layers
        if self.sliding_window is not None:
            self.sliding_window = int(self.sliding_window)
            if self.sliding_window <= 0:
                raise ValueError(f"sliding_window must be a positive number of keys or None, got {self.sliding_window}")
        assert self.num_attention_heads % self.num_key_value_heads == 0
        if self.num_labels is not None and int(self.num_labels) != 1:
            raise ValueError(f"num_labels must be None (causal LM) or 1 (reward model), got {self.num_labels}")
        if self.num_labels is not None:
            self.num_labels = 1

    # ------------------------------------------------------------------ helpers
    @property
    def q_size(self) -> int:
        return self.num_attention_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.num_key_value_heads * self.head_dim

    @property
    def qkv_size(self) -> int:
        return self.q_size + 2 * self.kv_size

    def uses_rope(self, layer_idx: int) -> bool:
        return bool(self.no_rope_layers[layer_idx])

    def num_parameters(self) -> int:
        h, i, v = self.hidden_size, self.intermediate_size, self.vocab_size
        per_layer = h * self.qkv_size + self.q_size * h + 3 * h * i + 2 * h
        if self.qk_norm:
            per_layer += 2 * self.head_dim
        if self.qkv_bias:
            per_layer += self.qkv_size
        emb = v * h
        head = 0 if self.tie_word_embeddings else v * h
        return self.num_hidden_layers * per_layer + emb + head + h

    def flops_per_token(self, seq_len: int, training: bool = True, recompute: bool = False) -> float:
        """Analytic matmul FLOPs per token. Attention counted causal, and within the sliding window
        where the model has one."""
        h = self.hidden_size
        dense = self.num_hidden_layers * (h * self.qkv_size + self.q_size * h + 3 * h * self.intermediate_size)
        dense += self.vocab_size * h
        fwd = 2.0 * dense
        # causal attention: QK^T and PV, each 2*T*d per head per token, halved by the mask (T^2 / 2 pairs). With a
        # window W < T row i sees min(i + 1, W) keys instead of i + 1: exactly (T - W) (T - W + 1) / 2 pairs fewer.
        keys = seq_len / 2.0
        W = self.sliding_window
        if W is not None and W < seq_len:
            keys -= (seq_len - W) * (seq_len - W + 1) / 2.0 / seq_len
        fwd += self.num_hidden_layers * 2.0 * 2.0 * self.num_attention_heads * self.head_dim * keys
        if not training:
            return fwd
        mult = 4.0 if recompute else 3.0
        return fwd * mult

    # ------------------------------------------------------------------ (de)serialisation
    def to_hf_dict(self) -> Dict[str, Any]:
        arch = {"smollm3": "SmolLM3ForCausalLM", "llama": "LlamaForCausalLM",
                "qwen3": "Qwen3ForCausalLM", "qwen2": "Qwen2ForCausalLM"}.get(self.model_type, "LlamaForCausalLM")
        mtype = self.model_type
        if mtype == "llama" and self.sliding_window is not None:
            # Llama plus a window is Mistral (same weight names): transformers loads it with the same mask
            arch, mtype = "MistralForCausalLM", "mistral"
        d = {
            "architectures": [arch],
            "model_type": mtype,
            "vocab_size": self.vocab_size,
            "hidden_size": self.hidden_size,
            "intermediate_size": self.intermediate_size,
            "num_hidden_layers": self.num_hidden_layers,
            "num_attention_heads": self.num_attention_heads,
            "num_key_value_heads": self.num_key_value_heads,
            "head_dim": self.head_dim,
            "rms_norm_eps": self.rms_norm_eps,
            "rope_theta": self.rope_theta,
            "rope_scaling": self.rope_scaling,
            "max_position_embeddings": self.max_position_embeddings,
            "tie_word_embeddings": self.tie_word_embeddings,
            "hidden_act": "silu",
            "attention_bias": False,
            "mlp_bias": False,
            "initializer_range": self.initializer_range,
            "bos_token_id": self.bos_token_id,
            "eos_token_id": self.eos_token_id,
            "pad_token_id": self.pad_token_id,
            "torch_dtype": self.torch_dtype,
        }
        if self.model_type == "smollm3":
            d["no_rope_layers"] = list(self.no_rope_layers[: self.num_hidden_layers])
            d["no_rope_layer_interval"] = self.no_rope_layer_interval
        if mtype == "mistral":
            del d["mlp_bias"], d["attention_bias"]  # not MistralConfig keys
            d["sliding_window"] = self.sliding_window
        if self.model_type == "qwen3":
            del d["mlp_bias"]  # not a Qwen3Config key
            d["use_sliding_window"] = False
        if self.model_type == "qwen2":
            del d["mlp_bias"], d["attention_bias"]  # not Qwen2Config keys: the q / k / v biases are unconditional
            d["use_sliding_window"] = False
        if self.num_labels is not None:
            # a reward model: the model type's sequence-classification class with one label; transformers needs a pad
            # token to find each row's last token
            d["architectures"] = [arch.replace("ForCausalLM", "ForSequenceClassification")]
            d["num_labels"] = 1
            if d["pad_token_id"] is None:
                d["pad_token_id"] = self.eos_token_id if self.eos_token_id is not None else 0
        d.update(self.extra)
        return d

    @classmethod
    def from_hf_dict(cls, d: Dict[str, Any]) -> "ModelConfig":
        names = {f.name for f in dataclasses.fields(cls)}
        kw = {k: v for k, v in d.items() if k in names and k != "extra"}
        # transformers>=5 moves rope params into rope_parameters
        rp = d.get("rope_parameters")
        if isinstance(rp, dict):
            if "rope_theta" in rp:
                kw["rope_theta"] = rp["rope_theta"]
            if rp.get("rope_type", "default") not in ("default", None):
                kw["rope_scaling"] = rp
        if isinstance(kw.get("eos_token_id"), list):
            kw["eos_token_id"] = kw["eos_token_id"][0]
        kw.setdefault("model_type", d.get("model_type", "llama"))
        if kw["model_type"] not in ("smollm3", "llama", "qwen3", "qwen2"):
            kw["model_type"] = "llama"  # (mistral among them: Llama's weights plus sliding_window, read below)
        mt = kw["model_type"]
        kw.pop("sliding_window", None)
        kw.pop("num_labels", None)
        if any(str(a).endswith("ForSequenceClassification") for a in (d.get("architectures") or [])):
            # (transformers writes id2label in place of num_labels)
            n = d.get("num_labels", len(d["id2label"]) if d.get("id2label") else None)
            if n is None or int(n) != 1:
                raise NotImplementedError(f"sequence classification with num_labels={n}: only one-label reward models "
                                          "are supported")
            kw["num_labels"] = 1
        if mt == "llama":
            # Mistral: sliding_window (missing or null: full attention). One window for every layer: a layer_types
            # list may only repeat one type.
            if len(set(d.get("layer_types") or [])) > 1:
                raise NotImplementedError(f"layer_types {sorted(set(d['layer_types']))}: mixed layer types are not "
                                          "supported (one attention type for every layer)")
            if d.get("sliding_window") is not None and set(d.get("layer_types") or []) != {"full_attention"}:
                kw["sliding_window"] = int(d["sliding_window"])
        if mt in ("qwen3", "qwen2"):
            # what a Qwen config may ask for and this model does not implement: fail here, not in the weights loader
            if mt == "qwen3" and d.get("attention_bias"):
                raise NotImplementedError("qwen3: attention_bias=true is not supported (the projections have no bias)")
            if d.get("use_sliding_window"):
                raise NotImplementedError(f"{mt}: use_sliding_window=true is not supported (full attention only)")
            bad = sorted({t for t in (d.get("layer_types") or []) if t != "full_attention"})
            if bad:
                raise NotImplementedError(f"{mt}: layer_types {bad} are not supported (full_attention only)")
        if mt == "qwen2":
            # inert with use_sliding_window=false; kept so that a saved config says what the checkpoint's said
            extra = {k: d[k] for k in ("sliding_window", "max_window_layers") if k in d}
            if extra:
                kw["extra"] = extra
        return cls(**kw)

    @classmethod
    def from_pretrained(cls, path: str) -> "ModelConfig":
        with open(os.path.join(path, "config.json")) as f:
            return cls.from_hf_dict(json.load(f))

    def save_pretrained(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.to_hf_dict(), f, indent=2)


# ---------------------------------------------------------------------------- presets
def smollm3_3b() -> ModelConfig:
    """HuggingFaceTB/SmolLM3-3B (reference model, ``training.py:54``)."""
    return ModelConfig(model_type="smollm3")


def llama3_8b() -> ModelConfig:
    """Meta-Llama-3-8B shape (BASELINE.json config #5)."""
    return ModelConfig(
        model_type="llama", vocab_size=128256, hidden_size=4096, intermediate_size=14336,
        num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8, rope_theta=500000.0,
        max_position_embeddings=8192, tie_word_embeddings=False, rms_norm_eps=1e-5,
        eos_token_id=128001, pad_token_id=None,
    )


# The two Qwen3 shapes below are written from memory of the published config.json files (no copy of them was at hand):
# a real checkpoint directory's own config.json always wins (get_config on the directory).
def _qwen3(**kw) -> ModelConfig:
    base = dict(model_type="qwen3", vocab_size=151936, num_hidden_layers=36, num_attention_heads=32,
                num_key_value_heads=8, head_dim=128, rope_theta=1_000_000.0, rms_norm_eps=1e-6,
                max_position_embeddings=40960, bos_token_id=151643, eos_token_id=151645, pad_token_id=None)
    base.update(kw)
    return ModelConfig(**base)


def qwen3_4b() -> ModelConfig:
    """Qwen/Qwen3-4B shape (tied embeddings; q width 32 x 128 = 4096 > hidden 2560)."""
    return _qwen3(hidden_size=2560, intermediate_size=9728, tie_word_embeddings=True)


def qwen3_8b() -> ModelConfig:
    """Qwen/Qwen3-8B shape (untied lm_head)."""
    return _qwen3(hidden_size=4096, intermediate_size=12288, tie_word_embeddings=False)


# The Qwen2.5 shapes below are written from memory of the published config.json files too (no copy of them was at
# hand): a real checkpoint directory's own config.json always wins (get_config on the directory).
def _qwen2_5(**kw) -> ModelConfig:
    base = dict(model_type="qwen2", vocab_size=151936, head_dim=128, rope_theta=1_000_000.0, rms_norm_eps=1e-6,
                max_position_embeddings=32768, bos_token_id=151643, eos_token_id=151645, pad_token_id=None)
    base.update(kw)
    return ModelConfig(**base)


def qwen2_5_1_5b() -> ModelConfig:
    """Qwen/Qwen2.5-1.5B-Instruct shape (12 q / 2 kv heads, tied embeddings)."""
    return _qwen2_5(hidden_size=1536, intermediate_size=8960, num_hidden_layers=28, num_attention_heads=12,
                    num_key_value_heads=2, tie_word_embeddings=True)


def qwen2_5_3b() -> ModelConfig:
    """Qwen/Qwen2.5-3B-Instruct shape (16 q / 2 kv heads, tied embeddings)."""
    return _qwen2_5(hidden_size=2048, intermediate_size=11008, num_hidden_layers=36, num_attention_heads=16,
                    num_key_value_heads=2, tie_word_embeddings=True)


def qwen2_5_7b() -> ModelConfig:
    """Qwen/Qwen2.5-7B-Instruct shape (28 q / 4 kv heads, untied lm_head, vocabulary padded to 152064)."""
    return _qwen2_5(hidden_size=3584, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28,
                    num_key_value_heads=4, vocab_size=152064, tie_word_embeddings=False)


# Written from memory of the published config.json, like the Qwen shapes above (no copy of it was at hand): a real
# checkpoint directory's own config.json always wins (get_config on the directory).
def mistral_7b() -> ModelConfig:
    """mistralai/Mistral-7B-v0.1 shape: Llama's architecture (model_type "llama" here) plus a 4096-key sliding
    window; saved as MistralForCausalLM."""
    return ModelConfig(
        model_type="llama", vocab_size=32000, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
        num_attention_heads=32, num_key_value_heads=8, head_dim=128, rope_theta=10000.0, rms_norm_eps=1e-5,
        max_position_embeddings=32768, tie_word_embeddings=False, bos_token_id=1, eos_token_id=2, pad_token_id=None,
        sliding_window=4096,
    )


def tiny(model_type: str = "smollm3", **kw) -> ModelConfig:
    """Small config with the same structure (GQA, NoPE interval, tied head) for tests."""
    base = dict(
        model_type=model_type, vocab_size=1024, hidden_size=128, intermediate_size=256,
        num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, head_dim=32,
        rope_theta=10000.0, max_position_embeddings=1024, tie_word_embeddings=(model_type == "smollm3"),
        bos_token_id=1, eos_token_id=2, pad_token_id=2,
    )
    base.update(kw)
    return ModelConfig(**base)


PRESETS = {
    "smollm3-3b": smollm3_3b,
    "HuggingFaceTB/SmolLM3-3B": smollm3_3b,
    "llama3-8b": llama3_8b,
    "meta-llama/Meta-Llama-3-8B": llama3_8b,
    "tiny": tiny,
    "tiny-llama": lambda: tiny("llama"),
    # tiny depth/width with the real head_dim (128) the HIP attention kernels are built for (GPU tests)
    "tiny-gpu": lambda: tiny(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                             intermediate_size=512, vocab_size=1024, num_hidden_layers=3),
    "qwen3-4b": qwen3_4b,
    "Qwen/Qwen3-4B": qwen3_4b,
    "qwen3-8b": qwen3_8b,
    "Qwen/Qwen3-8B": qwen3_8b,
    "tiny-qwen3": lambda: tiny("qwen3"),
    "tiny-gpu-qwen3": lambda: tiny("qwen3", hidden_size=256, num_attention_heads=2, num_key_value_heads=1,
                                   head_dim=128, intermediate_size=512, vocab_size=1024, num_hidden_layers=3),
    "qwen2.5-1.5b": qwen2_5_1_5b,
    "Qwen/Qwen2.5-1.5B": qwen2_5_1_5b,
    "qwen2.5-3b": qwen2_5_3b,
    "Qwen/Qwen2.5-3B": qwen2_5_3b,
    "qwen2.5-7b": qwen2_5_7b,
    "Qwen/Qwen2.5-7B": qwen2_5_7b,
    "tiny-qwen2": lambda: tiny("qwen2"),
    "tiny-gpu-qwen2": lambda: tiny("qwen2", hidden_size=256, num_attention_heads=2, num_key_value_heads=1,
                                   head_dim=128, intermediate_size=512, vocab_size=1024, num_hidden_layers=3),
    "mistral-7b": mistral_7b,
    "mistralai/Mistral-7B-v0.1": mistral_7b,
    "tiny-mistral": lambda: tiny("llama", sliding_window=8),
    # head_dim 128, GQA 4 (the forward's four waves share their positions), a window below one 64-key tile
    "tiny-gpu-mistral": lambda: tiny("llama", hidden_size=256, num_attention_heads=4, num_key_value_heads=1,
                                     head_dim=128, intermediate_size=512, vocab_size=1024, num_hidden_layers=2,
                                     sliding_window=40),
}


def get_config(name_or_path: str) -> ModelConfig:
    if name_or_path in PRESETS:
        return PRESETS[name_or_path]()
    if os.path.isdir(name_or_path) and os.path.exists(os.path.join(name_or_path, "config.json")):
        return ModelConfig.from_pretrained(name_or_path)
    raise ValueError(f"unknown model {name_or_path!r}; presets: {sorted(PRESETS)}")
