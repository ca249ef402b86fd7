"""KV-cache text generation (reference I1/I2: ``model.generate`` in ask_tuned_model.py:55-65).

Prefill runs the training kernels (fused RMSNorm, packed QKV GEMM, in-place RoPE, the varlen
flash-attention forward) over the prompt and stores K/V in a preallocated cache sized for the
whole generation (288 GB of HBM: no paging needed at this scale). On the GPU the decode step is
shape-static — the token, its position and the live cache length sit in device tensors, the KV
append is an ``index_copy_`` and attention is the HIP split-K decode kernel that reads the
length from device memory — so ONE decode step is captured into a hipGraph and replayed per
token (no per-layer launch overhead, no host sync inside the step). On CPU the same step runs
eagerly. Sampling matches HF's logits-processor order: repetition penalty -> temperature ->
top-k -> top-p -> multinomial.

``generate_batch`` decodes many prompts per step: one packed varlen prefill, one cache slab per
sequence (``BatchKVCache``), and a ``BatchGraphDecoder`` whose captured step runs B rows through
the batched decode attention and the batched sampler, so the weights are read once per step for
the whole batch. Element b of its result is what ``generate`` returns for prompt b with seed + b.

``rollout_batch`` is the sampling side of reinforcement learning (train/grpo.py): the same batched decoder with
``FullVocabSampler`` (``sample_tokens_full``: an unbiased draw from the whole softmax(logits / temperature), with the
drawn tokens' log-probabilities) in the captured step.

Structure: the layer sequence is written once (``_run_layers``), the final norm + lm_head once (``_logits``). A path
is the ``attend(li, qkv)`` it passes in, which stores the step's K/V and attends: ``forward_cached`` prefill (slice
store, flash attention), ``forward_cached`` decode (slice store, eager fp32 attention: the CPU step),
``GraphDecoder`` (``index_copy_`` at the device position, ``ops.decode_attention``), ``prefill_batch`` (scatter
into the slabs, varlen flash attention) and ``BatchGraphDecoder`` (``ops.decode_attention_batched`` stores and
attends). What a layer does to q|k before attention is ``Attention.rotate_qk_``, shared with training. ``_capture``
turns a step into a hipGraph; the two sampler classes share ``_presence`` and ``_sampler_params``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from .. import ops


class KVCache:
    def __init__(self, cfg, max_len: int, device, dtype=torch.bfloat16):
        L = cfg.num_hidden_layers
        self.k = torch.empty(L, max_len, cfg.num_key_value_heads, cfg.head_dim, device=device, dtype=dtype)
        self.v = torch.empty_like(self.k)
        self.len = 0


def _heads(cfg):
    return cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim


def _windows(model) -> List[int]:
    """Every layer's sliding window (0: none), as its Attention module holds it. The cache stays a full-length slab
    either way: a window only narrows the rows a step attends over."""
    return [layer.self_attn.window for layer in model.model.layers]


def _kv_rows(cfg, qkv: torch.Tensor):
    """The k and v columns of the packed qkv [M, (nq + 2 nkv) D] as [M, nkv, D] views."""
    nq, nkv, D = _heads(cfg)
    M = qkv.shape[0]
    return qkv[:, nq * D:(nq + nkv) * D].view(M, nkv, D), qkv[:, (nq + nkv) * D:].view(M, nkv, D)


@torch.no_grad()
def _run_layers(model, ids: torch.Tensor, pos: torch.Tensor, attend):
    """Embeds ``ids`` [M] and runs every decoder layer on them at positions ``pos`` [M]: norm, qkv projection (plain
    or LoRA), the layer's q|k op (Attention.rotate_qk_; the RoPE tables are built once per pass), attention, o
    projection, norm, MLP. ``attend(li, qkv) -> a [M, nq * D]`` is the part the paths differ in: it stores the rows'
    K/V of layer li in its cache and attends. Returns the last MLP output and the residual stream before adding it
    (``_logits`` adds and norms them)."""
    cfg = model.config
    x = ops.embedding(ids, model.model.embed_tokens)
    residual = None
    cos = sin = None
    for li, layer in enumerate(model.model.layers):
        at = layer.self_attn
        h, residual = ops.add_rms_norm(x, residual, layer.input_layernorm.weight, cfg.rms_norm_eps)
        qkv = ops.linear(h, at.qkv_proj) if at.lora is None else ops.lora_linear(h, at.qkv_proj, at.lora["qkv"])
        if at.use_rope:
            if cos is None:
                cos, sin = model.rope_tables(pos)
            qkv = at.rotate_qk_(qkv, cos, sin)
        a = attend(li, qkv)
        o = ops.linear(a, at.o_proj) if at.lora is None else ops.lora_linear(a, at.o_proj, at.lora["o"])
        h, residual = ops.add_rms_norm(o, residual, layer.post_attention_layernorm.weight, cfg.rms_norm_eps)
        x = layer.mlp(h)
    return x, residual


@torch.no_grad()
def _logits(model, x: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """Final norm and lm_head over the given rows of a ``_run_layers`` result: fp32 logits [rows, V]."""
    h, _ = ops.add_rms_norm(x, residual, model.model.norm.weight, model.config.rms_norm_eps)
    return torch.nn.functional.linear(h, model.lm_head_weight).float()


@torch.no_grad()
def forward_cached(model, ids: torch.Tensor, cache: KVCache, prefill: bool) -> torch.Tensor:
    """ids: [M] tokens appended at positions cache.len ... Returns last-token logits [V] (fp32)."""
    nq, nkv, D = _heads(model.config)
    M, s = ids.numel(), cache.len
    W = _windows(model)
    cu = torch.tensor([0, M], dtype=torch.int32, device=ids.device) if prefill else None

    def store(li, qkv):
        cache.k[li, s:s + M], cache.v[li, s:s + M] = _kv_rows(model.config, qkv)

    def attend_prefill(li, qkv):
        store(li, qkv)
        return ops.flash_attention(qkv.contiguous(), cu, M, nq, nkv, D, window=W[li])

    def attend_decode(li, qkv):  # one row, eagerly in fp32 over the cache (the CPU path's decode step)
        store(li, qkv)
        q = qkv[:, :nq * D].view(nq, D).float()
        lo = max(0, s + 1 - W[li]) if W[li] else 0  # the layer's sliding window: the last W rows
        K = cache.k[li, lo:s + 1].float()  # [S, nkv, D]
        V = cache.v[li, lo:s + 1].float()
        att = torch.einsum("grd,sgd->grs", q.view(nkv, nq // nkv, D), K) / math.sqrt(D)
        return torch.einsum("grs,sgd->grd", att.softmax(-1), V).reshape(1, nq * D).to(qkv.dtype)

    pos = torch.arange(s, s + M, device=ids.device)
    x, residual = _run_layers(model, ids, pos, attend_prefill if prefill else attend_decode)
    cache.len += M
    return _logits(model, x[-1:], residual[-1:])[0]


def sample_next(logits: torch.Tensor, history: torch.Tensor, temperature: float = 0.6, top_k: int = 40,
                top_p: float = 0.95, repetition_penalty: float = 1.1, do_sample: bool = True,
                generator: Optional[torch.Generator] = None) -> int:
    logits = logits.clone()
    if repetition_penalty and repetition_penalty != 1.0 and history.numel():
        sc = logits[history]
        logits[history] = torch.where(sc < 0, sc * repetition_penalty, sc / repetition_penalty)
    if not do_sample:
        return int(logits.argmax())
    logits = logits / max(temperature, 1e-5)
    if top_k and top_k > 0:
        kth = torch.topk(logits, min(top_k, logits.numel())).values[-1]
        logits[logits < kth] = -float("inf")
    if top_p is not None and top_p < 1.0:
        sl, si = torch.sort(logits, descending=True)
        cp = sl.softmax(-1).cumsum(-1)
        remove = cp > top_p
        remove[1:] = remove[:-1].clone()
        remove[0] = False
        logits[si[remove]] = -float("inf")
    p = logits.softmax(-1)
    return int(torch.multinomial(p, 1, generator=generator))


def _presence(vocab_size: int, histories, device) -> torch.Tensor:
    """Token histories as presence bitmasks [B, ceil(V / 32)] (int32 words; bit t & 31 of word t >> 5 is token t)."""
    import numpy as np
    words = np.zeros((len(histories), (vocab_size + 31) // 32), dtype=np.uint32)
    for b, hist in enumerate(histories):
        ids = np.asarray(list(hist), dtype=np.int64)
        np.bitwise_or.at(words[b], ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32).copy()).to(device)


def _sampler_params(temperature, top_k, top_p, repetition_penalty, do_sample, seed):
    """The scalar arguments of the two sampler ops, in their order. Greedy is top-1; no seed draws one."""
    return (float(temperature), int(top_k) if do_sample else 1, float(top_p if top_p is not None else 1.0),
            float(repetition_penalty or 1.0), bool(do_sample),
            int(seed if seed is not None else torch.randint(0, 2 ** 31 - 1, (1,)).item()))


class DeviceSampler:
    """GPU-resident sampling state of one sequence for the fused HIP sampler (csrc/sampler.hip): the
    history as a presence bitmask (repetition penalty is a set operation), a step counter that keys the
    counter-based RNG, the running position / KV length, and a device log of the generated tokens."""

    def __init__(self, vocab_size: int, device, history_ids, max_new_tokens: int, seed: Optional[int],
                 temperature: float, top_k: int, top_p: Optional[float], repetition_penalty: float, do_sample: bool):
        self.presence = _presence(vocab_size, [history_ids], device)[0]
        self.state = torch.zeros(4, dtype=torch.long, device=device)
        self.log = torch.full((max(1, max_new_tokens),), -1, dtype=torch.long, device=device)
        self.params = _sampler_params(temperature, top_k, top_p, repetition_penalty, do_sample, seed)

    @staticmethod
    def supported(top_k: int, do_sample: bool) -> bool:
        return (not do_sample) or (top_k is not None and 1 <= top_k <= 64)

    def sample(self, logits: torch.Tensor, tok_out=None, pos_out=None, len_out=None) -> None:
        t, k, p, rp, ds, seed = self.params
        ops_ext().sample_token(logits.contiguous(), self.presence, self.state, tok_out, pos_out, len_out, self.log,
                               t, k, p, rp, ds, seed)


def ops_ext():
    from ..ops import _ext
    return _ext.ops()


def _capture(body, live=()) -> "torch.cuda.CUDAGraph":
    """``body`` as a hipGraph. It first runs twice on a side stream (allocator, kernel and library set-up outside
    the capture); ``live`` are the tensors body advances (counters, sampler state), restored after the warm-up so
    the real sequence state is untouched."""
    saved = [t.clone() for t in live]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(s)
    for t, v in zip(live, saved):
        t.copy_(v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


class GraphDecoder:
    """Static-shape decode step over a KVCache, captured once into a hipGraph (GPU)."""

    def __init__(self, model, cache: KVCache):
        self.model, self.cache = model, cache
        dev = model.model.embed_tokens.device
        self.tok = torch.zeros(1, dtype=torch.long, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)
        self.len = torch.ones(1, dtype=torch.int32, device=dev)
        self.graph = None
        self.logits = None
        self.windows = _windows(model)  # launch constants of the decode op: the captured graph stays shape-static

    def _attend(self, li: int, qkv: torch.Tensor) -> torch.Tensor:
        nq, nkv, D = _heads(self.model.config)
        k, v = _kv_rows(self.model.config, qkv)
        self.cache.k[li].index_copy_(0, self.pos, k)
        self.cache.v[li].index_copy_(0, self.pos, v)
        return ops.decode_attention(qkv[0, :nq * D].contiguous(), self.cache.k[li], self.cache.v[li], self.len,
                                    nq, nkv, window=self.windows[li]).view(1, nq * D)

    def _step(self) -> torch.Tensor:
        x, residual = _run_layers(self.model, self.tok, self.pos, self._attend)
        return _logits(self.model, x, residual)[0]

    def run_sampled(self, sampler: DeviceSampler, n: int, use_graph: bool = True) -> None:
        """n decode steps entirely on the device: each step runs the model on self.tok at self.pos and the
        fused sampler writes the next token / position / KV length back into the step's inputs (one
        hipGraph holds both, so consecutive replays need no host involvement)."""
        def body():
            sampler.sample(self._step(), self.tok, self.pos, self.len)
        if not use_graph:
            for _ in range(n):
                body()
            return
        if self.graph is None:
            self.graph = _capture(body, (self.tok, self.pos, self.len, sampler.state, sampler.presence, sampler.log))
        for _ in range(n):
            self.graph.replay()

    def step(self, token: int, position: int, use_graph: bool = True) -> torch.Tensor:
        self.tok.fill_(token)
        self.pos.fill_(position)
        self.len.fill_(position + 1)
        if not use_graph:
            return self._step()
        if self.graph is None:
            def body():  # the captured call's logits are the graph's static output
                self.logits = self._step()
            self.graph = _capture(body)
        self.graph.replay()
        return self.logits


@torch.no_grad()
def generate(model, prompt_ids: List[int], max_new_tokens: int = 256, eos_token_id: Optional[int] = None,
             temperature: float = 0.6, top_k: int = 40, top_p: float = 0.95, repetition_penalty: float = 1.1,
             do_sample: bool = True, seed: Optional[int] = None, use_graph: Optional[bool] = None,
             device_sampling: Optional[bool] = None) -> List[int]:
    model.eval()
    dev = model.model.embed_tokens.device
    cache = KVCache(model.config, len(prompt_ids) + max_new_tokens + 1, dev, model.model.embed_tokens.dtype)
    g = torch.Generator(device=dev).manual_seed(seed) if seed is not None else None
    ids = torch.tensor(prompt_ids, device=dev)
    logits = forward_cached(model, ids, cache, prefill=True)
    gpu_path = dev.type == "cuda" and model.config.head_dim == 128 and ops.use_hip(ids)
    dec = GraphDecoder(model, cache) if gpu_path else None
    graph = gpu_path if use_graph is None else (use_graph and gpu_path)
    if device_sampling is None:
        device_sampling = DeviceSampler.supported(top_k, do_sample)
    if gpu_path and max_new_tokens > 0 and device_sampling:
        return _generate_device(model, dec, cache, prompt_ids, logits, max_new_tokens, eos_token_id, temperature, top_k,
                                top_p, repetition_penalty, do_sample, seed, graph)
    hist = ids.clone()
    out: List[int] = []
    for _ in range(max_new_tokens):
        t = sample_next(logits, hist, temperature, top_k, top_p, repetition_penalty, do_sample, g)
        out.append(t)
        if eos_token_id is not None and t == eos_token_id:
            break
        nt = torch.tensor([t], device=dev)
        hist = torch.cat([hist, nt])
        if dec is not None:
            logits = dec.step(t, cache.len, use_graph=graph).clone()
            cache.len += 1
        else:
            logits = forward_cached(model, nt, cache, prefill=False)
    return out


def _generate_device(model, dec: GraphDecoder, cache: KVCache, prompt_ids, logits, max_new_tokens, eos_token_id,
                     temperature, top_k, top_p, repetition_penalty, do_sample, seed, use_graph, check_every: int = 16):
    """Decode loop with sampling on the device (fused HIP sampler inside the decode hipGraph). The host
    only reads the token log every ``check_every`` steps to stop at EOS."""
    dev = model.model.embed_tokens.device
    sm = DeviceSampler(model.config.vocab_size, dev, prompt_ids, max_new_tokens, seed, temperature, top_k, top_p,
                       repetition_penalty, do_sample)
    sm.state[2] = cache.len - 1  # the first sampled token gets position len(prompt)
    sm.sample(logits, dec.tok, dec.pos, dec.len)  # token 1 from the prefill logits
    done = 1
    out: List[int] = []
    while True:
        if eos_token_id is not None or done >= max_new_tokens:
            toks = sm.log[:done].tolist()
            if eos_token_id is not None and eos_token_id in toks:
                out = toks[:toks.index(eos_token_id) + 1]
                break
            if done >= max_new_tokens:
                out = toks
                break
        n = min(check_every, max_new_tokens - done)
        dec.run_sampled(sm, n, use_graph=use_graph)
        done += n
    cache.len = len(prompt_ids) + len(out)
    return out


# ----------------------------------------------------------------------------- batched generation
class BatchKVCache:
    """One slab [S_max, nkv, D] per sequence and layer: ``k[li]`` is the [B, S_max, nkv, D] cache of layer li.
    ``lens[b]`` is the number of tokens of sequence b already in the cache."""

    def __init__(self, cfg, batch: int, max_len: int, device, dtype=torch.bfloat16):
        L = cfg.num_hidden_layers
        self.k = torch.empty(L, batch, max_len, cfg.num_key_value_heads, cfg.head_dim, device=device, dtype=dtype)
        self.v = torch.empty_like(self.k)
        self.lens = [0] * batch


@torch.no_grad()
def prefill_batch(model, prompts: List[List[int]], cache: BatchKVCache) -> torch.Tensor:
    """All prompts in ONE packed varlen pass (cu_seqlens, per-sample positions) through the ops forward_cached
    uses; K/V are scattered into each sequence's slab. Returns the last-token logits [B, V] (fp32)."""
    dev = model.model.embed_tokens.device
    nq, nkv, D = _heads(model.config)
    W = _windows(model)
    n = [len(p) for p in prompts]
    assert len(n) == len(cache.lens) and min(n) > 0 and max(n) <= cache.k.shape[2], "prompts do not fit the cache"
    ids = torch.tensor([t for p in prompts for t in p], device=dev)
    bounds = [0]
    for x in n:
        bounds.append(bounds[-1] + x)
    cu = torch.tensor(bounds, dtype=torch.int32, device=dev)
    pos = torch.cat([torch.arange(x) for x in n]).to(dev)
    seq = torch.repeat_interleave(torch.arange(len(n)), torch.tensor(n)).to(dev)

    def attend(li, qkv):
        cache.k[li][seq, pos], cache.v[li][seq, pos] = _kv_rows(model.config, qkv)
        return ops.flash_attention(qkv.contiguous(), cu, max(n), nq, nkv, D, window=W[li])

    x, residual = _run_layers(model, ids, pos, attend)
    cache.lens = list(n)
    last = (cu[1:] - 1).long()
    return _logits(model, x[last], residual[last])


class BatchDeviceSampler:
    """DeviceSampler for B rows (``sample_tokens`` in csrc/sampler.hip): presence [B, words], state [B, 4],
    log [B, cap] and a ``done`` flag per row. Row b draws with ``seed + b``; a row that draws EOS logs it, sets its
    flag and is skipped from then on."""

    def __init__(self, vocab_size: int, device, histories, max_new_tokens: int, seed: Optional[int],
                 eos_token_id: Optional[int], temperature: float, top_k: int, top_p: Optional[float],
                 repetition_penalty: float, do_sample: bool):
        B = len(histories)
        self.presence = _presence(vocab_size, histories, device)
        self.state = torch.zeros(B, 4, dtype=torch.long, device=device)
        self.log = torch.full((B, max(1, max_new_tokens)), -1, dtype=torch.long, device=device)
        self.done = torch.zeros(B, dtype=torch.int32, device=device)
        self.eos = -1 if eos_token_id is None else int(eos_token_id)
        self.params = _sampler_params(temperature, top_k, top_p, repetition_penalty, do_sample, seed)

    def sample(self, logits: torch.Tensor, tok_out=None, pos_out=None, len_out=None) -> None:
        t, k, p, rp, ds, seed = self.params
        ops_ext().sample_tokens(logits.contiguous(), self.presence, self.state, tok_out, pos_out, len_out, self.log,
                                self.done, self.eos, t, k, p, rp, ds, seed)

    def live_tensors(self):
        """What a step advances (restored after a graph capture's warm-up runs)."""
        return (self.state, self.presence, self.log, self.done)


class FullVocabSampler(BatchDeviceSampler):
    """BatchDeviceSampler drawing from softmax(penalised logits / temperature) over the whole vocabulary
    (``sample_tokens_full``: Gumbel-max, no top-k / top-p), with the drawn tokens' log-probabilities under that
    distribution in ``logp`` [B, cap]: the behaviour policy's side of a policy-gradient ratio."""

    def __init__(self, vocab_size: int, device, histories, max_new_tokens: int, seed: Optional[int],
                 eos_token_id: Optional[int], temperature: float, repetition_penalty: float):
        super().__init__(vocab_size, device, histories, max_new_tokens, seed, eos_token_id, temperature, 0, 1.0,
                         repetition_penalty, True)
        self.logp = torch.zeros(self.log.shape, dtype=torch.float32, device=device)

    def sample(self, logits: torch.Tensor, tok_out=None, pos_out=None, len_out=None) -> None:
        t, _, _, rp, _, seed = self.params
        ops_ext().sample_tokens_full(logits.contiguous(), self.presence, self.state, tok_out, pos_out, len_out,
                                     self.log, self.logp, self.done, self.eos, t, rp, seed)

    def live_tensors(self):
        return super().live_tensors() + (self.logp,)


class BatchGraphDecoder:
    """GraphDecoder for B sequences over a BatchKVCache: the step runs M = B rows through the same ops, with the
    batched HIP decode attention (csrc/decode_attention.hip) appending each row's K/V and attending over its own
    slab. ``tok`` / ``pos`` / ``len`` are [B] device tensors, so one captured step serves every token."""

    def __init__(self, model, cache: BatchKVCache):
        self.model, self.cache = model, cache
        dev = model.model.embed_tokens.device
        B = cache.k.shape[1]
        self.tok = torch.zeros(B, dtype=torch.long, device=dev)
        self.pos = torch.zeros(B, dtype=torch.long, device=dev)
        self.len = torch.ones(B, dtype=torch.int32, device=dev)
        self.graph = None          # model step only (step())
        self.sampled_graph = None  # model step + sampler (run_sampled())
        self.logits = None
        self.windows = _windows(model)  # launch constants, as in GraphDecoder

    def _attend(self, li: int, qkv: torch.Tensor) -> torch.Tensor:  # the op appends each row's K/V itself
        nq, nkv, _ = _heads(self.model.config)
        return ops.decode_attention_batched(qkv.contiguous(), self.cache.k[li], self.cache.v[li], self.len, nq, nkv,
                                            window=self.windows[li])

    def _step(self) -> torch.Tensor:
        return _logits(self.model, *_run_layers(self.model, self.tok, self.pos, self._attend))

    def run_sampled(self, sampler: BatchDeviceSampler, n: int, use_graph: bool = True) -> None:
        """n decode steps of every row entirely on the device (model step + fused sampler in one hipGraph)."""
        def body():
            sampler.sample(self._step(), self.tok, self.pos, self.len)
        if not use_graph:
            for _ in range(n):
                body()
            return
        if self.sampled_graph is None:
            self.sampled_graph = _capture(body, (self.tok, self.pos, self.len, *sampler.live_tensors()))
        for _ in range(n):
            self.sampled_graph.replay()

    def step(self, tokens, use_graph: bool = True, advance=None) -> torch.Tensor:
        """Decode ``tokens[b]`` at position ``cache.lens[b]`` for every row; returns the logits [B, V] (the graph's
        static output: clone to keep). Rows with ``advance[b]`` false keep their length (finished sequences)."""
        lens = self.cache.lens
        dev = self.tok.device
        self.tok.copy_(torch.as_tensor(tokens, dtype=torch.long).to(dev))
        self.pos.copy_(torch.tensor(lens, dtype=torch.long).to(dev))
        self.len.copy_(torch.tensor([x + 1 for x in lens], dtype=torch.int32).to(dev))
        for b in range(len(lens)):
            if advance is None or advance[b]:
                lens[b] += 1
        if not use_graph:
            return self._step()
        if self.graph is None:
            def body():  # the captured call's logits are the graph's static output
                self.logits = self._step()
            self.graph = _capture(body)
        self.graph.replay()
        return self.logits


@torch.no_grad()
def generate_batch(model, prompts: List[List[int]], max_new_tokens: int = 256, eos_token_id: Optional[int] = None,
                   temperature: float = 0.6, top_k: int = 40, top_p: float = 0.95, repetition_penalty: float = 1.1,
                   do_sample: bool = True, seed: Optional[int] = None, use_graph: Optional[bool] = None,
                   device_sampling: Optional[bool] = None) -> List[List[int]]:
    """Element b is what ``generate(model, prompts[b], ..., seed=seed + b)`` returns: every sequence stops at its
    own EOS (included) or at ``max_new_tokens``. All prompts are prefilled in one packed pass and decoded one
    token per sequence and step, so the weights are read once per step for the whole batch."""
    model.eval()
    B = len(prompts)
    if B == 0:
        return []
    if max_new_tokens <= 0:
        return [[] for _ in prompts]
    dev = model.model.embed_tokens.device
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    cache = BatchKVCache(model.config, B, max(len(p) for p in prompts) + max_new_tokens + 1, dev,
                         model.model.embed_tokens.dtype)
    logits = prefill_batch(model, prompts, cache)
    gpu_path = dev.type == "cuda" and model.config.head_dim == 128 and ops.use_hip(logits)
    graph = gpu_path if use_graph is None else (use_graph and gpu_path)
    dec = BatchGraphDecoder(model, cache)
    if device_sampling is None:
        device_sampling = DeviceSampler.supported(top_k, do_sample)
    if gpu_path and device_sampling:
        return _generate_batch_device(model, dec, prompts, logits, max_new_tokens, eos_token_id, temperature, top_k,
                                      top_p, repetition_penalty, do_sample, seed, graph)
    gens = [torch.Generator(device=dev).manual_seed(seed + b) for b in range(B)]
    hist = [torch.tensor(p, device=dev) for p in prompts]
    out: List[List[int]] = [[] for _ in prompts]
    live = [True] * B
    last = [0] * B
    for i in range(max_new_tokens):
        for b in range(B):
            if not live[b]:
                continue
            t = sample_next(logits[b], hist[b], temperature, top_k, top_p, repetition_penalty, do_sample, gens[b])
            out[b].append(t)
            last[b] = t
            if eos_token_id is not None and t == eos_token_id:
                live[b] = False  # its later steps re-decode the last token in place: wasted, not wrong
            else:
                hist[b] = torch.cat([hist[b], torch.tensor([t], device=dev)])
        if not any(live) or i + 1 == max_new_tokens:
            break
        logits = dec.step(last, use_graph=graph, advance=live)
    return out


def _generate_batch_device(model, dec: BatchGraphDecoder, prompts, logits, max_new_tokens, eos_token_id, temperature,
                           top_k, top_p, repetition_penalty, do_sample, seed, use_graph, check_every: int = 16):
    """Batched decode loop with sampling on the device. Between bursts of ``check_every`` replays the host reads
    only the finished flags; it stops when every row is done or has reached its cap, then reads the logs."""
    dev = model.model.embed_tokens.device
    sm = BatchDeviceSampler(model.config.vocab_size, dev, prompts, max_new_tokens, seed, eos_token_id, temperature,
                            top_k, top_p, repetition_penalty, do_sample)
    return _decode_with_sampler(dec, sm, prompts, logits, max_new_tokens, use_graph, check_every)[0]


def _decode_with_sampler(dec: BatchGraphDecoder, sm: BatchDeviceSampler, prompts, logits, max_new_tokens, use_graph,
                         check_every: int = 16):
    """The device decode loop for a given sampler. Returns (the rows' tokens, their draw counts)."""
    dev = dec.tok.device
    sm.state[:, 2] = torch.tensor([len(p) - 1 for p in prompts], device=dev)  # first sampled token: position len(p)
    sm.sample(logits, dec.tok, dec.pos, dec.len)  # token 1 of every row from the prefill logits
    steps = 1
    while steps < max_new_tokens and not bool(sm.done.all()):
        n = min(check_every, max_new_tokens - steps)
        dec.run_sampled(sm, n, use_graph=use_graph)
        steps += n
    counts = sm.state[:, 0].tolist()  # tokens drawn per row: a finished row stops counting
    log = sm.log.tolist()
    return [log[b][:counts[b]] for b in range(len(prompts))], counts


# ----------------------------------------------------------------------------- on-policy rollouts
@torch.no_grad()
def rollout_batch(model, prompts: List[List[int]], max_new_tokens: int = 256, eos_token_id: Optional[int] = None,
                  temperature: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0,
                  seed: Optional[int] = None, use_graph: Optional[bool] = None,
                  device_sampling: Optional[bool] = None) -> Tuple[List[List[int]], Optional[List[List[float]]]]:
    """Sampled completions for reinforcement learning: ``(tokens, logps)``, row b drawn with ``seed + b`` and ending at
    its EOS (included) or at ``max_new_tokens``. With ``top_k == 0`` every token is a draw from softmax(penalised
    logits / temperature) over the WHOLE vocabulary and ``logps[b][i]`` is its log-probability under that distribution;
    on the HIP path the batched graph decoder runs with ``sample_tokens_full`` inside the captured step, off it (or with
    ``device_sampling=False``) the host loop draws with ``multinomial``. With ``1 <= top_k <= 64`` the existing device
    sampler draws from the top k and ``logps`` is None (a truncated behaviour policy has no full-vocabulary ratio).
    The model's ``training`` flag is restored on return."""
    was_training = model.training
    model.eval()
    try:
        B = len(prompts)
        if B == 0:
            return [], ([] if not top_k else None)
        if max_new_tokens <= 0:
            return [[] for _ in prompts], ([[] for _ in prompts] if not top_k else None)
        if not float(temperature) > 0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        if top_k is None or int(top_k) < 0:
            raise ValueError(f"top_k must be >= 0 (0: the whole vocabulary), got {top_k}")
        top_k = int(top_k)
        dev = model.model.embed_tokens.device
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        cache = BatchKVCache(model.config, B, max(len(p) for p in prompts) + max_new_tokens + 1, dev,
                             model.model.embed_tokens.dtype)
        logits = prefill_batch(model, prompts, cache)
        gpu_path = dev.type == "cuda" and model.config.head_dim == 128 and ops.use_hip(logits)
        graph = gpu_path if use_graph is None else (use_graph and gpu_path)
        dec = BatchGraphDecoder(model, cache)
        if device_sampling is None:
            device_sampling = top_k == 0 or DeviceSampler.supported(top_k, True)
        if gpu_path and device_sampling:
            V = model.config.vocab_size
            if top_k == 0:
                sm = FullVocabSampler(V, dev, prompts, max_new_tokens, seed, eos_token_id, temperature,
                                      repetition_penalty)
            else:
                sm = BatchDeviceSampler(V, dev, prompts, max_new_tokens, seed, eos_token_id, temperature, top_k, 1.0,
                                        repetition_penalty, True)
            toks, counts = _decode_with_sampler(dec, sm, prompts, logits, max_new_tokens, graph)
            if top_k:
                return toks, None
            lp = sm.logp.tolist()
            return toks, [lp[b][:counts[b]] for b in range(B)]
        gens = [torch.Generator(device=dev).manual_seed(seed + b) for b in range(B)]
        hist = [torch.tensor(p, device=dev) for p in prompts]
        out: List[List[int]] = [[] for _ in prompts]
        lps: List[List[float]] = [[] for _ in prompts]
        live = [True] * B
        last = [0] * B
        for i in range(max_new_tokens):
            for b in range(B):
                if not live[b]:
                    continue
                t = sample_next(logits[b], hist[b], temperature, top_k, None, repetition_penalty, True, gens[b])
                if not top_k:
                    z = logits[b].clone()
                    if repetition_penalty != 1.0 and hist[b].numel():
                        sc = z[hist[b]]
                        z[hist[b]] = torch.where(sc < 0, sc * repetition_penalty, sc / repetition_penalty)
                    lps[b].append(float(torch.log_softmax(z / max(temperature, 1e-5), -1)[t]))
                out[b].append(t)
                last[b] = t
                if eos_token_id is not None and t == eos_token_id:
                    live[b] = False
                else:
                    hist[b] = torch.cat([hist[b], torch.tensor([t], device=dev)])
            if not any(live) or i + 1 == max_new_tokens:
                break
            logits = dec.step(last, use_graph=graph, advance=live)
        return out, (lps if not top_k else None)
    finally:
        model.train(was_training)
