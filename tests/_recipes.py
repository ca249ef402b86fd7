"""Training recipes on the gradient plumbing of ops/fused.py and parallel/ddp.py (a helper module, not a conftest).

One accumulation window of a small model is driven through a ``DDPEngine`` exactly as the trainer drives it
(``zero_grad``, then ``prepare_backward`` / forward / backward / ``finish_backward`` per micro-batch, ``no_sync`` on all
but the last) under a freeze policy, a micro-batch count and gradient checkpointing on or off, and the state the
deferred weight-gradient work leaves behind is checked. The checks carry the numbers used by
tests/test_train_recipes_gpu.py and tests/test_train_recipes_cpu.py:

1. every trainable parameter's ``main_grad`` against the fp32 reference, per 256 x 256 tile (``check_gradients``);
2. nothing stale, nothing missing: every ``main_grad`` is filled with NaN before ``zero_grad`` and the flat buffer is
   finite after the window (only the parameter slices are filled: the alignment padding between them is written by
   nobody and stays zero, as the optimizer and the clip norm expect);
3. every ready hook fires once per trainable parameter per backward, ``_sftamd_remaining == 0`` and
   ``_sftamd_fresh is False`` afterwards, frozen parameters are outside the engine's layout and nobody has a ``.grad``;
4. no ``MLPLink`` / ``AttnLink`` made during the window still holds a job or a delta after a backward (looked at while
   the loss still holds the graph whose nodes hold the links);
5. the fused clip norm equals the flat buffer's sum of squares, and the parameters with ``_sftamd_norm_done`` are
   recorded for the caller to compare with the set its recipe implies;
6. the dispatch trace of every micro-batch is recorded (GPU).

Checks 2-5 do not raise where they stand: they append ``(check number, subject, message)`` to ``Run.failures`` so that a
seeded fault can be shown to trip the check it should and no other; ``Run.raise_if_failed`` raises the lot.
"""
import contextlib
import math
import os
import weakref
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from _blockwise import block_rel_err, global_rel_err, rounding_floor
from llm_fine_tune_distributed_amd import ops as ops_pkg
from llm_fine_tune_distributed_amd.models import build_model
from llm_fine_tune_distributed_amd.models.freeze import apply_freeze_policy
from llm_fine_tune_distributed_amd.models.lora import LoRAConfig
from llm_fine_tune_distributed_amd.ops import _ext, fused
from llm_fine_tune_distributed_amd.parallel.ddp import DDPEngine

TILE = 256  # the weight-gradient kernels' output tile
MODEL_SEED = 11
ADAPTER_SEED = 5


# ----------------------------------------------------------------------------- recipes
@dataclass(frozen=True)
class Recipe:
    policy: str                # apply_freeze_policy's name
    batches: Tuple[int, ...]   # indices into the window, in the order they run; the last one synchronises
    ckpt: bool                 # gradient checkpointing
    n_last: int = 2


# The window is (padded, ragged, padded, padded): the ragged batch second, so that it accumulates onto kernel output
# and kernel launches accumulate onto it. lora runs (ragged, padded): a first contribution from the library route and a
# synchronising pass on the kernels.
RECIPES: Dict[str, Recipe] = {
    "plain": Recipe("full", (0,), False),
    "ga": Recipe("full", (0, 1, 2, 3), False),
    "ckpt": Recipe("full", (0, 1, 2, 3), True),
    "last2": Recipe("last_n_layers", (0, 1, 2, 3), False),
    "cli": Recipe("last_n_layers", (0, 1, 2, 3), True),  # cli/train.py's defaults
    "lora": Recipe("lora", (1, 2), False),
    "lora_ckpt": Recipe("lora", (1, 2), True),
    # two more windows, for what real (padding-free) data does: it synchronises on a ragged batch
    "ragged_sync": Recipe("full", (0, 2, 1), False),  # ... whose weight gradients all take the library route
    "rings": Recipe("full", (0, 4), False),           # ... or the lone-launch kernels (window[4], where there is one)
}


# ----------------------------------------------------------------------------- batches
@dataclass
class Batch:
    ids: torch.Tensor
    labels: torch.Tensor
    cu_seqlens: Optional[torch.Tensor] = None  # None: a padded [B, T] batch
    max_seqlen: Optional[int] = None

    @property
    def padded(self) -> bool:
        return self.cu_seqlens is None

    def forward(self, model):
        if self.padded:
            return model(self.ids, labels=self.labels)
        return model(self.ids, labels=self.labels, cu_seqlens=self.cu_seqlens, max_seqlen=self.max_seqlen)


def make_window(vocab: int, padded_shape: Tuple[int, int], ragged_lens: List[int], device, seed: int = 0,
                ragged_lens2: Optional[List[int]] = None) -> List[Batch]:
    """Four micro-batches with fixed seeds: padded, padding-free (ragged lengths), padded, padded — and a fifth,
    padding-free with ``ragged_lens2``, drawn last (so the first four do not depend on it). Labels are the ids with an
    ignored tail: the last fifth of every padded row and of every ragged sequence."""
    g = torch.Generator().manual_seed(seed)
    B, T = padded_shape

    def padded():
        ids = torch.randint(0, vocab, (B, T), generator=g)
        labels = ids.clone()
        labels[:, T - T // 5:] = -100
        return Batch(ids.to(device), labels.to(device))

    def ragged(ragged_lens=ragged_lens):
        n = sum(ragged_lens)
        ids = torch.randint(0, vocab, (n,), generator=g)
        labels = ids.clone()
        cu = [0]
        for L in ragged_lens:
            cu.append(cu[-1] + L)
            labels[cu[-1] - L // 5:cu[-1]] = -100
        return Batch(ids.to(device), labels.to(device), torch.tensor(cu, dtype=torch.int32, device=device),
                     max(ragged_lens))

    return [padded(), ragged(), padded(), padded(), ragged(ragged_lens2 or ragged_lens[::-1])]


# ----------------------------------------------------------------------------- models
@contextlib.contextmanager
def hip_path(enabled: bool):
    """SFTAMD_DISABLE_HIP=1 while ``enabled`` is false (ops/_ext.py reads it per call), restored afterwards."""
    old = os.environ.get("SFTAMD_DISABLE_HIP")
    if not enabled:
        os.environ["SFTAMD_DISABLE_HIP"] = "1"
    try:
        yield
    finally:
        if not enabled:
            if old is None:
                os.environ.pop("SFTAMD_DISABLE_HIP", None)
            else:
                os.environ["SFTAMD_DISABLE_HIP"] = old


def build(cfg, recipe: Recipe, device, dtype, param_dtype=None):
    """The recipe's model: the weights of ``build_model(seed=MODEL_SEED)`` in ``param_dtype`` (what the path under test
    holds: every build has the same values) cast to ``dtype``, the freeze policy applied, checkpointing as the recipe
    says. lora: r 16, no dropout, adapters drawn at N(0, 0.05) from a fixed seed and rounded through ``param_dtype``, so
    that the fp32 reference holds the adapters of the bf16 model."""
    param_dtype = param_dtype or dtype
    m = build_model(cfg, device=device, dtype=param_dtype, seed=MODEL_SEED)
    if dtype != param_dtype:
        for p in m.parameters():
            p.data = p.data.to(dtype)
    if recipe.policy == "lora":
        apply_freeze_policy(m, "lora", lora_config=LoRAConfig(r=16, lora_alpha=16, lora_dropout=0.0))
        g = torch.Generator().manual_seed(ADAPTER_SEED)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if ".lora." in n and p.numel() > 0:
                    v = torch.randn(p.shape, generator=g).mul_(0.05).to(param_dtype)
                    p.copy_(v.to(device=device, dtype=dtype))
    else:
        apply_freeze_policy(m, recipe.policy, n_last=recipe.n_last)
    if recipe.ckpt:
        m.gradient_checkpointing_enable()
    m.train()
    return m


def reference_grads(cfg, recipe: Recipe, window: List[Batch], device, param_dtype) -> List[Dict[str, torch.Tensor]]:
    """Per micro-batch of the window: {name: plain ``p.grad``} of the fp32 model on the PyTorch path (no engine, no
    main_grad). ``recipe`` only chooses the parameter set (full, or the adapters): every non-lora recipe trains a subset
    of the same parameters on the same loss, so it is compared against the full set."""
    with hip_path(False):
        m = build(cfg, Recipe(recipe.policy, recipe.batches, False), device, torch.float32, param_dtype)
        out = []
        for b in window:
            m.zero_grad(set_to_none=True)
            b.forward(m).loss.backward()
            out.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    return out


def reference_sum(per_batch: List[Dict[str, torch.Tensor]], batches, name: str) -> torch.Tensor:
    """The window's reference gradient of one parameter, summed in fp64."""
    return sum(per_batch[i][name].double() for i in batches)


# ----------------------------------------------------------------------------- one window
@dataclass
class Run:
    model: torch.nn.Module
    eng: DDPEngine
    recipe: Recipe
    failures: List[tuple] = field(default_factory=list)  # (check number, subject, message)
    traces: List[Optional[dict]] = field(default_factory=list)  # per micro-batch (None off the GPU)
    losses: List[float] = field(default_factory=list)
    norm: Optional[Tuple[float, float]] = None  # (fused clip norm^2, sum of squares of the flat buffer)
    norm_done: Optional[set] = None  # names with _sftamd_norm_done after the synchronising pass
    links_seen: int = 0
    links_checked: int = 0  # links that were alive when check 4 looked at them
    pass_index: int = -1

    def fail(self, check: int, subject: str, msg: str) -> None:
        self.failures.append((check, subject, msg))

    def failed(self, check: int) -> List[str]:
        """Subjects (parameter names, link kinds, ...) check ``check`` failed on."""
        return [s for c, s, _ in self.failures if c == check]

    def raise_if_failed(self) -> None:
        if self.failures:
            ordered = sorted(self.failures, key=lambda f: f[0])  # (stable: by check, then as they happened)
            raise AssertionError("; ".join(f"check {c} [{s}]: {m}" for c, s, m in ordered[:12])
                                 + (f" ... and {len(ordered) - 12} more" if len(ordered) > 12 else ""))

    def named_trainable(self):
        return [(self.eng.param_names[id(p)], p) for p, _, _, _ in self.eng.layout]


def read_trace() -> dict:
    out = {}
    for item in _ext.ops().dispatch_trace_read().split(";"):
        if item:
            k, v = item.split("=")
            out[k] = int(v)
    return out


@contextlib.contextmanager
def _patched(items):
    """setattr every (object, attribute, value) of ``items``; restore on exit."""
    saved = [(o, a, getattr(o, a)) for o, a, _ in items]
    try:
        for o, a, v in items:
            setattr(o, a, v)
        yield
    finally:
        for o, a, v in reversed(saved):
            setattr(o, a, v)


def _recording_links(store: list):
    """Subclasses of the two link classes that keep a weak reference to every instance in ``store``."""
    class RecMLPLink(fused.MLPLink):
        __slots__ = ("__weakref__",)

        def __init__(self):
            super().__init__()
            store.append(("MLPLink", weakref.ref(self)))

    class RecAttnLink(fused.AttnLink):
        __slots__ = ("__weakref__",)

        def __init__(self):
            super().__init__()
            store.append(("AttnLink", weakref.ref(self)))

    items = [(fused, "MLPLink", RecMLPLink), (fused, "AttnLink", RecAttnLink)]
    for name, cls in (("MLPLink", RecMLPLink), ("AttnLink", RecAttnLink)):
        if hasattr(ops_pkg, name):  # models/transformer.py makes its links through the package's re-export
            items.append((ops_pkg, name, cls))
    return items


_LINK_FIELDS = {"MLPLink": ("down_job", "attn_jobs"), "AttnLink": ("o_job", "delta")}


def run_window(model, recipe: Recipe, window: List[Batch], hip: bool = True, checks: bool = True,
               patches: Optional[Callable] = None, post: Optional[Callable] = None) -> Run:
    """One accumulation window of ``recipe`` on ``model`` through ``DDPEngine(model, 1, 0)``, with checks 2-6 of the
    module docstring (``checks=False``: just the window, for the PyTorch-path twin). ``patches(run)`` returns
    ``(object, attribute, value)`` triples that are set for the duration of the window (seeded faults read
    ``run.pass_index``); ``post(run)`` runs after the window and its checks (a fault seeded into the result)."""
    eng = DDPEngine(model, 1, 0)
    run = Run(model, eng, recipe)
    on_gpu = eng.device.type == "cuda"
    trainable = run.named_trainable()
    fired = {n: 0 for n, _ in trainable}
    name_of = eng.param_names

    def counted(orig):
        def hook(p):
            fired[name_of[id(p)]] += 1
            return orig(p)
        return hook

    # every road to "this parameter is complete": the hook the fused ops call on the parameter, and the engine's own
    # method, which DDPEngine._post_accumulate calls for plain-autograd parameters. The first wraps the bound method
    # captured here, not the instance attribute, so no firing counts twice.
    for _, p in trainable:
        p._sftamd_ready_hook = counted(p._sftamd_ready_hook)
    eng._on_param_ready = counted(eng._on_param_ready)

    links: list = []
    items = _recording_links(links) if checks else []
    if patches is not None:
        items += list(patches(run))
    with hip_path(hip), _patched(items):
        if checks:
            for _, p in trainable:
                p.main_grad.fill_(float("nan"))
        eng.zero_grad()
        for k, bi in enumerate(recipe.batches):
            run.pass_index = k
            last = k == len(recipe.batches) - 1
            for n in fired:
                fired[n] = 0
            tracing = on_gpu and hip and checks
            if tracing:
                _ext.ops().dispatch_trace(True)
            try:
                with (contextlib.nullcontext() if last else eng.no_sync()):
                    eng.prepare_backward()
                    loss = window[bi].forward(model).loss
                    loss.backward()
                    eng.finish_backward()
                if on_gpu:
                    torch.cuda.synchronize()
            finally:
                if tracing:
                    _ext.ops().dispatch_trace(False)
            run.traces.append(read_trace() if tracing else None)
            run.losses.append(loss.item())
            if checks:
                _check_counters(run, fired, k)
                # while ``loss`` holds the graph: its nodes hold the links, which would otherwise be gone (and the check
                # empty) by now
                _check_links(run, links, k)
            del loss
        if checks:
            if not bool(torch.isfinite(eng.grad_flat).all()):
                for n, p in trainable:
                    if not bool(torch.isfinite(p.main_grad).all()):
                        run.fail(2, n, "main_grad is not finite after the window: a slice was neither overwritten by a "
                                       "first contribution nor cleared by _zero_untouched")
            if eng.fused_norm:
                run.norm_done = {n for n, p in trainable if getattr(p, "_sftamd_norm_done", False)}
                got = eng.grad_norm_sq()
                want = eng.grad_flat.float().pow(2).sum().item()
                if got is None:
                    run.fail(5, "grad_norm_sq", "no fused norm after a synchronising pass")
                else:
                    run.norm = (got.item(), want)
                    if not abs(got.item() - want) <= 1e-4 * want:  # the bound of test_fused_grad_norm_world1
                        run.fail(5, "grad_norm_sq", f"fused norm^2 {got.item():.6e} vs buffer {want:.6e}")
    run.links_seen = len(links)
    if post is not None:
        post(run)
    return run


def _check_counters(run: Run, fired: dict, k: int) -> None:
    eng, model = run.eng, run.model
    in_layout = {id(p) for p, _, _, _ in eng.layout}
    for n, p in run.named_trainable():
        if fired[n] != 1:
            run.fail(3, n, f"pass {k}: ready hook fired {fired[n]} times")
        rem = getattr(p, "_sftamd_remaining", None)
        if rem != 0:
            run.fail(3, n, f"pass {k}: _sftamd_remaining == {rem}")
        if getattr(p, "_sftamd_fresh", None) is not False:
            run.fail(3, n, f"pass {k}: _sftamd_fresh is {getattr(p, '_sftamd_fresh', None)!r}")
    for n, p in model.named_parameters():
        if p.requires_grad != (id(p) in in_layout):
            run.fail(3, n, f"requires_grad {p.requires_grad} but in the engine's layout: {id(p) in in_layout}")
        if p.grad is not None:
            run.fail(3, n, f"pass {k}: .grad is set")


def _check_links(run: Run, links: list, k: int) -> None:
    for kind, ref in links:
        link = ref()
        if link is None:
            continue
        run.links_checked += 1
        for f in _LINK_FIELDS[kind]:
            if getattr(link, f) is not None:
                run.fail(4, f"{kind}.{f}", f"pass {k}: a {kind} still holds {f} after the backward")


# ----------------------------------------------------------------------------- check 1: every gradient, per tile
def param_class(name: str) -> str:
    """``model.layers.2.self_attn.qkv_proj`` -> ``self_attn.qkv_proj``: the name without layer / adapter indices."""
    parts = [s for s in name.split(".") if not s.isdigit() and s not in ("layers",)]
    if len(parts) > 2 and parts[0] == "model":
        parts = parts[1:]
    return ".".join(parts)


def _as2d(t: torch.Tensor):
    """(the tensor as a matrix, block rows, block columns): 256 x 256 tiles; a 1-D parameter is one block."""
    if t.dim() == 1:
        return t.reshape(1, -1), 1, t.numel()
    return t, TILE, TILE


def block_errors(got: torch.Tensor, want64: torch.Tensor) -> torch.Tensor:
    g, br, bc = _as2d(got)
    w, _, _ = _as2d(want64)
    return block_rel_err(g, w, br, bc)


def grad_errors(run: Run, ref_per_batch) -> Dict[str, float]:
    """Worst block error of every trainable parameter's main_grad against the window's fp32 reference."""
    return {n: block_errors(p.main_grad, reference_sum(ref_per_batch, run.recipe.batches, n)).max().item()
            for n, p in run.named_trainable()}


def reference_bounds(ref_per_batch, batches, twin_errs: Optional[Dict[str, float]], names) -> Dict[str, float]:
    """Per parameter: 2 x the twin's worst block error against the fp32 reference (the project's margin over an
    emulation: swiglu_bwd_reference, row_bound), never below 2 x the rounding floor of the reference itself. Without a
    twin (the CPU harness, where the twin is the path) the floor decides."""
    out = {}
    for n in names:
        w, br, bc = _as2d(reference_sum(ref_per_batch, batches, n))
        floor = rounding_floor(w, br, bc)
        out[n] = 2 * max(floor, twin_errs[n] if twin_errs is not None else 0.0)
    return out


def check_gradients(run: Run, ref_per_batch, bounds: Dict[str, float], verbose: bool = True) -> Dict[str, float]:
    """Check 1. Every block of every trainable parameter within its bound; failures go to ``run.failures`` with the
    worst tile named. Returns {name: worst block error}."""
    errs = {}
    for n, p in run.named_trainable():
        want = reference_sum(ref_per_batch, run.recipe.batches, n)
        e = block_errors(p.main_grad, want)
        worst = e.max().item()
        errs[n] = worst
        if not worst <= bounds[n]:
            flat = int(torch.where(torch.isnan(e), torch.full_like(e, math.inf), e).argmax())
            i, j = divmod(flat, e.shape[1])
            g2, _, _ = _as2d(p.main_grad)
            w2, _, _ = _as2d(want)
            run.fail(1, n, f"worst tile ({i}, {j}) has error {e[i, j].item():.3e} > bound {bounds[n]:.3e}; "
                           f"{int((~(e <= bounds[n])).sum())} of {e.numel()} tiles over; "
                           f"whole-parameter error {global_rel_err(g2, w2):.3e}")
    if verbose:
        for cls, (worst, bound) in by_class(errs, bounds).items():
            print(f"  {cls:40s} worst tile {worst:.3e}  bound {bound:.3e}")
    return errs


def by_class(errs: Dict[str, float], bounds: Optional[Dict[str, float]] = None) -> Dict[str, tuple]:
    """{parameter class: (worst error, smallest bound)} over the parameters of the class."""
    out: Dict[str, tuple] = {}
    for n, e in errs.items():
        c = param_class(n)
        b = bounds[n] if bounds is not None else math.nan
        if c in out:
            out[c] = (max(out[c][0], e), min(out[c][1], b) if bounds is not None else b)
        else:
            out[c] = (e, b)
    return out


# ----------------------------------------------------------------------------- seeded faults (Python only)
def fault_drop_carried(layer: int):
    """(a) The qkv node of ``layer`` loses the jobs it hands on: ``_carry_or_launch`` drops them instead of leaving them
    with the previous layer's MLP link. On tensors that never reach that function (CPU: the projections are plain
    LinearFn nodes whose jobs go straight to ``_accumulate_weight_grad_jobs``) the same two jobs are dropped there."""
    def patches(run: Run):
        at = run.model.model.layers[layer].self_attn
        mine = (at.o_proj, at.qkv_proj)
        carry_or_launch, launch_jobs = fused._carry_or_launch, fused._accumulate_weight_grad_jobs

        def dropping_carry(carry, jobs):
            would_carry = (carry is not None and carry.gate_up_runs and carry.attn_jobs is None and len(jobs) == 2
                           and all(getattr(p, "main_grad", None) is not None for p, _, _ in jobs))
            if would_carry and any(jobs[-1][0] is w for w in mine):
                return None
            return carry_or_launch(carry, jobs)

        items = [(fused, "_carry_or_launch", dropping_carry)]
        if run.eng.device.type != "cuda":
            def dropping_launch(jobs):
                jobs = [j for j in jobs if not any(j[0] is w for w in mine)]
                if jobs:
                    launch_jobs(jobs)
            items.append((fused, "_accumulate_weight_grad_jobs", dropping_launch))
        return items
    return patches


def fault_overwrite(param_of: Callable, pass_index: int = 2):
    """(b) On micro-batch ``pass_index`` the launch that holds ``param_of(model)`` gets ``accumulate = False`` for that
    parameter: ``_accumulate_weight_grad_jobs`` reads the flag from ``_sftamd_fresh``, which is raised just before."""
    def patches(run: Run):
        target = param_of(run.model)
        launch_jobs = fused._accumulate_weight_grad_jobs

        def overwriting(jobs):
            if run.pass_index == pass_index and any(j[0] is target for j in jobs):
                target._sftamd_fresh = True
            return launch_jobs(jobs)

        return [(fused, "_accumulate_weight_grad_jobs", overwriting)]
    return patches


def fault_scale_tile(param_of: Callable, tile: Tuple[int, int], factor: float = 0.75):
    """(c) One 256 x 256 tile of a finished main_grad scaled: a quarter of four micro-batch contributions lost there."""
    def post(run: Run):
        i, j = tile
        with torch.no_grad():
            param_of(run.model).main_grad[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE].mul_(factor)
    return post


def fault_keep_o_job():
    """(d) ``_take`` hands out an AttnLink's o_job without clearing it: the weight gradient is issued as it should be,
    but the link keeps the job (and its two activations) — only check 4 can see it."""
    def patches(run: Run):
        take = fused._take

        def keeping(link, field_name):
            if link is not None and field_name == "o_job":
                return getattr(link, field_name)
            return take(link, field_name)

        return [(fused, "_take", keeping)]
    return patches


def fault_early_norm_slots():
    """(e) ``_norm_slots`` hands out a parameter's clip-norm slots on every contribution, not only the last: the tied
    embedding's slots are filled by the lm_head launch and the embedding backward then adds rows nobody squares."""
    def patches(run: Run):
        return [(fused, "_norm_slots", lambda param: getattr(param, "_sftamd_norm_slots", None))]
    return patches


def fault_drop_and_keep_stale(layer: int):
    """(a) on every pass, with ``_zero_untouched`` switched off: the slices nobody wrote keep what was there before
    ``zero_grad`` — check 2's NaN."""
    drop = fault_drop_carried(layer)

    def patches(run: Run):
        return list(drop(run)) + [(run.eng, "_zero_untouched", lambda: None)]
    return patches
