"""Training recipes on the HIP path: every gradient per tile, and the state the deferred weight-gradient work leaves.

tests/test_default_path_gpu.py reads gradients out of the flat buffer under one recipe (``full``, one micro-batch, no
checkpointing) and one Frobenius norm per parameter. cli/train.py trains with ``last_n_layers``, four micro-batches and
gradient checkpointing, and the code that decides on ``requires_grad``, on an open carry scope and on the first pass of
a window (AttnLink.o_job, MLPLink.down_job / attn_jobs, _plan_wgrad's accumulate flags, _norm_slots, the delta hand-off,
the use counters, zero_grad's skipped memset) runs only on GPU tensors. Here a window of four micro-batches is driven
through ``DDPEngine(m, 1, 0)`` under every recipe of tests/_recipes.py (its docstring lists the checks) on two
four-layer models at the smallest widths where every launch kind is taken at the CU budget of 256:

hidden 1024, 8 q / 2 kv heads x 128, intermediate 5120, vocabulary 2048 — 256 x 256 tiles per layer: o_proj 4 x 4 =
16, qkv 6 x 4 = 24, gate_up 40 x 4 = 160, down 4 x 20 = 80. Tied: SmolLM3 (layer 3 is the NoPE layer); untied: Llama.

Launches ``_plan_wgrad`` implies per PADDED micro-batch (2 x 1024 tokens: T % 128 == 0, T >= 1024), B = 256:
  * [down, gate_up, next o_proj, next qkv] = 80 + 160 + 16 + 24 = 280 >= B: ONE wgrad_gemm_multi of four problems with a
    partial last round of 24 tiles (``wgrad.multi4``);
  * [o_proj, qkv] alone = 40 < B: _pair_split > 1, a pair with every tile split (``wgrad.pair``);
  * [down, gate_up] alone = 240 < B: a pair with every tile split (``wgrad.pair``);
  * the lm_head / tied embedding (2048 x 1024 = 32 tiles) is a lone job: one ``wgrad.c<cfg>`` launch.
  plain / ga: layers 1..3's attention ride in MLP 0..2's launches -> multi4 == 3; layer 0's attention and layer 3's MLP
    -> pair == 2.
  ckpt: no carry scope under checkpointing -> every layer's attention and MLP on their own: pair == 8, no multi4.
  last2: layers 2, 3 train. Layer 3's attention rides in MLP 2 -> multi4 == 1; MLP 3 is a pair; layer 2's attention
    finds the frozen MLP 1 (gate_up_runs false: nothing on offer) and launches its own pair -> pair == 2.
  cli (last2 + checkpointing): pair == 4.
  lora: the base is frozen: no pair, no multi4.
  ``dgrad.c14.delta`` (o_proj's dgrad with the attention delta in its epilogue) runs once per layer whose attention
  backward runs: 4 under ``full``; under last_n_layers 4 on the tied model (its embedding trains, so the input gradient
  flows through the frozen layers too) and 2 on the untied one; and no ``attn.delta_kernel``.
The RAGGED micro-batch (1000 tokens < 1024, not a multiple of 256): every weight gradient falls to addmm_ — no
``wgrad.*`` launch at all — and no delta epilogue.
Two windows beyond the table of recipes, because real padding-free data synchronises on a ragged batch:
``ragged_sync`` ends on that batch (no launch fills a clip-norm slot: the leftover pass covers everything), and
``rings`` ends on a second ragged batch of 1088 tokens (>= 1024, 34 x 32, not a multiple of 128): nothing is shared, and
_wgrad_cfg sends each lone job to an 8-wave ring — gate_up (40 x 8 = 320 half tiles >= 160) cfg 9, down (80 tiles)
cfg 210, o_proj / qkv / lm_head (32 / 48 / 64 half tiles, an even count of 32-token steps) cfg 209: per pass
``wgrad.c9`` == 4, ``wgrad.c210`` == 4, ``wgrad.c209`` == 9, every one of them filling its slots on the last pass.
"""
import math
import types

import pytest
import torch

import _recipes as R
from _blockwise import global_rel_err
from llm_fine_tune_distributed_amd.models import tiny
from llm_fine_tune_distributed_amd.ops import _ext, fused
from test_default_path_gpu import SMOLLM3_BOUNDS

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYERS = 4
WIDTHS = dict(hidden_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128, intermediate_size=5120,
              vocab_size=2048, num_hidden_layers=LAYERS, max_position_embeddings=2048)
PADDED = (2, 1024)
RAGGED = [300, 17, 129, 66, 488]  # 1000 tokens
RAGGED_RINGS = [300, 17, 129, 66, 576]  # 1088 tokens: window[4]

# (multi4, pair) per padded micro-batch: the module docstring derives them
LAUNCHES = {"plain": (3, 2), "ga": (3, 2), "ckpt": (0, 8), "last2": (1, 2), "cli": (0, 4), "lora": (0, 0),
            "lora_ckpt": (0, 0), "ragged_sync": (3, 2), "rings": (3, 2)}


def _cfg(kind):
    cfg = tiny("smollm3" if kind == "tied" else "llama", **WIDTHS)
    if kind == "tied":
        assert cfg.tie_word_embeddings and [cfg.uses_rope(i) for i in range(LAYERS)] == [True, True, True, False]
    else:
        assert not cfg.tie_word_embeddings and all(cfg.uses_rope(i) for i in range(LAYERS))
    return cfg


def _twin_errors(cfg, recipe, window, ref):
    """Worst block error per parameter of the bf16 model on the PyTorch path, through a DDPEngine into main_grad."""
    run = R.run_window(R.build(cfg, recipe, DEV, torch.bfloat16), recipe, window, hip=False, checks=False)
    return R.grad_errors(run, ref)


@pytest.fixture(scope="module")
def world(request):
    """Per model, once: the window, the fp32 reference gradients of every micro-batch and the twin's block errors for
    every distinct sequence of micro-batches (a recipe that trains fewer parameters, or recomputes its activations,
    computes the same gradients for those it trains: it shares them)."""
    assert _ext.load(), _ext.load_error()
    kind = request.param
    cfg = _cfg(kind)
    assert fused.cu_budget() == 256
    window = R.make_window(cfg.vocab_size, PADDED, RAGGED, DEV, ragged_lens2=RAGGED_RINGS)
    w = types.SimpleNamespace(kind=kind, cfg=cfg, window=window, cache={})

    def refs(policy):
        """(reference gradients per micro-batch, {batches: twin errors}) of the parameter set ``policy`` trains."""
        key = "lora" if policy == "lora" else "full"
        if key not in w.cache:
            rec = R.RECIPES["lora" if key == "lora" else "ga"]
            ref = R.reference_grads(cfg, rec, window, DEV, torch.bfloat16)
            twins = {}
            for name in (("lora",) if key == "lora" else ("plain", "ga", "ragged_sync", "rings")):
                r = R.RECIPES[name]
                twins[r.batches] = _twin_errors(cfg, r, window, ref)
            w.cache[key] = (ref, twins)
        return w.cache[key]

    w.refs = refs
    yield w
    w.cache.clear()
    del w.refs
    torch.cuda.empty_cache()


def _bounds(world, recipe, names):
    """Check 1's bound per parameter, from the reference side alone: 2 x max(twin's worst block error, rounding floor of
    the fp32 reference). No class needed the per-class bounds of tests/test_default_path_gpu.py instead: the HIP path's
    worst block is 0.93-1.08 times the twin's everywhere (profiles/train_recipes.md)."""
    ref, twins = world.refs(recipe.policy)
    return ref, twins[recipe.batches], R.reference_bounds(ref, recipe.batches, twins[recipe.batches], names)


def _projections(layers, kind):
    names = {f"model.layers.{i}.{w}" for i in layers
             for w in ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj")}
    return names | ({"lm_head"} if kind == "untied" else set())


def _expected_norm_done(recipe, kind):
    """Check 5's set. On a padded synchronising micro-batch each trainable projection's last contribution is a 4-wave
    launch that fills its slots (pair / multi4, the untied lm_head alone); on the 1088-token one (``rings``) an 8-wave
    ring that does; on the 1000-token one (``ragged_sync``) an addmm_ that does not. The tied embedding's last
    contribution is the embedding backward, norm weights and adapters have no slots: the leftover pass."""
    if recipe.policy == "lora" or recipe.batches[-1] == 1:  # (the library route fills no slot)
        return set()
    return _projections(range(LAYERS) if recipe.policy == "full" else range(LAYERS - recipe.n_last, LAYERS), kind)


def _check_traces(run, name, kind, window):
    """Check 6 (the module docstring derives the counts)."""
    recipe = run.recipe
    multi4, pair = LAUNCHES[name]
    if recipe.policy == "full" or kind == "tied":
        deltas = LAYERS
    else:
        deltas = recipe.n_last
    if recipe.policy == "lora":
        deltas = 0  # the LoRA attention nodes take no link
    for k, (bi, tr) in enumerate(zip(recipe.batches, run.traces)):
        lone = sum(v for key, v in tr.items() if key.startswith("wgrad.c"))
        multi = {key: v for key, v in tr.items() if key.startswith("wgrad.multi")}
        if window[bi].padded:
            assert tr.get("wgrad.pair", 0) == pair, (name, k, tr)
            assert multi == ({"wgrad.multi4": multi4} if multi4 else {}), (name, k, tr)
            assert lone == (0 if recipe.policy == "lora" else 1), (name, k, tr)  # the lm_head / tied embedding
            assert tr.get("dgrad.c14.delta", 0) == deltas, (name, k, tr)
            if recipe.policy != "lora":
                assert "attn.delta_kernel" not in tr, (name, k, tr)
        elif bi == 4:  # 1088 tokens: lone launches on the 8-wave rings
            assert "wgrad.pair" not in tr and not multi, (name, k, tr)
            rings = {key: v for key, v in tr.items() if key.startswith("wgrad.c")}
            assert rings == {"wgrad.c9": LAYERS, "wgrad.c210": LAYERS, "wgrad.c209": 2 * LAYERS + 1}, (name, k, tr)
            assert "dgrad.c14.delta" not in tr, (name, k, tr)
        else:
            assert "wgrad.pair" not in tr and not multi and lone == 0, (name, k, tr)
            assert "dgrad.c14.delta" not in tr, (name, k, tr)
        if not window[bi].padded and recipe.policy != "lora":  # M % 256 != 0: the attention node's own delta kernel
            assert tr.get("attn.delta_kernel", 0) == deltas, (name, k, tr)


def _print_table(tag, hip, twin, bounds):
    print(f"\n[{tag}] worst 256 x 256 block per parameter class: HIP path | PyTorch-path twin | smallest bound | "
          "smallest bound / error of one parameter")
    hc, tc = R.by_class(hip, bounds), R.by_class(twin)
    for cls in hc:
        room = min(bounds[n] / max(hip[n], 1e-300) for n in hip if R.param_class(n) == cls)
        print(f"  {cls:36s} {hc[cls][0]:.3e} | {tc[cls][0]:.3e} | {hc[cls][1]:.3e} | {room:.2f}")


CASES = [(k, n) for k in ("tied", "untied") for n in ("plain", "ga", "ckpt", "last2", "cli")] + \
        [("tied", "lora"), ("tied", "lora_ckpt")] + \
        [(k, n) for k in ("tied", "untied") for n in ("ragged_sync", "rings")]


@pytest.mark.parametrize("world,name", CASES, indirect=["world"], ids=[f"{k}-{n}" for k, n in CASES])
def test_recipe(world, name):
    recipe = R.RECIPES[name]
    run = R.run_window(R.build(world.cfg, recipe, DEV, torch.bfloat16), recipe, world.window)
    names = [n for n, _ in run.named_trainable()]
    ref, twin, bounds = _bounds(world, recipe, names)
    errs = R.check_gradients(run, ref, bounds, verbose=False)  # check 1
    _print_table(f"{world.kind} {name}", errs, {n: twin[n] for n in names}, bounds)
    for k, tr in zip(recipe.batches, run.traces):
        keep = {key: v for key, v in tr.items() if key.startswith(("wgrad.", "dgrad.c14", "attn.delta"))}
        print(f"  trace, micro-batch {k}: {keep}")
    print(f"  clip norm^2: fused {run.norm[0]:.6e}, buffer {run.norm[1]:.6e}; links recorded: {run.links_seen}")
    run.raise_if_failed()  # checks 1-5
    assert all(math.isfinite(v) for v in run.losses), run.losses
    if recipe.policy != "lora":  # (the recording subclasses were the ones the model made, and check 4 saw them alive)
        live = LAYERS if recipe.policy == "full" else recipe.n_last  # (a frozen layer may make no node to hold a link)
        assert run.links_seen > 0 and run.links_checked >= 2 * live * len(recipe.batches)
    assert run.norm_done == _expected_norm_done(recipe, world.kind), sorted(run.norm_done)  # check 5
    _check_traces(run, name, world.kind, world.window)  # check 6


_BACKWARD_KERNELS = ("wgrad.", "dgrad.", "attn.dkdv", "attn.dq", "attn.bwd", "attn.delta")


def _backward_trace(tr):
    return {k: v for k, v in tr.items() if k.startswith(_BACKWARD_KERNELS)}


@pytest.mark.parametrize("world", ["tied", "untied"], indirect=True)
def test_checkpointing_changes_no_bit(world):
    """Check 7. With the carry scope off (``_WGRAD_CARRY``: what checkpointing closes), ``ga`` and ``ckpt`` launch the
    same backward kernels on the same inputs — recomputed activations are bit-equal to the saved ones — so the flat
    gradient buffer is equal bit for bit; two runs of ``ga`` itself are, first (the project holds its reductions
    deterministic). The traces are compared on the backward kernels: the recomputation adds forward launches."""
    def once(name):
        recipe = R.RECIPES[name]
        run = R.run_window(R.build(world.cfg, recipe, DEV, torch.bfloat16), recipe, world.window,
                           patches=lambda run: [(fused, "_WGRAD_CARRY", False)])
        run.raise_if_failed()
        return run

    a, b, c = once("ga"), once("ga"), once("ckpt")
    assert [_backward_trace(t) for t in a.traces] == [_backward_trace(t) for t in b.traces]
    assert torch.equal(a.eng.grad_flat, b.eng.grad_flat), "two runs of ga differ: a reduction is not deterministic"
    assert all("wgrad.multi4" not in t for t in a.traces), a.traces
    assert [_backward_trace(t) for t in a.traces] == [_backward_trace(t) for t in c.traces]
    assert a.losses == c.losses
    assert torch.equal(a.eng.grad_flat, c.eng.grad_flat)


def _gate_up(layer):
    return lambda m: m.model.layers[layer].mlp.gate_up_proj


@pytest.mark.parametrize("world", ["tied"], indirect=True)
@pytest.mark.parametrize("fault", ["a", "b", "c", "d", "e"])
def test_seeded_faults_are_seen(world, fault):
    """The checks can fail: three faults seeded in Python (no kernel changes) into the ``ga`` recipe on the tied model.
    (a) layer 2's qkv node drops the o_proj + qkv jobs it would carry: check 1 fails on exactly those two, check 3
        (counters, hooks) on them too;
    (b) micro-batch 2 overwrites instead of accumulating layer 1's gate_up in its four-problem launch: check 1 fails on
        that parameter only, nothing else notices;
    (c) one tile of layer 0's gate_up scaled by 0.75 after the window: check 1 names the tile, while the whole-parameter
        norm stays under the bound of tests/test_default_path_gpu.py — the reason this file exists.
    Two more, for the checks that (a)-(c) leave untried:
    (d) an AttnLink keeps its o_job after handing it out: gradients are right, only check 4 fails;
    (e) the clip-norm slots are handed out before a parameter's last contribution: the tied embedding is marked done by
        the lm_head launch, and check 5 fails on the norm (the set of marked parameters is wrong too)."""
    recipe = R.RECIPES["ga"]
    kw = {"a": dict(patches=R.fault_drop_carried(2)),
          "b": dict(patches=R.fault_overwrite(_gate_up(1), 2)),
          "c": dict(post=R.fault_scale_tile(_gate_up(0), (1, 2))),
          "d": dict(patches=R.fault_keep_o_job()),
          "e": dict(patches=R.fault_early_norm_slots())}[fault]
    run = R.run_window(R.build(world.cfg, recipe, DEV, torch.bfloat16), recipe, world.window, **kw)
    names = [n for n, _ in run.named_trainable()]
    ref, _, bounds = _bounds(world, recipe, names)
    before = len(run.failures)
    R.check_gradients(run, ref, bounds, verbose=False)
    print([f for f in run.failures[before:]])
    if fault == "a":
        hit = {"model.layers.2.self_attn.o_proj", "model.layers.2.self_attn.qkv_proj"}
        assert set(run.failed(1)) == hit, run.failures
        assert set(run.failed(3)) == hit and not run.failed(4), run.failures
    elif fault == "b":
        assert run.failed(1) == ["model.layers.1.mlp.gate_up_proj"], run.failures
        assert len(run.failures) == 1, run.failures
    elif fault == "d":
        assert set(run.failed(4)) == {"AttnLink.o_job"} and len(run.failed(4)) == len(run.failures), run.failures
    elif fault == "e":
        assert run.failed(5) == ["grad_norm_sq"] and len(run.failures) == 1, run.failures
        assert run.norm_done == _expected_norm_done(recipe, world.kind) | {"model.embed_tokens"}, run.norm_done
    else:
        n = "model.layers.0.mlp.gate_up_proj"
        assert run.failed(1) == [n] and len(run.failures) == 1, run.failures
        assert "worst tile (1, 2)" in run.failures[0][2], run.failures
        whole = global_rel_err(_gate_up(0)(run.model).main_grad, R.reference_sum(ref, recipe.batches, n))
        lim = next(b for key, b in SMOLLM3_BOUNDS if key in n)
        print(f"whole-parameter error {whole:.3e} < {lim:.3e}")
        assert whole < lim, (whole, lim)
    with pytest.raises(AssertionError, match={"d": "check 4", "e": "check 5"}.get(fault, "check 1")):
        run.raise_if_failed()
