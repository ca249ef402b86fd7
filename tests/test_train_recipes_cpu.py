"""The training-recipe harness of tests/_recipes.py on CPU tensors in fp32: the functions of ops/fused.py are
device-agnostic, so the recipe table, checks 2-4, the per-block bound machinery and the seeded faults are exercised
without a GPU (tests/test_train_recipes_gpu.py runs them on the HIP path, where the shared launches, the clip-norm slots
and the dispatch trace exist). Here the path under test IS the PyTorch path, so there is no twin: the bound of check 1
is 2 x the bf16 rounding floor of the reference, and on top of it path and reference agree to fp32 tolerance
(atol 1e-5, rtol 1e-3, as tests/test_model_cpu.py).

Tiny widths: hidden 256, 2 q / 1 kv heads x 128, intermediate 8192 (gate_up is 64 tiles tall, so that one
tile is a small share of the parameter: fault (c)), vocabulary 512, four layers (tied: one NoPE layer);
a window of three padded 2 x 32 batches and a padding-free one of 49 tokens, second."""
import types

import pytest
import torch

import _recipes as R
from _blockwise import global_rel_err
from llm_fine_tune_distributed_amd.models import tiny
from test_default_path_gpu import SMOLLM3_BOUNDS

WIDTHS = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=8192,
              vocab_size=512, num_hidden_layers=4)


@pytest.fixture(scope="module")
def world(request):
    kind = request.param
    cfg = tiny("smollm3" if kind == "tied" else "llama", **WIDTHS)
    assert cfg.tie_word_embeddings == (kind == "tied")
    window = R.make_window(cfg.vocab_size, (2, 32), [20, 7, 13, 9], "cpu")
    w = types.SimpleNamespace(kind=kind, cfg=cfg, window=window, cache={})

    def refs(policy):
        key = "lora" if policy == "lora" else "full"
        if key not in w.cache:
            w.cache[key] = R.reference_grads(cfg, R.RECIPES["lora" if key == "lora" else "ga"], window, "cpu",
                                             torch.float32)
        return w.cache[key]

    w.refs = refs
    yield w
    w.cache.clear()


CASES = [(k, n) for k in ("tied", "untied") for n in R.RECIPES]


@pytest.mark.parametrize("world,name", CASES, indirect=["world"], ids=[f"{k}-{n}" for k, n in CASES])
def test_recipe(world, name):
    recipe = R.RECIPES[name]
    run = R.run_window(R.build(world.cfg, recipe, "cpu", torch.float32), recipe, world.window)
    trainable = run.named_trainable()
    names = [n for n, _ in trainable]
    # the recipe table: which parameters train
    if recipe.policy == "full":
        assert len(names) == len(list(run.model.parameters()))
    elif recipe.policy == "lora":
        assert names and all(".lora." in n for n in names)
    else:
        head = "model.embed_tokens" if world.kind == "tied" else "lm_head"
        assert all(n == head or n.startswith(("model.layers.2.", "model.layers.3.")) for n in names), names
        assert head in names and "model.norm.weight" not in names
    assert run.model.gradient_checkpointing == recipe.ckpt and len(run.traces) == len(recipe.batches)
    ref = world.refs(recipe.policy)
    bounds = R.reference_bounds(ref, recipe.batches, None, names)  # no twin: the floor decides
    assert all(5e-4 < b < 1e-2 for b in bounds.values()), bounds  # 2 x the bf16 rounding floor of a block
    R.check_gradients(run, ref, bounds, verbose=False)
    run.raise_if_failed()  # checks 1-4
    assert run.norm is None and run.norm_done is None  # (the fused clip norm is GPU-only)
    if recipe.policy != "lora":
        assert run.links_seen > 0  # (on CPU tensors no node keeps its link: check 4 has little to look at)
    for n, p in trainable:
        want = R.reference_sum(ref, recipe.batches, n).float()
        assert torch.allclose(p.main_grad, want, atol=1e-5, rtol=1e-3), (n, (p.main_grad - want).abs().max().item())


def _gate_up(layer):
    return lambda m: m.model.layers[layer].mlp.gate_up_proj


@pytest.mark.parametrize("world", ["tied"], indirect=True)
@pytest.mark.parametrize("fault", ["a", "a_stale", "c"])
def test_seeded_faults_are_seen(world, fault):
    """(a) and (c) of tests/test_train_recipes_gpu.py (its docstring) on the ``ga`` recipe; on CPU tensors the jobs of
    (a) never pass through _carry_or_launch, so the fault drops the same two at _accumulate_weight_grad_jobs. a_stale:
    (a) with DDPEngine._zero_untouched switched off, which is what check 2 is there to see."""
    recipe = R.RECIPES["ga"]
    kw = {"a": dict(patches=R.fault_drop_carried(2)),
          "a_stale": dict(patches=R.fault_drop_and_keep_stale(2)),
          "c": dict(post=R.fault_scale_tile(_gate_up(0), (1, 0)))}[fault]
    run = R.run_window(R.build(world.cfg, recipe, "cpu", torch.float32), recipe, world.window, **kw)
    names = [n for n, _ in run.named_trainable()]
    ref = world.refs(recipe.policy)
    R.check_gradients(run, ref, R.reference_bounds(ref, recipe.batches, None, names), verbose=False)
    if fault in ("a", "a_stale"):
        hit = {"model.layers.2.self_attn.o_proj", "model.layers.2.self_attn.qkv_proj"}
        assert set(run.failed(1)) == hit, run.failures
        assert set(run.failed(3)) == hit and not run.failed(4), run.failures
        # _zero_untouched clears what nobody wrote; without it the NaN from before zero_grad is still there
        assert set(run.failed(2)) == (hit if fault == "a_stale" else set()), run.failures
    else:
        n = "model.layers.0.mlp.gate_up_proj"
        assert run.failed(1) == [n] and len(run.failures) == 1, run.failures
        assert "worst tile (1, 0)" in run.failures[0][2], run.failures
        # one tile of 64 scaled by 0.75 moves the whole-parameter norm by about 0.25 / sqrt(64) = 0.03: under the bound
        # tests/test_default_path_gpu.py holds the MLP weights to
        whole = global_rel_err(_gate_up(0)(run.model).main_grad, R.reference_sum(ref, recipe.batches, n))
        assert whole < next(b for key, b in SMOLLM3_BOUNDS if key in n), whole
    with pytest.raises(AssertionError, match="check 1"):
        run.raise_if_failed()
