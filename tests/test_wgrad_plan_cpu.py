"""The weight-gradient launch planner (ops.fused._plan_wgrad: integers in, launches out) and the executor that walks
its plan (ops.fused._accumulate_weight_grad_jobs, here on CPU tensors where every job falls back to its own launch).

The expected plans were worked out with the functions of the commit before the planner existed (_pair_ok, _multi_ok and
the recursion of its _accumulate_weight_grad_jobs, evaluated on these tile counts at each CU budget), not read off the
planner. Tile counts: SmolLM3 down 344, gate_up 688, o_proj 64, qkv 96; Llama 896, 1792, 256, 384."""
import pytest
import torch

import llm_fine_tune_distributed_amd.ops.fused as F

L = F._Launch
T = 8192
# (tiles, tokens (one T for all, or one per job), expected plan at budget 256, at budget 248)
CASES = {
    "smollm3_layer": ([344, 688, 64, 96], T, [L(0, 4, split_left=1)], [L(0, 4, split_left=1)]),
    "smollm3_mlp": ([344, 688], T, [L(0, 2, split_all=0)], [L(0, 2, split_all=0)]),  # 1032 % 256 = 8 <= 688
    "smollm3_attn": ([64, 96], T, [L(0, 2, split_all=3)], [L(0, 2, split_all=3)]),
    # 3328 tiles are whole rounds of 256; of 248 they leave 104, cheapest split 2 ways
    "llama_layer": ([896, 1792, 256, 384], T, [L(0, 4, split_left=1)], [L(0, 4, split_left=2)]),
    "llama_mlp": ([896, 1792], T, [L(0, 2, split_all=0)], [L(0, 2, split_all=0)]),
    "llama_attn": ([256, 384], T, [L(0, 2, split_all=0)], [L(0, 2, split_all=0)]),
    "three_below_budget": ([64, 96, 64], T, [L(0, 2, split_all=3), L(2, 1)], [L(0, 2, split_all=3), L(2, 1)]),
    # 304 >= budget so no whole-pair split, and the partial round (48 / 56 tiles) does not fit in the second problem
    "leftover_in_first": ([300, 4], T, [L(0, 1), L(1, 1)], [L(0, 1), L(1, 1)]),
    "one_job": ([344], T, [L(0, 1)], [L(0, 1)]),
    # the gate: the same T for every job, T % 128 == 0, T >= 1024, every job a 4-wave multi-problem job (a tile count)
    "mixed_T": ([344, 688, 64, 96], [T, T, T, 4096], [L(0, 2, split_all=0), L(2, 1), L(3, 1)],
                [L(0, 2, split_all=0), L(2, 1), L(3, 1)]),
    "mixed_T_pair": ([64, 96], [T, 4096], [L(0, 1), L(1, 1)], [L(0, 1), L(1, 1)]),
    "T_512": ([344, 688, 64, 96], 512, [L(i, 1) for i in range(4)], [L(i, 1) for i in range(4)]),
    "T_not_128": ([344, 688, 64, 96], T + 64, [L(i, 1) for i in range(4)], [L(i, 1) for i in range(4)]),
    # T = 256 is below the gate's 1024: singles, although _pair_split itself would split such a pair 2 ways (below)
    "T_256": ([64, 96], 256, [L(0, 1), L(1, 1)], [L(0, 1), L(1, 1)]),
    "job_not_eligible": ([344, None, 64, 96], T, [L(0, 1), L(1, 1), L(2, 2, split_all=3)],
                         [L(0, 1), L(1, 1), L(2, 2, split_all=3)]),
}


@pytest.fixture(params=[256, 248])
def budget(request, monkeypatch):
    monkeypatch.setattr(F, "_CU_BUDGET", request.param)
    monkeypatch.setattr(F, "_WGRAD_MODE", "auto")
    monkeypatch.setattr(F, "_WGRAD_PAIR", True)
    monkeypatch.delenv("SFTAMD_MULTI_SPLIT", raising=False)
    return request.param


def _plan(tiles, tokens):
    return F._plan_wgrad(tiles, tokens if isinstance(tokens, list) else [tokens] * len(tiles))


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan(name, budget):
    tiles, tokens, at256, at248 = CASES[name]
    assert _plan(tiles, tokens) == (at256 if budget == 256 else at248)


def test_plan_covers_every_job_once_in_order(budget):
    for tiles, tokens, _, _ in CASES.values():
        plan = _plan(tiles, tokens)
        assert [i for l in plan for i in range(l.first, l.first + l.count)] == list(range(len(tiles)))
        assert all(1 <= l.count <= 4 for l in plan)


def test_pair_split_at_256_tokens(budget):
    """At most T / 128 pieces per tile: the split a pair of 64 + 96 tiles would get at T = 256 (the planner never asks:
    case T_256)."""
    assert F._pair_split(64, 96, 256) == 2


def test_plan_forced_multi_split(budget, monkeypatch):
    monkeypatch.setenv("SFTAMD_MULTI_SPLIT", "3")
    assert _plan([344, 688, 64, 96], T) == [L(0, 4, split_left=3)]
    assert _plan([344, 688], T) == [L(0, 2, split_all=0)]  # pairs do not read it


@pytest.mark.parametrize("switch", ["pair_off", "blas", "cfg"])
def test_plan_switched_off(switch, budget, monkeypatch):
    """SFTAMD_WGRAD_PAIR=0, or SFTAMD_WGRAD naming a library / one kernel config: every job launches alone."""
    if switch == "pair_off":
        monkeypatch.setattr(F, "_WGRAD_PAIR", False)
    else:
        monkeypatch.setattr(F, "_WGRAD_MODE", "blas" if switch == "blas" else "14")
    for tiles in ([344, 688, 64, 96], [64, 96], [64, 96, 64]):
        assert _plan(tiles, T) == [L(i, 1) for i in range(len(tiles))]


def test_cpu_jobs_have_no_tile_count():
    p = torch.nn.Parameter(torch.zeros(256, 256, dtype=torch.bfloat16))
    p.main_grad = torch.zeros(256, 256, dtype=torch.bfloat16)
    x = torch.zeros(1024, 256, dtype=torch.bfloat16)
    assert F._job_tiles(p, x, x) is None


def test_executor_on_cpu_jobs():
    """Four fp32 jobs on CPU tensors (each falls back to its own launch): every main_grad = dy^T x, every ready-hook
    fires exactly once, fresh is cleared, and a second call accumulates."""
    torch.manual_seed(0)
    fired = []

    def job(n, k):
        p = torch.nn.Parameter(torch.zeros(n, k))
        p.main_grad = torch.full((n, k), 7.0)  # stale values: the first contribution overwrites them (fresh)
        p._sftamd_fresh = True
        p._sftamd_remaining = 1
        p._sftamd_ready_hook = fired.append
        return p, torch.randn(64, n), torch.randn(64, k)

    jobs = [job(8, 16), job(24, 16), job(16, 32), job(64, 16)]
    F._accumulate_weight_grad_jobs(jobs)
    for p, dy, x in jobs:
        assert torch.allclose(p.main_grad, dy.t() @ x, atol=1e-4)
        assert p._sftamd_fresh is False and p._sftamd_remaining == 0
    assert len(fired) == 4 and {id(p) for p in fired} == {id(p) for p, _, _ in jobs}
    F._accumulate_weight_grad_jobs(jobs)
    for p, dy, x in jobs:
        assert torch.allclose(p.main_grad, 2 * (dy.t() @ x), atol=1e-4)
