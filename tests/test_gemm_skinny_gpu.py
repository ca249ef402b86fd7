"""The decode GEMM (csrc/gemm_skinny.hip, M <= 64): exact on integer operands over every tail and split, rows
independent of M, the fp32-sum bound at a real width, its routing from ops.linear, and generate_batch on it."""
import pytest
import torch

from llm_fine_tune_distributed_amd import ops
from llm_fine_tune_distributed_amd.inference.generation import generate_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"


def traced(fn):
    """fn()'s result and how often gemm_skinny was recorded in the dispatch trace meanwhile."""
    _ext.ops().dispatch_trace(True)
    try:
        out = fn()
    finally:
        _ext.ops().dispatch_trace(False)
    hits = dict(kv.split("=") for kv in _ext.ops().dispatch_trace_read().split(";") if kv)
    return out, int(hits.get("gemm_skinny", 0))


# (16400, 1088): 257 strip blocks run unsplit, one strip past a workgroup's four, 17 k-units turn the 8-slot ring twice
# plus one; (1040, 2112) splits into six slices of 5 units and one of 3, (256, 11008) into 43 of 4.
@pytest.mark.parametrize("N,K", [(16, 64), (48, 192), (1040, 2112), (256, 11008), (16400, 1088)])
@pytest.mark.parametrize("M", [1, 7, 16, 17, 48, 64])
def test_exact_on_integers(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M * 131 + N + K)
    x = torch.randint(-2, 3, (M, K), device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randint(-2, 3, (N, K), device=DEV, generator=g).to(torch.bfloat16)
    ref = (x.double() @ w.double().T).to(torch.bfloat16)
    assert torch.equal(_ext.ops().gemm_skinny(x, w), ref)


@pytest.mark.parametrize("N,K", [(1040, 2112), (256, 11008)])
def test_rows_independent_of_m(N, K):
    g = torch.Generator(device=DEV).manual_seed(N)
    buf = torch.full((80, K), float("nan"), device=DEV, dtype=torch.bfloat16)
    buf[:64] = torch.randn(64, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g).to(torch.bfloat16)
    full = _ext.ops().gemm_skinny(buf[:64], w)
    assert torch.isfinite(full.float()).all()
    for m in (1, 16, 17):
        assert torch.equal(_ext.ops().gemm_skinny(buf[:m], w), full[:m]), m


def test_gaussian_within_fp32_sum_bound():
    M, N, K = 64, 2048, 11008
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, device=DEV, generator=g).to(torch.bfloat16)
    y = _ext.ops().gemm_skinny(x, w).double()
    ref = x.double() @ w.double().T
    # one bf16 rounding of the result + the worst case of an fp32 sum of K terms in any order
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (x.double().abs() @ w.double().abs().T)
    assert bool(((y - ref).abs() <= bound).all()), float(((y - ref).abs() / bound).max())


def test_routing():
    w = torch.randn(512, 256, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(256, 256, device=DEV, dtype=torch.bfloat16)
    y, hits = traced(lambda: ops.linear(x[:16], w))
    assert hits == 1 and torch.equal(y, _ext.ops().gemm_skinny(x[:16], w))
    assert traced(lambda: ops.linear(x, w))[1] == 0
    y, hits = traced(lambda: ops.linear(x[:16, :96], w[:, :96].contiguous()))  # K = 96: the library, silently
    assert hits == 0 and y.shape == (16, 512)
    for bad_x, bad_w in [(torch.cat([x[:64], x[:1]]), w), (x[:16, :96].contiguous(), w[:, :96].contiguous()),
                         (x[:16].float(), w.float())]:
        with pytest.raises(RuntimeError):
            _ext.ops().gemm_skinny(bad_x, bad_w)


def test_generate_batch_on_the_decode_gemm():
    cfg = get_config("tiny-gpu")
    model = build_model(cfg, device=DEV, dtype=torch.bfloat16, seed=2)
    g = torch.Generator().manual_seed(1)
    # 79 prompt tokens: the prefill's layer GEMMs (M = 79) stay off the op, its LM head (3 rows) is on it
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (40, 9, 30)]
    kw = dict(max_new_tokens=8, do_sample=False)
    eager, hits = traced(lambda: generate_batch(model, prompts, use_graph=False, **kw))
    per_step = 4 * cfg.num_hidden_layers + 1  # qkv, o, gate_up, down per layer + the LM head
    assert (hits - 1) % per_step == 0 and (hits - 1) // per_step in (7, 8), hits
    graph, hits = traced(lambda: generate_batch(model, prompts, use_graph=True, **kw))
    assert hits >= 1 + per_step  # the prefill's LM head + the capture of one step
    assert graph == eager and all(len(o) == 8 for o in eager)
