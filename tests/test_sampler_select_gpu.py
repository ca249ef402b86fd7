"""The threshold sampler of csrc/sampler.hip: sample_token / sample_tokens with top_k == 0 or top_k > 64.

The kept set comes from the rule alone, in float64 on the CPU (z itself is formed in fp32, as the kernels form it):
top-k keeps z >= the k-th largest value, top-p keeps the survivors whose mass strictly above, M, is <= top_p. The draw
must then be the token sample_tokens_full draws from the same rows masked to that set, seed and step counters equal.
The rows have a head of seven tokens (two of them tied) that holds all but ~0.1 % of the mass, so every M is far from
every top_p used (asserted, 1e-3) and top_p = 0.9 cuts at the tied pair; the top-k edges fall into the random tail,
which in bf16 is full of exact ties."""
import math

import pytest
import torch

from llm_fine_tune_distributed_amd.inference.generation import DeviceSampler, generate, generate_batch
from llm_fine_tune_distributed_amd.models import build_model, get_config
from llm_fine_tune_distributed_amd.ops import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
HEAD = [0.0, -1.5, -2.0, -2.0, -2.5, -4.0, -5.5]  # mass above each: 0, .626, .765, .765, .935, .986, .997


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    yield


def make_rows(B, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g)
    for b in range(B):
        x[b, torch.randperm(V, generator=g)[:len(HEAD)]] = math.ceil(math.log(V)) + 8.0 + torch.tensor(HEAD)
    return x.to(dtype)


def kept_set(x, present, temperature, penalty, k, p, margin=1e-3):
    x = x.float()
    x = torch.where(present, torch.where(x < 0, x * penalty, x / torch.full_like(x, penalty)), x)
    z = (x * torch.tensor(1.0 / temperature, dtype=F32)).double()
    keep = z >= torch.topk(z, k).values[-1] if k > 0 else torch.ones_like(z, dtype=torch.bool)
    if p < 1.0:
        u, cnt = torch.unique(z[keep], return_counts=True)
        u, w = u.flip(0), (cnt * torch.exp(u - u.max())).flip(0)
        M = (w.cumsum(0) - w) / w.sum()  # mass strictly above each distinct value
        assert (M - p).abs().min() >= margin, "these inputs leave the nucleus edge to rounding"
        keep = keep & (z >= u[M <= p].min())
    return keep, z


def call(x, present, steps, k, p, temperature=1.0, penalty=1.0, seed=11, eos=-1, done=None, full=False):
    """One sample_tokens (or sample_tokens_full) call on fresh state; everything it can write, by name."""
    B, V = x.shape
    o = dict(state=torch.zeros(B, 4, dtype=torch.long, device=DEV), tok=torch.full((B,), -1, device=DEV),
             pos=torch.full((B,), -1, device=DEV), len=torch.full((B,), -1, dtype=torch.int32, device=DEV),
             log=torch.full((B, 8), -1, device=DEV), done=torch.tensor(done or [0] * B, dtype=torch.int32, device=DEV))
    o["state"][:, 0] = torch.tensor(steps)
    o["state"][:, 2] = 20
    w = torch.zeros(B, (V + 31) // 32 * 32, dtype=torch.bool)
    w[:, :V] = present
    o["pres"] = (w.view(B, -1, 32).long() << torch.arange(32)).sum(-1).to(torch.int32).to(DEV)
    args = (x.to(DEV), o["pres"], o["state"], o["tok"], o["pos"], o["len"], o["log"])
    if full:
        _ext.ops().sample_tokens_full(*args, torch.zeros(B, 1, device=DEV), o["done"], eos, temperature, penalty, seed)
    else:
        _ext.ops().sample_tokens(*args, o["done"], eos, temperature, k, p, penalty, True, seed)
    return {n: t.cpu() for n, t in o.items()}


KP = [(0, 0.9), (0, 1.0), (65, 1.0), (65, 0.5), (None, 0.3), (1000, 0.95)]  # None: top_k = V
CASES = [(V, V if k is None else k, p, dt, 1.0, 1.0, False) for V in (8, 2047, 2049, 5001, 131075) for k, p in KP
         for dt in (F32, BF16) if (k or 0) <= V]
CASES += [(5001, 1000, 0.95, BF16, 0.7, 1.2, False), (2049, 0, 0.9, F32, 1.0, 1.0, True)]


@pytest.mark.parametrize("V,k,p,dtype,temperature,penalty,own_steps", CASES)
def test_draw_equals_the_full_draw_over_the_kept_set(V, k, p, dtype, temperature, penalty, own_steps):
    B = 64 if V < 100000 else 8
    x = make_rows(B, V, dtype, V + k)
    present = torch.rand(B, V, generator=torch.Generator().manual_seed(1)) < (0.3 if penalty != 1.0 else 0.0)
    steps = [3 * b + 1 for b in range(B)] if own_steps else [2] * B
    masked = x.clone()
    for b in range(B):
        masked[b, ~kept_set(x[b], present[b], temperature, penalty, k, p)[0]] = -math.inf
    got = call(x, present, steps, k, p, temperature, penalty)
    want = call(masked, present, steps, 0, 1.0, temperature, penalty, full=True)
    assert got["tok"].tolist() == want["tok"].tolist()
    for n in ("state", "pos", "len", "log", "done", "pres"):
        assert torch.equal(got[n], want[n]), n


def test_distribution_over_the_nucleus():
    V, B, p, T = 5001, 8192, 0.8, 0.7
    x = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 2
    none = torch.zeros(V, dtype=torch.bool)
    keep, z = kept_set(x, none, T, 1.0, 0, p, margin=1e-5)
    q = torch.softmax(z.masked_fill(~keep, -math.inf), 0)
    tok = call(x.expand(B, V).contiguous(), none, [0] * B, 0, p, temperature=T)["tok"]
    n = torch.bincount(tok, minlength=V).double()
    assert n[~keep].sum() == 0
    assert bool(((n - B * q).abs() <= 5 * (B * q * (1 - q)).sqrt())[keep].all())


@pytest.mark.parametrize("what", ["row0", "done", "eos", "repeat", "top_k > V"])
def test_contracts(what):
    B, V, k, p = 4, 2049, 100, 0.9
    x, none = make_rows(B, V, F32, 3), torch.zeros(B, V, dtype=torch.bool)
    a = call(x, none, [5] * B, k, p)
    if what == "row0":
        st, tok = torch.tensor([5, 0, 20, 0], device=DEV), torch.full((1,), -1, device=DEV)
        _ext.ops().sample_token(x[0].to(DEV), torch.zeros((V + 31) // 32, dtype=torch.int32, device=DEV), st, tok,
                                None, None, None, 1.0, k, p, 1.0, True, 11)
        assert int(tok) == int(a["tok"][0]) and st.tolist()[:2] == a["state"][0].tolist()[:2]
    elif what == "done":
        d = call(x, none, [5] * B, k, p, done=[0, 1, 0, 0])
        assert d["tok"].tolist() == [int(a["tok"][0]), -1] + a["tok"].tolist()[2:]
        assert d["state"][1].tolist() == [5, 0, 20, 0] and not d["pres"][1].any() and (d["log"][1] == -1).all()
        assert int(d["pos"][1]) == -1 and int(d["len"][1]) == -1
    elif what == "eos":
        e = call(x, none, [5] * B, k, p, eos=int(a["tok"][2]))
        hit = a["tok"] == a["tok"][2]
        assert e["tok"].tolist() == a["tok"].tolist() and e["done"].tolist() == hit.int().tolist()
        assert e["state"][:, 2].tolist() == [20 if h else 21 for h in hit] and int(e["pos"][2]) == -1
        assert int(e["log"][2, 5]) == int(a["tok"][2])
    elif what == "repeat":
        b = call(x, none, [5] * B, k, p)
        assert all(torch.equal(a[n], b[n]) for n in a)
    else:
        with pytest.raises(RuntimeError, match="top_k"):
            call(x, none, [5] * B, V + 1, p)


def test_generation_runs_on_the_device_sampler():
    assert DeviceSampler.supported(0, True) and DeviceSampler.supported(200, True)
    cfg = get_config("tiny-gpu")
    model = build_model(cfg, device=DEV, dtype=BF16, seed=5)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (37, 5, 90)]
    kw = dict(max_new_tokens=12, top_k=0, top_p=0.9)
    out = generate_batch(model, prompts, seed=3, **kw)
    assert out == [generate(model, q, seed=3 + b, **kw) for b, q in enumerate(prompts)]
    assert out == generate_batch(model, prompts, seed=3, use_graph=False, **kw)
