"""flash_fwd / flash_bwd under a component of q and k that is common to all tokens (what a large q / k bias gives:
Qwen2 / Qwen2.5), judged against the fp64 reference with bounds of 2 x a torch emulation of the kernels' arithmetic
(tests/_attn_emul.py): per (sequence, head) block, as token-reduced products X^T dq / X^T dk (the quantity a weight or
bias gradient sums), by the exact invariant sum_j dk_j = 0 per (sequence, kv head), and once more with the exact delta
handed to flash_bwd, which tells the cost of forming delta from the bf16-rounded output from a kernel that does not
follow its own arithmetic. Lengths straddle the 64 / 128 tile edges; the head layouts take the three dK/dV and dQ
workgroup shapes (GQA 2, 2 with one kv head, 7 = Qwen2.5-7B); both dQ routes.

Measured on MI355X: profiles/attention_common_mode.md."""
import math

import pytest
import torch

import _attn_emul as ae
from _blockwise import assert_blocks_close
from llm_fine_tune_distributed_amd.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = ae.D
LENS = [1, 65, 256, 129, 61]  # M = 512
LAYOUTS = [(4, 2), (2, 1), (7, 1)]
SCALE = 1 / math.sqrt(D)
FIXED = {"out": 2e-2, "dq": 3e-2, "dk": 3e-2, "dv": 3e-2}  # the suite's bounds, on the i.i.d. inputs


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()


@pytest.fixture(scope="module")
def cm_ref():
    """Inputs, the fp64 reference and the two emulations' metrics per (layout, causal, input): computed once, shared by
    the two dQ routes, never modified."""
    cache = {}

    def get(nq, nkv, causal, noise, common, v_common):
        key = (nq, nkv, causal, noise, common, v_common)
        if key not in cache:
            seed = 100 * nq + 10 * int(causal) + ae.INPUTS_V.index((noise, common, v_common))
            qkv, dout = ae.common_mode_inputs(LENS, nq, nkv, noise, common, seed, DEV, v_common)
            cu = ae.cu_of(LENS, DEV)
            o64, g64 = ae.reference64(qkv, dout, cu, nq, nkv, SCALE, causal)
            X = ae.token_matrix(sum(LENS), DEV)
            em = {}
            for mode in ("kernel", "exact"):
                out, _, dqkv, _ = ae.emulate(qkv, dout, cu, nq, nkv, SCALE, causal, delta=mode, o64=o64)
                em[mode] = ae.bounds_from(ae.metrics(out, dqkv, o64, g64, cu, nq, nkv, X))
            cache[key] = dict(qkv=qkv, dout=dout, cu=cu, o64=o64, g64=g64, X=X, bounds=em, em_out=out)
        return cache[key]
    yield get
    cache.clear()


@pytest.mark.parametrize("ds_mb", ["", "0"])
@pytest.mark.parametrize("noise,common,v_common", ae.INPUTS_V)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("nq,nkv", LAYOUTS)
def test_attention_common_mode(nq, nkv, causal, noise, common, v_common, ds_mb, cm_ref, monkeypatch):
    monkeypatch.setenv("SFTAMD_ATTN_DS_MB", ds_mb)  # "" = materialised dS^T + dq32, "0" = the dq3 recompute path
    r = cm_ref(nq, nkv, causal, noise, common, v_common)
    qkv, dout, cu, o64, g64, X = r["qkv"], r["dout"], r["cu"], r["o64"], r["g64"], r["X"]
    ops = _ext.ops()
    what = f"common_mode {nq}/{nkv} causal={causal} noise={noise} common={common} v_common={v_common} ds_mb={ds_mb!r}"
    args = (cu, max(LENS), nq, nkv, D, SCALE, causal)
    out, lse = ops.flash_fwd(qkv, *args)
    dqkv = ops.flash_bwd(dout, qkv, out, lse, *args)
    print(f"{what}: {(out != r['em_out']).float().mean().item():.2e} of out's elements differ from the emulation's")
    # 1 - 3: blocks, token-reduced gradients, the invariant; the kernel's own delta
    got = ae.metrics(out, dqkv, o64, g64, cu, nq, nkv, X)
    bad = ae.check(got, r["bounds"]["kernel"], LENS, what + " own delta", floors=FIXED if common == 0 and v_common == 0 else None)
    # 4: the exact delta handed over, against the exact-delta emulation
    dqkv_x = ops.flash_bwd(dout, qkv, out, lse, *args, ae.exact_delta(dout, o64, nq))
    got_x = ae.metrics(out, dqkv_x, o64, g64, cu, nq, nkv, X)
    bad_x = ae.check(got_x, r["bounds"]["exact"], LENS, what + " exact delta")
    assert not bad and not bad_x, (what, bad, bad_x)
    # ... and delta = rowsum(dO . O) of the kernel's own output handed over == the run that computes it
    d_self = (dout.float() * out.float()).view(-1, nq, D).sum(-1).t().contiguous()
    dqkv_s = ops.flash_bwd(dout, qkv, out, lse, *args, d_self)
    cul = cu.tolist()
    for name, lo, hi in (("dq", 0, nq * D), ("dk", nq * D, (nq + nkv) * D), ("dv", (nq + nkv) * D, (nq + 2 * nkv) * D)):
        w = assert_blocks_close(dqkv_s[:, lo:hi], dqkv[:, lo:hi].double(), 0, D, 1e-3, f"{what} given delta {name}",
                                row_splits=cul)
        print(f"{what} given delta vs own {name}: {w:.3e} (bound 1.000e-03)")
    # the sequence of one token: out is the V row bit for bit, dq = dk = 0 to 1e-4 rms (test_attention_blocks_gpu)
    v = qkv[:, (nq + nkv) * D:].view(-1, nkv, D).repeat_interleave(nq // nkv, 1).reshape(-1, nq * D)
    rms = {"dq": g64[:, :nq * D].pow(2).mean().sqrt().item(), "dk": g64[:, nq * D:(nq + nkv) * D].pow(2).mean().sqrt().item()}
    for b, l in enumerate(LENS):
        if l != 1:
            continue
        s = cul[b]
        assert torch.equal(out[s], v[s]), (what, "length-1 sequence", b)
        for g in (dqkv, dqkv_x, dqkv_s):
            assert g[s, :nq * D].abs().max().item() <= 1e-4 * rms["dq"], (what, b, g[s, :nq * D].abs().max().item())
            assert g[s, nq * D:(nq + nkv) * D].abs().max().item() <= 1e-4 * rms["dk"], (what, b)
