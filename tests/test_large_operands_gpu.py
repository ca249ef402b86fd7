"""Operands past 2^31 elements / 2^32 bytes: the [tokens, vocabulary] logits of a long batch and the flat optimizer
buffers of a 3B model, the two tensors of a real step that are orders of magnitude larger than anything else the suite
builds.

GEMMs. ``G`` is [17408, 128256] bf16 (4.47 GB) of small integers; sub-cases take the contiguous prefix ``G[:T]`` with
T = 16640 (4.268e9 bytes: the last T % 128 == 0 below 2^32), 16768 (the first past it) and 17408 (17 x 1024). Every
partial sum is an integer below 2^24 (entries in [-2, 2] x [-3, 3], reductions of at most 128256), so the one right
answer is bf16(exact), compared with torch.equal (tests/_blockwise.py); references are accumulated in fp32 over row
chunks, which is exact here, and nothing the size of ``G`` is ever widened whole.

The 4-wave ring (csrc/gemm_4w.hip, cfg 14 and its split forms) keeps its progress along the reduction in 32-bit byte
offsets. Before its launchers checked, T >= 16768 at a row pitch of 128256 returned wrong sums without a fault
(profiles/large_operands.md); now they raise, the routing (ops/fused.py) sends such operands to the pointer-advancing
8-wave rings, and every accepted call is exact.

Cross-entropy runs in place over random logits of the same shape; AdamW, sumsq and sumsq_chunks over 2^31 + 2^20 + 5
elements, so that whole vectors, the vector tail and the scalar tail all lie past element 2^31 (and, for fp32 state,
past byte 2^32 from element 2^30 on)."""
import time

import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import fused

from _blockwise import assert_exact, exact, int_operand, traced
import test_cross_entropy_edges_gpu as ce_edges
import test_optim_edges_gpu as optim_edges
from test_optim_edges_gpu import sumsq_bound  # noqa: F401  (the fixture: that file's bound, from its own buffers)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
V = 128256
T_MAX = 17408
T_UNDER, T_FIRST = 16640, 16768   # 16640 x 128256 x 2 = 4,268,359,680 < 2^32 <= 16768 x 128256 x 2 = 4,301,193,216
TS = (T_UNDER, T_FIRST, T_MAX)
ROWS = 1088                       # row chunk of every reference: 16 chunks of T_MAX, an fp32 image of 558 MB
G4_ERROR = "32-bit addressing"


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()
    total = torch.cuda.get_device_properties(0).total_memory
    if total < 64 * 2 ** 30:
        pytest.skip(f"needs a device with 64 GB (this one has {total / 2 ** 30:.0f} GB)")
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.empty_cache()
    print(f"\n[large] peak memory allocated by the file: {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


@pytest.fixture(autouse=True)
def _timed(request):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[large] {request.node.name}: {time.perf_counter() - t0:.2f} s")


def _chunks(T, rows=ROWS):
    return [(s, min(s + rows, T)) for s in range(0, T, rows)]


# ----------------------------------------------------------------------------- AdamW and the norms past 2^31 elements
N_BIG = 2 ** 31 + 2 ** 20 + 5      # whole vectors, the vector tail and the 5-element scalar tail all past 2^31
CHUNK = 2 ** 24
SR_OFFSET = 2 ** 32 - 2 ** 30      # even; the hashed index crosses 2^32 inside the buffer
REF_CHUNKS = (0, 63, 64, 127, 128)  # chunks also compared with ops/reference.py: ends, element 2^30, element 2^31


def _opt_chunks():
    return [(c, s, min(CHUNK, N_BIG - s)) for c, s in enumerate(range(0, N_BIG, CHUNK))]


def _chunk_state(base, c, n):
    """The state of chunk c before the step: the base chunk rotated by a per-chunk prime multiple, so that equal
    positions of different chunks hold different values (a read displaced by a multiple of 2^24, 2^31 or 2^32 elements
    would otherwise find the value it expected)."""
    return [None if t is None else torch.roll(t, 9973 * c + 1)[:n].clone() for t in base]


@pytest.mark.parametrize("variant,moments", [("sr", BF16), ("rne", torch.float32), ("master", torch.float32)])
def test_adamw_past_2_pow_31_elements(variant, moments):
    """One adamw_flat call over 2^31 + 2^20 + 5 elements against the same kernel on each 2^24-element chunk alone (even
    starts, sr_offset advanced by the chunk's start: the stochastic rounding hashes the global index), bit for bit and
    over the whole buffer: an element past a 32-bit boundary that is skipped, updated twice, read from elsewhere or
    rounded with another index's hash differs. The chunk size is the one tests/test_optim_edges_gpu.py checks against
    ops/reference.py (which differs from the kernel in the last bit of some fp32 results, so it cannot be compared bit
    for bit: that file's docstring); five of the chunks here are also held to that file's rules against it."""
    sr_seed = 777 if variant == "sr" else 0
    base = optim_edges._state(CHUNK, moments, variant == "master", 7700)   # p, grad, master, m, v
    whole = [None if t is None else torch.empty(N_BIG, dtype=t.dtype, device=DEV) for t in base]
    for c, s, n in _opt_chunks():
        for dst, src in zip(whole, _chunk_state(base, c, n)):
            if dst is not None:
                dst[s:s + n] = src
    optim_edges._kernel_step(*whole, sr_seed, SR_OFFSET)
    names = ("p", "grad", "master", "m", "v")
    for c, s, n in _opt_chunks():
        before = _chunk_state(base, c, n)
        alone = [None if t is None else t.clone() for t in before]
        optim_edges._kernel_step(*alone, sr_seed, SR_OFFSET + s)
        for name, a, b in zip(names, whole, alone):
            if a is not None:
                got = a[s:s + n]
                assert torch.equal(got, b), (variant, name, "chunk", c, int((got != b).sum()),
                                             s + int((got != b).nonzero()[0]))
        if c in REF_CHUNKS:
            after = [None if t is None else t[s:s + n] for t in whole]
            figs = optim_edges.check_against_reference(before, after, moments, sr_seed, SR_OFFSET + s)
            print(f"[large] adamw {variant} chunk {c} (start {s}) vs ops/reference.py: {figs}")
    assert torch.equal(whole[1][:CHUNK], _chunk_state(base, 0, CHUNK)[1])  # the gradient is only read


@pytest.fixture(scope="module")
def big_grad():
    g = torch.Generator(device=DEV).manual_seed(7800)
    x = torch.empty(N_BIG, dtype=BF16, device=DEV)
    for _, s, n in _opt_chunks():
        x[s:s + n] = torch.randn(n, device=DEV, generator=g).to(BF16)
    yield x
    del x
    torch.cuda.empty_cache()


def _sumsq64(x, s, n):
    return sum(x[a:min(a + CHUNK, s + n)].double().pow(2).sum().item() for a in range(s, s + n, CHUNK))


def test_sumsq_past_2_pow_31_elements(big_grad, sumsq_bound):
    got, want = _ext.ops().sumsq(big_grad).double().sum().item(), _sumsq64(big_grad, 0, N_BIG)
    err = abs(got - want) / want
    print(f"[large] sumsq n={N_BIG}: error {err:.3e} bound {sumsq_bound(N_BIG):.3e}")
    assert err <= sumsq_bound(N_BIG)


def test_sumsq_chunks_around_element_2_pow_31(big_grad, sumsq_bound):
    """Chunks that end before element 2^31, lie across it (aligned and misaligned starts), start at it and after it;
    the last one ends at the buffer's last element."""
    B31 = 2 ** 31
    chunks = [(B31 - 5003, 5000), (B31 - 4096, 8192), (B31 - 1001, 2 ** 20), (B31 - 3, 5), (B31, 4096 + 5),
              (B31 + 7, 1000), (B31 + 2 ** 19, 2 ** 18 + 2 ** 17 + 1), (N_BIG - 1, 1),
              (N_BIG - 2 ** 20 - 3, 2 ** 20 + 3), (0, 2 ** 20 + 5)]
    assert all(0 <= s and s + n <= N_BIG for s, n in chunks)  # the kernel trusts its chunk table
    assert chunks[-2][0] + chunks[-2][1] == N_BIG and any(s % 8 for s, _ in chunks)
    part = _ext.ops().sumsq_chunks(big_grad, torch.tensor(chunks, dtype=torch.int64, device=DEV))
    assert part.shape == (len(chunks),)
    for i, (s, n) in enumerate(chunks):
        got, want = part[i].double().item(), _sumsq64(big_grad, s, n)
        err = abs(got - want) / want
        print(f"[large] sumsq_chunks start 2^31{s - B31:+d} length {n}: error {err:.3e} bound {sumsq_bound(n):.3e}")
        assert err <= sumsq_bound(n), (i, s, n, err, sumsq_bound(n))


# ------------------------------------------------------------------------------------------- the big GEMM operand
@pytest.fixture(scope="module")
def G():
    """[17408, 128256] bf16 integers in [-2, 2], drawn on the device in row chunks (int_operand draws int32 first)."""
    g = torch.empty(T_MAX, V, dtype=BF16, device=DEV)
    for i, (s, e) in enumerate(_chunks(T_MAX)):
        g[s:e] = int_operand((e - s, V), -2, 2, 7000 + i, DEV)
    yield g
    del g
    torch.cuda.empty_cache()


def _prefix_products(dy, x):
    """{T: dy[:T]^T x[:T] in fp32} for the three T, accumulated over row chunks (exact on these integers)."""
    acc = torch.zeros(dy.shape[1], x.shape[1], dtype=torch.float32, device=DEV)
    out, cuts = {}, [0, *TS]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for s, e in _chunks(hi - lo):
            acc.addmm_(dy[lo + s:lo + e].float().t(), x[lo + s:lo + e].float())
        out[hi] = acc.clone()
    return out


def _want(prod, base, accumulate):
    return exact(prod + base.float() if accumulate else prod)


# ------------------------------------------------------------------------------------ wgrad, dy = G[:T]: direct routes
@pytest.fixture(scope="module")
def dy_side(G):
    """x [17408, 512] (cfg 10 needs 512 tiles: 501 x 2) and its first 256 columns apart, a base to accumulate into, and
    the exact products for the three T."""
    x512 = int_operand((T_MAX, 512), -3, 3, 7100, DEV)
    base = int_operand((V, 512), -8, 8, 7101, DEV)
    box = dict(x={512: x512, 256: x512[:, :256].contiguous()}, base=base, prod=_prefix_products(G, x512))
    yield box
    box.clear()
    torch.cuda.empty_cache()


def _run_wgrad(cfg, dy, x, base, prod, accumulate, what):
    """One wgrad_gemm call. The 4-wave cfgs refuse an operand of 2^32 bytes or more before launching anything (``out``
    is untouched); every accepted call is exact."""
    T = dy.shape[0]
    out = base.clone()
    over = T * max(dy.stride(0), x.stride(0)) * 2 >= 2 ** 32
    if cfg % 100 == 14 and over:
        with pytest.raises(RuntimeError, match=G4_ERROR):
            _ext.ops().wgrad_gemm(out, dy, x, accumulate, cfg)
        torch.cuda.synchronize()
        assert_exact(out, base, ("refused: out untouched",) + what)
        return
    with traced() as tr:
        _ext.ops().wgrad_gemm(out, dy, x, accumulate, cfg)
    assert f"wgrad.c{cfg}" in tr, tr
    assert_exact(out, _want(prod, base, accumulate), what)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("cfg", [14, 1214, 214, 10, 9])
@pytest.mark.parametrize("T", TS)
def test_wgrad_dy_side(T, cfg, accumulate, G, dy_side):
    """dW [128256, K] = G[:T]^T x: cfg 14 (501 whole tiles), 1214 (one whole round and 245 hybrid-split tiles), 214
    (every tile split in two) and the pointer-advancing 8-wave rings 10 (K = 512) and 9."""
    K = 512 if cfg == 10 else 256
    _run_wgrad(cfg, G[:T], dy_side["x"][K][:T], dy_side["base"][:, :K].contiguous(),
               dy_side["prod"][T][:, :K].contiguous(), accumulate, (cfg, T, accumulate))


def test_wgrad_only_the_last_token_block_counts(G, dy_side):
    """T = 17408, cfg 10, every row of dy zero except the last 128: out must be dy[-128:]^T x[-128:]. A kernel that
    re-reads early rows in place of the late ones returns zero (or the wrong rows' product) here."""
    dy = torch.zeros_like(G)
    dy[-128:] = G[-128:]
    x = dy_side["x"][512]
    out = torch.empty(V, 512, dtype=BF16, device=DEV)
    with traced() as tr:
        _ext.ops().wgrad_gemm(out, dy, x, False, 10)
    assert "wgrad.c10" in tr, tr
    assert_exact(out, exact(G[-128:].float().t() @ x[-128:].float()), "last 128 tokens")


# ----------------------------------------------------------------------------- wgrad, x = a column slice of G[:T]
@pytest.fixture(scope="module")
def x_side(G):
    """A narrow contiguous dy [17408, 256] against x = G[:, 256:512] read in place: row pitch 128256, the padded-pitch
    path of cfg 14. Two more narrow jobs for the planner test."""
    dy = int_operand((T_MAX, 256), -3, 3, 7200, DEV)
    x = G[:, 256:512]
    base = int_operand((256, 256), -8, 8, 7201, DEV)
    dy1 = int_operand((T_MAX, 256), -2, 2, 7202, DEV)
    x1 = int_operand((T_MAX, 256), -3, 3, 7203, DEV)
    box = dict(dy=dy, x=x, base=base, prod=_prefix_products(dy, x), dy1=dy1, x1=x1, prod1=_prefix_products(dy1, x1))
    yield box
    box.clear()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("cfg", [14, 1214, 214])
@pytest.mark.parametrize("T", TS)
def test_wgrad_x_side(T, cfg, accumulate, x_side):
    """The guard looks at both operands' pitches: dy spans 8.9 MB here, x 4.3 GB."""
    x = x_side["x"][:T]
    assert x.stride(0) == V and not x.is_contiguous()
    _run_wgrad(cfg, x_side["dy"][:T], x, x_side["base"], x_side["prod"][T], accumulate, ("x side", cfg, T, accumulate))


def _param(base, fresh):
    p = torch.nn.Parameter(torch.empty(0, device=DEV, dtype=BF16), requires_grad=False)
    p.main_grad = base.clone()
    p._sftamd_fresh = fresh
    return p


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("T", TS)
def test_wgrad_router_x_side(T, accumulate, x_side):
    """fused._wgrad_mm with the strided x: the 4-wave ring (one tile split 8 ways) while T x 128256 x 2 < 2^32, not past
    it; exact either way."""
    out = x_side["base"].clone()
    with traced() as tr:
        fused._wgrad_mm(out, x_side["dy"][:T], x_side["x"][:T], accumulate)
    four_wave = [k for k in tr if k.startswith("wgrad.c") and k[7:].isdigit() and int(k[7:]) % 100 == 14]
    assert four_wave == (["wgrad.c814"] if T == T_UNDER else []), tr
    assert_exact(out, _want(x_side["prod"][T], x_side["base"], accumulate), ("router, x side", T, accumulate))


@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("T", [T_UNDER, T_MAX])
def test_wgrad_planner_issues_an_oversized_job_alone(T, fresh, x_side):
    """Two one-tile jobs share a launch (wgrad_gemm_pair, every tile split) while both fit the 4-wave ring; the job
    whose x spans 2^32 bytes has no tile count (fused._job_tiles) and is issued alone, and both stay exact."""
    b = x_side
    p0, p1 = _param(b["base"], fresh), _param(b["base"], fresh)
    jobs = [(p0, b["dy"][:T], b["x"][:T]), (p1, b["dy1"][:T], b["x1"][:T])]
    assert (fused._job_tiles(*jobs[0]) is None) == (T == T_MAX) and fused._job_tiles(*jobs[1]) == 1
    with traced() as tr:
        fused._accumulate_weight_grad_jobs(jobs)
    assert ("wgrad.pair" in tr) == (T == T_UNDER), tr
    assert T == T_UNDER or "wgrad.c814" in tr, tr  # job 1 alone: its own 4-wave launch
    assert_exact(p0.main_grad, _want(b["prod"][T], b["base"], not fresh), ("job 0", T, fresh))
    assert_exact(p1.main_grad, _want(b["prod1"][T], b["base"], not fresh), ("job 1", T, fresh))
    assert p0._sftamd_fresh is False and p1._sftamd_fresh is False


def test_wgrad_multi_refuses_an_oversized_job(x_side):
    """The multi-problem launchers themselves (not only the planner above) refuse: pair and multi, either operand."""
    b, T = x_side, T_MAX
    outs = [b["base"].clone(), b["base"].clone()]
    empty = torch.empty(0, device=DEV)
    with pytest.raises(RuntimeError, match=G4_ERROR):
        _ext.ops().wgrad_gemm_pair(outs[0], b["dy1"][:T], b["x1"][:T], False, None, outs[1], b["dy"][:T], b["x"][:T],
                                   False, None, 2)
    with pytest.raises(RuntimeError, match=G4_ERROR):
        _ext.ops().wgrad_gemm_multi(outs, [b["dy"][:T], b["dy1"][:T]], [b["x"][:T], b["x1"][:T]], [0, 0],
                                    [empty, empty], 2, 0)
    torch.cuda.synchronize()
    for o in outs:
        assert_exact(o, b["base"], "refused: out untouched")


# ----------------------------------------------------------------------------------- wgrad, the router at the lm_head
@pytest.fixture(scope="module")
def lm_head(G):
    """N = 128256, K = 2048 (SmolLM3's lm_head): x, a base, the exact products for T = 16640 and 17408."""
    x = int_operand((T_MAX, 2048), -3, 3, 7300, DEV)
    base = int_operand((V, 2048), -8, 8, 7301, DEV)
    prod = _prefix_products(G, x)
    del prod[T_FIRST]
    box = dict(x=x, base=base, prod=prod)
    yield box
    box.clear()
    torch.cuda.empty_cache()


def _lm_head_route(tr, T):
    """16640 tokens: still the 4-wave hybrid (4008 tiles). 17408: the 8-wave 256 x 256 ring, and no 4-wave route."""
    assert ("wgrad.c1214" in tr) == (T == T_UNDER) and ("wgrad.c10" in tr) == (T == T_MAX), tr


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("T", [T_UNDER, T_MAX])
def test_wgrad_router_lm_head(T, accumulate, G, lm_head):
    assert fused._wgrad_cfg(T, V, 2048) == (1214 if T == T_UNDER else 10)
    out = lm_head["base"].clone()
    with traced() as tr:
        fused._wgrad_mm(out, G[:T], lm_head["x"][:T], accumulate)
    _lm_head_route(tr, T)
    assert_exact(out, _want(lm_head["prod"][T], lm_head["base"], accumulate), ("_wgrad_mm", T, accumulate))


@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("T", [T_UNDER, T_MAX])
def test_accumulate_weight_grad_lm_head(T, fresh, G, lm_head):
    p = _param(lm_head["base"], fresh)
    with traced() as tr:
        assert fused._accumulate_weight_grad(p, G[:T], lm_head["x"][:T]) is None
    _lm_head_route(tr, T)
    assert_exact(p.main_grad, _want(lm_head["prod"][T], lm_head["base"], not fresh), ("main_grad", T, fresh))


# ------------------------------------------------------------------------------------------------ dgrad with dy = G
@pytest.fixture(scope="module")
def dgrad_case(G):
    """w [128256, 256] and the exact dX = G w [17408, 256] (a reduction of 128256: sums up to 7.7e5)."""
    w = int_operand((V, 256), -3, 3, 7400, DEV)
    want = torch.cat([exact(G[s:e].float() @ w.float()) for s, e in _chunks(T_MAX)])
    yield w, want
    del w, want


@pytest.mark.parametrize("cfg", [14, 5, 7, "dgrad_mm"])
def test_dgrad_vocabulary_long(cfg, G, dgrad_case):
    """dX = G w with the 4.47 GB operand on the ROW side: cfg 14 (68 tiles split over the reduction), the 8-wave rings
    5 and 7, and fused.dgrad_mm, which picks 14 for a vocabulary-long reduction. Compared per chunk of output rows."""
    w, want = dgrad_case
    with traced() as tr:
        out = fused.dgrad_mm(G, w) if cfg == "dgrad_mm" else _ext.ops().dgrad_gemm(G, w, None, cfg)
    route = 14 if cfg == "dgrad_mm" else cfg
    assert f"dgrad.c{route}" in tr and ("dgrad.splitk" in tr) == (route == 14), tr
    for s, e in _chunks(T_MAX):
        assert_exact(out[s:e], want[s:e], (cfg, "rows", s, e))


def test_dgrad_refuses_a_weight_past_2_pow_32_bytes(G):
    """The 4-wave dgrad walks its TR operand, the weight [K, N], K x pitch x 2 bytes deep: G itself as the weight."""
    dy = int_operand((256, T_MAX), -2, 2, 7410, DEV)
    with pytest.raises(RuntimeError, match=G4_ERROR):
        _ext.ops().dgrad_gemm(dy, G, None, 14)
    assert fused._dgrad_cfg(dy, N=V, ld_w=G.stride(0)) != 14


# ------------------------------------------------------------------------------------ forward with a [T, V] output
@pytest.mark.parametrize("cfg,K", [(5, 128), (11, 128), (60, 256), (61, 256), ("fwd_gemm", 256)])
def test_forward_vocabulary_wide_output(cfg, K):
    """y [17408, 128256] = x w^T: 4.47 GB of output, every row chunk bit-exact."""
    x = int_operand((T_MAX, K), -2, 2, 7500 + K, DEV)
    w = int_operand((V, K), -3, 3, 7501 + K, DEV)
    with traced() as tr:
        out = fused.fwd_gemm(x, w) if cfg == "fwd_gemm" else _ext.ops().gemm_tn(x, w, cfg)
    assert f"tn.c{60 if cfg == 'fwd_gemm' else cfg}" in tr, tr
    assert out.shape == (T_MAX, V)
    wt = w.float().t().contiguous()
    for s, e in _chunks(T_MAX):
        assert_exact(out[s:e], exact(x[s:e].float() @ wt), (cfg, "rows", s, e))
    del out
    torch.cuda.empty_cache()


def test_forward_refuses_a_weight_past_2_pow_32_bytes(G):
    """cfg 60 / 61 address the whole weight from one descriptor in 32-bit bytes (csrc/gemm_tn.hip Stager5): G itself as
    a [17408, 128256] weight is refused before anything is launched."""
    x = int_operand((256, V), -3, 3, 7510, DEV)
    for cfg in (60, 61):
        with pytest.raises(RuntimeError, match=G4_ERROR):
            _ext.ops().gemm_tn(x, G, cfg)


# ------------------------------------------------------------------------- cross-entropy in place over [17408, 128256]
ROW_2_31, ROW_2_32 = 2 ** 31 // (2 * V), 2 ** 32 // (2 * V)   # rows 8371 and 16743 hold bytes 2^31 and 2^32
WINDOWS = [(0, 64), (ROW_2_31 - 31, ROW_2_31 + 33), (ROW_2_32 - 31, ROW_2_32 + 33), (T_MAX - 64, T_MAX)]


def _bits_sum(t):
    return sum(int(t[s:e].view(torch.int16).sum(dtype=torch.int64)) for s, e in _chunks(t.shape[0]))


@pytest.fixture(scope="module")
def ce_run():
    """Random bf16 logits at the scale of tests/test_cross_entropy_edges_gpu.py, one row in ten ignored, class 0, class
    V - 1 and -100 planted in every checked window. ce_fwd without the gradient, then with it (in place: the buffer
    then holds the gradient); the rows of the windows are kept aside as they went in."""
    assert ROW_2_31 * 2 * V < 2 ** 31 < (ROW_2_31 + 1) * 2 * V and ROW_2_32 * 2 * V < 2 ** 32 < (ROW_2_32 + 1) * 2 * V
    g = torch.Generator(device=DEV).manual_seed(7600)
    L = torch.empty(T_MAX, V, dtype=BF16, device=DEV)
    for s, e in _chunks(T_MAX):
        L[s:e] = (3 * torch.randn(e - s, V, device=DEV, generator=g)).to(BF16)
    labels = torch.randint(0, V, (T_MAX,), device=DEV, generator=g)
    labels[torch.rand(T_MAX, device=DEV, generator=g) < 0.1] = -100
    for lo, hi in WINDOWS:
        labels[lo], labels[lo + 1], labels[lo + 2] = 0, V - 1, -100
        labels[hi - 1], labels[hi - 2], labels[hi - 3] = 0, V - 1, -100
    # the whole objective in fp32, chunk by chunk: per-row losses (0 on ignored rows)
    rows32 = torch.cat([torch.nn.functional.cross_entropy(L[s:e].float(), labels[s:e], ignore_index=-100,
                                                          reduction="none") for s, e in _chunks(T_MAX)])
    kept = {w: L[w[0]:w[1]].clone() for w in WINDOWS}
    inv = torch.tensor([ce_edges.SCALE], device=DEV)
    before = _bits_sum(L)
    stats_off = _ext.ops().ce_fwd(L, labels, inv, False)
    torch.cuda.synchronize()
    untouched = _bits_sum(L) == before and all(torch.equal(L[lo:hi], k) for (lo, hi), k in kept.items())
    stats_on = _ext.ops().ce_fwd(L, labels, inv, True)
    torch.cuda.synchronize()
    box = dict(grad=L, labels=labels, rows32=rows32, kept=kept, untouched=untouched,
               stats={False: stats_off, True: stats_on})
    yield box
    box.clear()
    del L
    torch.cuda.empty_cache()


@pytest.mark.parametrize("write_grad", [False, True])
def test_ce_rows_at_the_ends_and_at_both_boundaries(write_grad, ce_run):
    """Loss, lse, entropy, correct and the gradient of the first and last 64 rows and of 64 rows around the rows that
    hold byte 2^31 and byte 2^32, each row against fp64 under the bounds of tests/test_cross_entropy_edges_gpu.py."""
    assert ce_run["untouched"]  # without the gradient the logits stay as they were, bit for bit, all 4.47 GB
    stats = ce_run["stats"][write_grad]
    assert stats.shape == (4, T_MAX)
    for lo, hi in WINDOWS:
        kept = ce_run["kept"][(lo, hi)]
        after = ce_run["grad"][lo:hi] if write_grad else kept
        figs = ce_edges.compare_rows(kept, ce_run["labels"][lo:hi], stats[:, lo:hi].contiguous(), after, write_grad)
        print(f"[large] ce rows {lo}..{hi} grad={write_grad}: {figs}")


@pytest.mark.parametrize("write_grad", [False, True])
def test_ce_total_and_count(write_grad, ce_run):
    """Over all 17408 rows: the summed loss against the chunked fp32 torch cross-entropy. The bound is the edges file's
    per-row bound, 1e-4 + 1e-5 |loss|, summed over the rows that count (a sum of per-row errors cannot exceed it; one
    dropped or doubled row moves the sum by a whole loss, about 16 here and several times the bound). Ignored rows
    report a loss of exactly zero, and the rows that count are the labels' own."""
    stats, rows32, labels = ce_run["stats"][write_grad], ce_run["rows32"].double(), ce_run["labels"]
    valid = labels != -100
    want, got = rows32.sum().item(), stats[0].double().sum().item()
    bound = (1e-4 * valid.sum() + 1e-5 * rows32.abs().sum()).item()
    print(f"[large] ce total grad={write_grad}: {got:.4f} vs {want:.4f}, |difference| {abs(got - want):.3e}, "
          f"bound {bound:.3e}, rows that count {int(valid.sum())}")
    assert abs(got - want) <= bound, (got, want, bound)
    assert bool((stats[0][~valid] == 0).all()) and int((stats[0] > 0).sum()) == int(valid.sum())
    assert rows32[valid].mean().item() > 2 * bound  # so a single lost or doubled row cannot hide inside the bound


def test_ce_ignored_rows_have_a_zero_gradient(ce_run):
    """Every row labelled -100, wherever it lies in the 4.47 GB: all bits zero."""
    rows = (ce_run["labels"] == -100).nonzero().flatten()
    assert rows.numel() > 1500 and int(rows.max()) > ROW_2_32
    bits = ce_run["grad"].view(torch.int16)
    for s in range(0, rows.numel(), 256):
        assert not bool(bits[rows[s:s + 256]].any()), ("non-zero gradient in ignored rows", rows[s:s + 256].tolist())
