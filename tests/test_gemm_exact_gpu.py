"""Bit-exact sweep over every GEMM route on random small-integer operands.

Every GEMM kernel here accumulates in fp32 and rounds once, to nearest even, when it stores bf16; the split-K slabs are
fp32 too (csrc/splitk_fixup.h). On small integers every partial sum is an integer below 2^24, so fp32 addition is
exact in any order and the kernel has one right answer: bf16(exact product), bit for bit. No tolerance is involved; one
dropped, doubled or misplaced k element, token block, row or column anywhere fails the comparison. The operands are
seeded random integers (tests/_blockwise.py int_operand), not arithmetic patterns, which cannot see a permutation by a
multiple of their period. Routes the launcher picks by itself (wave tails, hybrid split-K, multi-problem grids) are also
checked to have run, through the dispatch trace."""
import pytest
import torch

from llm_fine_tune_distributed_amd.ops import _ext
from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import assert_blocks_close, assert_exact, exact, int_operand, swiglu_bwd_reference, traced
from _blockwise import mismatch as _mismatch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _ext_loaded():
    assert _ext.load(), _ext.load_error()


# ------------------------------------------------------------------------------------------------ 1a: forward gemm_tn

def _tn_shapes(cfg):
    """(M, N, K, strided): one tile; a reduction longer than the ring (K % 128 != 0 where the cfg allows it); 272
    tiles = more tiles than CUs with a ragged last round; the K = 128 single-pair path of the row-contiguous kernels;
    a row-strided a. cfgs 5 / 11 take K % 64, cfgs 60 / 61 K % 128 (csrc/gemm_tn.hip gemm_tn)."""
    k1, klong = {5: (64, 2112), 11: (64, 2112), 60: (128, 2176), 61: (128, 2176)}[cfg]
    return [(256, 256, k1, False), (768, 512, klong, False), (4352, 4096, 256, False), (2304, 7424, 128, False),
            (512, 256, 256, True)]


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("cfg", [5, 11, 60, 61])
def test_gemm_tn_exact(cfg, case):
    M, N, K, strided = _tn_shapes(cfg)[case]
    x = int_operand((M, K + (128 if strided else 0)), -2, 2, 100 + case, DEV)
    if strided:
        x = x[:, :K]  # a column slice of a wider activation: row-strided
        assert not x.is_contiguous()
    w = int_operand((N, K), -3, 3, 200 + case, DEV)
    with traced() as tr:
        out = _ext.ops().gemm_tn(x, w, cfg)
    assert f"tn.c{cfg}" in tr
    assert_exact(out, exact(x.float() @ w.float().t()), (cfg, M, N, K))


# -------------------------------------------------------------------------------------------------- 1b: gemm_tn_rope

def _quarter_turns(M, seed):
    """cos / sin [M, 64] fp32 with every (row, frequency) drawn from the four quarter turns (1, 0), (0, 1), (-1, 0),
    (0, -1): the rotation then only moves and negates integers, so the rotated product is exact too."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 4, (M, 64), generator=g)
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[q]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[q]
    return cos.contiguous().to(DEV), sin.contiguous().to(DEV)


def _rope_case(M, K, nq, nkv, cfg, seed):
    D = 128
    x = int_operand((M, K), -2, 2, seed, DEV)
    w = int_operand(((nq + 2 * nkv) * D, K), -3, 3, seed + 1, DEV)
    cos, sin = _quarter_turns(M, seed + 2)
    y = x.float() @ w.float().t()
    rc = (nq + nkv) * D
    want = exact(torch.cat([ref.apply_rope(y[:, :rc].reshape(M, nq + nkv, D), cos, sin).reshape(M, rc), y[:, rc:]], 1))
    with traced() as tr:
        out = _ext.ops().gemm_tn_rope(x, w, cos, sin, rc, cfg)
    assert f"tn.rope.c{cfg}" in tr
    # q, k and v column ranges apart: a shifted RoPE boundary (k rotated / v not) is named by the range that fails
    for name, lo, hi in (("q", 0, nq * D), ("k", nq * D, rc), ("v", rc, (nq + 2 * nkv) * D)):
        assert_exact(out[:, lo:hi], want[:, lo:hi], (name, cfg, M, K))
    assert_exact(out[:, rc:], exact(y[:, rc:].contiguous()), ("v == the plain product", cfg))
    return tr


@pytest.mark.parametrize("cfg", [5, 11, 60, 61])
def test_gemm_tn_rope_exact(cfg):
    _rope_case(512, 256, 2, 1, cfg, 300)


@pytest.mark.parametrize("tail", ["1", "0"])
def test_gemm_tn_rope_wave_tail_exact(tail, monkeypatch):
    """The SmolLM3 qkv grid (32 x 12 tiles = 1.5 rounds): cfg 11 runs the whole round and a 256 x 128 tail launch whose
    RoPE boundary moves with its pointers (SFTAMD_TN_TAIL=0: one launch)."""
    monkeypatch.setenv("SFTAMD_TN_TAIL", tail)
    tr = _rope_case(8192, 128, 16, 4, 11, 310)
    assert ("tn.rope.tail" in tr) == (tail == "1"), tr


# ------------------------------------------------------------------------------------------------ 1c: gemm_tn_swiglu

@pytest.mark.parametrize("cfg,M,I,K", [(5, 512, 384, 320), (5, 512, 128, 384), (5, 4352, 2048, 256),
                                       (11, 512, 384, 320), (11, 512, 128, 384), (11, 4352, 2048, 256),
                                       (60, 256, 128, 128), (60, 768, 1280, 2176), (60, 4352, 2048, 256),
                                       (60, 2304, 3712, 128),
                                       (61, 256, 128, 128), (61, 768, 1280, 2176), (61, 4352, 2048, 256),
                                       (61, 2304, 3712, 128)])
def test_gemm_tn_swiglu_exact(cfg, M, I, K):
    """gu = [gate | up] bit-exact; act == swiglu_fwd(gu) bit for bit: every SwiGLU epilogue of csrc/gemm_tn.hip rounds
    gate and up to bf16 first (rbf) and then applies silu(g) * u = g / (1 + __expf(-g)) * u in fp32, the expression of
    the standalone kernel (csrc/elementwise.hip swiglu_fwd_kernel) on the same bf16 values."""
    x = int_operand((M, K), -2, 2, 400, DEV)
    w = int_operand((2 * I, K), -1, 1, 401, DEV)
    with traced() as tr:
        gu, act = _ext.ops().gemm_tn_swiglu(x, w, cfg)
    assert f"tn.swiglu.c{cfg}" in tr
    assert_exact(gu, exact(x.float() @ w.float().t()), ("gu", cfg, M, I, K))
    assert_exact(act, _ext.ops().swiglu_fwd(gu), ("act", cfg, M, I, K))


# ------------------------------------------------------------------------------------------------ 1d: dgrad_gemm plain

def _dgrad_exact(M, K, N, cfg, seed, wpad=0):
    dy = int_operand((M, K), -2, 2, seed, DEV)
    w = int_operand((K, N + wpad), -3, 3, seed + 1, DEV)[:, :N]
    with traced() as tr:
        out = _ext.ops().dgrad_gemm(dy, w, None, cfg)
    assert_exact(out, exact(dy.float() @ w.float()), (cfg, M, K, N, wpad))
    return tr


@pytest.mark.parametrize("cfg,M,K,N,wpad", [(2, 384, 64, 256, 0), (2, 256, 96, 512, 64), (2, 512, 2048, 768, 0),
                                            (5, 256, 64, 256, 0), (5, 256, 96, 512, 64), (5, 512, 2048, 768, 0),
                                            (7, 256, 64, 256, 0), (7, 256, 192, 512, 64), (7, 512, 2048, 768, 0),
                                            (14, 256, 128, 256, 0), (14, 256, 384, 512, 64), (14, 512, 2048, 768, 0)])
def test_dgrad_gemm_exact(cfg, M, K, N, wpad):
    """One tile, a column-sliced w (row pitch N + 64), reductions longer than the ring, several tiles."""
    tr = _dgrad_exact(M, K, N, cfg, 500, wpad)
    assert f"dgrad.c{cfg}" in tr and "dgrad.tail" not in tr and "dgrad.splitk" not in tr, tr


@pytest.mark.parametrize("M,K,N", [(10240, 1024, 2048), (2560, 4096, 2048), (4352, 512, 4096)])
def test_dgrad_hybrid_splitk_exact(M, K, N):
    """Grids that are not whole rounds: cfg 14 splits the leftover tiles over the reduction for K >= 8192 only on the
    whole chip, so these shapes run unsplit here and split under a CU budget (test_dgrad_cu_budget_exact); either way
    the result is the one exact answer."""
    tr = _dgrad_exact(M, K, N, 14, 510)
    assert "dgrad.c14" in tr, tr


def test_dgrad_long_reduction_splitk_exact():
    """K >= 8192 on a grid below one round: the leftover (= all 16) tiles split over the reduction, fp32 slabs summed in
    order by the fixup."""
    tr = _dgrad_exact(512, 8192, 2048, 14, 515)
    assert "dgrad.splitk" in tr, tr


@pytest.mark.parametrize("cfg,K", [(5, 64), (7, 64), (5, 128), (14, 128)])
@pytest.mark.parametrize("tail", ["0", "2"])
def test_dgrad_wave_tail_exact(cfg, K, tail, monkeypatch):
    """The SmolLM3 down projection grid (43 x 32 tiles = 5.375 rounds): whole rounds on ``cfg`` + the leftover columns
    as 256 x 128 half tiles of cfg 2 (SFTAMD_DGRAD_TAIL=2), or one launch (0)."""
    monkeypatch.setenv("SFTAMD_DGRAD_TAIL", tail)
    tr = _dgrad_exact(8192, K, 11008, cfg, 520)
    assert f"dgrad.c{cfg}" in tr
    assert ("dgrad.tail" in tr) == (tail == "2") and ("dgrad.c2" in tr) == (tail == "2"), tr


def test_dgrad_cu_budget_exact():
    """set_cu_budget(248): a 256-tile input gradient splits its leftover 8 tiles over K (the hybrid split-K route)."""
    from llm_fine_tune_distributed_amd import ops
    try:
        assert ops.set_cu_budget(248) == 248
        tr = _dgrad_exact(4096, 2048, 4096, 14, 530)
        assert "dgrad.splitk" in tr, tr
        tr = _dgrad_exact(10240, 1024, 2048, 14, 531)  # 320 tiles: 248 whole + 72 split 3 ways
        assert "dgrad.splitk" in tr, tr
    finally:
        ops.set_cu_budget(0)
    assert ops.cu_budget() == 256


# ------------------------------------------------------------------- 1e: dgrad_gemm with the SwiGLU-backward epilogue

def _dgrad_swiglu_case(M, K, N, cfgs, seed):
    """dy, w in {-1, 0, 1} with at most 256 non-zeros per w column: |dact| <= 256, so dact is the same number in the
    kernel's fp32 accumulator and in the bf16 tensor handed to the standalone kernel. gu is ordinary randn."""
    dy = int_operand((M, K), -1, 1, seed, DEV)
    w = int_operand((K, N), -1, 1, seed + 1, DEV, nnz_per_col=256)
    torch.manual_seed(seed + 2)
    gu = torch.randn(M, 2 * N, device=DEV, dtype=torch.bfloat16)
    dact = dy.float() @ w.float()
    assert dact.abs().max().item() <= 256
    alone = _ext.ops().swiglu_bwd(dact.to(torch.bfloat16), gu)
    want, bound = swiglu_bwd_reference(dact.double(), gu)
    outs, trs = {}, {}
    for cfg in cfgs:
        with traced() as tr:
            outs[cfg] = _ext.ops().dgrad_gemm(dy, w, gu, cfg)
        assert f"dgrad.swiglu.c{cfg}" in tr, tr
        trs[cfg] = tr
    first = outs[cfgs[0]]
    for cfg in cfgs[1:]:  # every tile config rounds identically (the epilogue pins its fma)
        assert_exact(outs[cfg], first, ("cfg", cfg, "vs cfg", cfgs[0]))
    worst = assert_blocks_close(first, want, 32, 32, bound, f"dgrad swiglu {M}x{K}x{N}")
    print(f"dgrad_swiglu_exact {M}x{K}x{N}: worst 32x32 block {worst:.3e}, bound {bound:.3e}")
    # the standalone kernel on the same dact: the same real number computed in fp32 by two orders of multiplication
    # (see the docstring of test_dgrad_swiglu_exact), so after the bf16 store the two are equal or neighbours: one bf16
    # ulp = 2^-7 relative at the most
    a, f = alone.float(), first.float()
    off = (f - a).abs() > 2.0 ** -7 * a.abs() + 1e-30
    assert not bool(off.any()), (int(off.sum()), off.nonzero()[0].tolist())
    return trs


@pytest.mark.parametrize("M,K,N", [(256, 256, 256), (2048, 2048, 2816)])
def test_dgrad_swiglu_exact(M, K, N):
    """dgu = swiglu_bwd(dy @ w, gu) from the fused epilogue, cfgs 2 / 5 / 7 bitwise equal to each other.

    Not bitwise the standalone swiglu_bwd kernel, by the source: csrc/common.h swiglu_grad (standalone kernel, LoRA
    epilogue) computes dup = (d g) sg and dgate = ((d u) sg) (1 + g (1 - sg)); the ring epilogue of csrc/gemm_dgrad.hip
    folds sg into d first, t = d sg, dup = t g, dgate = (t u) (1 + g (1 - sg)) — one multiplication fewer per element,
    a different fp32 rounding. With an integer dact of at most 256 the GEMM part is exact, so all that is left between
    the two is that last-bit difference: every element must be within one bf16 ulp of the standalone kernel's, and
    every 32 x 32 block within 2 x the error of a torch emulation (fp32 expression, one bf16 rounding) of the fp64
    result."""
    _dgrad_swiglu_case(M, K, N, (5, 2, 7), 600)


@pytest.mark.parametrize("tail", ["0", "2"])
def test_dgrad_swiglu_wave_tail_exact(tail, monkeypatch):
    """(8192, 64, 11008): the whole rounds + the half-tile tail launch, whose gate / up / output pointers are shifted to
    the leftover columns while ea.N keeps the full width for the up half."""
    monkeypatch.setenv("SFTAMD_DGRAD_TAIL", tail)
    for cfg, tr in _dgrad_swiglu_case(8192, 64, 11008, (5, 7), 610).items():
        assert ("dgrad.tail" in tr) == (tail == "2") and ("dgrad.swiglu.c2" in tr) == (tail == "2"), (cfg, tr)


# --------------------------------------------------------------------------------------------- 1f: dgrad_gemm_delta

@pytest.mark.parametrize("M,K,N", [(256, 256, 256), (1024, 2048, 2048), (8192, 2048, 2048)])
def test_dgrad_delta_exact(M, K, N):
    """Dense random integer w (not a shifted identity), |dx| <= 256 so the stored bf16 dx is the exact product and
    delta[h, m] = sum over the head's 128 columns of dx . a is an exact fp32 integer: both outputs bit for bit."""
    dy = int_operand((M, K), -1, 1, 700, DEV)
    w = int_operand((K, N), -1, 1, 701, DEV, nnz_per_col=256)
    a = int_operand((M, N), -2, 2, 702, DEV)
    with traced() as tr:
        dx, delta = _ext.ops().dgrad_gemm_delta(dy, w, a)
    assert "dgrad.c14.delta" in tr and "dgrad.splitk" not in tr, tr
    want = dy.float() @ w.float()
    assert want.abs().max().item() <= 256
    assert_exact(dx, exact(want), ("dx", M, K, N))
    wd = (want * a.float()).view(M, N // 128, 128).sum(-1).t().contiguous()
    assert wd.abs().max().item() < 2 ** 24
    assert delta.shape == (N // 128, M) and delta.dtype == torch.float32
    assert torch.equal(delta, wd), _mismatch(delta, wd)


# ----------------------------------------------------------------------------------------------------- 1g: wgrad_gemm

WGRAD_CASES = [(9, 416, 512, 384), (9, 32, 256, 128), (10, 352, 512, 512), (10, 96, 256, 256),
               (209, 64, 256, 128), (210, 512, 512, 512), (309, 384, 512, 384), (310, 320, 256, 256),
               (410, 1024, 256, 256), (1310, 96, 4096, 4352), (1309, 128, 4096, 2304), (1210, 160, 4352, 4096),
               (14, 128, 256, 256), (14, 256, 512, 768), (14, 1024, 2304, 4352), (214, 512, 512, 512),
               (314, 384, 512, 256), (414, 1024, 256, 256), (1314, 256, 4096, 4352), (1214, 384, 4352, 4096),
               (1214, 1024, 2048, 11008)]


@pytest.mark.parametrize("cfg,T,N,K", WGRAD_CASES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_exact(cfg, T, N, K, accumulate):
    """dW = dy^T x (+ an integer base when accumulating): the 8-wave rings (9 / 10), their split-K (2xx-4xx) and hybrid
    (1xxx) variants, the 4-wave ring (14) and its variants; the 4-wave kernel also through a padded x pitch."""
    dy = int_operand((T, N), -2, 2, 800, DEV)
    x = int_operand((T, K), -3, 3, 801, DEV)
    base = int_operand((N, K), -8, 8, 802, DEV)
    want = dy.float().t() @ x.float()
    if accumulate:
        want = want + base.float()
    want = exact(want)
    out = base.clone()
    with traced() as tr:
        _ext.ops().wgrad_gemm(out, dy, x, accumulate, cfg)
    assert f"wgrad.c{cfg}" in tr, tr
    assert_exact(out, want, (cfg, T, N, K, accumulate))
    if cfg % 100 == 14:  # x as a view into a wider buffer (e.g. the gate_up input written by the norm with y_ld)
        buf = int_operand((T, K + 64), -3, 3, 803, DEV)
        buf[:, :K] = x
        out2 = base.clone()
        _ext.ops().wgrad_gemm(out2, dy, buf[:, :K], accumulate, cfg)
        assert_exact(out2, want, ("padded x pitch", cfg, T, N, K, accumulate))


@pytest.fixture(scope="module")
def norm_bound():
    """4 x the relative error of a plain fp32 sum of squares against fp64, per size, measured on the reference alone;
    never below 4 x 2^-24, the half-ulp of writing any sum into an fp32 at all."""
    def bound(out):
        s64 = out.double().pow(2).sum().item()
        e32 = abs(out.float().pow(2).sum().item() - s64) / s64
        return 4 * max(e32, 2.0 ** -24), s64, e32
    return bound


@pytest.mark.parametrize("cfg,T,N,K", [c for c in WGRAD_CASES if c[0] % 100 in (9, 10, 14)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_norm_slots_exact(cfg, T, N, K, accumulate, norm_bound):
    """The gradient-norm partial slots sum to the squared norm of the stored gradient. Operands in {-1, 0, 1} keep
    |dW| <= 256, exactly representable in bf16, so the whole tiles' partials (squared from the fp32 values before the
    store, csrc/gemm_wgrad.hip epilogue) and the split tiles' (squared from the stored bf16, csrc/splitk_fixup.h) mean
    the same number; the slots are summed in fp64 here, so what is judged is the kernel's own fp32 partial sums."""
    dy = int_operand((T, N), -1, 1, 810, DEV)
    x = int_operand((T, K), -1, 1, 811, DEV)
    base = int_operand((N, K), -2, 2, 812, DEV)
    want = dy.float().t() @ x.float() + (base.float() if accumulate else 0)
    assert want.abs().max().item() <= 256
    cap = -(-N // 256) * -(-K // 128) * 32
    slots = torch.zeros(cap + 64, device=DEV)
    slots[cap:] = 7.0  # sentinel past the capacity handed to the kernel
    torch.full((1 << 24,), float("nan"), device=DEV)  # garbage in the allocator's free blocks (parked hybrid slots)
    out = base.clone()
    with traced() as tr:
        _ext.ops().wgrad_gemm(out, dy, x, accumulate, cfg, slots[:cap])
    assert "wgrad.norm_slots" in tr, tr
    assert_exact(out, exact(want), (cfg, T, N, K, accumulate))
    bound, s64, e32 = norm_bound(out)
    got = slots[:cap].double().sum().item()
    print(f"wgrad_norm_slots cfg {cfg} {T}x{N}x{K} acc {accumulate}: slots {abs(got - s64) / s64:.3e}, "
          f"plain fp32 sum {e32:.3e}, bound {bound:.3e}")
    assert abs(got - s64) <= bound * s64, (got, s64)
    assert torch.all(slots[cap:] == 7.0)


# ------------------------------------------------------------------------- 1h: wgrad_gemm_pair and wgrad_gemm_multi

def _problems(T, shapes, seed):
    dys = [int_operand((T, n), -2, 2, seed + 3 * i, DEV) for i, (n, _) in enumerate(shapes)]
    xs = [int_operand((T, k), -3, 3, seed + 3 * i + 1, DEV) for i, (_, k) in enumerate(shapes)]
    bases = [int_operand((n, k), -8, 8, seed + 3 * i + 2, DEV) for i, (n, k) in enumerate(shapes)]
    prods = [dy.float().t() @ x.float() for dy, x in zip(dys, xs)]
    return dys, xs, bases, prods


def _wants(bases, prods, accumulate):
    return [exact(p + b.float()) if accumulate else exact(p) for b, p in zip(bases, prods)]


@pytest.fixture(scope="module")
def pair_problems():
    cache = {}

    def get(N0, K0, N1, K1, T):
        key = (N0, K0, N1, K1, T)
        if key not in cache:
            cache.clear()  # one shape set alive at a time
            cache[key] = _problems(T, [(N0, K0), (N1, K1)], 900)
        return cache[key]
    yield get
    cache.clear()


@pytest.mark.parametrize("N0,K0,N1,K1,T", [(2048, 10752, 5632, 2048, 256),    # 336 + 176 = 512 tiles: 2 whole rounds
                                           (2048, 11008, 22016, 2048, 256),   # the SmolLM3 MLP: 1032 = 4 rounds + 8
                                           (2048, 11008, 22016, 2048, 1024)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_pair_exact(N0, K0, N1, K1, T, accumulate, pair_problems):
    """wgrad_gemm_pair: both gradients bit-exact, the 8 leftover tiles of problem 1 (split over the tokens into fp32
    slabs and summed by the fixup) included."""
    dys, xs, bases, prods = pair_problems(N0, K0, N1, K1, T)
    outs = [b.clone() for b in bases]
    with traced() as tr:
        _ext.ops().wgrad_gemm_pair(outs[0], dys[0], xs[0], accumulate, None, outs[1], dys[1], xs[1], accumulate, None)
    assert "wgrad.pair" in tr, tr
    for i, (o, w) in enumerate(zip(outs, _wants(bases, prods, accumulate))):
        assert_exact(o, w, ("problem", i, T, accumulate))


@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_pair_split_all_exact(accumulate):
    """o_proj + qkv as one launch with every tile split 3 ways over T = 1024 (8 token blocks: uneven pieces)."""
    T = 1024
    dys, xs, bases, prods = _problems(T, [(2048, 2048), (3072, 2048)], 910)
    outs = [b.clone() for b in bases]
    with traced() as tr:
        _ext.ops().wgrad_gemm_pair(outs[0], dys[0], xs[0], accumulate, None, outs[1], dys[1], xs[1], accumulate, None, 3)
    assert "wgrad.pair" in tr, tr
    for i, (o, w) in enumerate(zip(outs, _wants(bases, prods, accumulate))):
        assert_exact(o, w, ("problem", i, accumulate))


@pytest.fixture(scope="module")
def layer_problems():
    """down, gate_up, o, qkv at SmolLM3 widths: 1192 tiles = 4 whole rounds + 168 leftover tiles spanning three
    problems. The operands and the exact products, computed once per token count."""
    cache = {}

    def get(T):
        if T not in cache:
            cache.clear()
            cache[T] = _problems(T, [(2048, 11008), (22016, 2048), (2048, 2048), (3072, 2048)], 920)
        return cache[T]
    yield get
    cache.clear()


@pytest.mark.parametrize("T", [1024, 8192])
@pytest.mark.parametrize("split_left", [0, 3])
@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_multi_four_problems_exact(T, split_left, accumulate, layer_problems):
    dys, xs, bases, prods = layer_problems(T)
    outs = [b.clone() for b in bases]
    empty = torch.empty(0, device=DEV)
    with traced() as tr:
        _ext.ops().wgrad_gemm_multi(outs, dys, xs, [1 if accumulate else 0] * 4, [empty] * 4, 0, split_left)
    assert "wgrad.multi4" in tr, tr
    for i, (o, w) in enumerate(zip(outs, _wants(bases, prods, accumulate))):
        assert_exact(o, w, ("problem", i, T, split_left, accumulate))


@pytest.mark.parametrize("split_all", [2, 4])
def test_wgrad_multi_three_small_problems_exact(split_all):
    T = 1024
    dys, xs, bases, prods = _problems(T, [(512, 256), (256, 512), (768, 256)], 930)
    outs = [b.clone() for b in bases]
    empty = torch.empty(0, device=DEV)
    with traced() as tr:
        _ext.ops().wgrad_gemm_multi(outs, dys, xs, [0, 0, 0], [empty] * 3, split_all, 0)
    assert "wgrad.multi3" in tr, tr
    for i, (o, w) in enumerate(zip(outs, _wants(bases, prods, False))):
        assert_exact(o, w, ("problem", i, split_all))
