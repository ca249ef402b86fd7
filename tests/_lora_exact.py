"""Exact references, case tables and the bit-for-bit comparison of the LoRA adapter kernel tests (csrc/lora.hip; a
helper module, not a conftest; device-agnostic).

With small-integer bf16 operands every fp32 partial sum of these kernels is an exact integer, a dropout probability of
0.5 makes 1 / (1 - p) exactly 2 and a power-of-two adapter scale keeps every factor a power of two: whatever order a
kernel adds in, each output has exactly one right bit pattern as long as every partial sum stays below 2^24. The
references here are written from the definitions in fp64 (independent of ops/reference.py, except for the dropout hash
``dropout_keep``, the bit-exact twin of csrc/common.h drop_keep, which has CPU tests of its own) and rounded once.

The case tables of tests/test_lora_exact_gpu.py live here, each with ``*_operands`` and a worst-case magnitude
``*_bound`` (the sum of the largest possible |terms|, which bounds every partial sum in every summation order), so that
tests/test_lora_exact_cpu.py proves on the CPU that every GPU case is in the exact regime."""
import torch

from llm_fine_tune_distributed_amd.ops import reference as ref

from _blockwise import int_operand

BF16 = torch.bfloat16
EXACT_LIMIT = 2 ** 24
SEED = 99  # dropout seed of every case


# ------------------------------------------------------------------------------------------------ comparison
def bits(t: torch.Tensor) -> torch.Tensor:
    """The bit patterns of a bf16 / fp32 tensor as integers of the same width."""
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    assert t.dtype == torch.float32, t.dtype
    return t.view(torch.int32)


def _some(values, limit=12):
    values = [int(v) for v in values]
    return str(values[:limit])[:-1] + (f", ... {len(values)} in all]" if len(values) > limit else "]")


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str = "") -> None:
    """``got`` and ``want`` hold the same bit patterns. On failure: the first differing (row, column), how many elements
    differ, and the rows and 8-column groups they fall in (a 1-D tensor counts as one row, leading dimensions of a 3-D
    one are folded into the rows)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = bits(got), bits(want)
    if torch.equal(g, w):
        return
    cols = g.shape[-1] if g.dim() else 1
    bad = (g != w).reshape(-1, cols)
    idx = bad.nonzero()
    r0, c0 = (int(v) for v in idx[0])
    rows, groups = idx[:, 0].unique(), (idx[:, 1] // 8).unique()
    raise AssertionError(
        f"{what + ': ' if what else ''}first difference at (row {r0}, column {c0}): got "
        f"{got.reshape(-1, cols)[r0, c0].item()!r}, want {want.reshape(-1, cols)[r0, c0].item()!r}; "
        f"{idx.shape[0]} of {bad.numel()} elements differ, in {rows.numel()} rows {_some(rows)} and "
        f"{groups.numel()} 8-column groups {_some(groups)} (group g = columns 8 g .. 8 g + 7)")


def exact_or_fail(want64: torch.Tensor) -> torch.Tensor:
    """The condition under which "one right answer" holds for a computed reference; a case that breaks it is a bug in
    the case table, not a tolerance to widen. Returns ``want64`` with -0 folded into +0 (an fp32 sum that starts from
    +0 never yields -0)."""
    assert want64.dtype == torch.float64
    if want64.numel():
        assert want64.abs().max().item() < EXACT_LIMIT, want64.abs().max().item()
    return want64 + 0.0


def to_bf16(want64: torch.Tensor) -> torch.Tensor:
    return want64.float().to(BF16)


# ------------------------------------------------------------------------------------------------ references
def keep_mask(T: int, K: int, seed: int, p: float, device="cpu") -> torch.Tensor:
    """[T, K] bool: element (t, k) survives dropout (the hash of its index t * K + k); all True for p == 0."""
    if p <= 0:
        return torch.ones(T, K, dtype=torch.bool, device=device)
    idx = torch.arange(T * K, dtype=torch.int64, device=device).view(T, K)
    return ref.dropout_keep(idx, seed, p)


def _masked(x: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    return torch.where(keep, x.double(), torch.zeros((), dtype=torch.float64, device=x.device))


def fwd_want(x, A, s, p, seed, ldX, keep=None):
    """(X' [T, ldX or K + R], xd [T, K]): X'[:, :K] = x, X'[:, K:K + R] = bf16(s / (1 - p) ((x * keep) @ A^T)), zeros
    beyond; xd = bf16(x * keep / (1 - p)). ``keep`` replaces the hash mask (the sensitivity tests)."""
    T, K = x.shape
    R = A.shape[0]
    keep = keep_mask(T, K, seed, p, x.device) if keep is None else keep
    xk = _masked(x, keep)
    xa = exact_or_fail(xk @ A.double().t()) * (s / (1.0 - p))
    X = torch.zeros(T, ldX or K + R, dtype=BF16, device=x.device)
    X[:, :K] = x
    X[:, K:K + R] = to_bf16(exact_or_fail(xa))
    return X, to_bf16(exact_or_fail(xk / (1.0 - p)))


def bwd_dx_want(base, dxa, A, p, seed, keep=None):
    """bf16(base + keep / (1 - p) (dxa @ A)): one fma and one rounding, the product is not rounded before the add."""
    T, K = base.shape
    keep = keep_mask(T, K, seed, p, base.device) if keep is None else keep
    prod = exact_or_fail(dxa.double() @ A.double())
    return to_bf16(exact_or_fail(base.double() + _masked(prod, keep) / (1.0 - p)))


def tsum_want(X, K, S, p, seed, keep=None):
    """fp32 [R, K] = S^T (X[:, :K] * keep) / (1 - p), the sum of lora_tsum's slabs."""
    T = X.shape[0]
    keep = keep_mask(T, K, seed, p, X.device) if keep is None else keep
    return exact_or_fail(S.double().t() @ _masked(X[:, :K], keep) / (1.0 - p)).float()


def grad_out_want(sum_, out_old, r0, c0, tr, acc):
    """The new value of one lora_grad_out output: block [r0, r0 + nr) x [c0, c0 + nc) of the slab sum ([R, K] or
    [ns, R, K] fp32), transposed when ``tr``, plus the old value when ``acc``; added in fp64, rounded once."""
    total = sum_.double().sum(0) if sum_.dim() == 3 else sum_.double()
    nr, nc = (out_old.shape[1], out_old.shape[0]) if tr else out_old.shape
    blk = total[r0:r0 + nr, c0:c0 + nc]
    blk = blk.t() if tr else blk
    want = exact_or_fail(blk + out_old.double() if acc else blk.clone())
    return want.float().to(out_old.dtype)


# ------------------------------------------------------------------------------------------------ lora_fwd cases
# K: 256 half a 512-column chunk, 768 one and a half, 2048 the NCH = 4 all-loads-in-flight instantiation, 2560 five
# chunks on the generic path (both LDS tiles reused). T: one row, one past a 16-row block, ragged. pad: ldX = 0 (K + R),
# K + R + 8, K + R + 128. Rotated so that every value of every column meets every R (asserted on the CPU).
FWD_K, FWD_T, FWD_PAD, FWD_R = (256, 768, 2048, 2560), (1, 17, 203), (None, 8, 128), (16, 32, 48, 64)


def _fwd_cases():
    cases = []
    for ri, R in enumerate(FWD_R):
        for i in range(7):
            cases.append(dict(T=FWD_T[(i + ri) % 3], K=FWD_K[(i + ri) % 4], R=R, pad=FWD_PAD[(i + 2 * ri) % 3],
                              p=(0.0, 0.5)[(i + ri) % 2], s=(0.5, 2.0)[(i // 2 + ri) % 2], save_xd=(i // 2) % 2 == 0))
    return cases


FWD_CASES = _fwd_cases()
FWD_SW_CASES = [dict(T=T, K=K, R=R, pad=pad, p=p, s=s)
                for (T, K, R, pad, p, s) in [(17, 256, 16, 8, 0.5, 0.5), (203, 768, 64, 128, 0.0, 2.0),
                                             (203, 2560, 16, None, 0.5, 2.0), (1, 256, 64, 128, 0.5, 0.5),
                                             (17, 768, 16, None, 0.0, 0.5), (19, 2560, 64, 8, 0.5, 0.5)]]


def case_id(c) -> str:
    return "-".join(f"{k}{v}" for k, v in c.items())


def fwd_ldX(c) -> int:
    return 0 if c["pad"] is None else c["K"] + c["R"] + c["pad"]


def fwd_operands(c, device):
    T, K, R = c["T"], c["K"], c["R"]
    return (int_operand((T, K), -4, 4, 11 + T + K + R, device), int_operand((R, K), -2, 2, 12 + T + K + R, device))


def fwd_bound(c) -> float:
    return c["K"] * 4 * 2 * max(1.0, c["s"] / (1 - c["p"]))


# ------------------------------------------------------------------------------------------------ lora_bwd_dx cases
# K: 8 a wave whose only valid lane is c = 0, 136 one full 128-column wave + 8 columns, 520 one block + 8 columns
BWD_K, BWD_T, BWD_R = (8, 136, 520, 1032, 2048), (1, 19, 203), (16, 32, 48, 64)
BWD_CASES = [dict(T=BWD_T[(ki + ri) % 3], K=K, R=R, p=(0.0, 0.5)[(ki + ri) % 2], sliced=(ki // 2 + ri) % 2 == 1)
             for ri, R in enumerate(BWD_R) for ki, K in enumerate(BWD_K)]
# every T, p and base layout with every R
BWD_CASES += [dict(T=203, K=136, R=16, p=0.5, sliced=False), dict(T=1, K=520, R=32, p=0.0, sliced=True),
              dict(T=19, K=8, R=48, p=0.5, sliced=True), dict(T=1, K=1032, R=64, p=0.0, sliced=False),
              dict(T=203, K=136, R=48, p=0.0, sliced=False), dict(T=19, K=520, R=64, p=0.5, sliced=True)]


def bwd_operands(c, device):
    """(base, dxa, A): base contiguous or the left columns of a [T, K + 64] tensor."""
    T, K, R = c["T"], c["K"], c["R"]
    wide = int_operand((T, K + 64), -4, 4, 21 + T + K + R, device)
    base = wide[:, :K] if c["sliced"] else wide[:, :K].contiguous()
    return base, int_operand((T, R), -2, 2, 22 + T + K + R, device), int_operand((R, K), -2, 2, 23 + T + K + R, device)


def bwd_bound(c) -> float:
    return 4 + c["R"] * 2 * 2 / (1 - c["p"])


# ------------------------------------------------------------------------------------------------ lora_tsum cases
# prop: "multi" a chunk of more than one 64-token stage (splits * 64 < T), "tail3" 64-token chunks, the last with 3
# tokens (splits == ceil(T / 64), T % 64 == 3), None nothing asserted about the split
def _tsum_cases():
    cases = []
    for T, K in ((1100, 4096), (1000, 8200)):  # narrow / wide (8 valid columns in the last 256-column workgroup)
        cases += [dict(T=T, K=K, R=R, p=p, prop="multi") for R in (16, 32, 48, 64) for p in (0.0, 0.5)]
    cases += [dict(T=67, K=8200, R=16, p=0.5, prop="tail3"), dict(T=67, K=8200, R=64, p=0.0, prop="tail3"),
              dict(T=203, K=520, R=32, p=0.5, prop=None), dict(T=203, K=520, R=48, p=0.0, prop=None),
              dict(T=2051, K=1032, R=64, p=0.5, prop="tail3"), dict(T=2051, K=1032, R=16, p=0.0, prop="tail3"),
              dict(T=1, K=64, R=16, p=0.0, prop=None), dict(T=1, K=64, R=64, p=0.5, prop=None)]
    return cases


TSUM_CASES = _tsum_cases()


def tsum_operands(c, device):
    """(X, S): X the left K columns of a [T, K + 72] tensor, S a 16-byte aligned column slice of a [T, R + 24] one
    (fresh integers: the adapter columns of a computed X' reach 2^14 and would leave the exact range over T tokens)."""
    T, K, R = c["T"], c["K"], c["R"]
    X = int_operand((T, K + 72), -4, 4, 31 + T + K + R, device)[:, :K]
    S = int_operand((T, R + 24), -2, 2, 32 + T + K + R, device)[:, 8:8 + R]
    return X, S


def tsum_bound(c) -> float:
    return c["T"] * 4 * 2 / (1 - c["p"])
