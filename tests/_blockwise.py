"""Block-wise error metrics and exact-integer operands for the kernel tests (a helper module, not a conftest).

One Frobenius-norm relative error over a whole output dilutes a fault confined to one tile, one 128-token block or one
row by the square root of the number of tiles: a 32 x 32 block of a 4096 x 4096 result that lost 1/8 of its reduction
moves the global error from 1.66e-3 to 1.91e-3 (tests/test_blockwise_cpu.py). The functions here judge every
``br x bc`` block on its own, and build small-integer operands on which a GEMM with fp32 accumulation and one
round-to-nearest-even store has exactly one right answer."""
import contextlib
import math

import torch


def _pad_blocks(t: torch.Tensor, br: int, bc: int) -> torch.Tensor:
    """[R, C] -> [ceil(R / br), ceil(C / bc), br * bc]; the ragged last blocks are zero-padded (zeros add nothing to a
    sum of squares, so every element counts exactly once and no block is left out)."""
    R, C = t.shape
    nr, nc = -(-R // br), -(-C // bc)
    if nr * br != R or nc * bc != C:
        t = torch.nn.functional.pad(t, (0, nc * bc - C, 0, nr * br - R))
    return t.reshape(nr, br, nc, bc).permute(0, 2, 1, 3).reshape(nr, nc, br * bc)


def block_rel_err(got: torch.Tensor, want: torch.Tensor, br: int, bc: int, rms=None) -> torch.Tensor:
    """Per ``br x bc`` block: ||got - want|| / max(||want_block||, rms(want) * sqrt(br * bc)), as a [blocks_r, blocks_c]
    fp64 tensor. The floor makes a block whose reference is zero or tiny (dq / dk of a length-1 sequence) count against
    the typical magnitude of the whole reference instead of dividing by zero. ``want`` is the fp64 reference; ``rms``
    overrides rms(want) when ``want`` is a slice of a larger reference."""
    assert got.dim() == 2 and got.shape == want.shape, (got.shape, want.shape)
    w = want.double()
    d = _pad_blocks(got.double() - w, br, bc).pow(2).sum(-1).sqrt()
    n = _pad_blocks(w, br, bc).pow(2).sum(-1).sqrt()
    if rms is None:
        rms = w.pow(2).mean().sqrt() if w.numel() else w.new_zeros(())
    rms = torch.as_tensor(rms, dtype=torch.float64, device=w.device)
    floor = rms * math.sqrt(br * bc)
    den = torch.maximum(n, floor.expand_as(n))
    # an all-zero reference: any non-zero output is infinitely wrong, an all-zero output is right
    return torch.where(den > 0, d / den.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), d))


def global_rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    w = want.double()
    return ((got.double() - w).norm() / w.norm().clamp_min(1e-300)).item()


def assert_blocks_close(got: torch.Tensor, want: torch.Tensor, br: int, bc: int, bound: float, what: str = "",
                        row_splits=None) -> float:
    """Every ``br x bc`` block of ``got`` within ``bound`` of the fp64 ``want`` (block_rel_err); returns the worst block's
    error. On failure: the worst block's index and error, how many blocks are over the bound, the global error.
    ``row_splits`` (boundaries [0, ..., R], e.g. cu_seqlens) replaces the uniform ``br`` by one row block per range: the
    block index then reads (sequence, column block) and ``br`` is ignored."""
    if row_splits is not None:
        rs = [int(v) for v in row_splits]
        assert rs[0] == 0 and rs[-1] == got.shape[0], (rs, got.shape)  # no row is left out
        rms = want.double().pow(2).mean().sqrt()
        rs = [s for s, t in zip(rs[:-1], rs[1:]) if t > s] + [rs[-1]]  # empty ranges hold no element
        e = torch.cat([block_rel_err(got[s:t], want[s:t], t - s, bc, rms) for s, t in zip(rs[:-1], rs[1:])])
        br = "seq"
    else:
        e = block_rel_err(got, want, br, bc)
    worst = e.max().item() if e.numel() else 0.0
    if not worst <= bound:  # also catches NaN
        bad = ~(e <= bound)
        flat = int(torch.where(torch.isnan(e), torch.full_like(e, math.inf), e).argmax())
        i, j = divmod(flat, e.shape[1])
        raise AssertionError(
            f"{what + ': ' if what else ''}worst {br}x{bc} block ({i}, {j}) = "
            f"rows {i * br if row_splits is None else rs[i]}.., cols {j * bc}.. has "
            f"error {e[i, j].item():.3e} > bound {bound:.3e}; {int(bad.sum())} of {e.numel()} blocks over the bound; "
            f"global error {global_rel_err(got, want):.3e}")
    return worst


def rounding_floor(want64: torch.Tensor, br: int, bc: int) -> float:
    """The worst per-block error of the reference itself rounded once to bf16: the irreducible output rounding,
    computed from the reference alone."""
    return block_rel_err(want64.float().to(torch.bfloat16), want64, br, bc).max().item()


def int_operand(shape, lo: int, hi: int, seed: int, device, nnz_per_col=None) -> torch.Tensor:
    """Seeded random integers in [lo, hi] as bf16 (|lo|, |hi| <= 256: exact). Random, not an arithmetic pattern: a
    periodic pattern cannot see a permutation by a multiple of its period. ``nnz_per_col`` keeps that many non-zeros
    per column, at random rows (2-D only): with entries in {-1, 0, 1} a product over that operand's rows is then bounded
    by nnz_per_col in magnitude, so it stays exactly representable in bf16 when nnz_per_col <= 256."""
    assert -256 <= lo <= hi <= 256
    g = torch.Generator(device=device)  # drawn on the target device: the large operands take no host pass
    g.manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int32, device=device)
    if nnz_per_col is not None:
        R, C = shape
        if nnz_per_col < R:
            # rank of an i.i.d. key within its column: the nnz_per_col smallest keys of every column are kept
            keep = torch.rand(R, C, generator=g, device=device).argsort(0).argsort(0) < nnz_per_col
            t = t * keep
    return t.to(torch.bfloat16)


def swiglu_bwd_expr(d: torch.Tensor, g: torch.Tensor, u: torch.Tensor):
    """(dgate, dup) of act = silu(gate) * up for an upstream gradient d, in the dtype of the arguments: the expression
    of csrc/common.h swiglu_grad, dgate = d u sg (1 + g (1 - sg)), dup = d g sg with sg = sigmoid(g)."""
    sg = 1.0 / (1.0 + torch.exp(-g))
    return ((d * u) * sg) * (g * (1.0 - sg) + 1.0), (d * g) * sg


def swiglu_bwd_reference(dact64: torch.Tensor, gu: torch.Tensor, br: int = 32, bc: int = 32):
    """The fp64 SwiGLU backward of (dact64, bf16 gu = gate | up) and the block bound of a fused dgrad epilogue: 2 x the
    worst block error of a torch emulation that takes the fp64 product to fp32 (the kernel hands its fp32 accumulators to
    the epilogue unrounded), applies the expression in fp32 and rounds the result once to bf16."""
    g, u = gu.double().chunk(2, dim=-1)
    want = torch.cat(swiglu_bwd_expr(dact64, g, u), dim=-1)
    emul = torch.cat(swiglu_bwd_expr(dact64.float(), g.float(), u.float()), dim=-1).to(torch.bfloat16)
    return want, 2 * block_rel_err(emul, want, br, bc).max().item()


# ------------------------------------------------------------------ exact comparison and the dispatch trace
@contextlib.contextmanager
def traced():
    """Collects the dispatch trace of the launches inside the block: ``box`` maps kernel-route names to counts."""
    from llm_fine_tune_distributed_amd.ops import _ext
    ops, box = _ext.ops(), {}
    ops.dispatch_trace(True)
    try:
        yield box
    finally:
        ops.dispatch_trace(False)
        box.update(kv.split("=") for kv in ops.dispatch_trace_read().split(";") if kv)


def exact(a32: torch.Tensor) -> torch.Tensor:
    """bf16 of an exact fp32 integer result (the one rounding the kernel may make)."""
    assert a32.dtype == torch.float32 and a32.abs().max().item() < 2 ** 24
    return a32.to(torch.bfloat16)


def mismatch(out, want):
    """Where two tensors differ, for the assertion message: count, first index, the 256 x 256 tiles touched."""
    bad = (out != want).nonzero()
    if bad.numel() == 0:
        return "equal"
    tiles = torch.unique(bad // 256, dim=0)
    first = tuple(bad[0].tolist())
    return (f"{bad.shape[0]} of {out.numel()} elements differ, first at {list(first)} "
            f"(got {out[first].item()}, want {want[first].item()}), "
            f"{tiles.shape[0]} 256x256 tiles touched, e.g. {tiles[:4].tolist()}")


def assert_exact(out, want, what=""):
    assert out.shape == want.shape and out.dtype == want.dtype, (what, out.shape, want.shape)
    assert torch.equal(out, want), (what, mismatch(out, want))
