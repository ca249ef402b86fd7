"""Stale-memory poisoning for the kernel tests (a helper module, not a conftest).

The extension allocates its outputs and scratch buffers with at::empty, so a kernel that reads an element nothing wrote
computes with whatever the previous owner of that block left behind: in a fresh process usually zeros, the one fill
that hides the bug. ``poison`` fills the free memory of PyTorch's caching allocator with one byte value;
``assert_fill_independent`` runs an op under three fills and requires bit-equal results:

  0x00  the lucky case;
  0xFF  NaN as bf16 and as fp32, -1 as int32: a stale value that is consumed shows;
  0x4B  about 1.3e7 as bf16 and as fp32: finite, so it also shows where a ``0 * x`` or a masked lane would hide a NaN.

No kernel of csrc/ uses global atomics, so every op is run-to-run deterministic and bit equality is the bar."""
import torch

FILLS = (0x00, 0xFF, 0x4B)
NAN_FILL = 0xFF
FLOOR = 32 << 20
_SMALL = 1 << 20         # the allocator's small pool serves requests below 1 MiB out of 2 MiB segments
_CHUNK = 1 << 19         # four of these fill a small-pool segment with no remainder
_SMALL_SEGMENTS = 8


def _inactive(pool):
    """Ascending sizes of the free blocks of this device's ``pool`` ('small' / 'large') segments."""
    dev = torch.cuda.current_device()
    return sorted(b["size"] for s in torch.cuda.memory_snapshot()
                  if s["device"] == dev and s["segment_type"] == pool for b in s["blocks"] if b["state"] == "inactive")


def poison(byte: int, nbytes: int = FLOOR) -> None:
    """After this call every free block of the caching allocator holds ``byte``: the remnants of the segments that live
    tensors pin (empty_cache cannot release those), a fresh large-pool block of ``nbytes`` and fresh small-pool segments.
    The next torch.empty / at::empty of up to ``nbytes`` in total reads back as ``byte``."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held = []

    def fill(n):
        held.append(torch.full((n,), byte, dtype=torch.uint8, device="cuda"))

    # large-pool remnants: best fit hands the block of exactly the size asked for (ascending, so ties resolve)
    for size in _inactive("large"):
        fill(size)
    # small-pool remnants: for every chunk size c as many requests as the free blocks hold whole chunks of c; each
    # request takes exactly c out of a free block (the small pool always splits), so none opens a new segment
    c = _CHUNK
    while c >= 512:
        for _ in range(sum(s // c for s in _inactive("small"))):
            fill(c)
        c >>= 1
    fill(max(int(nbytes), FLOOR))
    for _ in range(4 * _SMALL_SEGMENTS):
        fill(_CHUNK)
    torch.cuda.synchronize()
    del held


def peak_bytes(fn) -> int:
    """Peak of the bytes ``fn()`` allocates above what is live before it, measured on an unpoisoned call."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return max(int(peak), 0)


def _segments() -> int:
    return torch.cuda.memory_stats().get("segment.all.allocated", 0)


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _where(a, b, row_splits, col_block):
    """The first differing element of two equal-shape tensors, as text: rows / columns, the sequence when
    ``row_splits`` (cu_seqlens as a list, rows on dim 0) is given, the head when ``col_block`` (head_dim) is."""
    d = (bits(a) != bits(b))
    if a.dim() == 0:
        return "scalar differs"
    d2 = d.reshape(d.shape[0], -1)
    rows = d2.any(1).nonzero().flatten()
    r = int(rows[0])
    cols = d2[r].nonzero().flatten()
    txt = (f"{int(d2.sum())} of {d2.numel()} elements differ in {rows.numel()} rows; first rows {rows[:8].tolist()}, "
           f"row {r}: {cols.numel()} columns from {int(cols[0])} to {int(cols[-1])}")
    if row_splits is not None:
        seq = [i for i, (s, t) in enumerate(zip(row_splits[:-1], row_splits[1:])) if s <= r < t]
        txt += f"; sequence {seq[0]} row {r - row_splits[seq[0]]}" if seq else "; past the last sequence"
    if col_block:
        txt += f"; head {int(cols[0]) // col_block}"
    return txt


def assert_fill_independent(fn, what: str, row_splits=None, col_block: int = 0, takes_poison: bool = False):
    """``fn()`` (no input building, no allocation of inputs) returns a tuple of every tensor the op returns or modifies
    in place. It runs under each of FILLS, poisoned at twice its measured peak (at least 32 MiB); the three results must
    be bit-for-bit equal and the NaN fill's result has no NaN where the zero fill's has none. Every pass's result is
    copied before the next pass runs, so fn may hand back the same in-place buffer each time. Returns the NaN fill's
    result for a reference check by the caller. ``takes_poison``: fn takes one argument, a callable that poisons again
    with the pass's fill (between a forward and its backward)."""
    call = (lambda again: fn(again)) if takes_poison else (lambda again: fn())
    nbytes = max(2 * peak_bytes(lambda: call(lambda: None)), FLOOR)
    res = {}
    for byte in FILLS:
        poison(byte, nbytes)
        seg = _segments()
        out = call(lambda: poison(byte, nbytes))
        torch.cuda.synchronize()
        # a buffer taken from a fresh segment (straight from the driver) would not have been poisoned
        assert takes_poison or _segments() == seg, f"{what}: the op outgrew the {nbytes} poisoned bytes"
        # copies: an in-place target is the same buffer in every pass, and the next pass overwrites it
        res[byte] = tuple(t.clone() for t in (out if isinstance(out, (tuple, list)) else (out,)))
        del out
    base = res[FILLS[0]]
    for byte in FILLS[1:]:
        assert len(res[byte]) == len(base), what
        for i, (a, b) in enumerate(zip(base, res[byte])):
            assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape)
            if a.is_floating_point():
                fresh_nan = torch.isnan(b) & ~torch.isnan(a)
                assert not fresh_nan.any(), (f"{what}: output {i} has NaN under fill 0x{byte:02X} where fill 0x00 has "
                                             f"none: " + _where(a, b, row_splits, col_block))
            assert torch.equal(bits(a), bits(b)), (f"{what}: output {i} under fill 0x{byte:02X} differs from fill 0x00: "
                                                   + _where(a, b, row_splits, col_block))
    return res[NAN_FILL]
