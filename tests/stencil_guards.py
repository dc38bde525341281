"""Helpers of the guard-band and non-finite-footprint tests (test_guards_cpu.py, test_gpu_guards.py, test_gpu_footprint.py).

Guard bands: a view is laid inside a larger allocation the test owns, with a band of at least four plane pitches plus
four rows (rounded up to whole quads) before and after it and whatever gaps its pitches leave between rows / planes.  No
tap reaches further than three cells along an axis, so a kernel that loads a neighbour it should have taken from the
zero padding reads the band - owned memory - and the test sees it as a result that changes with the band's contents.

Footprints: from the dense operator kernel and the positions of the non-finite input cells, by index arithmetic alone,
the set of output cells that MUST be non-finite (a non-zero tap lies on a bad cell) and the set that MAY be (a tap of
the kernel's full extent box, zero or not, lies on one: where the reference's dense conv can produce 0 * inf).
"""
import numpy as np
import torch

PATTERN = 0x5A5AC3C3            # what an output allocation is filled with (compared as int32; as a float it is ~1.5e16)
POISONS = (float("nan"), 0.0, 1e30)


def _strides(shape, order, gaps):
    """Element strides of ``shape`` laid out with the axes ``order`` (slowest first); ``gaps[axis]`` extra elements are
    added to that axis' stride (a pitched row / plane / sample; on the fastest axis: a view with no unit stride)."""
    order = list(range(len(shape))) if order is None else list(order)
    assert sorted(order) == list(range(len(shape)))
    gaps = gaps or {}
    strides, acc = [0] * len(shape), 1
    for d in reversed(order):
        strides[d] = acc + gaps.get(d, 0)
        acc = strides[d] * shape[d]
    return strides, acc


def guard_elems(shape, strides):
    """Four plane pitches + four row pitches + four cells of the view, whole quads: the largest three strides of the grid
    axes (every axis but the batch) are the plane, row and cell pitch whatever the memory order."""
    grid = sorted((s for s in strides[1:]), reverse=True)[:3]
    return (4 * sum(grid) + 3) // 4 * 4 + 4


def guarded(shape, order=None, gaps=None, offset=0, device="cpu", dtype=torch.float32):
    """(allocation, view): a 1-D allocation and a ``shape`` view inside it, ``guard_elems`` + ``offset`` elements from its
    start (``offset`` = 1 puts the base 4 bytes off a 16-byte boundary) and ``guard_elems`` before its end."""
    strides, _ = _strides(shape, order, gaps)
    span = 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if all(shape) else 0
    g = guard_elems(shape, strides)
    alloc = torch.zeros(g + offset + span + g, dtype=dtype, device=device)
    return alloc, alloc.as_strided(tuple(shape), tuple(strides), g + offset)


def outside_mask(alloc, *views):
    """bool [alloc.numel()]: True where no element of any of ``views`` (views of ``alloc``) lies."""
    inside = np.zeros(alloc.numel(), bool)
    base = alloc.storage_offset()
    for v in views:
        idx = np.full((), v.storage_offset() - base, np.int64)
        for n, s in zip(v.shape, v.stride()):
            idx = idx[..., None] + np.arange(n, dtype=np.int64) * s
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < alloc.numel()), "view outside its allocation"
        inside[idx.reshape(-1)] = True
    return torch.from_numpy(~inside).to(alloc.device)


def poison(alloc, mask, value):
    alloc.masked_fill_(mask, value)


def guarded_out(shape, order=None, gaps=None, offset=0, device="cpu"):
    """(allocation, view, mask): an output view in an allocation filled with PATTERN; ``mask`` = ``outside_mask``."""
    alloc, view = guarded(shape, order, gaps, offset, device)
    alloc.view(torch.int32).fill_(PATTERN)
    return alloc, view, outside_mask(alloc, view)


def untouched(alloc, mask):
    """True if every bit of ``alloc`` under ``mask`` still holds PATTERN."""
    return bool((alloc.view(torch.int32)[mask] == PATTERN).all())


def memory_order(view):
    """The axes of ``view``, slowest in memory first (``order`` of ``guarded`` for an output laid out like ``view``)."""
    return sorted(range(view.dim()), key=lambda d: (-view.stride(d), d))


def bits(t):
    """The fp32 bits of ``t`` in logical order, as an int32 device tensor (bit-for-bit comparisons that NaN does not break)."""
    return t.contiguous().view(torch.int32).clone()


def embed(x, order=None, gaps=None, offset=0, device="cpu"):
    """(allocation, view) with ``view`` holding the values of the CPU tensor ``x``."""
    alloc, view = guarded(tuple(x.shape), order, gaps, offset, device)
    view.copy_(x.to(device))
    return alloc, view


def three_ways(alloc, owned, run):
    """Run ``run()`` with everything of ``alloc`` outside the views ``owned`` set to NaN, 0.0 and 1e30 in turn (the same
    allocation and views: the same launch); assert the three results bit-identical and return the last."""
    mask = outside_mask(alloc, *owned)
    seen, last = [], None
    for value in POISONS:
        poison(alloc, mask, value)
        last = run()
        seen.append(bits(last))
    assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]), \
        "the result depends on memory outside the view (NaN / 0.0 / 1e30 around it give different bits)"
    return last


# ------------------------------------------------------------------------------------------------ footprints
def footprint(kernel, bad):
    """(must, may) bool arrays of ``bad``'s shape [B, *grid] for the zero-padded cross-correlation with the dense
    ``kernel`` (one axis per grid axis, odd extents): ``must`` - a NON-ZERO tap of the output cell lies on a bad input cell;
    ``may`` - some tap of the kernel's extent box (|offset| <= k//2 per axis) does."""
    kernel = np.asarray(kernel)
    bad = np.asarray(bad, bool)
    assert kernel.ndim == bad.ndim - 1 and all(k % 2 for k in kernel.shape)
    must, may = np.zeros_like(bad), np.zeros_like(bad)
    grid = bad.shape[1:]
    for idx in np.ndindex(*kernel.shape):
        off = [i - k // 2 for i, k in zip(idx, kernel.shape)]          # out[o] += k[idx] * in[o + off]
        if any(abs(o) >= n for o, n in zip(off, grid)):
            continue
        dst = (slice(None),) + tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, grid))
        src = (slice(None),) + tuple(slice(max(0, o), n + min(0, o)) for o, n in zip(off, grid))
        may[dst] |= bad[src]
        if kernel[idx] != 0:
            must[dst] |= bad[src]
    return must, may


def footprint_union(terms):
    """Footprint of an expression of several operators: ``terms`` = [(dense kernel, bad mask of the field it is applied
    to), ...]; a field used pointwise enters with a 1x..x1 kernel [[[1.]]]."""
    must = may = None
    for k, bad in terms:
        a, b = footprint(k, bad)
        must, may = (a, b) if must is None else (must | a, may | b)
    return must, may


def bad_positions(grid, extra=()):
    """Cells of a [*grid] box: the centre, every corner, one cell on every face and edge (all index combinations of
    {0, mid, last} per axis), plus ``extra``; duplicates (extents 1, 2) removed."""
    per_axis = [sorted({0, n // 2, n - 1}) for n in grid]
    cells = {tuple(c) for c in np.stack(np.meshgrid(*per_axis, indexing="ij"), -1).reshape(-1, len(grid)).tolist()}
    cells |= {tuple(e) for e in extra if all(0 <= i < n for i, n in zip(e, grid))}
    return sorted(cells)


def check_sandwich(got, oracle_clean, must, may, tol, lone_nan=False):
    """Assert the two-sided contract on ``got`` (numpy): non-finite on ``must`` (NaN for a lone NaN), finite and equal to
    ``oracle_clean`` (the float64 oracle of the field with the bad cells replaced by finite values) off ``may``."""
    got = np.asarray(got)
    if lone_nan:
        assert np.isnan(got[must]).all(), "a NaN input under a non-zero tap did not reach the output as NaN"
    else:
        assert (~np.isfinite(got[must])).all(), "a non-finite input under a non-zero tap was hidden"
    clean = ~may
    leaked = clean & ~np.isfinite(got)
    assert not leaked.any(), f"a non-finite value leaked beyond the kernel's extent box, e.g. at {np.argwhere(leaked)[:4].tolist()}"
    if clean.any():
        ref = np.asarray(oracle_clean, np.float64)
        scale = np.max(np.abs(ref))                                     # tensor-scale, as conftest.rel_err
        err = np.max(np.abs(got[clean].astype(np.float64) - ref[clean])) / (scale if scale > 0 else 1.0)
        assert err <= tol, f"cells outside the footprint differ from the oracle: rel err {err:.3e}"
