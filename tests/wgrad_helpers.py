"""Helpers shared by tests/test_wgrad_cpu.py and tests/test_gpu_wgrad.py: the gradient of the residual losses with respect to
a trainable operator kernel (``wgrad=True`` / ``kernel_vjp`` of cp_pre_amd.losses, csrc/loss_wgrad.hip).

``geometry`` restates the tile, t-segment, flush and grid rule written in the header of csrc/loss_wgrad.hip; the seams of the
GPU tests and their error bound are taken from it.  ``ref_dk`` is the float64 reference: one masked shifted inner product per
tap (tests/test_wgrad_cpu.py pins it against ``F.conv3d`` / ``F.conv2d`` autograd in float64)."""
import itertools

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------ the rule of csrc/loss_wgrad.hip, restated
FLUSH_PLANES = 8                 # WG_FLUSH_PLANES
L = 4 * FLUSH_PLANES             # products an fp32 accumulator takes between two flushes, at most
MIN_UNITS, MIN_TSEG, MAX_BLOCKS, NARROW_Y = 1024, 8, 2048, 32
WORKSPACE = 27 * MAX_BLOCKS      # PRE_WGRAD_WORKSPACE
EPS = 2.0 ** -24
# Per tap, |dk - dk64| <= BOUND_FACTOR * S with S = |scale| * sum m |g| |x - y| over the shifted cells (float64):
#   L roundings of the fp32 accumulator between two flushes (fma: the product is not rounded), each at most 2^-24 of the
#   running sum's magnitude <= the run's share of S;  1 for the fp32 subtraction x - y on load;  1 for the one rounding of
#   the result to fp32;  2 more cover the second-order terms and the fp64 additions and scale (2^-53 each).
BOUND_FACTOR = (L + 4) * EPS


def geometry(B, T, X, Y):
    """dict(rows, cols, tilesR, tilesC, tSeg, nSeg, units, grid, batch_extent) for the KERNEL's axes (T marched, Y unit
    stride).  ``batch_extent``: the samples one sweep of the grid covers."""
    rows, cols = (32, 32) if Y <= NARROW_Y else (16, 64)
    tr, tc = -(-X // rows), -(-Y // cols)
    tseg = T
    while B * tr * tc * -(-T // tseg) < MIN_UNITS and tseg > MIN_TSEG:
        tseg = (tseg + 1) // 2
    nseg = -(-T // tseg)
    units = B * tr * tc * nseg
    return dict(rows=rows, cols=cols, tilesR=tr, tilesC=tc, tSeg=tseg, nSeg=nseg, units=units, grid=min(units, MAX_BLOCKS),
                batch_extent=MAX_BLOCKS // (tr * tc * nseg))


BASE = (2, 6, 10, 16)
# (B, T, X, Y) in the kernel's axes, by the seam they cross
SEAM_SHAPES = {
    "base": BASE,
    **{"Y=%d" % y: (2, 6, 10, y) for y in (1, 3, 4, 5, 32, 33, 36, 64, 65, 68)},      # quad tails; narrow / wide column tile, +1, +4
    **{"X=%d" % x: (2, 6, x, 16) for x in (1, 2, 32, 33)},                            # narrow tile: 32 rows, +1
    **{"X=%d,wide" % x: (2, 6, x, 40) for x in (16, 17)},                             # wide tile: 16 rows, +1
    **{"T=%d" % t: (2, t, 10, 16) for t in (1, 2, 3, 8, 9)},                          # 8: one t segment; 9: segments of 5 + 4
    "batch": (MAX_BLOCKS + 1, 6, 10, 16),                                             # one more than the grid's batch extent
    "flush": (1024, 12, 3, 4),                                                        # a segment of 12 planes: flushes after 8
}


def mask(shape, crop_axes):
    """float64 0/1 mask of [B,*ext]: 0 on the first and last cell of every axis in ``crop_axes`` (1-based axes of shape)"""
    m = torch.ones(shape, dtype=torch.float64)
    for ax in crop_axes:
        idx = [slice(None)] * len(shape)
        for edge in (0, shape[ax] - 1):
            idx[ax] = edge
            m[tuple(idx)] = 0
    return m


def ref_dk(g, x, y, ext, crop, scale=1.0):
    """(dk64, S): dk64[k] = scale * sum_c m_c g_c (x - y)_{c + k - ext//2} (zero padding) and S[k] = |scale| * the same sum
    of absolute values, in float64.  g, x, y: CPU tensors [B,*n] (y may be None); ``crop``: mask the rim of every axis."""
    nd = len(ext)
    n = tuple(x.shape[1:])
    z = x.double() if y is None else x.double() - y.double()
    mg = g.double()
    if crop:                                            # (a select, as the kernel's: a non-finite g in the rim is dropped)
        mg = torch.where(mask(tuple(g.shape), range(1, nd + 1)) > 0, mg, torch.zeros((), dtype=torch.float64))
    pad = []
    for e in reversed(ext):
        pad += [e // 2, e // 2]
    zp = F.pad(z, pad)
    dk, S = torch.zeros(ext, dtype=torch.float64), torch.zeros(ext, dtype=torch.float64)
    for idx in itertools.product(*[range(e) for e in ext]):
        sl = (slice(None),) + tuple(slice(i, i + m) for i, m in zip(idx, n))
        dk[idx] = scale * (mg * zp[sl]).sum()
        S[idx] = abs(scale) * (mg.abs() * zp[sl].abs()).sum()
    return dk, S


def worst_ratio(dk, dk64, S):
    """max over taps of |dk - dk64| / (BOUND_FACTOR * S); a tap with S == 0 must be exactly 0 (ratio inf if it is not)"""
    err = (dk.detach().cpu().double() - dk64).abs()
    zero = S == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (BOUND_FACTOR * S[~zero])).max())


def inputs(shape, seed=0, with_y=True):
    """(g, x, y) float32 CPU tensors of ``shape``: g standard normal, x and y in [0.5, 1.5)"""
    gen = torch.Generator().manual_seed(1000 * seed + sum(shape))
    g = torch.randn(shape, generator=gen)
    x = torch.rand(shape, generator=gen) + 0.5
    y = torch.rand(shape, generator=gen) + 0.5 if with_y else None
    return g, x, y
