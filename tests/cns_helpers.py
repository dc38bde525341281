"""Test infrastructure for ``cp_pre_amd.cns``: the right-hand side of ``Active_Learning/CNS.py:18-31`` restated on
``oracle.spatial.VectorOp`` (the pinned restatement of the reference's spatial operators), in fp32 and in fp64, for
arbitrary per-side boundary conditions and arbitrary operator kernels.  The fp64 form is the reference of the GPU tests;
``tests/test_cns_cpu.py`` pins the fp32 form to ``tests/golden/cns.npz``, which the reference's own ``forward`` produced.

Tolerance.  ``TOL`` = 1e-5 tensor-scale relative error ``max|a-b| / max|b|`` per output channel against fp64: the project's
residual parity bar.  Every input has ``rho, p`` in U(0.5, 1.5), so ``1/rho`` is tame; ``test_cns_cpu.py`` asserts that the
fp32 restatement alone stays within ``TOL / 4`` of fp64 at every shape the GPU tests use, so a miss belongs to the kernel.
"""
import numpy as np
import torch

from oracle.spatial import VectorOp

TOL = 1e-5
DX = 0.0078
SIDES = ("left", "right", "top", "bottom")
BC_KINDS = ("periodic", "dirichlet", "neumann", "outflow", "symmetric")
MIXED = {"left": ("dirichlet", 1.5), "right": ("neumann", 0.0), "top": ("symmetric", 0.0), "bottom": ("periodic", 0.0)}
# MIXED is the case the feature request names.  Its bottom 'periodic' under top 'symmetric' makes the last row's neighbour
# row 1 (pad_signal copies the first row of the ALREADY top-padded field), which ``vector_convops_spatial._bc_struct`` has
# no mode for: it is the rows' twin of "left symmetric under right periodic", so the fused pass declines it and the
# composed route serves it.  MIXED_FUSABLE has all four kinds, a constant reached through the 'periodic' quirk, and a mapping.
MIXED_FUSABLE = {"left": ("dirichlet", 1.5), "right": ("periodic", 0.0), "top": ("symmetric", 0.0), "bottom": ("neumann", 0.0)}
TRUE_WRAP = {"left": ("neumann", 0.0), "right": ("periodic", 0.0), "top": ("neumann", 0.0), "bottom": ("periodic", 0.0)}
KERNEL_NAMES = ("gx", "gy", "dx", "dy", "lap")


def sides(bc, value=0.0):
    """{side: (type, value)} from a name (all sides alike) or such a dict."""
    return dict(bc) if isinstance(bc, dict) else {s: (bc, value) for s in SIDES}


def default_kernels(dx=DX):
    """The five kernels the module's constructor makes (fp32), from the pinned restatement."""
    one = torch.tensor(dx, dtype=torch.float32)
    g = VectorOp("gradient", scale=float(1 / one))
    d = VectorOp("divergence", scale=float(1 / one))
    lap = VectorOp("laplace", scale=float(1 / (one ** 2)))
    return {"gx": g.gx, "gy": g.gy, "dx": d.gx, "dy": d.gy, "lap": lap.lap}


def asymmetric_kernels(seed=0):
    """Crosses with five distinct non-zero weights each; the gradient and the divergence on different scales."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, scale in zip(KERNEL_NAMES, (3.0, 5.0, 7.0, 11.0, 40.0)):
        k = np.zeros((3, 3), np.float32)
        w = scale * (rng.permutation(5) + 1.0) * rng.choice([-1.0, 1.0], 5) / 5.0
        k[1, 1], k[0, 1], k[2, 1], k[1, 0], k[1, 2] = w
        out[name] = torch.from_numpy(k)
    return out


def make_ops(kernels, bc, dtype=torch.float32, device="cpu", detach=True):
    """(gradient, divergence, laplace) as ``VectorOp`` objects holding the given kernels and per-side conditions."""
    t = sides(bc)
    ops = VectorOp("gradient"), VectorOp("divergence"), VectorOp("laplace")
    for op in ops:
        op.types = {s: t[s][0] for s in SIDES}
        op.values = {s: t[s][1] for s in SIDES}
    cast = {n: (k.detach() if detach else k).to(device=device, dtype=dtype) for n, k in kernels.items()}
    ops[0].gx, ops[0].gy = cast["gx"], cast["gy"]
    ops[1].gx, ops[1].gy = cast["dx"], cast["dy"]
    ops[2].lap = cast["lap"]
    return ops


def dot(a, b):
    return a[:, 0:1] * b[:, 0:1] + a[:, 1:2] * b[:, 1:2]


def expression(vars, gradient, divergence, laplace, gamma):
    """``Active_Learning/CNS.py:18-31`` on the restated operators, in ``vars``' dtype."""
    rho, u, v, uv, p = vars[:, 0:1], vars[:, 1:2], vars[:, 2:3], vars[:, 1:3], vars[:, 3:4]
    rhs_mass = - rho * divergence(u, v) - dot(uv, gradient(rho))
    rhs_mom = -dot(uv, gradient(u)) - dot(uv, gradient(v)) + laplace(u, v) + (1 / rho) * gradient(p)
    rhs_energy = -gamma * p * divergence(u, v) - dot(uv, gradient(rho))
    return torch.cat((rhs_mass, rhs_mom[:, 0:1], rhs_mom[:, 1:2], rhs_energy), dim=1)


def gamma32():
    return torch.tensor(5 / 3, dtype=torch.float32)


def rhs(vars, bc="periodic", kernels=None, dtype=torch.float32):
    """The right-hand side of fp32 ``vars`` (a CPU or device tensor), evaluated in ``dtype`` with the fp32 kernels and the
    fp32 gamma cast to it."""
    kernels = default_kernels() if kernels is None else kernels
    ops = make_ops(kernels, bc, dtype, vars.device)
    return expression(vars.to(dtype), *ops, gamma32().to(device=vars.device, dtype=dtype))


def rhs64(vars, bc="periodic", kernels=None):
    return rhs(vars.detach(), bc, kernels, torch.float64)


def make_vars(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32) + 0.5


def zero_scale(vars, kernels=None):
    """The scale an output channel is compared on when its fp64 reference is ZERO throughout, where ``max|a-b| / max|b|``
    is undefined.  It happens: on a 2-row grid under 'symmetric' both x-neighbours of a row are the other row, so every
    first derivative of the reference's kernels cancels exactly and the mass and energy channels are 0.  What fp32 leaves
    there is the rounding of the terms that cancel, products of a tap, a neighbour and a pointwise factor; the scale is a
    lower estimate of the largest such term: the smallest of the five kernels' largest |tap|, times max|vars|, times
    min|vars|."""
    kernels = default_kernels() if kernels is None else kernels
    tap = min(float(k.detach().abs().max()) for k in kernels.values())
    return tap * float(vars.detach().abs().max()) * float(vars.detach().abs().min())


def channel_err(a, b, zero=1.0):
    """Largest tensor-scale relative error ``max|a-b| / max|b|`` over the four output channels; a channel whose reference is
    zero throughout is compared on the scale ``zero`` (``zero_scale``)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return max(float((a[:, c] - b[:, c]).abs().max() / (b[:, c].abs().max() or zero)) for c in range(b.shape[1]))


def gpu_extents(nr, nc):
    """(row counts, column counts) of tests/test_gpu_cns.py for a tile of nr x nc: below, at and beyond every seam."""
    return (2, 3, nr - 1, nr, nr + 1, 2 * nr + 1), (4, 8, nc - 4, nc, nc + 4, 2 * nc + 4)
