"""Shared by tests/test_bcres_cpu.py and tests/test_gpu_bcres.py: a restatement, in any dtype and with no code of the package,
of the residuals under boundary conditions on the x-y rim,

    r_bc(fields) = r_zero_pad(pad(f) for f in fields)[..., :, 1:-1, 1:-1],

``pad`` being ``BoundaryManager(3).pad_signal`` of the reference restated as index moves (left, right, top, bottom in
sequence, each on the result of the one before: a 'periodic' high side copies the low side's padding cell) and ``r_zero_pad``
the expression of the reference script, operator by operator, as ``F.conv3d`` / ``F.conv2d`` with zero padding.  In fp32 it
is pinned by tests/golden/bcres.npz (the reference's own pad and residual code); in fp64 it is the oracle of the GPU tests.
"""
import torch

from oracle.convops import xcorr_torch

TOL = 1e-5                      # README: "Residuals match the reference within 1e-5" of the tensor scale
SIDES = ("left", "right", "top", "bottom")
BC_KINDS = ("periodic", "dirichlet", "neumann", "outflow", "symmetric")
MIXED = {"left": ("dirichlet", 1.5), "right": ("neumann", 0.0), "top": ("neumann", 0.0), "bottom": ("periodic", 0.0)}
# a low side 'symmetric' under a high side 'periodic': the wrap lands on cell 1, which pre_bc_t cannot say
MIXED_INEXPRESSIBLE = {"left": ("symmetric", 0.0), "right": ("periodic", 0.0), "top": ("neumann", 0.0), "bottom": ("neumann", 0.0)}
KINDS_2D = ("wave", "ns_continuity", "ns_momentum", "mhd_continuity", "mhd_momentum", "mhd_energy", "mhd_induction", "mhd_gauss")
KINDS_1D = ("burgers", "advection")
FIELDS = {"wave": (0,), "ns_continuity": (0, 1), "ns_momentum": (0, 1, 2), "mhd_continuity": (0, 1, 2),
          "mhd_momentum": tuple(range(6)), "mhd_energy": tuple(range(6)), "mhd_induction": (1, 2, 4, 5), "mhd_gauss": (4, 5)}
DT, DX, DY = 0.01, 1.0 / 64, 1.0 / 48
BURGERS = (2.0 / 14, 1.25 / 9, 0.002)           # dx, dt, nu
WAVE = (0.01, 0.02, 1.0)                        # dt, dx, c
ADVECTION = (1.0, 0.005, 0.01)                  # v, dt, dx


def sides(bc, value=0.0):
    """``bc``: 'wrap', a dict side -> (type, value), or a type name for all four sides."""
    if bc == "wrap" or isinstance(bc, dict):
        return bc
    return {s: (bc, value) for s in SIDES}


def _grow(r, dim, t, v, front):
    n = r.shape[dim]
    if t == "dirichlet":
        piece = torch.full_like(r.narrow(dim, 0, 1), v)
    elif t in ("neumann", "outflow"):
        piece = r.narrow(dim, 0 if front else n - 1, 1)
    elif t == "periodic":
        piece = r.narrow(dim, n - 1 if front else 0, 1)
    elif t == "symmetric":
        piece = r.narrow(dim, 1 if front else n - 2, 1)
    else:
        raise ValueError(t)
    return torch.cat([piece, r] if front else [r, piece], dim=dim)


def pad(f, bc, nd=3):
    """One cell per side of x and y of a [BS,Nt,Nx,Ny] field (``nd == 3``), of x of a [BS,Nt,Nx] field (``nd == 2``)."""
    bc = sides(bc)
    if bc == "wrap":
        f = torch.cat([f[..., -1:], f, f[..., :1]], dim=-1)
        return f if nd == 2 else torch.cat([f[..., -1:, :], f, f[..., :1, :]], dim=-2)
    f = _grow(f, -1, *bc["left"], True)
    f = _grow(f, -1, *bc["right"], False)
    if nd == 3:
        f = _grow(f, -2, *bc["top"], True)
        f = _grow(f, -2, *bc["bottom"], False)
    return f


class Op:
    """A zero-padded cross-correlation with a caller's kernel, in the dtype of the field."""

    def __init__(self, kernel):
        self.kernel = kernel

    def __call__(self, x):
        return xcorr_torch(x, self.kernel.detach().to(device=x.device, dtype=x.dtype))


def default_ops():
    """name -> Op with the kernels the package's constructors build (CPU, fp32)."""
    from cp_pre_amd import residuals as R
    ns, bu = R.NavierStokes(DT, DX, DY), R.Burgers(*BURGERS)
    ops = {n: Op(getattr(ns, n).kernel) for n in ("D_t", "D_x", "D_y", "D_xx_yy")}
    ops.update({"B_" + n: Op(getattr(bu, n).kernel) for n in ("D_t", "D_x", "D_xx")})
    ops["wave"] = Op(R.PRE_Wave(*WAVE[:2], c=WAVE[2]).D.kernel)
    ops["advection"] = Op(R.Advection(ADVECTION[0], ADVECTION[1], ADVECTION[2]).D.kernel)
    return ops


def expression(kind, ops, dtype, dt=DT, dx=DX, dy=DY, nu=0.001, gamma=5 / 3):
    """The zero-pad expression of ``kind`` as a function of its fields (the scripts' own order of evaluation)."""
    D_t, D_x, D_y, L = (ops.get(n) for n in ("D_t", "D_x", "D_y", "D_xx_yy"))
    if kind == "wave":
        return lambda u: ops["wave"](u)
    if kind == "advection":
        return lambda u: ops["advection"](u)
    if kind == "burgers":
        bdx, bdt, bnu = (torch.tensor(v, dtype=torch.float32).to(dtype) for v in BURGERS)
        return lambda u: bdx * ops["B_D_t"](u) + bdt * u * ops["B_D_x"](u) - bnu * ops["B_D_xx"](u) * (2 * bdt / bdx)
    if kind == "ns_continuity":
        return lambda u, v: D_x(u) + (dx / dy) * D_y(v)
    if kind == "mhd_gauss":
        return lambda Bx, By: D_x(Bx) + D_y(By)
    if kind == "ns_momentum":
        def f(u, v, p):
            res_x = D_t(u)*dx*dy + u*D_x(u)*dt*dy + v*D_y(u)*dt*dx - nu*L(u)*dt + D_x(p)*dt*dy
            res_y = D_t(v)*dx*dy + u*D_x(v)*dt*dx + v*D_y(v)*dt*dy - nu*L(v)*dt + D_y(p)*dt*dx
            return res_x + res_y
        return f
    if kind == "mhd_continuity":
        return lambda rho, u, v: D_t(rho) + u*D_x(rho) + rho*D_x(u) + v*D_y(rho) + rho*D_y(v)
    if kind == "mhd_momentum":
        def f(rho, u, v, p, Bx, By):
            res_x = D_t(u) + u*D_x(u) + (1/rho)*D_x(p) - 2*(Bx/rho)*D_x(Bx) + v*D_y(u) - (By/rho)*D_y(Bx) - (Bx/rho)*D_y(By)
            res_y = D_t(v) + u*D_x(v) + (1/rho)*D_y(p) - 2*(By/rho)*D_y(By) + v*D_y(v) - (By/rho)*D_x(Bx) - (Bx/rho)*D_x(By)
            return res_x + res_y
        return f
    if kind == "mhd_energy":
        def f(rho, u, v, p, Bx, By):
            p_gas = p - 0.5*(Bx**2 + By**2)
            return (D_t(rho) + u*D_x(p) + v*D_y(p) + (gamma-2)*(u*Bx+v*By)*(D_x(Bx) + D_y(By))
                    + (gamma*p_gas+By**2)*D_x(u) + (gamma*p_gas+Bx**2)*D_y(v) - Bx*By*(D_y(u) + D_x(v)))
        return f
    if kind == "mhd_induction":
        def f(u, v, Bx, By):
            res_x = D_t(Bx) - By*D_y(u) + Bx*D_y(v) - v*D_y(Bx) + u*D_y(By)
            res_y = D_t(By) + By*D_x(u) - Bx*D_x(v) - v*D_x(Bx) + u*D_x(By)
            return res_x + res_y
        return f
    raise KeyError(kind)


def residual(kind, vars, bc, dtype=torch.float32, ops=None, boundary=True, padder=pad):
    """``kind`` of ``vars`` ([BS,F,Nt,Nx,Ny]; the 1-D kinds: [BS,Nt,Nx]) under ``bc``, computed in ``dtype`` on vars' device."""
    ops = ops or default_ops()
    nd = 2 if kind in KINDS_1D else 3
    fields = [vars.to(dtype)] if nd == 2 else [vars[:, i].to(dtype) for i in FIELDS[kind]]
    r = expression(kind, ops, dtype)(*[padder(f, bc, nd) for f in fields])
    r = r[..., 1:-1, 1:-1] if nd == 3 else r[..., 1:-1]
    return r if boundary else r[:, 1:-1]


def residual64(kind, vars, bc, ops=None, boundary=True):
    return residual(kind, vars, bc, torch.float64, ops, boundary)


def err(got, want):
    """Tensor-scale error max|got - want| / max|want| (want: fp64)."""
    want = want.double().cpu()
    scale = float(want.abs().max())
    return float((got.double().cpu() - want).abs().max()) / (scale if scale > 0 else 1.0)


def make_vars(shape, seed=0):
    """U(0.5, 1.5): rho and p stay positive."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) + 0.5


def module(kind, cond=None, **kw):
    """(the package's object for ``kind``, the name of its method) with the coefficients of this file; ``cond``: its ``bc``
    (None: the constructor is called without the keyword)."""
    from cp_pre_amd import residuals as R
    extra = {} if cond is None else {"bc": cond}
    extra.update(kw)
    if kind == "wave":
        return R.PRE_Wave(*WAVE[:2], c=WAVE[2], **extra), "residual"
    if kind == "advection":
        return R.Advection(*ADVECTION, **extra), "residual"
    if kind == "burgers":
        return R.Burgers(*BURGERS, **extra), "residual"
    if kind.startswith("ns_"):
        return R.NavierStokes(DT, DX, DY, **extra), "residual_" + kind[3:]
    return R.MHD(**extra), "residual_" + kind[4:]


def call(kind, vars, bc=None, ctor=None, **kw):
    """The package's residual of ``kind``: ``vars`` [BS,F,Nt,Nx,Ny] (all six fields for MHD, the first three for NS; the wave
    takes field 0) or [BS,Nt,Nx]."""
    obj, name = module(kind, bc, **(ctor or {}))
    return getattr(obj, name)(package_input(kind, vars), **kw)


def package_input(kind, vars):
    if kind in KINDS_1D:
        return vars
    if kind == "wave":
        return vars[:, 0]
    return vars


def with_torch_ops(obj):
    """Replace the HIP operators of a package object by ``Op`` (torch) on the same kernels: the composed route then runs on a
    host without a device."""
    for n in ("D_t", "D_x", "D_y", "D_xx_yy", "D_xx", "D"):
        if hasattr(obj, n) and hasattr(getattr(obj, n), "kernel"):
            setattr(obj, n, Op(getattr(obj, n).kernel))
    return obj
