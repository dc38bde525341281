"""Test infrastructure for the fused backward of the ideal-MHD residual losses (``mhd=True`` of cp_pre_amd.losses,
libcp_pre_vjpmhd.so, include/cp_pre_vjpmhd.h).

``MHDRoute`` is the counterpart of ``losses_helpers.Route`` for the five MHD equations: the composed expressions restated
ONCE in terms of ``D(f, k)`` from the float32 taps the operator objects hold now, so that ``losses_helpers.ref64`` /
``ref_vjp`` / ``ref_loss`` / ``seam_inputs`` take it as they take a ``Route``.  fp64 autograd through it is the reference
of every test.  ``closed_form`` is a literal restatement of the header's formulas with shifted adds.

Tolerance: the project's TOL = 1e-5 (tests/LOSSES_TESTS.md), tensor-scale relative error overall and per gradient channel.
"""
import torch

from losses_helpers import SEAM_SHAPES, Dshift, asym_star

TOL = 1e-5
EQS = ("continuity", "induction", "momentum", "energy", "gauss")
CHAN = {"continuity": (0, 1, 2), "induction": (1, 2, 4, 5), "momentum": tuple(range(6)), "energy": tuple(range(6)),
        "gauss": (4, 5)}
KIND = {"continuity": "mhd_continuity", "induction": "mhd_induction", "momentum": "mhd_momentum", "energy": "mhd_energy",
        "gauss": "linear2"}
# default: the reference's construction (MODE 0 of the march: D_t and D_y along Nt); yfix: D_y along Ny (MODE 1); rescaled:
# the default set with every .kernel multiplied by its own factor after construction (D_y is no longer D_t: a stale or
# swapped tap shows); stars: every operator a general asymmetric star (MODE 2: built for momentum only)
OPSETS = ("default", "yfix", "rescaled")
RESCALE = {"D_t": 1.25, "D_x": 0.75, "D_y": 1.5}
DEGENERATE = [(1, 1, 1, 1), (1, 3, 3, 3), (2, 3, 3, 4)]


class MHDRoute:
    """One MHD equation on one operator set: ``method`` (what ``cp_pre_amd.losses`` takes), ``ops`` (D_t, D_x, D_y: their
    CURRENT ``.kernel`` is read at every call), ``chan`` the channels it reads, ``kind`` its fused kind."""
    nd, nchan = 3, 6

    def __init__(self, eq, opset="default", device="cpu", pre=False):
        from cp_pre_amd import residuals as R
        self.eq, self.opset, self.name = eq, opset, "mhd_%s_%s" % (eq, opset)
        kw = dict(device=device, y_axis_fix=(opset == "yfix"))
        self.obj = o = R.PRE_MHD(0.01, 1 / 64, 1 / 32, **kw) if pre else R.MHD(**kw)
        self.ops = (o.D_t, o.D_x, o.D_y)
        if opset == "rescaled":
            for a, s in RESCALE.items():
                getattr(o, a).kernel = getattr(o, a).kernel * s
        elif opset == "stars":
            for i, op in enumerate(self.ops):
                op.kernel = (asym_star(3) * (1.0 + 0.25 * i)).to(device)
        self.method = o.residual if pre else getattr(o, "residual_" + eq)
        self.chan, self.kind = CHAN[eq], KIND[eq]

    def input_shape(self, s):
        return (s[0], self.nchan) + tuple(s[1:])

    def kernels(self, dtype):
        return tuple(o.kernel.detach().cpu().to(dtype) for o in self.ops)

    def has_t_taps(self):
        ks = self.kernels(torch.float32)
        return any(bool(k[0].any() or k[2].any()) for k in (ks[1:] if self.eq == "gauss" else ks))

    def full(self, x, D=Dshift):
        """The uncropped residual of ``x`` [BS,F>=6,Nt,Nx,Ny] in ``x``'s dtype: Marginal/MHD_Residuals_CP.py:225-278."""
        Kt, Kx, Ky = self.kernels(x.dtype)
        gamma = float(self.obj.gamma)
        rho, u, v, p, Bx, By = (x[:, i] for i in range(6))
        Dt, Dx, Dy = (lambda f: D(f, Kt)), (lambda f: D(f, Kx)), (lambda f: D(f, Ky))
        if self.eq == "continuity":
            return Dt(rho) + u*Dx(rho) + rho*Dx(u) + v*Dy(rho) + rho*Dy(v)
        if self.eq == "momentum":
            rx = Dt(u) + u*Dx(u) + (1/rho)*Dx(p) - 2*(Bx/rho)*Dx(Bx) + v*Dy(u) - (By/rho)*Dy(Bx) - (Bx/rho)*Dy(By)
            ry = Dt(v) + u*Dx(v) + (1/rho)*Dy(p) - 2*(By/rho)*Dy(By) + v*Dy(v) - (By/rho)*Dx(Bx) - (Bx/rho)*Dx(By)
            return rx + ry
        if self.eq == "energy":
            pg = p - 0.5*(Bx**2 + By**2)
            return (Dt(rho) + u*Dx(p) + v*Dy(p) + (gamma-2)*(u*Bx+v*By)*(Dx(Bx) + Dy(By))
                    + (gamma*pg+By**2)*Dx(u) + (gamma*pg+Bx**2)*Dy(v) - Bx*By*(Dy(u) + Dx(v)))
        if self.eq == "induction":
            rx = Dt(Bx) - By*Dy(u) + Bx*Dy(v) - v*Dy(Bx) + u*Dy(By)
            ry = Dt(By) + By*Dx(u) - Bx*Dx(v) - v*Dx(Bx) + u*Dx(By)
            return rx + ry
        return Dx(Bx) + Dy(By)                                       # gauss

    def residual(self, x, boundary, D=Dshift):
        r = self.full(x, D)
        return r if boundary else r[(Ellipsis,) + (slice(1, -1),) * 3]


def closed_form(route, x, gfull):
    """The formulas of include/cp_pre_vjpmhd.h, literally, with shifted adds in ``x``'s dtype: ``gfull`` [BS,Nt,Nx,Ny] is the
    gradient arriving at the UNCROPPED residual (zero on the rim under the crop).  Returns [BS,F,Nt,Nx,Ny]."""
    Kt, Kx, Ky = route.kernels(x.dtype)
    flip = lambda k: torch.flip(k, (0, 1, 2))                      # noqa: E731
    Dt_T = lambda f: Dshift(f, flip(Kt))                           # noqa: E731
    Dx, Dy = (lambda f: Dshift(f, Kx)), (lambda f: Dshift(f, Ky))
    DxT, DyT = (lambda f: Dshift(f, flip(Kx))), (lambda f: Dshift(f, flip(Ky)))
    M, P = (lambda f: Dshift(f, Kx - Ky)), (lambda f: Dshift(f, Kx + Ky))
    MT, PT = (lambda f: Dshift(f, flip(Kx - Ky))), (lambda f: Dshift(f, flip(Kx + Ky)))
    g = gfull.to(x.dtype)
    rho, u, v, p, Bx, By = (x[:, i] for i in range(6))
    out = torch.zeros_like(x)
    gamma = float(route.obj.gamma)
    k = gamma - 2
    if route.eq == "continuity":
        out[:, 0] = Dt_T(g) + DxT(g*u) + DyT(g*v) + g*(Dx(u) + Dy(v))
        out[:, 1] = g*Dx(rho) + DxT(g*rho)
        out[:, 2] = g*Dy(rho) + DyT(g*rho)
    elif route.eq == "induction":
        out[:, 1] = MT(g*By) + g*P(By)
        out[:, 2] = -MT(g*Bx) - g*P(Bx)
        out[:, 4] = Dt_T(g) - g*M(v) - PT(g*v)
        out[:, 5] = Dt_T(g) + g*M(u) + PT(g*u)
    elif route.eq == "momentum":
        q = 1/rho
        sx, sy = 2*Dx(Bx) + P(By), 2*Dy(By) + P(Bx)
        S, T = Bx*sx + By*sy, Dt_T(g) + DxT(g*u) + DyT(g*v)
        out[:, 1] = T + g*Dx(u + v)
        out[:, 2] = T + g*Dy(u + v)
        out[:, 0] = -g*q*q*(P(p) - S)
        out[:, 3] = PT(g*q)
        out[:, 4] = -(g*q*sx + 2*DxT(g*q*Bx) + PT(g*q*By))
        out[:, 5] = -(g*q*sy + 2*DyT(g*q*By) + PT(g*q*Bx))
    elif route.eq == "energy":
        pg = p - 0.5*(Bx*Bx + By*By)
        A, C, E, W = gamma*pg + By*By, gamma*pg + Bx*Bx, Bx*By, u*Bx + v*By
        dv, sh = Dx(Bx) + Dy(By), Dy(u) + Dx(v)
        out[:, 0] = Dt_T(g)
        out[:, 1] = g*(Dx(p) + k*Bx*dv) + DxT(g*A) - DyT(g*E)
        out[:, 2] = g*(Dy(p) + k*By*dv) + DyT(g*C) - DxT(g*E)
        out[:, 3] = DxT(g*u) + DyT(g*v) + gamma*g*(Dx(u) + Dy(v))
        out[:, 4] = k*(g*u*dv + DxT(g*W)) + g*(Bx*((2 - gamma)*Dy(v) - gamma*Dx(u)) - By*sh)
        out[:, 5] = k*(g*v*dv + DyT(g*W)) + g*(By*((2 - gamma)*Dx(u) - gamma*Dy(v)) - Bx*sh)
    else:
        out[:, 4], out[:, 5] = DxT(g), DyT(g)
    return out


def pad_g(g, boundary, shape):
    """``g`` of the (cropped) residual as the gradient arriving at the uncropped residual [BS,Nt,Nx,Ny] = ``shape``"""
    if boundary:
        return g
    return torch.nn.functional.pad(g, (1, 1) * 3) if g.numel() else torch.zeros(shape, dtype=g.dtype)


def seam_shapes(eq, opset):
    """The shapes (BS, Nt, Nx, Ny) of one equation on one operator set: ``losses_helpers.SEAM_SHAPES`` by mechanism (the
    t-segment group of a march with t-taps, the tap-free group for gauss under y_axis_fix, where no operator has one) and
    the degenerate extents."""
    t = "tfree3d" if (eq == "gauss" and opset == "yfix") else "tseg"
    return [s for grp in (t, "narrow_x", "narrow_y", "wide_x", "wide_y", "two_seams") for s in SEAM_SHAPES[grp]] + DEGENERATE


def unread(route, nchan=6):
    return [c for c in range(nchan) if c not in route.chan]
