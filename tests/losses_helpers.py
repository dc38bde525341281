"""Helpers shared by tests/test_losses_cpu.py and tests/test_gpu_losses.py: the zero-padded cross-correlation of the oracle
(``oracle.convops.xcorr_torch``'s arithmetic) for any dtype, its adjoint, the crop mask and the oracle's NS kernels."""
import torch
import torch.nn.functional as F

from oracle import residuals as orr


def D(f, k):
    """zero-padded cross-correlation of [B,*ext] with a 3^nd kernel (the arithmetic of oracle.convops.xcorr_torch)"""
    conv = F.conv3d if k.dim() == 3 else F.conv2d
    return conv(f.unsqueeze(1), k[None, None], padding=1).squeeze(1)


def DT_(g, k):
    """the adjoint: the same star with mirrored taps"""
    return D(g, torch.flip(k, dims=tuple(range(k.dim()))))


def _mask(shape, crop):
    m = torch.zeros(shape, dtype=torch.float64)
    if crop:
        m[(Ellipsis,) + (slice(1, -1),) * (len(shape) - 1)] = 1
    else:
        m[...] = 1
    return m


def _k64(op):
    return op.kernel.detach().double()


def ns_kernels():
    o = orr.Ops2D()
    return _k64(o.D_t), _k64(o.D_x), _k64(o.D_y), _k64(o.D_xx_yy)


# ------------------------------------------------------------------------------------------------ the fp64 reference
# Every fused route of cp_pre_amd.losses restated ONCE in terms of D(f, k), from the float32 taps the cp_pre_amd operator
# objects hold (cast to the dtype of the input) and the scalar factors as Python doubles.  The same text runs in float64
# (the reference of tests/test_gpu_losses_seams.py / test_gpu_losses_guards.py) and in float32 (the rounding a correct
# fp32 kernel may show: the headroom measured by tests/test_losses_ref_cpu.py).
ROUTE_KIND = {"op3d": "stencil3d", "op2d": "stencil2d", "wave": "stencil3d", "advection": "stencil2d",
              "ns_continuity": "linear2", "ns_momentum": "ns_momentum", "pre_ns": "ns_momentum", "burgers": "burgers",
              # y_axis_fix=True: D_y with its taps along Ny (the default, like the reference, has them along Nt), which makes
              # NS continuity free of taps along the marched axis and gives the NS functors y-neighbours of u and v
              "ns_continuity_yfix": "linear2", "ns_momentum_yfix": "ns_momentum"}
ROUTES = tuple(ROUTE_KIND)
ROUTES_3D_T = ("ns_momentum", "ns_momentum_yfix", "pre_ns", "ns_continuity", "wave", "op3d")     # a tap along the marched axis
ROUTES_2D = ("burgers", "advection", "op2d")             # [BS,Nt,Nx] views: marched along BS, never a tap there
NS_DT, NS_DX, NS_DY, NS_NU = 0.01, 1 / 64, 1 / 32, 0.001
BG_DX, BG_DT, BG_NU = 0.05, 0.01, 0.002


def Dshift(f, k):
    """D(f, k) by shifted adds over the non-zero taps (zero padding, taps added in index order): the arithmetic of ``D``
    without the im2col buffer of a float64 convolution.  tests/test_losses_ref_cpu.py holds it against ``D``."""
    nd = k.dim()
    p = F.pad(f, (1, 1) * nd)
    out = None
    for idx in torch.nonzero(k).tolist():
        sl = (slice(None),) + tuple(slice(i, i + n) for i, n in zip(idx, f.shape[1:]))
        term = k[tuple(idx)] * p[sl]
        out = term if out is None else out + term
    return torch.zeros_like(f) if out is None else out


def asym_star(nd, seed=0):
    """A 7-point (3-D) / 5-point (2-D) star whose taps are all unequal in magnitude and sign pattern: tm != tp, xm != xp,
    ym != yp, so a mirrored tap or a wrong neighbour changes the answer (fixed values, fp32-exact)."""
    k = torch.zeros((3,) * nd)
    taps3 = {(1, 1, 1): -1.75, (0, 1, 1): 0.5, (2, 1, 1): -1.25, (1, 0, 1): 0.875, (1, 2, 1): -0.375, (1, 1, 0): 1.5, (1, 1, 2): -0.625}
    taps2 = {(1, 1): -1.75, (0, 1): 0.875, (2, 1): -0.375, (1, 0): 1.5, (1, 2): -0.625}
    for idx, w in (taps3 if nd == 3 else taps2).items():
        k[idx] = w
    return k


def _skew(k):
    """``k`` plus a fixed antisymmetric weight on each of its non-zero off-centre tap pairs: a symmetric star (the wave
    kernel) gets unequal taps on every axis it has any, no tap appears or disappears."""
    k = k.clone()
    c = tuple(1 for _ in k.shape)
    for ax in range(k.dim()):
        lo, hi = list(c), list(c)
        lo[ax], hi[ax] = 0, 2
        lo, hi = tuple(lo), tuple(hi)
        if k[lo] != 0 or k[hi] != 0:
            k[lo] += 0.09375 * (ax + 1)
            k[hi] -= 0.03125 * (ax + 1)
    return k


class Route:
    """One fused route: ``method`` (what ``cp_pre_amd.losses`` takes), its operator objects ``ops`` (their CURRENT
    ``.kernel`` is read at every call), ``nd`` residual axes, ``nchan`` stacked channels (None: the input is the field)."""

    def __init__(self, name, device="cpu", asym=False):
        from cp_pre_amd import residuals as R
        from cp_pre_amd.convops_1d import ConvOperator as C1
        from cp_pre_amd.convops_2d import ConvOperator as C2
        self.name, self.kind, self.nchan, self.nd = name, ROUTE_KIND[name], None, 3
        y_axis_fix = name.endswith("_yfix")
        name = name[:-5] if y_axis_fix else name
        if name == "op3d":
            op = C2(("x", "y"), 2, device=device)
            if asym:
                op.kernel = asym_star(3).to(device)
            self.obj, self.method, self.ops = op, op, (op,)
        elif name == "op2d":
            op = C1("x", 2, device=device)
            if asym:
                op.kernel = asym_star(2).to(device)
            self.obj, self.method, self.ops, self.nd = op, op, (op,), 2
        elif name == "wave":
            self.obj = R.PRE_Wave(0.01, 0.02, device=device)
            if asym:
                self.obj.D.kernel = _skew(self.obj.D.kernel.cpu()).to(device)
            self.method, self.ops = self.obj.residual, (self.obj.D,)
        elif name == "advection":
            self.obj = R.Advection(1.0, 0.005, 0.01, device=device)
            self.method, self.ops, self.nd = self.obj.residual, (self.obj.D,), 2
        elif name in ("ns_continuity", "ns_momentum", "pre_ns"):
            kw = dict(device=device, y_axis_fix=y_axis_fix)
            self.obj = R.PRE_NS(NS_DT, NS_DX, NS_DY, **kw) if name == "pre_ns" else R.NavierStokes(NS_DT, NS_DX, NS_DY, nu=NS_NU, **kw)
            o = self.obj
            if name == "ns_continuity":
                self.method, self.ops, self.nchan = o.residual_continuity, (o.D_x, o.D_y), 2
            else:
                self.method = o.residual if name == "pre_ns" else o.residual_momentum
                self.ops, self.nchan = (o.D_t, o.D_x, o.D_y, o.D_xx_yy), 3
        elif name == "burgers":
            self.obj = R.Burgers(BG_DX, BG_DT, BG_NU, device=device)
            self.method, self.ops, self.nd = self.obj.residual, (self.obj.D_t, self.obj.D_x, self.obj.D_xx), 2
        else:
            raise KeyError(name)

    def input_shape(self, s):
        """(BS, Nt, Nx, Ny) -> the shape of the route's input: stacked [BS,F,Nt,Nx,Ny], a field [BS,Nt,Nx,Ny], or the 2-D
        view [BS*Nt,Nx,Ny] (marched along its first axis)."""
        if self.nd == 2:
            return (s[0] * s[1],) + tuple(s[2:])
        return tuple(s) if self.nchan is None else (s[0], self.nchan) + tuple(s[1:])

    def kernels(self, dtype):
        return tuple(o.kernel.detach().cpu().to(dtype) for o in self.ops)

    def has_t_taps(self):
        return self.nd == 3 and any(bool(k[0].any() or k[2].any()) for k in self.kernels(torch.float32))

    def full(self, x, D=Dshift):
        """The uncropped residual of ``x`` in ``x``'s dtype."""
        ks, o = self.kernels(x.dtype), self.obj
        if self.kind in ("stencil3d", "stencil2d"):
            return D(x[:, 0] if x.dim() == self.nd + 2 else x, ks[0])
        if self.kind == "linear2":
            return D(x[:, 0], ks[0]) + (o.dx / o.dy) * D(x[:, 1], ks[1])
        if self.kind == "ns_momentum":
            Kt, Kx, Ky, KL = ks
            dt, dx, dy, nu = float(o.dt), float(o.dx), float(o.dy), float(o.nu)
            u, v, p = x[:, 0], x[:, 1], x[:, 2]
            rx = D(u, Kt)*dx*dy + u*D(u, Kx)*dt*dy + v*D(u, Ky)*dt*dx - nu*D(u, KL)*dt + D(p, Kx)*dt*dy
            ry = D(v, Kt)*dx*dy + u*D(v, Kx)*dt*dx + v*D(v, Ky)*dt*dy - nu*D(v, KL)*dt + D(p, Ky)*dt*dx
            return rx + ry
        Kt, Kx, Kxx = ks                                           # burgers (the coefficients are fp32 0-d tensors: exact in double)
        dx, dt, nu = float(o.dx), float(o.dt), float(o.nu)
        return dx*D(x, Kt) + dt*x*D(x, Kx) - nu*D(x, Kxx)*(2*dt/dx)

    def residual(self, x, boundary, D=Dshift):
        r = self.full(x, D)
        return r if boundary else r[(Ellipsis,) + (slice(1, -1),) * self.nd]


def ref64(route, x64, boundary, D=Dshift):
    """The residual of route ``route`` (a ``Route`` or its name) in the dtype of ``x64``."""
    route = Route(route) if isinstance(route, str) else route
    return route.residual(x64, boundary, D)


def ref_vjp(route, x, g, boundary):
    """d <g, residual(x)> / dx by autograd of ``ref64`` in ``x``'s dtype (float64: the reference)."""
    x = x.detach().clone().requires_grad_(True)
    y = ref64(route, x, boundary)
    if y.numel() == 0:
        return torch.zeros_like(x)
    y.backward(g.to(x.dtype))
    return x.grad


def ref_loss(route, x, boundary, yy=None, upstream=1.0):
    """(value, gradient) of ``upstream * mean((r(x) - r(yy))^2)`` by autograd in ``x``'s dtype; the mean is taken in
    float64 whatever the dtype (as ``pre_vjp_sumsq_f32`` does)."""
    x = x.detach().clone().requires_grad_(True)
    r = ref64(route, x, boundary)
    if yy is not None:
        r = r - ref64(route, yy.detach(), boundary)
    loss = r.double().pow(2).mean()
    (upstream * loss).backward()
    return float(loss.detach()), x.grad


def seam_inputs(route, shape, boundary, seed=0):
    """(x, g) float32 CPU inputs of one case: fields in [0.5, 1.5), g standard normal of the residual's shape."""
    gen = torch.Generator().manual_seed(1000 * seed + sum(shape))
    x = torch.rand(route.input_shape(shape), generator=gen) + 0.5
    rs = x.shape if route.nchan is None else (x.shape[0],) + tuple(x.shape[2:])
    if not boundary:
        rs = rs[:1] + tuple(max(n - 2, 0) for n in rs[1:])
    return x, torch.randn(rs, generator=gen)


def channel_errs(got, want):
    """{'all': tensor-scale rel err, per channel of a stacked gradient: the same against that channel's own scale}"""
    import numpy as np

    def rel(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        d = np.max(np.abs(b)) if b.size else 0.0
        return float(np.max(np.abs(a - b)) / (d if d > 0 else 1.0)) if b.size else 0.0
    got, want = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
    out = {"all": rel(got, want)}
    if got.ndim == 5:
        for i in range(got.shape[1]):
            out["ch%d" % i] = rel(got[:, i], want[:, i])
    return out


# The seam shapes (BS, Nt, Nx, Ny) of tests/test_gpu_losses_seams.py, by mechanism (vjp_march_kernel: narrow tile 32 rows x
# 64 columns for Ny < 192, wide tile 8 x 256; pick_tseg halves T until <= 16; tap-free marches of 8 planes).  2-D routes
# see (BS*Nt, Nx, Ny): marched along BS*Nt, rows Nx, columns Ny.
SEAM_SHAPES = {
    "tseg": [(2, T, 5, 12) for T in (17, 23, 27, 33, 40, 64)],                       # routes with t-taps
    "tfree3d": [(2, T, 5, 12) for T in (9, 12, 16, 17)],                             # NS continuity (taps along Nx / Ny only)
    "tfree2d": [(1, n, 5, 12) for n in (9, 10, 11, 13, 16, 17)],                     # 2-D routes: B*Nt
    "narrow_x": [(1, 4, X, Y) for X in (33, 64, 65) for Y in (16, 61, 64)],
    "narrow_y": [(1, 4, 9, Y) for Y in (65, 100, 130, 191)],
    "wide_x": [(1, 4, X, 200) for X in (17, 25)],
    "wide_y": [(1, 4, 9, Y) for Y in (192, 255, 257, 513, 770)],
    "two_seams": [(1, 17, 33, 16), (1, 17, 5, 65), (1, 17, 17, 192), (1, 17, 5, 257)],
}
LOSS_SHAPES = [(4, 16, 140, 300), (3, 7, 400, 13)]


def seam_groups(name):
    """The groups of SEAM_SHAPES route ``name`` runs."""
    t = ["tseg"] if name in ROUTES_3D_T else ["tfree3d"] if name == "ns_continuity_yfix" else ["tfree2d"]
    return t + ["narrow_x", "narrow_y", "wide_x", "wide_y", "two_seams"]
