"""Helpers shared by tests/test_jorekvjp_cpu.py and tests/test_gpu_jorekvjp.py: the fused backward of the reduced-MHD (JOREK)
residual losses on the layout the scripts hold (``jorek=True`` of cp_pre_amd.losses, csrc/vjp_flat_jorek.hip,
libcp_pre_vjpjorek.so).

``JorekRoute`` is the counterpart of ``mhdvjp_helpers.MHDRoute``: the two composed expressions restated ONCE in terms of
``D(f, k)`` from the float32 taps the operator objects hold now and the four scalars of ``JOREK._coef``, so that
``losses_helpers.ref_vjp`` / ``ref_loss`` / ``seam_inputs`` take it as they take a ``Route``.  fp64 autograd through it is the
reference of every test (tests/test_jorekvjp_cpu.py pins the restatement to ``oracle.residuals.jorek_*`` in fp64);
``closed_form`` is a literal restatement of the header's formulas with shifted adds, ``terms`` the same formulas one term at a
time.  The reference works on the LOGICAL [BS,3,Nt,Nx,Ny]; ``to_vars`` is the script's ``vars`` [BS,3,Nx,Ny,Nt] (a view).

Tolerance: the project's TOL = 1e-5 (``mhdvjp_helpers``), tensor-scale relative error overall and per gradient channel.
Inputs are ``rand + 0.5``, ``R = linspace(1, 2, Ny)``.  Shapes are the logical (BS, Nt, Nx, Ny): the seams of
``vjpflat_helpers.SEAM_SHAPES`` - the split is vjp_flat.hip's, asked the same way - and the three degenerate shapes of
``vjpflatmhd_helpers``.  The LDS ring of a launch is 4 x streams x (512 + 2) quads: 98 688 B at three streams, 131 584 B at
four - ONE workgroup per CU, 256 resident on an MI355X; the assertions below keep every seam crossed at that count."""
import torch

import vjpflat_helpers as vf
from losses_helpers import Dshift
from mhdvjp_helpers import TOL, pad_g  # noqa: F401  (re-exported)
from vjpflat_helpers import SEAM_SHAPES, nt_fastest_embedded, split  # noqa: F401
from vjpflatmhd_helpers import DEGENERATE

EQS = ("continuity", "temperature")
NREAD = {"continuity": 2, "temperature": 3}
OPSETS = ("default", "rescaled")             # the built tap structure
DECLINED_SETS = ("yfix", "general")          # declined by the library
RESCALE = {"D_t": 1.25, "D_R": 0.75, "D_Z": 1.5, "D_RR": 0.625, "D_ZZ": 1.375}
K_BIG = 0.75                                 # at the default K = 2.25e-7 the whole a3 term of d T is below the tolerance
NORM_DX, NORM_DY, NORM_DT = 1 / 64, 1 / 32, 1 / 128      # powers of two: the folded scalars of norms=True are exact

SLOTS = 256
RING_LDS = {3: 4 * 3 * (vf.FLAT_NT + 2) * 16, 4: 4 * 4 * (vf.FLAT_NT + 2) * 16}
assert RING_LDS == {3: 98688, 4: 131584} and all(160 * 1024 // b == 1 for b in RING_LDS.values()) and SLOTS == vf.MIN_SLOTS

_sp = {k: split(s, SLOTS) for k, s in SEAM_SHAPES.items()}
for _k, _s in SEAM_SHAPES.items():
    assert _s[0] * _sp[_k]["nCh"] * _sp[_k]["nTSeg"] < SLOTS and _sp[_k] == split(_s, 1 << 20), _k
assert _sp["one_chunk_one_march"]["nCh"] == 1 and _sp["one_chunk_one_march"]["nTSeg"] == 1
assert all(SEAM_SHAPES[k][1] % 4 == 2 and _sp[k]["nCh"] == 1 for k in ("straddle_10", "straddle_6"))
assert (_sp["chunk_seam"]["nCh"], _sp["chunk_seam"]["last"], _sp["chunk_seam"]["hq"]) == (2, 220, 15)
assert SEAM_SHAPES["bound"][1] == vf.FLAT_MAX_Y - 4 and _sp["bound"]["nCh"] == 2
assert (_sp["two_marches"]["nTSeg"], _sp["two_marches"]["last_planes"]) == (2, 8)
assert (_sp["full_last_march"]["nTSeg"], _sp["full_last_march"]["last_planes"]) == (2, 9)
assert (_sp["one_plane_last_march"]["nTSeg"], _sp["one_plane_last_march"]["last_planes"]) == (16, 1)
GPU_SHAPES = list(SEAM_SHAPES.values()) + list(DEGENERATE)
assert all((s[1] * s[3]) % 4 == 0 and s[1] < vf.FLAT_MAX_Y for s in GPU_SHAPES)
DECLINED_SHAPES = {(2, 96, 5, 12): "fallback:Nt >= 96", (2, 7, 5, 9): "fallback:merged row Ny*Nt not a multiple of 4"}


def radius(ny):
    return torch.linspace(1, 2, ny, dtype=torch.float32)


def to_vars(x):
    """the logical [B,F,Nt,Nx,Ny] as the script's ``vars`` [BS,F,Nx,Ny,Nt] (a view)"""
    return x.permute(0, 1, 3, 4, 2)


def to_logical(v):
    """``vars`` [BS,F,Nx,Ny,Nt] (or its gradient) as the logical [B,F,Nt,Nx,Ny] (a view)"""
    return v.permute(0, 1, 4, 2, 3)


def vars_on(x, device):
    """the logical CPU tensor ``x`` [B,F,Nt,Nx,Ny] as a dense ``vars`` [BS,F,Nx,Ny,Nt] on ``device``"""
    return to_vars(x).contiguous().to(device)


def general_kernel(k):
    """``D_R``'s kernel with weight on all three axes: the general star"""
    k = k.clone()
    k[0, 1, 1], k[1, 1, 2] = 0.25, -0.25
    return k


class JorekRoute:
    """One JOREK equation on one operator set for fields of ``ny`` columns: ``method`` (what ``cp_pre_amd.losses`` takes),
    ``ops`` (D_t, D_R, D_Z, D_RR, D_ZZ: their CURRENT ``.kernel`` is read at every call), ``kind`` its fused kind."""
    nd, nchan = 3, 3

    def __init__(self, eq, ny, opset="default", K=None, norms=False, device="cpu"):
        import functools

        from cp_pre_amd import residuals as R
        self.eq, self.opset, self.ny, self.norms = eq, opset, ny, norms
        self.name = "jorek_%s_%s_ny%d%s%s" % (eq, opset, ny, "" if K is None else "_K%g" % K, "_norms" if norms else "")
        kw = dict(device=device, y_axis_fix=(opset == "yfix"))
        if K is not None:
            kw["K"] = K
        if norms:
            kw.update(dx=NORM_DX, dy=NORM_DY, dt=NORM_DT)
        self.obj = o = R.JOREK(radius(ny), **kw)
        self.ops = o._ops()
        if opset == "rescaled":
            for a, s in RESCALE.items():
                getattr(o, a).kernel = getattr(o, a).kernel * s
        elif opset == "general":
            o.D_R.kernel = general_kernel(o.D_R.kernel)
        bound = getattr(o, "residual_" + eq)
        self.method = functools.partial(bound, norms=True) if norms else bound
        self.nread, self.kind = NREAD[eq], "jorek_" + eq
        self.chan = tuple(range(self.nread))

    def input_shape(self, s):
        assert s[3] == self.ny
        return (s[0], self.nchan) + tuple(s[1:])

    def kernels(self, dtype):
        return tuple(o.kernel.detach().cpu().to(dtype) for o in self.ops)

    def coef(self):
        return self.obj._coef(EQS.index(self.eq), self.norms)

    def full(self, x, D=Dshift):
        """The uncropped residual of the logical ``x`` [BS,3,Nt,Nx,Ny] in ``x``'s dtype: Joint/JOREK_residuals_CP.py:210-243."""
        Kt, KR, KZ, KRR, KZZ = self.kernels(x.dtype)
        a0, a1, a2, a3 = self.coef()
        R = radius(self.ny).to(x.dtype)
        rho, phi, T = x[:, 0], x[:, 1], x[:, 2]
        Dt, DR, DZ = (lambda f: D(f, Kt)), (lambda f: D(f, KR)), (lambda f: D(f, KZ))
        X = lambda f: DR(f)*DZ(phi) - DR(phi)*DZ(f)                  # noqa: E731
        Y = lambda f: D(f, KRR) + (1/R)*DR(f) + D(f, KZZ)             # noqa: E731
        if self.eq == "continuity":
            return a0*Dt(rho) - a1*R*X(rho) - a2*rho*DZ(phi) - a3*Y(rho)
        return T*Dt(rho) + rho*Dt(T) - rho*R*X(T) + T*R*X(rho) + a0*rho*T*DZ(phi) + a3*Y(T)

    def residual(self, x, boundary, D=Dshift):
        r = self.full(x, D)
        return r if boundary else r[(Ellipsis,) + (slice(1, -1),) * 3]


def terms(route, x, gfull):
    """The formulas of include/cp_pre_vjpjorek.h one term at a time, with shifted adds in ``x``'s dtype: {channel: [terms]},
    their sum the gradient.  ``gfull`` [BS,Nt,Nx,Ny]: the gradient arriving at the UNCROPPED residual."""
    Kt, KR, KZ, KRR, KZZ = route.kernels(x.dtype)
    a0, a1, a2, a3 = route.coef()
    flip = lambda k: torch.flip(k, (0, 1, 2))                          # noqa: E731
    Dt, DR, DZ = (lambda f: Dshift(f, Kt)), (lambda f: Dshift(f, KR)), (lambda f: Dshift(f, KZ))
    DtT, DRT, DZT = (lambda f: Dshift(f, flip(Kt))), (lambda f: Dshift(f, flip(KR))), (lambda f: Dshift(f, flip(KZ)))
    R = radius(route.ny).to(x.dtype)
    g = gfull.to(x.dtype)
    h = g * R
    rho, phi, T = x[:, 0], x[:, 1], x[:, 2]
    X = lambda f: DR(f)*DZ(phi) - DR(phi)*DZ(f)                        # noqa: E731
    J = lambda f, s=1: (DRT(h*s*DZ(f)), -DZT(h*s*DR(f)))               # noqa: E731
    Yt = (Dshift(g, flip(KRR)), DRT(g/R), Dshift(g, flip(KZZ)))
    if route.eq == "continuity":
        return {0: [a0*DtT(g)] + [-a1*t for t in J(phi)] + [-a2*g*DZ(phi)] + [-a3*t for t in Yt],
                1: [a1*t for t in J(rho)] + [-a2*DZT(g*rho)]}
    return {0: [DtT(g*T), g*Dt(T), -h*X(T)] + list(J(phi, T)) + [a0*g*T*DZ(phi)],
            2: [g*Dt(rho), DtT(g*rho)] + [-t for t in J(phi, rho)] + [h*X(rho), a0*g*rho*DZ(phi)] + [a3*t for t in Yt],
            1: list(J(T, rho)) + [-t for t in J(rho, T)] + [a0*DZT(g*rho*T)]}


def closed_form(route, x, gfull, drop=None):
    """The sum of ``terms`` -> [BS,3,Nt,Nx,Ny]; ``drop`` = (channel, index): without that one term."""
    out = torch.zeros_like(x)
    for c, ts in terms(route, x, gfull).items():
        for i, t in enumerate(ts):
            if drop != (c, i):
                out[:, c] = out[:, c] + t
    return out


def unread(route, nchan=3):
    return [c for c in range(nchan) if c >= route.nread]
