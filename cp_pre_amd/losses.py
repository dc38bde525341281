"""Physics-informed residual losses with fused HIP backward passes.

The reference trains its surrogates with the PDE residual in the loss (``Physics_Informed/Wave_FNO_PISL.py:209-217``,
``Wave_FNO_PI.py:202-228``, ``Advection_FNO_PI.py:207-217``)::

    PI_loss(pred)      = residual(pred).pow(2).mean()
    PISL(pred, yy)     = (residual(pred) - residual(yy)).pow(2).mean()
    combined(pred, yy) = lp + 1000 * PISL(pred, yy)

and calls ``loss.backward()`` on the device.  Here::

    ns = NavierStokes(dt, dx, dy)
    loss = pi_loss(ns.residual_momentum, pred)                 # mean(r^2), 0-d fp32 device tensor
    loss = pisl_loss(ns.residual_momentum, pred, yy)           # mean((r(pred) - r(yy))^2)
    (lp + 1000 * loss).backward()                              # pred.grad by the fused VJP
    gu = residual_vjp(ns.residual_momentum, vars, g)           # a general upstream g, same kernels

Forward: the existing fused residual pass (the paired pass for PISL) writes the uncropped residual r, then
``pre_vjp_sumsq_f32`` sums ``m * r^2`` deterministically in fp64 (``m``: the cells the loss averages over).  Without a
gradient r is dropped at once; with one it is the only new tensor kept.  Backward: ONE launch of ``libcp_pre_vjp.so``
(``include/cp_pre_vjp.h``) reads r - masked and scaled by ``2 / N * upstream`` on load, the upstream gradient staying
on the device - and the fields the residual is non-linear in, and writes the gradient of every field into its slot of
one tensor of ``pred``'s shape.

Fused routes: a single linear operator (a ``ConvOperator`` of ``convops_2d`` / ``convops_1d``, ``PRE_Wave``,
``Advection``), NS continuity, NS momentum (``PRE_NS``), Burgers.  Everything else - MHD, JOREK, operator kernels that
require grad or have weight off the 7-point star, inputs on the CPU or without unit stride on their last axis,
``fused=False``, a ``yy`` that requires grad - falls back to what ran before: ``method(...).pow(2).mean()`` through
autograd.  ``last_route()`` says which route the last call took.

``flat=True`` (off by default: nothing above changes) offers an input WITHOUT unit stride on its last axis to
``libcp_pre_vjpflat.so`` (``include/cp_pre_vjpflat.h``) when its unit-stride axis is the logical Nt axis - the view the
reference's scripts pass, ``field[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2)``.  The forward pass is the one above (it
already evaluates such views in their memory order); the sum of squares reads that residual where it lies, and ONE launch
of the merged-row VJP writes the gradient, dense in the input's memory order.  Routes ``fused:flat_stencil3d``,
``fused:flat_linear2``, ``fused:flat_ns_momentum``; whatever the library or the host checks decline (Nt at or above
``FLAT_MAX_NT``, a merged row Ny*Nt that is no multiple of 4, u / v whose rows are not dense, the 1-D family, everything
that falls back above) takes the fallback with its reason.

``wgrad=True`` (off by default: nothing above changes, ``libcp_pre_wgrad.so`` is never loaded) lets the operator kernel
itself be trained, as the reference's wave scripts do (``Physics_Informed/Wave_FNO_PI.py:202-210``:
``D.kernel.requires_grad = True``).  For the kinds that are ONE linear operator - ``stencil3d``, ``stencil2d`` and
``flat_stencil3d``: a ``ConvOperator``, ``PRE_Wave.residual``, ``Advection.residual`` - a kernel that requires grad no
longer declines the fused route: forward pass and field VJP are the launches above on a snapshot of the kernel, and in the
same ``backward`` ONE launch of ``pre_wgrad_stencil3d_f32`` (``include/cp_pre_wgrad.h``) reads the saved r, ``pred`` (and
``yy``) where they lie and returns ``kernel.grad``: mask and scale on load, no atomics, the same bytes every run.  Routes
``fused:stencil3d+wgrad``, ``fused:stencil2d+wgrad``, ``fused:flat_stencil3d+wgrad``.  NS momentum, NS continuity and
Burgers (several operators, or a non-linear residual), any residual where several operator kernels require grad, and
``residual_vjp`` keep ``fallback:operator kernel requires grad``.  ``kernel_vjp`` is the same launch for a general g.

``mhd=True`` (off by default: nothing above changes, ``libcp_pre_vjpmhd.so`` is never loaded) gives the ideal-MHD residuals
a fused backward pass (``include/cp_pre_vjpmhd.h``): on a CUDA ``[BS,F>=6,Nt,Nx,Ny]`` input with unit stride on Ny,
``MHD.residual_continuity`` and ``residual_induction`` (``PRE_MHD.residual``) are ONE launch, ``residual_momentum`` and
``residual_energy`` TWO, split by output group (in one they need scratch), ``residual_gauss`` is ``pre_vjp_linear2_f32``.
Routes ``fused:mhd_continuity``, ``fused:mhd_induction``, ``fused:mhd_momentum``, ``fused:mhd_energy``, ``fused:linear2``.
The forward pass is the fused MHD residual as before.  The kernels are built for the tap structures of the forward march;
with operators that are general stars only momentum is built, the others take ``fallback:declined by the library``.
Together with ``flat=True`` an Nt-fastest input takes ``fallback:no flat VJP for MHD``.  The channels an equation does not
read get a zero gradient.

``mhd="flat"`` (a further opt-in value: ``mhd=True`` is unchanged) does everything ``mhd=True`` does and additionally offers
an Nt-fastest MHD input - ``pred.permute(0,1,4,2,3)`` of a surrogate's ``[BS,F,Nx,Ny,Nt]`` output, the view
``Joint/MHD_Residuals_CP.py`` and ``Marginal/MHD_Residuals_CP.py`` pass - to ``libcp_pre_vjpflatmhd.so``
(``include/cp_pre_vjpflatmhd.h``: the merged-row march of ``libcp_pre_vjpflat.so`` with the MHD functors), whatever ``flat``
says; the library loads only when that route is taken.  Routes ``fused:flat_mhd_continuity``, ``fused:flat_mhd_induction``
(one launch), ``fused:flat_mhd_momentum``, ``fused:flat_mhd_energy`` (two); ``residual_gauss`` takes
``fused:flat_linear2`` through ``pre_vjpflat_linear2_f32``.  The host checks are those of ``flat=True`` with their reasons,
``rows of the fields not dense`` for the channels a non-linear equation reads, and ``declined by the library`` where the
library has no instantiation for the operators' tap structure (general stars: momentum and energy).  The gradient is dense
in the input's memory order; a unit-stride input takes ``fused:mhd_*`` as with ``mhd=True``.

``jorek=True`` (off by default: nothing above changes, ``libcp_pre_vjpjorek.so`` is never loaded and the reduced-MHD residuals
keep ``fallback:no fused VJP for JOREK``) gives ``JOREK.residual_continuity`` / ``residual_temperature`` a fused backward pass
on the layout ``Joint/JOREK_residuals_CP.py`` holds: a CUDA ``vars`` ``[BS,F>=3,Nx,Ny,Nt]`` whose field views
(``JOREK.unstack_fields``) are Nt-fastest with dense rows, whatever ``flat`` says (``include/cp_pre_vjpjorek.h``: the merged-row
march with three planes of rho, phi (and T) in LDS, because the gradient at a cell reads phi at the four corners of the
(R, Z) plane).  Routes ``fused:flat_jorek_continuity`` (one launch) and ``fused:flat_jorek_temperature`` (two, split by output
group).  ``norms=True`` of the continuity equation: hand over ``functools.partial(jorek.residual_continuity, norms=True)``.
The library is built for the tap structure the reference constructs; ``y_axis_fix`` operators and general stars take
``fallback:declined by the library``, Ny-fastest field views ``fallback:fields not Nt-fastest``, and the host checks of
``flat=True`` keep their reasons (``Nt >= 96``, ``merged row Ny*Nt not a multiple of 4``, ``rows of the fields not dense``,
``operator kernel requires grad``).  The gradient is dense in ``vars``' memory order; T (continuity) and every channel
from 3 on get a zero gradient.

Host side: what a method is, what it reads and what declines a fused launch whatever the layout is resolved in
``_method.Method`` (shared with ``screen``); ``_Spec`` adds the kinds that have a fused VJP, the order of the reasons of
``prepare`` / ``prepare_flat`` and ONE launcher (``vjp``; ``flat=True``: the merged-row library).  ``_LossFn`` is the one
``autograd.Function`` of every fused route.
"""
from __future__ import annotations

import ctypes
import functools

import torch

from . import _dispatch, _lib
from . import residuals as R
from ._method import FLAT_MAX_NT, JOREK_ROWS, MHD_EQ, MHD_ROWS, Method

_last_route = None


def last_route():
    """'fused:<kind>' (kind: stencil3d, stencil2d, linear2, burgers, ns_momentum; with ``flat=True`` also flat_stencil3d,
    flat_linear2, flat_ns_momentum; with ``mhd=True`` also mhd_continuity, mhd_induction, mhd_momentum, mhd_energy; with
    ``mhd="flat"`` also flat_mhd_continuity, flat_mhd_induction, flat_mhd_momentum, flat_mhd_energy, and flat_linear2 for
    ``residual_gauss``; with ``jorek=True`` also flat_jorek_continuity, flat_jorek_temperature) or 'fallback:<why>' of the last ``pi_loss`` / ``pisl_loss`` / ``residual_vjp`` call."""
    return _last_route


# ------------------------------------------------------------------------------------------- what a method is
class _Spec(Method):
    """One residual method, resolved (``_method.Method``) for the fused VJPs: ``kind`` (None: no fused VJP), ``nd``
    residual axes, ``chan`` - the channels of a stacked ``[BS,F,...]`` input the residual reads (None: the input is the
    field itself), ``why`` a fallback is taken."""
    KIND = {"op3d": "stencil3d", "op2d": "stencil2d", "wave": "stencil3d", "advection": "stencil2d",
            "ns_momentum": "ns_momentum", "ns_continuity": "linear2", "burgers": "burgers"}
    WHY = {"spectral": "spectral operator", **dict.fromkeys(MHD_ROWS + JOREK_ROWS, "no fused VJP for {cls}")}
    # ``mhd=True``: the kinds of libcp_pre_vjpmhd.so (gauss is two linear operators: ``pre_vjp_linear2_f32``)
    MHD_KIND = {**{"mhd_" + e: "mhd_" + e for e in MHD_EQ}, "mhd_gauss": "linear2"}

    JOREK_EQ = {"residual_continuity": 0, "residual_temperature": 1}

    def __init__(self, method, mhd=False, jorek=False):
        bound, self.norms = method, False
        if jorek and isinstance(method, functools.partial) and not method.args and set(method.keywords) <= {"norms"} and \
                isinstance(getattr(method.func, "__self__", None), R.JOREK):
            bound, self.norms = method.func, bool(method.keywords.get("norms", False))      # (the one keyword of the equations)
        super().__init__(bound)
        self.method = method
        name = getattr(bound, "__name__", "")
        self.jorek = bool(jorek) and self.row == "jorek" and name in self.JOREK_EQ
        if self.jorek:                                           # the kinds of libcp_pre_vjpjorek.so
            self.eq = self.JOREK_EQ[name]
            self.kind, self.why, self.ops = "jorek_" + name[len("residual_"):], None, tuple(self.obj._ops())
        self.mhd = bool(mhd) and self.row in self.MHD_KIND
        self.mhd_flat = self.mhd and isinstance(mhd, str) and mhd == "flat"     # Nt-fastest inputs too: libcp_pre_vjpflatmhd.so
        if self.mhd:
            self.kind, self.why = self.MHD_KIND[self.row], None
        if self.kind is None and not self.is_op:
            self.chan, self.ops = (), ()                         # (no launch reads them: a stacked input, shapes not checked here)

    def out_shape(self, x, boundary):
        s = self.field_shape(x)
        return s if boundary else s[:1] + tuple(max(n - 2, 0) for n in s[1:])

    # -------- the method itself
    def call(self, x, boundary, minus=None):
        """``method(x)`` (``- method(minus)``), cropped unless ``boundary``: the differentiable route that ran before."""
        if self.is_op:
            r = self.method(x) if minus is None else self.method(x) - self.method(minus)
            return r if boundary else r[(Ellipsis,) + (slice(1, -1),) * self.nd]
        if minus is None:
            return self.method(x, boundary=boundary)
        return self.method(x, boundary=boundary, minus=minus)

    def full(self, x, minus):
        """The uncropped residual by the existing fused passes (no autograd)."""
        with torch.no_grad():
            if not self.is_op:
                return self.call(x, True, minus)
            if minus is None:
                return _dispatch._xcorr_impl(x, self.method.kernel, self.nd)
            r = _dispatch.xcorr_pair(x, minus, self.method.kernel, self.nd)
            return r if r is not None else self.method(x) - self.method(minus)

    # -------- can the fused VJP run?  (host checks + one download of the operator kernels)
    def prepare(self, x, minus=None, wgrad=False):
        """(why, kernels): ``why`` is None if the fused VJP can run on ``x`` - ``kernels`` are then the host copies of the
        operator kernels the launch takes - else the reason for the fallback.  Changes nothing on ``self``.  ``wgrad``: a
        kernel that requires grad does not decline a kind that is one linear operator."""
        if self.kind is None:
            return self.why, ()
        if not x.is_cuda or (minus is not None and not minus.is_cuda):
            return "input on the CPU", ()
        if x.numel() == 0:
            return "empty input", ()
        if x.stride(-1) != 1 or (minus is not None and minus.stride(-1) != 1):
            return "no unit stride on the last axis", ()
        why = self.declined(x, minus, wgrad and self.trains_kernel())
        if why is not None:
            return why, ()
        why, kernels = self.star_kernels(self.kind)
        if why is None and self.kind.startswith("mhd_"):         # a tap structure the library has no instantiation for
            eq = MHD_EQ.index(self.kind[4:])
            if _lib.load_vjpmhd().pre_vjpmhd_supported(eq, *kernels) == _lib.PRE_E_UNSUPPORTED:
                return "declined by the library", ()
        return why, kernels

    def trains_kernel(self):
        """Is this ONE linear operator whose kernel requires grad - what ``wgrad=True`` hands to ``pre_wgrad_stencil3d_f32``?"""
        return self.kind in ("stencil3d", "stencil2d") and len(self.ops) == 1 and _dispatch.needs_grad(self.ops[0].kernel)

    # -------- flat=True: an input without unit stride on its last axis (host checks + one download)
    def wants_flat(self, x):
        """Is ``x`` an input ``flat=True`` (``mhd="flat"``: an MHD residual) offers to the merged-row VJP at all?
        (Everything else: ``prepare``.)"""
        return x.is_cuda and x.numel() > 0 and x.dim() > 0 and x.stride(-1) != 1

    def prepare_flat(self, x, minus=None, wgrad=False):
        """``prepare`` for the merged-row VJP of ``libcp_pre_vjpflat.so`` (``mhd="flat"``: ``libcp_pre_vjpflatmhd.so``):
        (why, kernels).  The layout conditions are the library's own (include/cp_pre_vjpflat.h), stated here so that the
        reason has a name."""
        if self.kind is None:
            return self.why, ()
        if self.mhd and not self.mhd_flat:
            return "no flat VJP for MHD", ()
        if self.nd != 3:
            return "no flat VJP for the 1-D family", ()
        why = self.declined(x, minus, wgrad and self.trains_kernel())
        if why is not None:
            return why, ()
        f = self.fields(x)
        Nt, Ny = f[0].shape[1], f[0].shape[3]
        if f[0].stride(1) != 1:
            return "the unit-stride axis is not Nt", ()
        if Nt >= FLAT_MAX_NT:
            return "Nt >= %d" % FLAT_MAX_NT, ()
        if (Ny * Nt) % 4 != 0:
            return "merged row Ny*Nt not a multiple of 4", ()
        if self.kind == "ns_momentum" and any(v.stride(1) != 1 or v.stride(3) != Nt or v.stride(2) != Ny * Nt for v in f[:2]):
            return "rows of u, v not dense", ()
        mhd = self.kind.startswith("mhd_")               # (gauss is linear: its launch reads no field)
        if mhd and any(v.stride(1) != 1 or v.stride(3) != Nt or v.stride(2) != Ny * Nt for v in f):
            return "rows of the fields not dense", ()
        why, kernels = self.star_kernels(self.kind)
        if why is None and mhd:                          # a tap structure the library has no instantiation for
            eq = MHD_EQ.index(self.kind[4:])
            if _lib.load_vjpflatmhd().pre_vjpflatmhd_supported(eq, *kernels) == _lib.PRE_E_UNSUPPORTED:
                return "declined by the library", ()
        return why, kernels

    # -------- jorek=True: vars [BS,F,Nx,Ny,Nt] as the script holds it (host checks + one download)
    def prepare_jorek(self, x, minus=None):
        """``prepare_flat`` for ``libcp_pre_vjpjorek.so``: (why, kernels).  The layout is decided on the field views of
        ``JOREK.unstack_fields``; the conditions are the library's own (include/cp_pre_vjpjorek.h)."""
        if not x.is_cuda or (minus is not None and not minus.is_cuda):
            return "input on the CPU", ()
        if x.numel() == 0:
            return "empty input", ()
        why = self.declined(x, minus)
        if why is not None:
            return why, ()
        if x.shape[1] < 3:
            return "fewer than three JOREK channels", ()
        f = R.JOREK.unstack_fields(x)[:2 + self.eq]
        Nt, Nx, Ny = f[0].shape[1:]
        if Nt > 1 and any(v.stride(1) != 1 for v in f):
            return "fields not Nt-fastest", ()
        if Nt >= FLAT_MAX_NT:
            return "Nt >= %d" % FLAT_MAX_NT, ()
        if (Ny * Nt) % 4 != 0:
            return "merged row Ny*Nt not a multiple of 4", ()
        if any(n != 1 and st != w for v in f for n, st, w in zip((Nx, Ny), v.stride()[2:], (Ny * Nt, Nt))):
            return "rows of the fields not dense", ()
        if self.obj.R.numel() != Ny:                             # (``JOREK._R_view`` raises: so does every route)
            return "len(R) is not Ny", ()
        why, kernels = self.star_kernels(self.kind)
        if why is None and _lib.load_vjpjorek().pre_vjpjorek_supported(self.eq, *kernels) == _lib.PRE_E_UNSUPPORTED:
            return "declined by the library", ()                 # (y_axis_fix, general stars: not the reference's tap structure)
        return why, kernels

    def vjp_jorek(self, kernels, gfull, x, crop, host_scale, dev_scale):
        """``gfull`` [BS,Nt,Nx,Ny], dense in memory order [BS,Nx,Ny,Nt]; ``x`` the ``vars`` ``prepare_jorek`` accepted.  The
        gradient is dense in ``x``'s memory order.  None if the library declines."""
        nf = 2 + self.eq
        grad = _lib.empty_like_layout(x)
        gfull = _nt_fastest_strides(gfull)
        fs = [_nt_fastest_strides(v) for v in R.JOREK.unstack_fields(x)[:3]]
        os_ = [_nt_fastest_strides(v) for v in R.JOREK.unstack_fields(grad)[:3]]
        Rb = self.obj._R_view(fs[0])
        with torch.cuda.device(x.device):
            rc = _lib.load_vjpjorek().pre_vjpjorek_flat_f32(
                self.eq, ctypes.byref(_lib.field(gfull)), R._arr(fs), ctypes.byref(_lib.field(Rb)), R._arr(os_), *kernels,
                _lib.farr(self.obj._coef(self.eq, self.norms)), float(host_scale), _lib.ptr(dev_scale), *gfull.shape,
                _lib.PRE_VJP_CROP if crop else 0, _lib.stream())
        if rc == _lib.PRE_E_UNSUPPORTED:
            return None
        _lib.check(rc, "pre_vjpjorek_flat_f32")
        grad[:, nf:].zero_()                                     # (T under continuity, every channel from 3 on: not read)
        return grad

    # -------- the VJP launch: gfull [BS,*field] -> gradient of x's shape
    def vjp(self, kernels, gfull, x, crop, host_scale, dev_scale, flat=False):
        """``kernels``: what ``prepare`` returned; ``gfull`` [BS,*field] (copied unless its last axis has unit stride).
        ``flat``: the merged-row launch - ``kernels``: what ``prepare_flat`` returned; ``gfull`` [BS,Nt,Nx,Ny], dense in
        memory order [BS,Nx,Ny,Nt]; the gradient is dense in ``x``'s memory order.  None if the library declines."""
        if self.jorek:
            return self.vjp_jorek(kernels, gfull, x, crop, host_scale, dev_scale)
        mhd = self.kind.startswith("mhd_")
        if mhd:
            lib = _lib.load_vjpflatmhd() if flat else _lib.load_vjpmhd()
        else:
            lib = _lib.load_vjpflat() if flat else _lib.load_vjp()
        name = (("pre_vjpflatmhd_" if flat else "pre_vjpmhd_") + self.kind[4:] if mhd else
                ("pre_vjpflat_" if flat else "pre_vjp_") + self.kind) + "_f32"
        scalars = self.scalars() if not mhd or self.kind == "mhd_energy" else ()
        grad = _lib.empty_like_layout(x) if flat else torch.empty(x.shape, dtype=torch.float32, device=x.device)
        if flat and self.mhd_flat:                       # (what this module allocates: an extent of 1 may carry any stride)
            grad, gfull = _nt_fastest_strides(grad), _nt_fastest_strides(gfull)
        if not flat and gfull.stride(-1) != 1:
            gfull = gfull.contiguous()
        if self.kind == "ns_momentum":
            views = [gfull, R._arr([x[:, 0], x[:, 1]]), R._arr([grad[:, 0], grad[:, 1], grad[:, 2]])]
        elif mhd:                                        # the fields the equation reads, a gradient slot for each
            views = [gfull, R._arr([x[:, c] for c in self.chan]), R._arr([grad[:, c] for c in self.chan])]
        elif self.kind == "linear2":
            views = [gfull, R._arr([grad[:, c] for c in self.chan])]
        elif self.kind == "burgers":
            views = [gfull, x, grad]
        else:
            views, kernels = [gfull, grad[:, 0] if grad.dim() == self.nd + 2 else grad], _dispatch.tap_args(*kernels)
        if self.nd == 3:                                 # PreField arguments in 3-D, pointer + stride array in 2-D
            args = [ctypes.byref(_lib.field(v)) if isinstance(v, torch.Tensor) else v for v in views]
        else:
            args = [a for v in views for a in (_lib.ptr(v), _lib.iarr64(v.stride()))]
        with torch.cuda.device(x.device):
            rc = getattr(lib, name)(*args, *kernels, *scalars, float(host_scale), _lib.ptr(dev_scale), *gfull.shape,
                                    _lib.PRE_VJP_CROP if crop else 0, _lib.stream())
        if rc == _lib.PRE_E_UNSUPPORTED:
            return None
        _lib.check(rc, name)
        if self.chan is not None and self.chan != tuple(range(len(self.chan))):
            for c in set(range(x.shape[1])) - set(self.chan):      # (MHD induction, gauss: the channels read are no prefix)
                grad[:, c].zero_()
        elif self.chan is not None and x.shape[1] > len(self.chan):
            grad[:, len(self.chan):].zero_()                       # (after the launch, which writes the other channels)
        return grad

    def vjp_flat(self, kernels, gfull, x, crop, host_scale, dev_scale):
        return self.vjp(kernels, gfull, x, crop, host_scale, dev_scale, True)

    # -------- the kernel-gradient launch: g [BS,*field], x (and minus) where they lie -> d / d kernel, on x's device
    def wgrad(self, g, x, minus, crop, host_scale, dev_scale):
        """``scale * sum_c m_c g_c (x - minus)_{c + k}`` for every tap k of the operator's kernel, by ONE launch of
        ``pre_wgrad_stencil3d_f32``.  None if the library declines (another layout, extents other than 1 / 3)."""
        ext = tuple(self.ops[0].kernel.shape)
        if len(ext) != self.nd:
            return None
        views = [g] + [v[:, 0] if v.dim() == self.nd + 2 else v for v in (x, minus) if v is not None]
        flags = _lib.PRE_VJP_CROP if crop else 0
        if self.nd == 2:                                 # [B,T,X] with a (kt,kx) kernel == [1,B,T,X] with (1,kt,kx)
            views, ext3, flags = [v.unsqueeze(0) for v in views], (1,) + ext, flags | _lib.PRE_VJP_VIEW3D
        else:
            ext3 = ext
        lib = _lib.load_wgrad()
        ws = torch.empty(_lib.PRE_WGRAD_WORKSPACE, dtype=torch.float64, device=x.device)
        dk = torch.empty(ext, dtype=torch.float32, device=x.device)
        fs = [ctypes.byref(_lib.field(v)) for v in views] + [None] * (3 - len(views))
        with torch.cuda.device(x.device):
            rc = lib.pre_wgrad_stencil3d_f32(*fs, *ext3, float(host_scale), _lib.ptr(dev_scale), *views[0].shape, flags,
                                             _lib.ptr(ws), _lib.ptr(dk), _lib.stream())
        if rc == _lib.PRE_E_UNSUPPORTED:
            return None
        _lib.check(rc, "pre_wgrad_stencil3d_f32")
        return dk


def _nt_fastest_strides(v):
    """``v`` [...,Nt,Nx,Ny], dense in memory order [...,Nx,Ny,Nt], with the strides of that order written out on its last
    three axes: torch is free to give an axis of extent 1 any stride, the merged-row libraries read them all.  The same
    memory; ``v`` itself where an axis longer than 1 has another stride."""
    Nt, Nx, Ny = v.shape[-3:]
    want = tuple(v.stride()[:-3]) + (1, Ny * Nt, Nt)
    if v.stride() == want or any(s != w and n != 1 for s, w, n in zip(v.stride(), want, v.shape)):
        return v
    return v.as_strided(tuple(v.shape), want, v.storage_offset())


def _nt_fastest_dense(r):
    """Is the [BS,Nt,Nx,Ny] tensor ``r`` dense in memory order [BS,Nx,Ny,Nt]?"""
    return r.dim() == 4 and r.permute(0, 2, 3, 1).is_contiguous()


# ------------------------------------------------------------------------------------------- validation (host only)
def _check_tensor(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} has dtype {t.dtype}: the residual losses take float32")


def _check_like(t, like, what, shape=None):
    """``t``: a float32 tensor of ``shape`` (default ``like``'s) on ``like``'s device; raises before any device work."""
    _check_tensor(t, what)
    shape = tuple(like.shape) if shape is None else tuple(shape)
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected {shape}")
    if t.device != like.device:
        raise ValueError(f"{what} is on {t.device}, pred on {like.device}")


# ------------------------------------------------------------------------------------------- the loss
def _mean_sq(r, boundary, where_it_lies=False):
    """(mean of ``m * r^2`` as a 0-d fp32 device tensor, N) by ``pre_vjp_sumsq_f32``; r: the uncropped residual.
    ``where_it_lies``: an Nt-fastest r is summed in its memory order [BS,Nx,Ny,Nt] instead of being copied (the crop is
    symmetric on every axis: the masked set is the same)."""
    dims = r.shape[1:]
    n = r.shape[0]
    for d in dims:
        n *= d if boundary else max(d - 2, 0)
    if where_it_lies and _nt_fastest_dense(r):
        r = r.permute(0, 2, 3, 1)
    if r.stride(-1) != 1:
        r = r.contiguous()
    r4 = r if r.dim() == 4 else r.unsqueeze(0)
    flags = (0 if boundary else _lib.PRE_VJP_CROP) | (_lib.PRE_VJP_VIEW3D if r.dim() == 3 else 0)
    ws = torch.empty(_lib.PRE_VJP_SUMSQ_WORKSPACE + 1, dtype=torch.float64, device=r.device)
    with torch.cuda.device(r.device):
        _lib.check(_lib.load_vjp().pre_vjp_sumsq_f32(ctypes.byref(_lib.field(r4)), *r4.shape, flags, _lib.ptr(ws),
                                                     ctypes.c_void_p(ws.data_ptr() + 8 * _lib.PRE_VJP_SUMSQ_WORKSPACE),
                                                     _lib.stream()), "pre_vjp_sumsq_f32")
    return (ws[-1] / float(n) if n else ws[-1] * float("nan")).to(torch.float32), n


def _recompute_grad(spec, x, minus, boundary, g):
    """The gradient by the route that ran before (what the fused backward does where the library declines)."""
    with torch.enable_grad():
        v = x.detach().requires_grad_(True)
        y = spec.call(v, boundary, minus)
        return torch.autograd.grad(y, v, g.to(y.device))[0]


def _recompute_kernel_grad(spec, x, minus, boundary, g):
    """d <g, method(x) - method(minus)> / d kernel by the route that ran before: the composed expression on a fresh leaf
    in the operator's ``kernel`` slot, differentiated by torch."""
    op = spec.ops[0]
    held = op.kernel
    with torch.enable_grad():
        k = held.detach().clone().requires_grad_(True)
        op.kernel = k
        try:
            y = spec.call(x.detach(), boundary, None if minus is None else minus.detach())
        finally:
            op.kernel = held
        if y.numel() == 0:
            return torch.zeros_like(k)
        return torch.autograd.grad(y, k, g.to(y.device))[0]


class _LossFn(torch.autograd.Function):
    """The loss of a fused route.  ``kernel``: the operator kernel where it trains (``wgrad=True``), else None; ``r``: the
    residual where the caller has evaluated it already (``flat``: it has checked where r lies, and the backward pass is
    the merged-row launch).  One field VJP launch for ``pred``, and ``pre_wgrad_stencil3d_f32`` for a kernel that trains,
    in the same backward."""

    @staticmethod
    def forward(ctx, pred, kernel, spec, kernels, yy, boundary, flat, r):
        if r is None:
            r = spec.full(pred, yy)
        loss, n = _mean_sq(r, boundary, where_it_lies=flat)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(r, pred, *(() if kernel is None else (kernel,)))     # r: the one new tensor kept
            ctx.spec, ctx.kernels, ctx.yy, ctx.boundary, ctx.n, ctx.flat = spec, kernels, yy, boundary, n, flat
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        # (once_differentiable: the VJP launch builds no graph, so create_graph=True raises instead of returning a gradient
        # that silently has none)
        r, pred = ctx.saved_tensors[:2]
        spec, n = ctx.spec, ctx.n
        up = gout.detach().to(device=pred.device, dtype=torch.float32).reshape(1)
        scale = 2.0 / n if n else 0.0
        composed_g = lambda: (2.0 / max(n, 1)) * up * (r if ctx.boundary else r[(Ellipsis,) + (slice(1, -1),) * spec.nd])  # noqa: E731
        grad = gk = None
        if ctx.needs_input_grad[0]:
            grad = spec.vjp(ctx.kernels, r, pred, not ctx.boundary, scale, up, ctx.flat)
            if grad is None:                             # (not expected after prepare(): the library declined)
                grad = _recompute_grad(spec, pred, ctx.yy, ctx.boundary, composed_g())
        if ctx.needs_input_grad[1]:
            gk = spec.wgrad(r, pred, ctx.yy, not ctx.boundary, scale, up)
            if gk is None:                               # the library declined (a layout it does not take): composed
                gk = _recompute_kernel_grad(spec, pred, ctx.yy, ctx.boundary, composed_g())
            gk = gk.to(ctx.saved_tensors[2].device)
        return grad, gk, None, None, None, None, None, None


def _loss(residual_method, pred, yy, boundary, flat=False, wgrad=False, mhd=False, jorek=False):
    global _last_route
    spec = _Spec(residual_method, mhd, jorek)
    _check_tensor(pred, "pred")
    spec.field_shape(pred)                               # (called for its raise: a rank the method does not take)
    if yy is not None:
        _check_like(yy, pred, "yy")
    data = None if yy is None else yy.detach()
    flat, r = bool(spec.jorek or ((flat or spec.mhd_flat) and spec.wants_flat(pred))), None
    if flat:
        why, kernels = spec.prepare_jorek(pred, yy) if spec.jorek else spec.prepare_flat(pred, yy, wgrad)
        if why is None:
            r = spec.full(pred, data)
            if not _nt_fastest_dense(r):
                why = "the forward pass returned the residual in another memory order"
    else:
        why, kernels = spec.prepare(pred, yy, wgrad)
    if why is not None:
        _last_route = "fallback:" + why
        return spec.call(pred, boundary, yy).pow(2).mean()
    trains = wgrad and spec.trains_kernel()
    _last_route = "fused:" + ("flat_" if flat else "") + spec.kind + ("+wgrad" if trains else "")
    return _LossFn.apply(pred, spec.ops[0].kernel if trains else None, spec, kernels, data, bool(boundary), flat, r)


def pi_loss(residual_method, pred, boundary=False, flat=False, wgrad=False, mhd=False, jorek=False):
    """``residual_method(pred, boundary).pow(2).mean()`` (``PI_loss``, Physics_Informed/Wave_FNO_PISL.py:213-214) as a
    0-d fp32 tensor on ``pred``'s device, differentiable with respect to ``pred``.  ``residual_method``: a bound
    ``residual*`` method of a class of ``cp_pre_amd.residuals``, or a ``ConvOperator`` (2-D: [BS,Nt,Nx,Ny], 1-D:
    [BS,Nt,Nx]).  ``boundary`` as on the residual methods (False: the mean runs over the interior ``[1:-1]`` of every
    residual axis; over an empty interior it is NaN, as ``torch.mean`` of an empty tensor).  ``flat=True``: an Nt-fastest
    ``pred`` (no unit stride on its last axis) is offered to the merged-row VJP (module docstring).  ``wgrad=True``: a
    single linear operator (a ``ConvOperator``, ``PRE_Wave.residual``, ``Advection.residual``) whose kernel requires grad
    keeps the fused route and gets ``kernel.grad`` from one launch of ``pre_wgrad_stencil3d_f32`` (route ``...+wgrad``);
    NS momentum, NS continuity, Burgers and any residual where several operator kernels require grad keep
    ``fallback:operator kernel requires grad``.  ``mhd=True``: the ideal-MHD residuals take the fused backward passes of
    ``libcp_pre_vjpmhd.so``; ``mhd="flat"``: the same, and an Nt-fastest ``pred`` takes those of
    ``libcp_pre_vjpflatmhd.so`` whatever ``flat`` says (module docstring).  ``jorek=True``: the reduced-MHD (JOREK) residuals
    take the fused backward passes of ``libcp_pre_vjpjorek.so`` on ``pred`` [BS,F>=3,Nx,Ny,Nt] (module docstring)."""
    return _loss(residual_method, pred, None, boundary, flat, wgrad, mhd, jorek)


def pisl_loss(residual_method, pred, yy, boundary=False, flat=False, wgrad=False, mhd=False, jorek=False):
    """``(residual(pred) - residual(yy)).pow(2).mean()`` (``PISL``, Physics_Informed/Wave_FNO_PISL.py:216-217).  ``yy``
    (``pred``'s shape, dtype and device) is data: the fused route does not differentiate it (one that requires grad takes
    the fallback, which does).  ``flat``, ``wgrad``, ``mhd`` and ``jorek`` as on ``pi_loss`` (the kernel gradient reads
    ``pred - yy``)."""
    return _loss(residual_method, pred, yy, boundary, flat, wgrad, mhd, jorek)


def residual_vjp(residual_method, vars, g, boundary=False, flat=False, mhd=False, jorek=False):
    """The vector-Jacobian product ``d <g, residual_method(vars, boundary)> / d vars`` for a general upstream gradient
    ``g`` (the shape of the method's result), by the kernels the losses use.  Returns a tensor of ``vars``' shape.
    ``flat``, ``mhd`` and ``jorek`` as on ``pi_loss`` (``flat``, ``jorek``: the gradient is then dense in ``vars``' memory order).  Operator
    kernels that require grad take ``fallback:operator kernel requires grad`` here (their own gradient: ``kernel_vjp``)."""
    global _last_route
    spec = _Spec(residual_method, mhd, jorek)
    _check_tensor(vars, "vars")
    _check_like(g, vars, "g", spec.out_shape(vars, boundary))
    if spec.jorek or ((flat or spec.mhd_flat) and spec.wants_flat(vars)):
        why, kernels = spec.prepare_jorek(vars) if spec.jorek else spec.prepare_flat(vars)
        if why is not None:
            _last_route = "fallback:" + why
            return _recompute_grad(spec, vars, None, boundary, g)
        _last_route = "fused:flat_" + spec.kind
        if g.numel() == 0:                               # (an empty interior: nothing reaches vars)
            return _lib.empty_like_layout(vars).zero_()
        with torch.no_grad():
            f0 = R.JOREK.unstack_fields(vars)[0] if spec.jorek else spec.fields(vars)[0]
            gfull = _lib.empty_like_layout(f0)                           # g in vars' memory order, the rim zero
            if boundary:
                gfull.copy_(g)
            else:
                gfull.zero_()
                gfull[:, 1:-1, 1:-1, 1:-1].copy_(g)
            grad = spec.vjp_flat(kernels, gfull, vars, False, 1.0, None) if _nt_fastest_dense(gfull) else None
        if grad is None:
            _last_route = "fallback:declined by the library"
            return _recompute_grad(spec, vars, None, boundary, g)
        return grad
    why, kernels = spec.prepare(vars)
    if why is not None:
        _last_route = "fallback:" + why
        return _recompute_grad(spec, vars, None, boundary, g)
    if g.numel() == 0:                                   # (an empty interior: nothing reaches vars)
        _last_route = "fused:" + spec.kind
        return torch.zeros(vars.shape, dtype=torch.float32, device=vars.device)
    with torch.no_grad():
        gfull = g if boundary else torch.nn.functional.pad(g, (1, 1) * spec.nd)
        grad = spec.vjp(kernels, gfull, vars, False, 1.0, None)
    if grad is None:
        _last_route = "fallback:declined by the library"
        return _recompute_grad(spec, vars, None, boundary, g)
    _last_route = "fused:" + spec.kind
    return grad


def kernel_vjp(residual_method, vars, g, boundary=False, minus=None):
    """The counterpart of ``residual_vjp`` for the operator kernel: ``d <g, method(vars) - method(minus)> / d kernel`` for a
    general upstream gradient ``g`` (the shape of the method's result), by the launch ``wgrad=True`` uses, with scale 1.
    ``residual_method``: one linear operator (a ``ConvOperator``, ``PRE_Wave.residual``, ``Advection.residual``); the kernel
    need not require grad.  Returns a tensor of the kernel's shape on the kernel's device.  Where the fused route declines
    (``last_route()`` says why) the same gradient comes from ``torch.autograd.grad`` through the composed expression."""
    global _last_route
    spec = _Spec(residual_method)
    if not (spec.is_op or isinstance(spec.obj, (R.PRE_Wave, R.Advection))):
        raise TypeError("kernel_vjp takes a residual that is one linear operator: a ConvOperator, PRE_Wave.residual, "
                        "Advection.residual")
    _check_tensor(vars, "vars")
    _check_like(g, vars, "g", spec.out_shape(vars, boundary))
    if minus is not None:
        _check_like(minus, vars, "minus")
    kernel = spec.ops[0].kernel
    why = spec.why
    if why is None:
        if not vars.is_cuda:
            why = "input on the CPU"
        elif vars.numel() == 0:
            why = "empty input"
        else:
            why = spec.declined(vars, kernel_trains=True)
    if why is None:
        f = spec.fields(vars)[0]
        m = None if minus is None else spec.fields(minus)[0]
        if any(s not in (1, 3) for s in kernel.shape) or kernel.dim() != spec.nd:
            why = "operator kernel extents other than 1 and 3"
        elif not (all(v.stride(-1) == 1 for v in (f, m) if v is not None) or
                  (spec.nd == 3 and all(v.stride(1) == 1 for v in (f, m) if v is not None))):
            why = "no unit stride on the last axis or on Nt"
    if why is not None:
        _last_route = "fallback:" + why
        return _recompute_kernel_grad(spec, vars, minus, boundary, g).to(kernel.device)
    flat = f.stride(-1) != 1
    _last_route = "fused:" + ("flat_" if flat else "") + spec.kind + "+wgrad"
    if g.numel() == 0:                                   # (an empty interior: nothing reaches the kernel)
        return torch.zeros(kernel.shape, dtype=torch.float32, device=kernel.device)
    with torch.no_grad():
        gfull = _lib.empty_like_layout(f)                # g in the field's memory order, the rim zero
        if boundary:
            gfull.copy_(g)
        else:
            gfull.zero_()
            gfull[(slice(None),) + (slice(1, -1),) * spec.nd].copy_(g)
        gk = spec.wgrad(gfull, vars, minus, False, 1.0, None)
    if gk is None:
        _last_route = "fallback:declined by the library"
        return _recompute_kernel_grad(spec, vars, minus, boundary, g).to(kernel.device)
    return gk.to(kernel.device)
