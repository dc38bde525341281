"""``Euler_FV_OS_rhs``: drop-in for ``Active_Learning/CNS.py:6-38``, the one caller of the 2-D spatial operator family.

The module maps ``vars[BS,4,Nx,Ny] = (rho, u, v, p)`` of one time instance to ``rhs[BS,4,Nx,Ny]``::

    rhs_mass   = -rho*div(u,v) - dot(uv, grad(rho))
    rhs_mom    = -dot(uv, grad(u)) - dot(uv, grad(v)) + laplace(u, v) + (1/rho)*grad(p)
    rhs_energy = -gamma*p*div(u,v) - dot(uv, grad(rho))
    rhs        = cat(rhs_mass, rhs_mom[:,0:1], rhs_mom[:,1:2], rhs_energy)

Reproduced, not fixed: ``Laplace`` is built with ``scalar=True``, so ``laplace(u, v)`` is the Laplacian of ``u`` alone; the
two ``dot`` terms are single-channel and broadcast, so both momentum channels carry the same advection and diffusion and
differ only in ``p_x/rho`` against ``p_y/rho``; the energy line uses ``grad(rho)``; and whatever the operators' constructors
do (the spatial 'y' operator differences along Nx, the 1/2-scaled first derivative, 'periodic' on all sides mapping the
high side onto the last cell itself) is inherited through their ``.kernel`` tensors and ``.bc``.

The reference composes seven operator calls - eleven stencil passes here - some 25 elementwise passes and a ``cat``.  The
fused route (``libcp_pre_cns.so``, ``include/cp_pre_cns.h``) is ONE launch that reads the four fields once and writes the
four channels once.  ``gradient``, ``laplace`` and ``divergence`` stay ordinary ``vector_convops_spatial`` objects built
with the reference's arguments: a caller may replace their ``.kernel`` tensors or their ``.bc``, and every call hands the
CURRENT ones to the library.  Whatever the fused route does not take falls back to the composed expression, and
``last_route()`` says which route the last call took and why.

``step(vars, h)`` is ``vars + h * rhs(vars)`` with the update folded into the same launch: what an explicit integrator or
a neural-ODE rollout does with the right-hand side.

Deviation (``param_grads=False``, the default): the operator kernels, ``dx`` and ``gamma`` are treated as constants.  In the
reference they carry ``requires_grad=True``, but the module has no ``nn.Parameter`` (``count_params() == 0``) and nothing
consumes those gradients; a backward through this module then differentiates with respect to ``vars`` only.
``param_grads=True`` delivers every gradient the reference would (the operator kernels, hence their ``scale``, and
``gamma``).  Either way the forward is the fused pass.  With ``backward="recompute"`` (the default) the backward recomputes
the composed expression (``_dispatch._Recompute``).  ``backward="fused"`` opts in to ONE launch of ``libcp_pre_cnsvjp.so``
(``include/cp_pre_cnsvjp.h``) for the gradient of all four fields; ``step`` is then differentiable with respect to ``vars``
and ``base`` too, and ``vjp`` is the bare product.  ``param_grads=True`` keeps the recompute route: the fused pass has no
gradient for the kernels or ``gamma``.  ``last_backward_route()`` says which route the last backward took.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _dispatch, _lib
from .convops_spatial import valid_conv
from .vector_convops_spatial import Divergence, Gradient, Laplace, _bc_struct, dot

TILE = (_lib.PRE_CNS_TILE_ROWS, _lib.PRE_CNS_TILE_COLS)     # rows x columns a workgroup of the fused pass owns

_last_route = None
_last_backward_route = None


def last_backward_route():
    """'fused:cns_vjp', 'fused:cns_vjp+axpy' (the epilogue: ``step`` with ``base`` being ``vars``, ``vjp(add_to=...)``) or
    'fallback:<why>' of the last backward through a module built with ``backward="fused"``, or of its last ``vjp`` call."""
    return _last_backward_route


def _set_backward_route(route):
    global _last_backward_route
    _last_backward_route = route
    return route


def last_route():
    """'fused:cns_rhs', 'fused:cns_rhs+axpy' (``step``) or 'fallback:<why>' of the last ``forward`` / ``step`` call."""
    return _last_route


def _set_route(route):
    global _last_route
    _last_route = route
    return route


def _planes(t):
    """Four ``pre_cns_plane_t`` for the channels of a [BS,4,Nx,Ny] device view."""
    sb, sc, sx, _ = t.stride()
    return (_lib.PreCnsPlane * 4)(*[_lib.PreCnsPlane(t.data_ptr() + 4 * c * sc, sb, sx) for c in range(4)])


def _aligned(t):
    sb, sc, sx, sy = t.stride()
    return sy == 1 and t.data_ptr() % 16 == 0 and sc % 4 == 0 and sx % 4 == 0 and (t.shape[0] == 1 or sb % 4 == 0)


def _aligned_or_copy(t):
    """``t`` if the fused passes can read it where it lies, else a dense copy (an allocation of its own is 16-byte aligned;
    ``contiguous()`` would hand a dense view that starts off a 16-byte boundary straight back)."""
    return t if _aligned(t) else t.clone(memory_format=torch.contiguous_format)


class _FusedVjp(torch.autograd.Function):
    """Attach the result of the fused forward (``h is None``) or of the fused step ``base + h * rhs(vars)`` to the autograd
    graph with ONE launch of ``pre_cns_vjp_f32`` as its backward: ``d_vars = J^T g``, or ``h * J^T g`` and ``d_base = g``, or
    ``g + h * J^T g`` in the launch's epilogue where ``base`` is ``vars`` (``base is None`` here).  ``taps`` are the operators'
    kernels, the boundary structure and gamma as of the forward call.  Once differentiable."""

    @staticmethod
    def forward(ctx, res, module, taps, h, vars, base):
        ctx.module, ctx.taps, ctx.h, ctx.own_base = module, taps, h, base is not None
        ctx.save_for_backward(vars)
        return res.view_as(res)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (vars,) = ctx.saved_tensors
        d_vars = None
        if ctx.needs_input_grad[4]:
            if ctx.h is None:
                d_vars = ctx.module._vjp_launch(vars, g, ctx.taps)
            elif ctx.own_base:                                       # (the entry's scale belongs to its epilogue)
                d_vars = ctx.module._vjp_launch(vars, g, ctx.taps).mul_(ctx.h)
            else:
                d_vars = ctx.module._vjp_launch(vars, g, ctx.taps, add_to=g, scale=ctx.h)
        return None, None, None, None, d_vars, (g if ctx.own_base and ctx.needs_input_grad[5] else None)


class Euler_FV_OS_rhs(nn.Module):
    """Compressible Navier-Stokes finite-volume operator-splitting right-hand side (``Active_Learning/CNS.py:6``).

    ``fused=False`` composes the operators as the reference does.  ``param_grads``, ``backward``: see the module docstring."""

    def __init__(self, configuration, device, fused=True, param_grads=False, backward="recompute"):
        super().__init__()
        if backward not in ("recompute", "fused"):
            raise ValueError("backward must be 'recompute' or 'fused'")
        self.dx = torch.tensor(configuration['Physics']['dx'], dtype=torch.float32, requires_grad=True).to(device)
        self.dy = torch.tensor(configuration['Physics']['dy'], dtype=torch.float32, requires_grad=True).to(device)
        self.gamma = torch.tensor(5 / 3, dtype=torch.float32, requires_grad=True).to(device)

        self.gradient = Gradient(scale=1 / (self.dx), taylor_order=2, boundary_cond='periodic', device=device, requires_grad=True)
        self.laplace = Laplace(scale=1 / (self.dx ** 2), taylor_order=2, boundary_cond='periodic', device=device, requires_grad=True)
        self.divergence = Divergence(scale=1 / (self.dx), taylor_order=2, boundary_cond='periodic', device=device, requires_grad=True)

        self.fused = fused
        self.param_grads = param_grads
        self.backward = backward
        self._gamma_seen = None                 # the value a stream capture is recorded with (as _dispatch.host_kernel)

    def count_params(self):
        nparams = 0
        for param in self.parameters():
            nparams += param.numel()
        return nparams

    # ------------------------------------------------------------------------------- the composed expression
    def _operators(self):
        return (self.gradient.grad_x, self.gradient.grad_y, self.divergence.grad_x, self.divergence.grad_y, self.laplace.laplace)

    def _reference_forward(self, vars):
        """The reference's forward, line by line, on this package's operators (each takes its own fused or composed route)."""
        rho = vars[:, 0:1]
        u = vars[:, 1:2]
        v = vars[:, 2:3]
        uv = vars[:, 1:3]
        p = vars[:, 3:4]

        rhs_mass = - rho * self.divergence(u, v) - dot(uv, self.gradient(rho))
        rhs_mom = -dot(uv, self.gradient(u)) - dot(uv, self.gradient(v)) + self.laplace(u, v) + (1 / rho) * self.gradient(p)
        rhs_energy = -self.gamma.to(vars.device) * p * self.divergence(u, v) - dot(uv, self.gradient(rho))

        return torch.cat((rhs_mass, rhs_mom[:, 0:1], rhs_mom[:, 1:2], rhs_energy), dim=1)

    def _expression(self, vars, k_gx, k_gy, k_dx, k_dy, k_lap, gamma):
        """The same expression as a function of its tensors (3x3 direct kernels): what a backward differentiates."""
        pad_g, pad_d, pad_l = self.gradient.bc.pad_signal, self.divergence.bc.pad_signal, self.laplace.bc.pad_signal
        rho, u, v, uv, p = vars[:, 0:1], vars[:, 1:2], vars[:, 2:3], vars[:, 1:3], vars[:, 3:4]

        def grad(f):
            return torch.cat((valid_conv(pad_g(f), k_gx), valid_conv(pad_g(f), k_gy)), dim=1)

        def div():
            return valid_conv(pad_d(u), k_dx) + valid_conv(pad_d(v), k_dy)

        rhs_mass = - rho * div() - dot(uv, grad(rho))
        rhs_mom = -dot(uv, grad(u)) - dot(uv, grad(v)) + valid_conv(pad_l(u), k_lap) + (1 / rho) * grad(p)
        rhs_energy = -gamma.to(vars.device) * p * div() - dot(uv, grad(rho))
        return torch.cat((rhs_mass, rhs_mom[:, 0:1], rhs_mom[:, 1:2], rhs_energy), dim=1)

    # ------------------------------------------------------------------------------- the fused route
    def _why_not(self, vars):
        """Host-side reason the fused pass cannot take ``vars`` with the operators as they are now, or None."""
        if vars.dim() != 4 or vars.shape[1] != 4:
            return "channel count other than 4"
        if vars.dtype != torch.float32:
            return "dtype other than fp32"
        for op in self._operators():
            if not hasattr(op, "kernel"):
                return "operator without a kernel"
            if op.conv != op.convolution:
                return "spectral operator"
        if any(tuple(op.kernel.shape) != (3, 3) for op in self._operators()):
            return "5x5 / 7x7 Taylor stencil"
        structs = [_bc_struct(o.bc) for o in (self.gradient, self.divergence, self.laplace)]
        if any(s is None for s in structs):
            return "boundary condition without a fused mapping"
        keys = [(tuple(s.mode), tuple(s.value)) for s in structs]
        if keys[1] != keys[0] or keys[2] != keys[0]:
            return "boundary conditions of the three operators differ"
        if vars.shape[3] % 4 != 0:
            return "Ny % 4 != 0"
        if vars.shape[2] < 2 or vars.shape[3] < 4 or vars.shape[0] < 1:
            return "grid below 2 x 4 cells"
        if vars.is_cuda and not _aligned(vars):
            return "misaligned view"
        return None

    def plan(self, vars):
        """The route ``forward(vars)`` would take, from the host-side checks alone (nothing is launched; the library may
        still decline): 'fused:cns_rhs' or 'fallback:<why>'."""
        if not self.fused:
            return "fallback:fused=False"
        why = self._why_not(vars)
        return "fused:cns_rhs" if why is None else "fallback:" + why

    def _gamma_host(self):
        if self.gamma.is_cuda and torch.cuda.is_current_stream_capturing():
            if self._gamma_seen is None:
                raise RuntimeError("gamma on the device under stream capture: call the module once eagerly first")
            return self._gamma_seen
        self._gamma_seen = float(self.gamma.detach())
        return self._gamma_seen

    def _taps(self):
        """(the five kernels as host floats, the boundary structure, gamma) as they are NOW: what one launch is handed."""
        return [_dispatch.dense9(op.kernel) for op in self._operators()], _bc_struct(self.gradient.bc), self._gamma_host()

    def _launch(self, vars, base=None, h=0.0, out=None, taps=None):
        """One launch of ``pre_cns_rhs_f32``.  Returns (result on the caller's device, None) or (None, why)."""
        why = self._why_not(vars)
        if why is not None:
            return None, why
        kernels, st, gamma = self._taps() if taps is None else taps
        dev, origin = _dispatch.to_device(vars)
        if not _aligned(dev):
            return None, "misaligned view"
        add = None
        if base is not None:
            add = dev if base is vars else _dispatch.to_device(base)[0]
            if not _aligned(add):
                return None, "misaligned view"
        if out is None:
            res = torch.empty(dev.shape, dtype=torch.float32, device=dev.device)
        else:
            if not (out.is_cuda and out.shape == dev.shape and out.dtype == torch.float32 and out.device == dev.device):
                raise ValueError("out must be an fp32 device tensor of vars' shape")
            if not _aligned(out):
                return None, "misaligned view"
            res = out
        with torch.cuda.device(dev.device):
            rc = _lib.load_cns().pre_cns_rhs_f32(_planes(dev), _planes(res), *kernels, ctypes.byref(st), gamma,
                                                 _planes(add) if add is not None else None, float(h),
                                                 dev.shape[0], dev.shape[2], dev.shape[3], 0, _lib.stream())
        if rc == _lib.PRE_E_UNSUPPORTED:
            return None, "declined by the library"
        if rc == _lib.PRE_E_RANGE and out is not None:
            raise ValueError("out must not overlap vars (a tile's halo is another tile's output), and may overlap base only "
                             "by being it")
        _lib.check(rc, "pre_cns_rhs_f32")
        return (res if out is not None else _dispatch.from_device(res, origin)), None

    def forward(self, vars, out=None):
        """``rhs[BS,4,Nx,Ny]``.  ``out``: optional fp32 device tensor (any view the fused pass takes: unit stride along Ny,
        16-byte aligned rows) to write into instead of a new tensor; it must not overlap ``vars``, and the call is then not
        differentiable."""
        if out is not None:
            if _dispatch.needs_grad(vars):
                raise RuntimeError("forward(vars, out=...) is not differentiable: leave out to autograd's own tensor")
            with torch.no_grad():
                res, why = (None, "fused=False") if not self.fused else self._launch(vars, out=out)
                _set_route("fused:cns_rhs" if why is None else "fallback:" + why)
                return res if why is None else out.copy_(self._reference_forward(vars))
        why = "fused=False" if not self.fused else self._why_not(vars)
        if why is not None:                                          # (the operators take it from here, each by its own route)
            _set_route("fallback:" + why)
            return self._reference_forward(vars)

        def fused():
            out, why = self._launch(vars)
            _set_route("fused:cns_rhs" if why is None else "fallback:" + why)
            return out

        ks = [op.kernel for op in self._operators()]
        if self.param_grads:
            expr = self._expression if self.backward != "fused" else self._noting("param_grads=True", self._expression)
            return _dispatch.fused_or_composed(fused, expr, vars, *ks, self.gamma)
        consts = [k.detach() for k in ks] + [self.gamma.detach()]
        if self.backward == "fused" and _dispatch.needs_grad(vars):
            with torch.no_grad():
                taps = self._taps()
                res, why = self._launch(vars, taps=taps)
            _set_route("fused:cns_rhs" if why is None else "fallback:" + why)
            if why is None:
                return _FusedVjp.apply(res, self, taps, None, vars, None)
            _set_backward_route("fallback:forward fell back: " + why)
            return self._expression(vars, *consts)
        return _dispatch.fused_or_composed(fused, lambda x: self._expression(x, *consts), vars)

    @staticmethod
    def _noting(why, fn):
        """``fn``, noting in ``last_backward_route()`` that the recompute route ran (it is called from the backward)."""
        def noted(*a):
            _set_backward_route("fallback:" + why)
            return fn(*a)
        return noted

    # ------------------------------------------------------------------------------- the fused backward
    def plan_backward(self, vars):
        """The route a backward through ``forward(vars)`` would take, from the host-side checks alone: 'fused:cns_vjp' or
        'fallback:<why>'."""
        if self.backward != "fused":
            return "fallback:backward='recompute'"
        if self.param_grads:
            return "fallback:param_grads=True"
        if not self.fused:
            return "fallback:fused=False"
        why = self._why_not(vars)
        return "fused:cns_vjp" if why is None else "fallback:" + why

    def _vjp_launch(self, vars, cotangent, taps, out=None, add_to=None, scale=1.0):
        """One launch of ``pre_cns_vjp_f32``: ``J(vars)^T cotangent``, or ``add_to + scale * J^T cotangent``.  A cotangent or an
        ``add_to`` that is not an aligned view (an expanded one, say) is made contiguous first.  Returns the gradient on
        ``vars``' device (``out`` itself if given)."""
        kernels, st, gamma = taps
        dev, origin = _dispatch.to_device(vars)
        if tuple(cotangent.shape) != tuple(dev.shape) or cotangent.dtype != torch.float32:
            raise ValueError("the cotangent must be an fp32 tensor of vars' shape")
        dev = _aligned_or_copy(dev)
        cot = _aligned_or_copy(cotangent.detach().to(dev.device))
        if out is None:
            res = torch.empty(dev.shape, dtype=torch.float32, device=dev.device)
        else:
            if not (out.is_cuda and out.shape == dev.shape and out.dtype == torch.float32 and out.device == dev.device and _aligned(out)):
                raise ValueError("out must be an fp32 device tensor of vars' shape, unit stride along Ny, 16-byte aligned rows")
            res = out
        add = None
        if add_to is not None:
            if add_to is cotangent:
                add = cot
            elif add_to is out:
                add = res
            else:
                if tuple(add_to.shape) != tuple(dev.shape) or add_to.dtype != torch.float32:
                    raise ValueError("add_to must be an fp32 tensor of vars' shape")
                add = _aligned_or_copy(add_to.detach().to(dev.device))
        with torch.cuda.device(dev.device):
            rc = _lib.load_cnsvjp().pre_cns_vjp_f32(_planes(dev), _planes(cot), _planes(res), *kernels, ctypes.byref(st), gamma,
                                                    _planes(add) if add is not None else None, float(scale),
                                                    dev.shape[0], dev.shape[2], dev.shape[3], 0, _lib.stream())
        if rc == _lib.PRE_E_RANGE and out is not None:
            raise ValueError("out must not overlap vars or the cotangent (a tile's halo is another tile's output), and may "
                             "overlap add_to only by being it")
        _lib.check(rc, "pre_cns_vjp_f32")
        _set_backward_route("fused:cns_vjp" if add is None else "fused:cns_vjp+axpy")
        return res if out is not None else _dispatch.from_device(res, origin)

    def vjp(self, vars, cotangent, out=None, add_to=None, scale=1.0):
        """The bare product ``J(vars)^T cotangent`` of the right-hand side, no autograd involved: what an adjoint-method
        stepper calls.  With ``add_to`` the result is ``add_to + scale * J^T cotangent`` in the same launch; ``add_to`` may be
        ``out`` itself (accumulation) or ``cotangent`` (the adjoint of an Euler step).  ``out``: optional fp32 device tensor to
        write into; it must not overlap ``vars`` or ``cotangent``.  Whatever the fused pass does not take is an error here."""
        why = "fused=False" if not self.fused else self._why_not(vars)
        if why is not None:
            raise ValueError("vjp: the fused pass does not take this call: " + why)
        with torch.no_grad():
            return self._vjp_launch(vars.detach(), cotangent, self._taps(), out, add_to, scale)

    def step(self, vars, h, out=None, base=None):
        """``base + h * rhs(vars)`` in the launch that forms the right-hand side; ``base`` defaults to ``vars`` (an explicit
        Euler step), a Runge-Kutta stage passes its own.  ``out``: optional fp32 device tensor of ``vars``' shape to write
        into; it may be ``base`` itself (an in-place update) but must not overlap ``vars``.  Not differentiable, unless the
        module was built with ``backward="fused"``: then it is, with respect to ``vars`` and ``base`` (``d_base = g``,
        ``d_vars = h * J^T g``; with ``base`` left to ``vars``, ``g + h * J^T g`` in one launch), as long as ``out`` is None."""
        ks = [op.kernel for op in self._operators() if hasattr(op, "kernel")] if self.param_grads else []
        if _dispatch.needs_grad(vars, base, *ks, *([self.gamma] if self.param_grads else [])):
            if self.backward != "fused" or self.param_grads:
                raise RuntimeError("step is not differentiable: use vars + h*forward(vars)")
            if out is not None:
                raise RuntimeError("step(vars, h, out=...) is not differentiable: leave out to autograd's own tensor")
            with torch.no_grad():
                taps = self._taps() if self.fused and self._why_not(vars) is None else None
                res, why = (None, "fused=False") if not self.fused else self._launch(vars, vars if base is None else base, float(h), taps=taps)
            if why is None:
                _set_route("fused:cns_rhs+axpy")
                return _FusedVjp.apply(res, self, taps, float(h), vars, base)
            return (vars if base is None else base) + float(h) * self.forward(vars)
        y = vars if base is None else base
        with torch.no_grad():
            res, why = (None, "fused=False") if not self.fused else self._launch(vars, y, float(h), out)
            if why is None:
                _set_route("fused:cns_rhs+axpy")
                return res
            _set_route("fallback:" + why)
            res = y + float(h) * self._reference_forward(vars)
            if out is None:
                return res
            out.copy_(res)
            return out
