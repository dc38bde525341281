"""PDE residual operators (PRE) over surrogate outputs, evaluated on the MI355X.

Mirrors the residual definitions the reference writes inline per experiment script and
packages in ``Other_UQ/Evaluation/PRE_estimations.py:5-80`` (``PRE_Wave``, ``PRE_NS``,
``PRE_MHD`` keep that file's class names, constructor arguments and ``.residual(vars,
boundary)`` signature).  Every class owns reference-style ``ConvOperator`` objects
(``D_t, D_x, D_y, D_xx_yy`` ...), whose ``.kernel`` tensors may be replaced by the caller.

Two evaluation routes, same numbers:
  * fused (default): one streaming HIP pass reads each field once and writes the residual
    once (``pre_residual_*_f32``); the operators' CURRENT dense kernels are handed to the
    library, so the reference's ``D_y == D_t`` construction quirk is inherited, not re-coded;
  * composed (``fused=False``, or automatically when a kernel is not a 3x3x3 star or a view
    is not streamable): the reference expression, operator by operator, each
    ``ConvOperator`` call being a HIP stencil pass and the products/sums torch device ops.

``vars`` is [BS,F,Nt,Nx,Ny]; ``boundary=False`` crops one cell per side like the reference
(a view of the full residual).  ``absolute=True`` returns |residual| (the marginal score).

Data-driven scores (every ``Marginal/`` and ``Joint/`` script, e.g. ``Marginal/NS_Residuals_CP.py:284-289``): every
``residual*`` method takes ``minus=`` - a second field set of ``vars``' shape (any strides) - and returns
``r(vars) - r(minus)`` (``|r(vars) - r(minus)|`` with ``absolute=True``), the script's
``cal_out_residual - cal_pred_residual``.  NS momentum / continuity, MHD continuity / gauss, the wave and advection
kernels and Burgers read both sets in ONE streaming pass (``libcp_pre_pair.so``, ``include/cp_pre_pair.h``); MHD
momentum / energy / induction (8-12 views) and JOREK are TWO-PASS: r(vars) into the result, r(minus) into one scratch
buffer, then an in-place subtract (or |.|).  Where the one-pass kernel declines (a kernel off the star, a layout
without a shared unit-stride axis) the same two-pass route runs.  The result feeds the existing calibration unchanged:
``JointCalibration.add_slab(d)``, ``calibrate(|d|)`` / ``marginal_qhat``, ``emp_cov_levels(qhats, d)`` (``centre=None``).
These equal the scripts' ``modulation_func(a, b)``, ``ncf_metric_joint(a, b, mod)`` and ``emp_cov([c - q*m, c + q*m], y)``
up to the fp32 rounding of the residuals; coverage in ``d`` form is not bit-identical to the bounds form (a value on
``c +- q*m`` can round to the other side), the ``centre=`` path stays the exact one.
"""
from __future__ import annotations

import ctypes

import torch

from . import _dispatch, _lib
from .convops_1d import ConvOperator as ConvOperator1D
from .convops_2d import ConvOperator as ConvOperator2D

_CROP3 = (Ellipsis, slice(1, -1), slice(1, -1), slice(1, -1))
_CROP2 = (Ellipsis, slice(1, -1), slice(1, -1))


def _stage(fields):
    """Device views of the fields (+ where the result has to go back to).  Views that do not
    share a unit-stride axis are made contiguous so the fused kernels can stream them."""
    origin = None
    out = []
    for f in fields:
        _dispatch._check_field(f)
        d, o = _dispatch.to_device(f)
        origin = origin or o
        out.append(d)
    if len(out) > 1 and not _lib.streamable(*out):
        out = [d.contiguous() for d in out]
    return out, origin


def _on_device(fields, fn):
    """Composed route: stage the fields once, evaluate ``fn`` on device tensors, return home."""
    devs, origin = _stage(fields)
    return _dispatch.from_device(fn(*devs), origin)


def _arr(views):
    """``pre_field_t[n]`` of n device views."""
    return (_lib.PreField * len(views))(*map(_lib.field, views))


def _fused(name, call, sets, absolute, out=None, skip_t_rim=False, halo_x=False, out_rule=None, decline=None):
    """The one way into a fused entry: stage, validate, launch, come home.  ``sets``: one field set, or two (r(a) - r(b)),
    staged TOGETHER so that both are made contiguous when they share no unit-stride axis.  ``call(dsets, out, flags)``
    launches ``name`` on the staged sets and returns its code.  ``out_rule`` says what a caller's ``out`` may be: None (the
    entry takes none), 'ns' (the field shape or, with ``skip_t_rim``, its interior planes) or 'mhd' (the field shape).
    Returns the result where the fields live, or None where the entry declines (the caller then composes, or runs two
    passes).  ``decline``: what a decline means when ``halo_x`` / an interior ('ns') or given ('mhd') ``out`` was asked
    for, which no other route serves: a text to raise RuntimeError with (the single-set calls), or None to fall through
    all the same (the paired calls: their two-pass route raises on its own, from its single-set passes)."""
    fields = sets[0] if len(sets) == 1 else [*sets[0], *sets[1]]
    # (asked here, where the caller's grad mode still holds, and only for the requests whose rules name autograd)
    grad = (halo_x or out is not None) and _dispatch.needs_grad(*fields)
    with torch.no_grad():
        devs, origin = _stage(fields)
        d0, given = devs[0], out is not None
        if out is None:
            out = _lib.empty_like_layout(d0, score_rows=absolute and origin is None)
        interior = False
        if out_rule == 'ns':
            interior = (skip_t_rim and out.dim() == 4 and d0.shape[1] >= 3 and
                        tuple(out.shape) == (d0.shape[0], d0.shape[1] - 2, d0.shape[2], d0.shape[3]))
            if not (out.is_cuda and out.dtype == torch.float32 and (out.shape == d0.shape or interior)):
                raise ValueError("out must be an fp32 device tensor of the field shape "
                                 "(or, with skip_t_rim, of its interior planes [BS,Nt-2,Nx,Ny])")
            # (the planes of an interior out must be dense, its batch and time strides are free: a t-slab driver that
            # shards the marginal calibration hands in a TIME-MAJOR buffer [Nt-2][BS][Nx][Ny] seen as [BS,Nt-2,Nx,Ny],
            # whose planes then are the contiguous send blocks of its all-to-all - pipeline.marginal_qhat)
            dense_planes = out.dim() == 4 and out.stride(3) == 1 and out.stride(2) == out.shape[3]
            if interior and not (dense_planes and origin is None and not grad):
                raise ValueError("an interior-plane out needs device-resident fields, dense [Nx,Ny] planes and no autograd")
        elif given and not (out.is_cuda and out.dtype == torch.float32 and out.shape == d0.shape and origin is None and not grad):
            raise ValueError("out must be an fp32 device tensor of the field shape, the fields device-resident, no autograd")
        if halo_x and (origin is not None or grad or
                       any(d.data_ptr() != f.data_ptr() or d.stride(3) != 1 for d, f in zip(devs, fields))):
            raise ValueError("halo_x needs device-resident, Ny-contiguous views of a larger grid and no autograd")
        flags = (_lib.PRE_FLAG_ABS if absolute else 0) | (_lib.PRE_FLAG_INTERIOR_T if skip_t_rim else 0) | \
                (_lib.PRE_FLAG_OUT_INTERIOR_T if interior else 0) | (_lib.PRE_FLAG_HALO_X if halo_x else 0)
        k = len(sets[0])
        with torch.cuda.device(d0.device):
            rc = call([devs] if len(sets) == 1 else [devs[:k], devs[k:]], out, flags)
    if rc == _lib.PRE_E_UNSUPPORTED:
        if decline is not None and (halo_x or (given if out_rule == 'mhd' else interior)):
            raise RuntimeError(decline)
        return None
    _lib.check(rc, name)
    return _dispatch.from_device(out, origin)


class _Residual2D:
    """Shared plumbing: the operator set of ``Marginal/NS_Residuals_CP.py:213-219``."""

    def __init__(self, device='cpu', fused=True, y_axis_fix=False, bc=None):
        """``bc``: boundary conditions on the x-y rim for every ``residual*`` of this object (``_BC``: 'wrap', a type name, a
        dict side -> type | (type, value), a ``BoundaryManager``); None = the zero padding of the reference."""
        self.fused = fused
        self.bc = None if bc is None else _BC(bc)
        self.D_t = ConvOperator2D(domain='t', order=1, device=device)
        self.D_x = ConvOperator2D(domain='x', order=1, device=device)
        self.D_y = ConvOperator2D(domain='y', order=1, device=device, y_axis_fix=y_axis_fix)
        self.D_x_y = ConvOperator2D(domain=('x', 'y'), order=1, device=device)     # kernel-less, as in the reference
        self.D_xx_yy = ConvOperator2D(domain=('x', 'y'), order=2, device=device)

    def _k27(self, *ops):
        ks = [_dispatch.dense27(o.kernel) for o in ops]
        return None if any(k is None for k in ks) else ks

    def _want_fused(self, *tensors):
        """The fused kernels run whatever the fields' ``requires_grad`` (``_attach`` keeps the result
        differentiable by recomputation); only operator KERNELS that require grad force the composed route, so
        that their gradients flow."""
        if any(isinstance(t, torch.Tensor) and t.numel() == 0 for t in tensors):
            return False                                    # empty batch: the composed route returns empty tensors
        return self.fused and not _dispatch.needs_grad(*[getattr(o, "kernel", None) for o in
                                                         (self.D_t, self.D_x, self.D_y, self.D_xx_yy)])

    def _linear2(self, i, j, ratio, composed, method, vars, minus, boundary, absolute):
        """``D_x(vars[:, i]) + ratio * D_y(vars[:, j])`` (``composed``): NS continuity, MHD gauss.  One set through
        ``vector_convops.linear2`` (which keeps the result differentiable itself, operator kernels included), two in one
        pass of ``pre_pair_linear2_f32``."""
        sets = ((vars[:, i], vars[:, j]),)
        if self.bc is not None:
            if minus is not None:
                _check_minus(vars, minus)
            return _bc_residual("linear2", self.bc, 3, sets[0], None if minus is None else (minus[:, i], minus[:, j]), composed,
                                (self.D_x, self.D_y), lambda d, o, ks, st, flags: _lib.load_bcres().pre_bcres_linear2_f32(
                                    _fld(d[0]), _fld(d[1]), _fld(o), *ks, float(ratio), ctypes.byref(st), *o.shape, flags,
                                    _lib.stream()), boundary, absolute, fused=self.fused)
        _no_bc()
        if minus is None:
            if self._want_fused(vars):
                from .vector_convops import linear2
                res = linear2(sets[0][0], self.D_x.kernel, sets[0][1], self.D_y.kernel, ratio, _lib.PRE_FLAG_ABS if absolute else 0)
                if res is not None:
                    return _finish(res, boundary, _CROP3, absolute, True)
            return _tail(None, sets, composed, boundary, _CROP3, absolute)
        _check_minus(vars, minus)
        sets += ((minus[:, i], minus[:, j]),)
        ks = self._k27(self.D_x, self.D_y) if self._want_fused(vars, minus) else None
        res = None if ks is None else _fused("pre_pair_linear2_f32", lambda d, o, flags: _lib.load_pair().pre_pair_linear2_f32(
            _arr(d[0]), _arr(d[1]), ctypes.byref(_lib.field(o)), *ks, float(ratio), *o.shape, flags, _lib.stream()), sets, absolute)
        return _tail(res, sets, composed, boundary, _CROP3, absolute, (method, vars, minus))


def _attach(res, sets, composed, absolute):
    """``res``: a fused result of one field set, or r(a) - r(b) of two (with |.| already applied if ``absolute``), or None.
    If a field requires grad the result is hooked into autograd: a backward recomputes ``composed`` (operator by
    operator; ``composed(*a) - composed(*b)`` for two sets, so gradients reach both) and differentiates that; a forward
    that is never differentiated pays nothing."""
    fields = sets[0] if len(sets) == 1 else [*sets[0], *sets[1]]
    if res is None or not _dispatch.needs_grad(*fields):
        return res
    k = len(sets[0])

    def fn(*f):
        d = _on_device(f[:k], composed)
        if len(f) > k:
            d = d - _on_device(f[k:], composed)
        return d.abs() if absolute else d
    return _dispatch._Recompute.apply(res, fn, *fields)


def _check_minus(vars, minus, device_view=False):
    """Validate ``minus=``: a tensor of ``vars``' shape and dtype on ``vars``' device.  Every ``minus=`` route calls this
    BEFORE any device work, so that a bad second set is reported as such on a machine without a GPU too.
    ``device_view`` (halo_x, an interior-plane out): both sets must be Ny-contiguous device views, like the x-slab views
    the flag reads past - views that staging never copies, so the halo rows read are those of the caller's grid."""
    if not isinstance(minus, torch.Tensor):
        raise TypeError("minus must be a torch.Tensor of the shape of vars")
    if minus.dtype != vars.dtype:
        raise TypeError(f"minus has dtype {minus.dtype}, vars {vars.dtype}")
    if tuple(minus.shape) != tuple(vars.shape):
        raise ValueError(f"minus has shape {tuple(minus.shape)}, vars {tuple(vars.shape)}: the two field sets must match")
    if minus.device != vars.device:
        raise ValueError(f"minus is on {minus.device}, vars on {vars.device}")
    if device_view and not (minus.is_cuda and vars.is_cuda and minus.stride(-1) == 1 and vars.stride(-1) == 1):
        raise ValueError("halo_x / an interior-plane out with minus= need both field sets as Ny-contiguous device views "
                         "of the same geometry")


def _two_pass(run, fa, fb, absolute):
    """The two-pass route of r(a) - r(b): ``run(fields, first)`` is a single-set fused pass on device tensors (or None),
    ``first`` telling the pass whose result is kept (it may write a caller's ``out``) from the one into a scratch buffer;
    then an in-place subtract / |.| on the first result.  None if the single-set pass declines too."""
    with torch.no_grad():
        da, db = [_dispatch.to_device(f) for f in fa], [_dispatch.to_device(f) for f in fb]
        origin = next((o for _, o in da + db if o is not None), None)
        a = run([d for d, _ in da], True)
        if a is None:
            return None
        b = run([d for d, _ in db], False)
        if b is None:
            return None
        a.sub_(b)
        if absolute:
            a.abs_()
    return _dispatch.from_device(a, origin)


def _pair_composed(method, vars, minus, boundary, crop, absolute):
    """``method(vars) - method(minus)`` on device (each a single-set route of its own, autograd included), returned
    where ``vars`` lives: what runs when neither pass can be fused."""
    dv, origin = _dispatch.to_device(vars)
    dm, _ = _dispatch.to_device(minus)
    d = method(dv, True) - method(dm, True)
    d = _dispatch.from_device(d.abs() if absolute else d, origin)
    return d if boundary else d[crop]


def _finish(res, boundary, crop, absolute, already_abs):
    if absolute and not already_abs:
        res = res.abs()
    return res if boundary else res[crop]


def _tail(res, sets, composed, boundary, crop, absolute, pair=None):
    """How every ``residual_*`` ends.  ``res``: what a fused route gave (|.| applied), or None: then the composed route
    runs, for two sets as ``_pair_composed(*pair, ...)`` with ``pair = (method, vars, minus)``.  A fused result is hooked
    into autograd (``_attach``); either is cropped unless ``boundary``."""
    if res is not None:
        return _finish(_attach(res, sets, composed, absolute), boundary, crop, absolute, True)
    if pair is not None:
        return _pair_composed(*pair, boundary, crop, absolute)
    return _finish(_on_device(sets[0], composed), boundary, crop, absolute, False)


# ======================================================================= Navier-Stokes
class NavierStokes(_Residual2D):
    """``Marginal/NS_Residuals_CP.py:203-240``: continuity and momentum residuals of (u, v, p)."""

    def __init__(self, dt, dx, dy, nu=0.001, **kw):
        super().__init__(**kw)
        self.dt, self.dx, self.dy, self.nu = dt, dx, dy, nu

    def residual_continuity(self, vars, boundary=False, absolute=False, minus=None):
        """``minus``: r(vars) - r(minus) in one pass (``pre_pair_linear2_f32``; see the module docstring)."""
        ratio = self.dx / self.dy
        return self._linear2(0, 1, ratio, lambda u, v: self.D_x(u) + ratio * self.D_y(v), self.residual_continuity,
                             vars, minus, boundary, absolute)

    def residual_momentum(self, vars, boundary=False, absolute=False, out=None, skip_t_rim=False, halo_x=False, minus=None):
        """``out``: optional preallocated device tensor [BS,Nt,Nx,Ny] for the uncropped residual
        (fused route only; lets a streaming driver reuse one buffer).  ``skip_t_rim``: the caller
        crops the first and last time plane anyway, so they need not be computed or stored
        (``PRE_FLAG_INTERIOR_T``; their content is then unspecified).  With ``skip_t_rim`` ``out`` may
        also be a [BS,Nt-2,Nx,Ny] tensor (contiguous, or any batch / time strides over dense planes): it then receives
        the interior planes only
        (``PRE_FLAG_OUT_INTERIOR_T``; what a t-slab driver that feeds slabs with their two halo planes
        wants) and the result is that tensor, cropped in x and y unless ``boundary``.
        ``halo_x``: ``vars`` is an x-slab ``full[:, :, :, x0:x1]`` (1 <= x0, x1 <= Nx - 1) of a larger grid whose rows
        x0 - 1 and x1 lie in the same memory: they are read as the x-neighbours of the slab's first and last row instead
        of the zero padding (``PRE_FLAG_HALO_X``), so the slab's residual rows are those of the whole grid.  What an
        x-slab driver wants: the T axis stays whole and a slab re-reads 2 rows of Nx_slab instead of 2 planes of
        Nt_slab.  Fused route only (raises otherwise).
        ``minus``: r(vars) - r(minus) (the data-driven score) in one pass of both sets (``pre_pair_ns_momentum_f32``);
        ``out``, ``skip_t_rim`` and ``halo_x`` apply to both sets with the same validation."""
        sets = ((vars[:, 0], vars[:, 1], vars[:, 2]),)
        dt, dx, dy, nu = self.dt, self.dx, self.dy, self.nu
        D_t, D_x, D_y, D_xx_yy = self.D_t, self.D_x, self.D_y, self.D_xx_yy

        def composed(u, v, p):
            res_x = D_t(u)*dx*dy + u*D_x(u)*dt*dy + v*D_y(u)*dt*dx - nu*D_xx_yy(u)*dt + D_x(p)*dt*dy
            res_y = D_t(v)*dx*dy + u*D_x(v)*dt*dx + v*D_y(v)*dt*dy - nu*D_xx_yy(v)*dt + D_y(p)*dt*dx
            return res_x + res_y
        interior_out = skip_t_rim and out is not None and out.dim() == 4 and vars.dim() == 5 and out.shape[1] == vars.shape[2] - 2
        if self.bc is not None:
            # (the x-y rim is valid under ``bc``; ``boundary=False`` crops the time rim only.  ``skip_t_rim`` is honoured:
            # PRE_FLAG_INTERIOR_T)
            if halo_x or interior_out:
                raise ValueError("bc with halo_x=True / an interior-plane out: an x-slab with a wrapped x, or a t-slab "
                                 "buffer, is not served under boundary conditions")
            if minus is not None:
                _check_minus(vars, minus)
            scal = (float(dt), float(dx), float(dy), float(nu))
            return _bc_residual("ns_momentum", self.bc, 3, sets[0], None if minus is None else (minus[:, 0], minus[:, 1], minus[:, 2]),
                                composed, (D_t, D_x, D_y, D_xx_yy),
                                lambda d, o, ks, st, flags: _lib.load_bcres().pre_bcres_ns_momentum_f32(
                                    *[_fld(t) for t in d + [o]], *ks, *scal, ctypes.byref(st), *o.shape, flags, _lib.stream()),
                                boundary, absolute, out, self.fused, _lib.PRE_FLAG_INTERIOR_T if skip_t_rim else 0)
        _no_bc()
        pair = None
        if minus is not None:
            _check_minus(vars, minus, device_view=halo_x or interior_out)
            sets += ((minus[:, 0], minus[:, 1], minus[:, 2]),)
            pair = (self.residual_momentum, vars, minus)
        ks = self._k27(D_t, D_x, D_y, D_xx_yy) if self._want_fused(vars, minus) else None
        res = None
        if ks is not None:
            tail = (*ks, float(dt), float(dx), float(dy), float(nu))
            if minus is None:
                res = _fused("pre_residual_ns_momentum_f32", lambda d, o, flags: _lib.load().pre_residual_ns_momentum_f32(
                    *[ctypes.byref(_lib.field(t)) for t in d[0] + [o]], *tail, *d[0][0].shape, flags, _lib.stream()),
                    sets, absolute, out, skip_t_rim, halo_x, 'ns',
                    "pre_residual_ns_momentum_f32: an interior-plane out / halo_x needs Ny-contiguous views and star-shaped "
                    "operator kernels")
            else:
                res = _fused("pre_pair_ns_momentum_f32", lambda d, o, flags: _lib.load_pair().pre_pair_ns_momentum_f32(
                    _arr(d[0]), _arr(d[1]), ctypes.byref(_lib.field(o)), *tail, *d[0][0].shape, flags, _lib.stream()),
                    sets, absolute, out, skip_t_rim, halo_x, 'ns')
            if res is None and minus is not None and not _dispatch.needs_grad(*sets[0], *sets[1]):
                # TWO-PASS (the general-star tap structure, whose paired kernel does not fit the registers): the single-set
                # fused pass of each set.  Only without autograd - its in-place subtract has no backward; fields that
                # require grad take the composed difference below.  With an interior-plane out r(minus) goes into a
                # scratch buffer of that shape and the caller's out is the result.
                res = _two_pass(lambda f, first: self.residual_momentum(
                    f[0], True, out=out if first else (torch.empty_like(out) if interior_out else None),
                    skip_t_rim=skip_t_rim, halo_x=halo_x), (vars,), (minus,), absolute)
        if res is None and halo_x:
            raise RuntimeError("halo_x: only the fused route reads the halo rows")
        # (an interior-plane out has lost its first and last time plane already: x and y are left to crop)
        crop = _CROP2 if res is not None and res.shape[1] == vars.shape[2] - 2 else _CROP3
        return _tail(res, sets, composed, boundary, crop, absolute, pair)

    _WALLS = {'top': 0, 'bottom': 1, 'left': 2, 'right': 3}

    def periodic_bc_residual(self, u, wall='right'):
        """``Marginal/NS_Residuals_CP.py:468-478``: (one edge of every [Nx,Ny] plane minus the opposite one) * dx ->
        ``u.shape[:-2] + (Ny,)`` for 'top' / 'bottom', ``+ (Nx,)`` for 'left' / 'right'.  One ``pre_edge_residual_f32``
        launch on the view where it lies (any strides); an unknown wall raises KeyError as the reference's dict lookup
        would."""
        code = self._WALLS[wall]
        if u.dim() < 2 or u.dtype != torch.float32:
            raise RuntimeError("periodic_bc_residual: float32 field with at least the two plane axes")
        d, origin = _dispatch.to_device(u)
        lead = tuple(d.shape[:-2])
        v = d.reshape((1,) * (4 - d.dim()) + tuple(d.shape)) if d.dim() < 4 else (d if d.dim() == 4 else d.reshape(-1, *d.shape[-3:]))
        B, T, X, Y = v.shape
        out = torch.empty(lead + ((Y,) if code < 2 else (X,)), dtype=torch.float32, device=d.device)
        if out.numel() == 0:                                     # (an empty batch has no device memory to point at)
            return _dispatch.from_device(out, origin)
        with torch.cuda.device(d.device):
            f = _lib.field(v)
            _lib.check(_lib.load().pre_edge_residual_f32(ctypes.byref(f), code, float(self.dx), B, T, X, Y, _lib.ptr(out),
                                                         _lib.stream()), "pre_edge_residual_f32")
        return _dispatch.from_device(out, origin)


class PRE_NS(NavierStokes):
    """``Other_UQ/Evaluation/PRE_estimations.py:24-50``: ``PRE_NS(dt, dx, dy).residual(vars)``."""

    def __init__(self, dt, dx, dy, **kw):
        super().__init__(dt, dx, dy, nu=0.001, **kw)

    def residual(self, vars, boundary=False, minus=None):
        return self.residual_momentum(vars, boundary, minus=minus)


# ======================================================================= MHD
_MHD_EQ = {'continuity': 0, 'momentum': 1, 'energy': 2, 'induction': 3}


class MHD(_Residual2D):
    """``Marginal/MHD_Residuals_CP.py:204-278``: ideal-MHD residuals of (rho,u,v,p,Bx,By)."""

    def __init__(self, gamma=5 / 3, **kw):
        super().__init__(**kw)
        self.gamma = gamma

    def _fused(self, eq, vars, absolute, halo_x=False, out=None, minus=None):
        """One pass of ``pre_residual_mhd_f32`` over the six fields or, with ``minus`` (the continuity equation only), of
        ``pre_pair_mhd_continuity_f32`` over the first three of both sets; None -> compose / two-pass.
        ``halo_x`` (every ``residual_*`` below takes it): ``vars`` is an x-slab ``full[:, :, :, x0:x1]`` whose rows
        x0 - 1 and x1 lie in the same memory and are read as x-neighbours instead of the zero padding
        (``PRE_FLAG_HALO_X``, see ``NavierStokes.residual_momentum``); fused route only.
        ``out`` (likewise): a preallocated fp32 device tensor [BS,Nt,Nx,Ny] for the uncropped residual - any batch / plane
        strides over rows that share the fields' contiguous axis (``pipeline.row_padded`` / ``time_major`` buffers: the
        sharded marginal calibration's send blocks); fused route only (raises otherwise)."""
        n = 6 if minus is None else 3
        ks = self._k27(self.D_t, self.D_x, self.D_y) if self._want_fused(vars, minus) else None
        if ks is None or vars.shape[1] < n:
            if minus is None and (halo_x or out is not None):
                raise RuntimeError("halo_x / out: only the fused route reads the halo rows / writes a caller's buffer")
            return None
        tail = (*ks, float(self.gamma))
        if minus is None:
            return _fused("pre_residual_mhd_f32", lambda d, o, flags: _lib.load().pre_residual_mhd_f32(
                _MHD_EQ[eq], _arr(d[0]), ctypes.byref(_lib.field(o)), *tail, *o.shape, flags, _lib.stream()),
                ([vars[:, i] for i in range(n)],), absolute, out, False, halo_x, 'mhd',
                "pre_residual_mhd_f32: halo_x / out need views that share a contiguous axis with the fields "
                "and star-shaped operator kernels")
        return _fused("pre_pair_mhd_continuity_f32", lambda d, o, flags: _lib.load_pair().pre_pair_mhd_continuity_f32(
            _arr(d[0]), _arr(d[1]), ctypes.byref(_lib.field(o)), *tail, *o.shape, flags, _lib.stream()),
            ([vars[:, i] for i in range(n)], [minus[:, i] for i in range(n)]), absolute, out, False, halo_x, 'mhd')

    def _residual(self, eq, idx, composed, vars, boundary, absolute, halo_x, out, minus):
        """``residual_<eq>`` of the fields ``vars[:, idx]``.  With ``minus=``: one pass (continuity), else TWO-PASS - the
        single-set fused pass of ``vars`` into the result (``out`` if given), that of ``minus`` into one scratch buffer, an
        in-place subtract (or |.|) - else the composed difference."""
        sets = (tuple(vars[:, i] for i in idx),)
        if self.bc is not None:
            if halo_x:
                raise ValueError("bc with halo_x=True: an x-slab with a wrapped x is not served under boundary conditions")
            if minus is not None:
                _check_minus(vars, minus)
            # (the entry takes the six views whatever the equation reads; with fewer the fields of the equation compose)
            six = vars.dim() == 5 and vars.shape[1] >= 6
            pick = (lambda *f: composed(*[f[i] for i in idx])) if six else composed
            views = lambda v: tuple(v[:, i] for i in (range(6) if six else idx))
            return _bc_residual("mhd_" + eq, self.bc, 3, views(vars), None if minus is None else views(minus), pick,
                                (self.D_t, self.D_x, self.D_y),
                                lambda d, o, ks, st, flags: _lib.load_bcres().pre_bcres_mhd_f32(
                                    _MHD_EQ[eq], _arr(d), _fld(o), *ks, float(self.gamma), ctypes.byref(st), *o.shape, flags,
                                    _lib.stream()) if six else _lib.PRE_E_UNSUPPORTED,
                                boundary, absolute, out, self.fused)
        _no_bc()
        if minus is None:
            return _tail(self._fused(eq, vars, absolute, halo_x, out), sets, composed, boundary, _CROP3, absolute)
        _check_minus(vars, minus, device_view=halo_x)
        res = self._fused(eq, vars, absolute, halo_x, out, minus) if eq == 'continuity' else None
        if res is None:
            res = _two_pass(lambda f, first: self._fused(eq, f[0], False, halo_x, out if first else None), (vars,), (minus,),
                            absolute)
        sets += (tuple(minus[:, i] for i in idx),)
        return _tail(res, sets, composed, boundary, _CROP3, absolute, (getattr(self, 'residual_' + eq), vars, minus))

    def residual_continuity(self, vars, boundary=False, absolute=False, halo_x=False, out=None, minus=None):
        """``minus``: r(vars) - r(minus) in one pass (``pre_pair_mhd_continuity_f32``)."""
        D_t, D_x, D_y = self.D_t, self.D_x, self.D_y

        def composed(rho, u, v):
            return D_t(rho) + u*D_x(rho) + rho*D_x(u) + v*D_y(rho) + rho*D_y(v)
        return self._residual('continuity', (0, 1, 2), composed, vars, boundary, absolute, halo_x, out, minus)

    def residual_momentum(self, vars, boundary=False, absolute=False, halo_x=False, out=None, minus=None):
        """``minus``: r(vars) - r(minus), TWO-PASS (see ``_residual``)."""
        D_t, D_x, D_y = self.D_t, self.D_x, self.D_y

        def composed(rho, u, v, p, Bx, By):
            res_x = D_t(u) + u*D_x(u) + (1/rho)*D_x(p) - 2*(Bx/rho)*D_x(Bx) + v*D_y(u) - (By/rho)*D_y(Bx) - (Bx/rho)*D_y(By)
            res_y = D_t(v) + u*D_x(v) + (1/rho)*D_y(p) - 2*(By/rho)*D_y(By) + v*D_y(v) - (By/rho)*D_x(Bx) - (Bx/rho)*D_x(By)
            return res_x + res_y
        return self._residual('momentum', range(6), composed, vars, boundary, absolute, halo_x, out, minus)

    def residual_energy(self, vars, boundary=False, absolute=False, halo_x=False, out=None, minus=None):
        """``minus``: r(vars) - r(minus), TWO-PASS (see ``_residual``)."""
        D_t, D_x, D_y, gamma = self.D_t, self.D_x, self.D_y, self.gamma

        def composed(rho, u, v, p, Bx, By):
            p_gas = p - 0.5*(Bx**2 + By**2)
            return (D_t(rho) + u*D_x(p) + v*D_y(p) + (gamma-2)*(u*Bx+v*By)*(D_x(Bx) + D_y(By))
                    + (gamma*p_gas+By**2)*D_x(u) + (gamma*p_gas+Bx**2)*D_y(v) - Bx*By*(D_y(u) + D_x(v)))
        return self._residual('energy', range(6), composed, vars, boundary, absolute, halo_x, out, minus)

    def residual_induction(self, vars, boundary=False, absolute=False, halo_x=False, out=None, minus=None):
        """``minus``: r(vars) - r(minus), TWO-PASS (see ``_residual``)."""
        D_t, D_x, D_y = self.D_t, self.D_x, self.D_y

        def composed(u, v, Bx, By):
            res_x = D_t(Bx) - By*D_y(u) + Bx*D_y(v) - v*D_y(Bx) + u*D_y(By)
            res_y = D_t(By) + By*D_x(u) - Bx*D_x(v) - v*D_x(Bx) + u*D_x(By)
            return res_x + res_y
        return self._residual('induction', (1, 2, 4, 5), composed, vars, boundary, absolute, halo_x, out, minus)

    def residual_gauss(self, vars, boundary=False, absolute=False, minus=None):
        """``minus``: r(vars) - r(minus) in one pass (``pre_pair_linear2_f32``)."""
        return self._linear2(4, 5, 1.0, lambda Bx, By: self.D_x(Bx) + self.D_y(By), self.residual_gauss,
                             vars, minus, boundary, absolute)


# ======================================================================= reduced MHD (JOREK)
class JOREK:
    """``Marginal/JOREK_residuals_CP.py:188-243`` (twin ``Joint/JOREK_residuals_CP.py``): continuity and temperature
    residuals of the reduced-MHD fields (rho, phi, T) on an (R, Z) grid.

    ``vars`` is what the script holds, [BS, F, Nx, Ny, Nt] (the surrogate's layout); like its ``unstack_fields``
    (:84-95) every field is taken as the [BS, Nt, Nx, Ny] permuted view, zero-copy.  ``R`` is the 1-D radius grid
    tensor; the script's expressions broadcast it along the LAST axis of those views (its grid is square), and so
    does this class - ``len(R)`` must equal Ny.  The five operators are built as the script builds them (:201-205):
    ``D_t`` with ``scale=alpha``, ``D_R`` / ``D_Z`` with ``scale=beta`` and ``D_RR`` / ``D_ZZ`` with the value the
    name ``gamma`` holds at that point of the script - already the adiabatic index (:199), hence the default
    ``lap_scale=None`` -> ``gamma``.  ``domain='y'`` carries the reference's kernel (taps along Nt).  All five
    ``.kernel`` tensors may be replaced by the caller; the fused route hands the current ones to the library."""

    def __init__(self, R, D=3.4, K=2.25 * 1e-7, gamma=5 / 3, alpha=1, beta=1, lap_scale=None, dx=None, dy=None, dt=None,
                 device='cpu', fused=True, y_axis_fix=False):
        self.fused = fused
        self.R = torch.as_tensor(R, dtype=torch.float32)
        self.D, self.K, self.gamma = D, K, gamma
        self.dx, self.dy, self.dt = dx, dy, dt
        lap = torch.tensor(gamma, dtype=torch.float32) if lap_scale is None else lap_scale
        self.D_t = ConvOperator2D(domain='t', order=1, scale=alpha, device=device)
        self.D_R = ConvOperator2D(domain='x', order=1, scale=beta, device=device)
        self.D_Z = ConvOperator2D(domain='y', order=1, scale=beta, device=device, y_axis_fix=y_axis_fix)
        self.D_RR = ConvOperator2D(domain='x', order=2, scale=lap, device=device)
        self.D_ZZ = ConvOperator2D(domain='y', order=2, scale=lap, device=device, y_axis_fix=y_axis_fix)

    @staticmethod
    def unstack_fields(vars):
        """The script's ``unstack_fields(vars, axis=1, ...)``: [BS,F,Nx,Ny,Nt] -> F views [BS,Nt,Nx,Ny]."""
        return [vars[:, i].permute(0, 3, 1, 2) for i in range(vars.shape[1])]

    def _ops(self):
        return (self.D_t, self.D_R, self.D_Z, self.D_RR, self.D_ZZ)

    def _t32(self, x, like):
        return torch.as_tensor(x, dtype=torch.float32).to(like.device)

    def _R_view(self, f0):
        """R as one more field view that repeats its row, for the device field view ``f0`` [BS,Nt,Nx,Ny]: unit stride on the
        axis the fields are contiguous on.  None: no layout of R goes with the fields'.  Shared by the residual pass and the
        fused screen (``screen._Spec``); raises before any launch if ``len(R)`` is not Ny."""
        if self.R.numel() != f0.shape[3]:
            raise RuntimeError(f"R has {self.R.numel()} points, the fields' last axis {f0.shape[3]} (the reference "
                               "broadcasts its 1-D R along the last axis)")
        Rd = self.R.to(f0.device)
        if f0.stride(3) == 1:
            return Rd.view(1, 1, 1, -1).expand(f0.shape)
        if f0.stride(1) == 1:                                             # Nt fastest (the surrogate's memory order)
            return Rd.view(-1, 1).expand(-1, f0.shape[1]).contiguous().as_strided(tuple(f0.shape), (0, 1, 0, f0.shape[1]))
        return None

    def _coef(self, eq, norms=False):
        """The four scalars a0..a3 ``pre_residual_jorek_f32`` takes for equation ``eq`` (0 continuity, 1 temperature): the
        script's scalars, folded in fp32 in its own order of operations."""
        t = lambda v: torch.tensor(v, dtype=torch.float32)
        if eq == 1:
            return [float(2 * t(self.gamma)), 0.0, 0.0, float(t(self.K))]
        if norms:
            dx, dy, dt, D = t(self.dx), t(self.dy), t(self.dt), t(self.D)
            return [float(2*dx*dy), float(dt), float((2*dt*dy)*2), float((4*dt)*D)]
        return [1.0, 1.0, 2.0, float(t(self.D))]

    def _fused(self, eq, fields, coef, absolute):
        """One streaming pass (``pre_residual_jorek_f32``); None -> compose.  No ``out`` / ``halo_x`` here."""
        if not self.fused or any(f.numel() == 0 for f in fields) or \
                _dispatch.needs_grad(*[getattr(o, "kernel", None) for o in self._ops()]):
            return None
        ks = [_dispatch.dense27(o.kernel) for o in self._ops()]
        if any(k is None for k in ks):
            return None

        def call(d, out, flags):
            devs, f0 = d[0], d[0][0]
            Rb = self._R_view(f0)
            if Rb is None:
                return _lib.PRE_E_UNSUPPORTED                             # (no layout of R to go with the fields': compose)
            return _lib.load().pre_residual_jorek_f32(
                eq, _arr([devs[i] if i < len(devs) else devs[0] for i in range(3)]), ctypes.byref(_lib.field(Rb)),
                ctypes.byref(_lib.field(out)), *ks, _lib.farr(coef), *out.shape, flags, _lib.stream())
        return _fused("pre_residual_jorek_f32", call, (fields,), absolute)

    def _residual(self, eq, fa, composed, coef, method, vars, minus, boundary, absolute):
        """How both equations end.  ``minus``: r(vars) - r(minus), TWO-PASS: the single-set fused pass of each set, then an
        in-place subtract (or |.|)."""
        _no_bc()
        if minus is None:
            return _tail(self._fused(eq, fa, coef, absolute), (fa,), composed, boundary, _CROP3, absolute)
        _check_minus(vars, minus)
        fb = tuple(self.unstack_fields(minus)[:len(fa)])
        res = _two_pass(lambda f, first: self._fused(eq, tuple(f), coef, False), fa, fb, absolute)
        return _tail(res, (fa, fb), composed, boundary, _CROP3, absolute, (method, vars, minus))

    def residual_continuity(self, vars, boundary=False, norms=False, absolute=False, minus=None):
        """:207-221.  ``minus``: r(vars) - r(minus), two-pass (``_residual``)."""
        D_t, D_R, D_Z, D_RR, D_ZZ = self._ops()
        rho, phi, _ = self.unstack_fields(vars)
        if norms and (self.dx is None or self.dy is None or self.dt is None):
            raise ValueError("norms=True needs dx, dy, dt")

        def composed(rho, phi):
            R, D = self._t32(self.R, rho), self._t32(self.D, rho)
            if norms:
                dx, dy, dt = (self._t32(v, rho) for v in (self.dx, self.dy, self.dt))
                return 2*dx*dy*D_t(rho) - (dt)*R*(D_R(rho)*D_Z(phi) - D_R(phi)*D_Z(rho)) - (2*dt*dy)*2*rho*D_Z(phi) \
                    - (4*dt)*D*(D_RR(rho) + (1/R)*D_R(rho) + D_ZZ(rho))
            return D_t(rho) - R*(D_R(rho)*D_Z(phi) - D_R(phi)*D_Z(rho)) - 2*rho*D_Z(phi) \
                - D*(D_RR(rho) + (1/R)*D_R(rho) + D_ZZ(rho))
        return self._residual(0, (rho, phi), composed, self._coef(0, norms),
                              lambda x, b: self.residual_continuity(x, b, norms),
                              vars, minus, boundary, absolute)

    def residual_temperature(self, vars, boundary=False, norms=False, absolute=False, minus=None):
        """:224-243.  ``minus``: r(vars) - r(minus), two-pass (``_residual``)."""
        if norms:
            raise Exception("Norm not implemented yet")              # (as the reference, :230)
        D_t, D_R, D_Z, D_RR, D_ZZ = self._ops()
        rho, phi, T = self.unstack_fields(vars)

        def composed(rho, phi, T):
            R, K, gamma = self._t32(self.R, rho), self._t32(self.K, rho), self._t32(self.gamma, rho)
            return T*D_t(rho) + rho*D_t(T) - rho*R*(D_R(T)*D_Z(phi) - D_R(phi)*D_Z(T)) + \
                T*R*(D_R(rho)*D_Z(phi) - D_R(phi)*D_Z(rho)) + \
                2*gamma*rho*T*D_Z(phi) + \
                K * (D_RR(T) + (1/R)*D_R(T) + D_ZZ(T))
        return self._residual(1, (rho, phi, T), composed, self._coef(1), self.residual_temperature, vars, minus, boundary, absolute)


class PRE_MHD(MHD):
    """``Other_UQ/Evaluation/PRE_estimations.py:54-80``: the energy equation."""

    def __init__(self, dt, dx, dy, **kw):
        super().__init__(gamma=5 / 3, **kw)
        self.dt, self.dx, self.dy = dt, dx, dy

    def residual(self, vars, boundary=False, minus=None):
        return self.residual_energy(vars, boundary, minus=minus)


# ======================================================================= linear: wave / advection
class PRE_Wave:
    """``Other_UQ/Evaluation/PRE_estimations.py:5-21`` / ``Marginal/Wave_Residuals_CP.py:170-184``:
    ONE additive kernel ``D_tt - (c dt/dx)^2 D_xx_yy`` applied in one pass."""

    def __init__(self, dt, dx, c=1.0, device='cpu', bc=None):
        self.bc = None if bc is None else _BC(bc)
        D_tt = ConvOperator2D('t', 2, device=device)
        D_xx_yy = ConvOperator2D(('x', 'y'), 2, device=device)
        self.D = ConvOperator2D()
        c = torch.tensor(c, dtype=torch.float32)
        self.D.kernel = D_tt.kernel - ((c * dt / dx) ** 2).to(device) * D_xx_yy.kernel

    def residual(self, uu, boundary=False, absolute=False, halo_x=False, out=None, minus=None):
        """``minus``: r(uu) - r(minus) in one pass of both fields (``pre_pair_stencil3d_f32``); ``halo_x`` / ``out`` apply
        to both (two single-field passes and an in-place subtract where the paired pass declines).
        ``out``: optional fp32 device tensor of the field's shape for the uncropped residual (any batch stride over dense
        [Nt,Nx,Ny] blocks: ``pipeline.row_padded`` - the per-cell select that follows is 4 % faster on rows that are not
        a power of two apart).  ``halo_x``: ``uu`` is an x-slab ``full[..., x0:x1, :]`` whose rows x0 - 1 and x1 lie in the same device memory and
        are read instead of the zero padding (``PRE_FLAG_HALO_X``, see ``NavierStokes.residual_momentum``)."""
        if minus is not None:
            _check_minus(uu, minus, device_view=halo_x)
            minus = minus[:, 0] if minus.dim() == 5 else minus
        uu = uu[:, 0] if uu.dim() == 5 else uu
        if self.bc is not None:
            if halo_x:
                raise ValueError("bc with halo_x=True: an x-slab with a wrapped x is not served under boundary conditions")
            return _bc_residual("linear1", self.bc, 3, (uu,), None if minus is None else (minus,), lambda u: self.D(u), (self.D,),
                                _bc_linear1, boundary, absolute, out)
        _no_bc()
        flags = (_lib.PRE_FLAG_ABS if absolute else 0) | (_lib.PRE_FLAG_HALO_X if halo_x else 0)
        if minus is not None:
            return self._minus(uu, minus, boundary, absolute, halo_x, out, flags)
        if halo_x and not (uu.is_cuda and uu.stride(-1) == 1 and not _dispatch.needs_grad(uu, self.D.kernel)):
            raise ValueError("halo_x needs a device-resident, Ny-contiguous view of a larger grid and no autograd")
        if out is not None:
            if _dispatch.needs_grad(uu, self.D.kernel) or not uu.is_cuda:
                raise ValueError("out needs a device-resident field and no autograd")
            res = _dispatch._xcorr_impl(uu, self.D.kernel, 3, flags, out=out)
        else:
            res = _dispatch.xcorr(uu, self.D.kernel, nd=3, flags=flags)  # (raises if no kernel reads the halo rows)
        return res if boundary else res[_CROP3]

    def _minus(self, uu, mm, boundary, absolute, halo_x, out, flags):
        if _dispatch.needs_grad(uu, mm, self.D.kernel):
            if halo_x or out is not None:
                raise ValueError("halo_x / out need device-resident fields and no autograd")
            return _pair_composed(lambda x, b: self.residual(x, b), uu, mm, boundary, _CROP3, absolute)
        if (halo_x or out is not None) and not (uu.is_cuda and mm.is_cuda):
            raise ValueError("halo_x / out need device-resident fields and no autograd")
        (uu, origin), (mm, _) = _dispatch.to_device(uu), _dispatch.to_device(mm)
        res = _dispatch.xcorr_pair(uu, mm, self.D.kernel, 3, flags, out=out)
        if res is None:
            # two-pass: r(uu) into the result, r(mm) into a scratch buffer.  PRE_FLAG_ABS is stripped from the two passes:
            # |.| applies to the difference, after the subtraction
            res = _two_pass(lambda f, first: _dispatch._xcorr_impl(f[0], self.D.kernel, 3, flags & _lib.PRE_FLAG_HALO_X,
                                                                  out=out if first else None), (uu,), (mm,), absolute)
        res = _dispatch.from_device(res, origin)
        return res if boundary else res[_CROP3]


class Advection:
    """``Marginal/Advection_Residuals_CP.py:156-164,234-235``: ``D_t + (v disc dt/dx) D_x`` on [BS,Nt,Nx]."""

    def __init__(self, v, dt, dx, disc=2, device='cpu', bc=None):
        self.bc = None if bc is None else _BC(bc)
        D_t = ConvOperator1D(domain='t', order=1, device=device)
        D_x = ConvOperator1D(domain='x', order=1, device=device)
        self.D = ConvOperator1D()
        self.D.kernel = D_t.kernel + (v * disc * dt / dx) * D_x.kernel

    def residual(self, uu, boundary=False, absolute=False, minus=None):
        """``minus``: r(uu) - r(minus) in one pass of both fields (``pre_pair_stencil2d_f32``)."""
        if self.bc is not None:
            if minus is not None:
                _check_minus(uu, minus)
            sq = lambda x: x[:, 0] if x is not None and x.dim() == 4 and x.shape[1] == 1 else x
            return _bc_residual("linear1_rows", self.bc, 2, (sq(uu),), None if minus is None else (sq(minus),),
                                lambda u: self.D(u), (self.D,), _bc_linear1_rows, boundary, absolute)
        _no_bc()
        if minus is not None:
            _check_minus(uu, minus)
            res = None
            if not _dispatch.needs_grad(uu, minus, self.D.kernel):
                res = _dispatch.xcorr_pair(uu, minus, self.D.kernel, 2, _lib.PRE_FLAG_ABS if absolute else 0)
            if res is None:
                return _pair_composed(lambda x, b: self.residual(x, b), uu, minus, boundary, _CROP2, absolute)
            return res if boundary else res[_CROP2]
        res = _dispatch.xcorr(uu, self.D.kernel, nd=2, flags=_lib.PRE_FLAG_ABS if absolute else 0)
        return res if boundary else res[_CROP2]


# ======================================================================= Burgers (1-D)
class Burgers:
    """``Joint/Burgers_Residuals_CP.py:171-187``:
    ``dx*D_t(u) + dt*u*D_x(u) - nu*D_xx(u)*(2*dt/dx)`` on [BS,Nt,Nx]."""

    def __init__(self, dx, dt, nu, device='cpu', fused=True, bc=None):
        self.fused = fused
        self.bc = None if bc is None else _BC(bc)
        self.D_t = ConvOperator1D(domain='t', order=1, device=device)
        self.D_x = ConvOperator1D(domain='x', order=1, device=device)
        self.D_xx = ConvOperator1D(domain='x', order=2, device=device)
        # the script turns the three coefficients into fp32 0-d tensors first
        self.dx, self.dt, self.nu = (torch.tensor(v, dtype=torch.float32) for v in (dx, dt, nu))

    def residual(self, uu, boundary=False, absolute=False, minus=None):
        """``minus``: r(uu) - r(minus) in one pass of both fields (``pre_pair_burgers_f32``)."""
        dx, dt, nu = self.dx, self.dt, self.nu
        def composed(uu):
            dxd, dtd, nud = (c.to(uu.device) for c in (dx, dt, nu))
            return dxd * self.D_t(uu) + dtd * uu * self.D_x(uu) - nud * self.D_xx(uu) * (2 * dtd / dxd)
        if self.bc is not None:
            if minus is not None:
                _check_minus(uu, minus)
            sq = lambda x: x[:, 0] if x is not None and x.dim() == 4 and x.shape[1] == 1 else x
            scal = (float(dx), float(dt), float(nu), float(2 * dt / dx))           # (2 dt / dx in fp32 like the reference)
            return _bc_residual("burgers", self.bc, 2, (sq(uu),), None if minus is None else (sq(minus),), composed,
                                (self.D_t, self.D_x, self.D_xx),
                                lambda d, o, ks, st, flags: _lib.load_bcres().pre_bcres_burgers_f32(
                                    _lib.ptr(d[0]), _lib.iarr64(d[0].stride()), _lib.ptr(o), _lib.iarr64(o.stride()), *ks, *scal,
                                    ctypes.byref(st), *o.shape, flags, _lib.stream()), boundary, absolute, fused=self.fused)
        _no_bc()
        # (the fused entries take [BS,Nt,Nx] only: a [BS,1,Nt,Nx] field composes)
        fused = self.fused and uu.numel() > 0 and uu.dim() == 3 and \
            not _dispatch.needs_grad(self.D_t.kernel, self.D_x.kernel, self.D_xx.kernel)
        ks = [_dispatch.dense9(o.kernel) for o in (self.D_t, self.D_x, self.D_xx)] if fused else [None]
        sets, pair, name, load = ((uu,),), None, "pre_residual_burgers_f32", _lib.load
        if minus is not None:
            _check_minus(uu, minus)
            sets, pair = ((uu,), (minus,)), (lambda x, b: self.residual(x, b), uu, minus)
            name, load = "pre_pair_burgers_f32", _lib.load_pair
        res = None
        if all(k is not None for k in ks):
            tail = (*ks, float(dx), float(dt), float(nu), float(2 * dt / dx))      # (2 dt / dx in fp32 like the reference)
            res = _fused(name, lambda d, o, flags: getattr(load(), name)(
                *[x for t in [s[0] for s in d] + [o] for x in (_lib.ptr(t), _lib.iarr64(t.stride()))], *tail, *o.shape, flags,
                _lib.stream()), sets, absolute)
        return _tail(res, sets, composed, boundary, _CROP2, absolute, pair)


# ======================================================================= boundary conditions on the x-y rim (bc=)
# r_bc(fields) = r_zero_pad(pad(f) for f in fields)[..., :, 1:-1, 1:-1]: ``pad`` is ``BoundaryManager(3).pad_signal`` on each
# [BS,Nt,Nx,Ny] field (Utils/boundary_conditions.py; Nt rides as the channel axis), the time axis keeps its zero padding.
# FUSED: one pass of ``libcp_pre_bcres.so`` (include/cp_pre_bcres.h) - the march and the functors of the zero-pad passes,
# the out-of-domain neighbour of a rim cell mapped by the kernel, no padded copy.  COMPOSED (the fallback, and the
# recomputation under autograd): pad every field, the composed operators on the padded grid, crop.  ``last_route()`` says
# which ran and why.
_route = None


def last_route():
    """The route of the last residual call in this process: ``'fused:bc_<kind>'``, ``'fallback:<why>'``, or None when that
    call had no ``bc``."""
    return _route


def _no_bc():
    global _route
    _route = None


class _BC:
    """A normalised ``bc=``: ``'wrap'`` (true periodicity on all four sides, ``F.pad(mode='circular')``; opt-in and no
    parity claim, like ``y_axis_fix``), or the reference's ``pad_signal`` semantics given as a ``BoundaryManager`` (held, not
    copied: later changes of its sides count), a type name for all four sides, or a dict ``side -> type | (type, value)``
    (sides left out are 'periodic', the manager's default).  A list / tuple with one such entry per field is accepted and
    always composes (the fused entries take one condition for every field)."""

    def __init__(self, bc):
        from .boundary_conditions import BoundaryManager
        self.wrap, self.manager, self.per_field = False, None, None
        if isinstance(bc, _BC):
            self.wrap, self.manager, self.per_field = bc.wrap, bc.manager, bc.per_field
        elif isinstance(bc, str) and bc == 'wrap':
            self.wrap = True
        elif isinstance(bc, (list, tuple)):
            self.per_field = [_BC(b) for b in bc]
        elif isinstance(bc, str):
            self.manager = BoundaryManager(3)
            self.manager.set_all_boundaries(bc)
        elif isinstance(bc, dict):
            self.manager = BoundaryManager(3)
            for side, v in bc.items():
                t, value = v if isinstance(v, (tuple, list)) else (v, 0.0)
                self.manager.set_boundary_type(side, t, value)
        elif hasattr(bc, 'pad_signal') and hasattr(bc, 'boundary_types') and hasattr(bc, 'boundary_values'):
            self.manager = bc
        else:
            raise TypeError("bc must be 'wrap', a boundary type name, a dict side -> type | (type, value), or a BoundaryManager")
        m = self.manager
        if m is not None and not (m.pad_left == m.pad_right == m.pad_top == m.pad_bottom == 1):
            raise ValueError("bc: the residual stencils have radius 1, the BoundaryManager must pad one cell per side "
                             "(kernel_size=3)")

    def _rows(self):
        """The manager of the 1-D family: left / right act on Nx, the rows (time) keep the zero padding."""
        from .boundary_conditions import BoundaryManager
        m = BoundaryManager((1, 3))
        for s in ('left', 'right'):
            m.boundary_types[s], m.boundary_values[s] = self.manager.boundary_types[s], self.manager.boundary_values[s]
        return m

    def pad(self, f, nd, i=0):
        """Field i padded by one cell per side of x and y (``nd == 3``, [BS,Nt,Nx,Ny]) or of x (``nd == 2``, [BS,Nt,Nx])."""
        if self.per_field is not None:
            return self.per_field[i].pad(f, nd)
        if self.wrap:
            return torch.nn.functional.pad(f, (1, 1, 1, 1) if nd == 3 else (1, 1), mode='circular')
        if nd == 3:
            return self.manager.pad_signal(f)
        return self._rows().pad_signal(f[:, None])[:, 0]

    def free_slip(self, nd=3):
        """Does a side the residuals of ``nd`` axes pad (all four; left / right for the 1-D family), of any field's condition,
        have 'free_slip'?  The reference pads nothing there: the residual under it has not the field's extents."""
        if self.per_field is not None:
            return any(b.free_slip(nd) for b in self.per_field)
        if self.manager is None:
            return False
        sides = ('left', 'right', 'top', 'bottom') if nd == 3 else ('left', 'right')
        return any(str(self.manager.boundary_types[s]).lower() == 'free_slip' for s in sides)

    def struct(self, nd):
        """(``pre_bc_t``, None) or (None, why the fused entries cannot take this condition)."""
        from .vector_convops_spatial import _bc_struct
        if self.per_field is not None:
            return None, "per-field boundary conditions"
        if self.wrap:
            return _lib.PreBC((ctypes.c_int * 4)(*([_lib.PRE_BC_PERIODIC] * 4)), (ctypes.c_float * 4)()), None
        m = self.manager
        if nd == 2:
            m = self._rows()
            m.pad_top = m.pad_bottom = 1                           # (for _bc_struct only: the rows are the constant 0)
            m.boundary_types.update(top='dirichlet', bottom='dirichlet')
        if 'free_slip' in m.boundary_types.values():
            return None, "'free_slip' has no padding rule"
        st = _bc_struct(m)
        if st is None:
            return None, "mixed condition without a fused mapping"
        return st, None


def _bc_kernels(ops, dense):
    """(the dense kernels of ``ops`` as the entries take them, None) or (None, why not)."""
    if any(getattr(o, "kernel", None) is None for o in ops):
        return None, "operator without a kernel"
    if _dispatch.needs_grad(*[o.kernel for o in ops]):
        return None, "operator kernel requires grad"
    ks = [dense(o.kernel) for o in ops]
    if any(k is None for k in ks):
        return None, "operator kernel off the 7-point star"
    for o in ops:
        _, off = _dispatch.taps_of(_dispatch.host_kernel(o.kernel))
        if not _dispatch.is_star(off):
            return None, "operator kernel off the 7-point star"
    return ks, None


def _bc_single(kind, spec, nd, fields, composed, ops, launch, absolute, out, fused, flags0=0, force=None):
    """One field set under ``spec``: the result [BS,Nt,Nx(,Ny)] (uncropped in t) where the fields live.  ``launch(devs, out,
    ks, st, flags)`` runs the fused entry and returns its code; ``composed(*fields)`` is the zero-pad expression from single
    operators.  ``force``: a reason to compose whatever the inputs."""
    global _route
    for f in fields:
        _dispatch._check_field(f)

    def padded(*f):
        r = composed(*[spec.pad(x, nd, i) for i, x in enumerate(f)])
        return r[..., 1:-1, 1:-1] if nd == 3 else r[..., 1:-1]
    f0 = fields[0]
    ax = "Ny" if nd == 3 else "Nx"
    ks = st = None
    why = force
    if why is None and not fused:
        why = "fused=False"
    if why is None:
        st, why = spec.struct(nd)
    if why is None:
        ks, why = _bc_kernels(ops, _dispatch.dense27 if nd == 3 else _dispatch.dense9)
    if why is None and f0.numel() == 0:
        why = "empty batch"
    if why is None and f0.shape[-1] % 4 != 0:
        why = f"{ax} % 4 != 0"
    if why is None and any(f.stride(-1) != 1 for f in fields):
        why = f"no unit stride on {ax}"
    if why is None and not all(f.is_cuda for f in fields):
        why = "CPU inputs"
    given = out is not None
    if given and not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == tuple(f0.shape) and
                      out.stride(-1) == 1 and not _dispatch.needs_grad(*fields)):
        raise ValueError(f"out with bc must be an fp32 device tensor of the field shape with unit stride on {ax}, no autograd")
    if why is None:
        with torch.no_grad():
            res = out if given else torch.empty(tuple(f0.shape), dtype=torch.float32, device=f0.device)
            with torch.cuda.device(f0.device):
                rc = launch(list(fields), res, ks, st, flags0 | (_lib.PRE_FLAG_ABS if absolute else 0))
        if rc == _lib.PRE_E_UNSUPPORTED:
            why = "the library declines (layout, or a tap structure that is not built)"
        else:
            _lib.check(rc, "pre_bcres_" + kind)
            _route = "fused:bc_" + kind
            return _attach(res, (tuple(fields),), padded, absolute)
    _route = "fallback:" + why
    res = padded(*fields)               # (pure data movement where the fields live; each operator stages its own input)
    if absolute:
        res = res.abs()
    if given:
        out.copy_(res)
        res = out
    return res


def _bc_residual(kind, spec, nd, fields, minus, composed, ops, launch, boundary, absolute, out=None, fused=True, flags0=0):
    """How every residual under ``bc`` ends.  ``minus``: the second field set - r(fields) - r(minus) as two passes and an
    in-place subtract, composed when a field requires grad.  ``boundary=False`` crops the time rim only: the x-y rim is
    valid."""
    run = lambda f, a, o, force=None: _bc_single(kind, spec, nd, f, composed, ops, launch, a, o, fused, flags0, force)
    if minus is None:
        res = run(fields, absolute, out)
    elif _dispatch.needs_grad(*fields, *minus):
        if out is not None:
            raise ValueError("out with bc and minus= needs fields without autograd")
        res = run(fields, False, None, "minus= with a field that requires grad") - \
            run(minus, False, None, "minus= with a field that requires grad")
        res = res.abs() if absolute else res
    else:
        res = run(fields, False, out)
        b = run(minus, False, None)
        with torch.no_grad():
            res.sub_(b.to(res.device))
            if absolute:
                res.abs_()
    return res if boundary else res[:, 1:-1]


def _fld(t):
    return ctypes.byref(_lib.field(t))


def _bc_linear1(d, o, ks, st, flags):
    return _lib.load_bcres().pre_bcres_linear1_f32(_fld(d[0]), _fld(o), ks[0], ctypes.byref(st), *o.shape, flags, _lib.stream())


def _bc_linear1_rows(d, o, ks, st, flags):
    return _lib.load_bcres().pre_bcres_linear1_rows_f32(_lib.ptr(d[0]), _lib.iarr64(d[0].stride()), _lib.ptr(o),
                                                        _lib.iarr64(o.stride()), ks[0], ctypes.byref(st), *o.shape, flags,
                                                        _lib.stream())


def apply_bc(D, field, bc):
    """A bare operator under boundary conditions: ``D(pad(field))`` cropped back to the field's shape - ``D`` a
    ``convops_2d.ConvOperator`` on [BS,Nt,Nx,Ny] (any star kernel, taps along Nt included) or a ``convops_1d.ConvOperator``
    on [BS,Nt,Nx].  ``ConvOperator.__call__`` itself stays the zero-padded operator."""
    nd = field.dim() - 1
    if nd not in (2, 3):
        raise RuntimeError(f"expected a [BS,Nt,Nx] or [BS,Nt,Nx,Ny] field, got {tuple(field.shape)}")
    return _bc_residual("linear1" if nd == 3 else "linear1_rows", _BC(bc), nd, (field,), None, lambda u: D(u), (D,),
                        _bc_linear1 if nd == 3 else _bc_linear1_rows, True, False)
