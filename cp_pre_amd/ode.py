"""Fused ODE residuals: ``out[b,t] = sum_i c_i[t] * (K_i * x_i)[b,t]`` in one HIP pass (``pre_ode_residual_f32``).

The reference's ODE scripts build their residuals from ``Utils/ConvOps_0d.py`` operators, one ``F.conv1d`` (or FFT)
pass per operator plus elementwise passes to scale and sum them.  ``ODEResidual`` evaluates the whole sum in one pass
over the state: terms on the same field share one load of it, and the components of one [BS,Nt,S] state tensor are
read where they lie.  The constructors below restate each script's operator algebra statement for statement:

    SHO(omega, dt)                 Inverse_residuals/SHO/SHO_node_test.py:334-342   (m = 1, k = omega^2)
    DHO(m, c, k, dt)               Inverse_residuals/DHO/DHO_NODE.py:475-482        (combined, on x)
    DHO(m, c, k, dt, split=True)   Inverse_residuals/DHO/DHO_NODE.py:509-515        D_R1(v) + D_R2(x)
    DHO_kinematic(dt)              Inverse_residuals/DHO/DHO_NODE.py:559-565        -D_R4(v) + D_R3(x)
    Bessel(x, n, dx)               Inverse_residuals/Bessel/Bessel_NODE.py:493-518

A state is a [BS,Nt,S] tensor (a term's component indexes its last axis; x is component 0, v component 1) or a list
of [BS,Nt] fields (a component indexes the list).  CPU tensors and numpy arrays are staged through the GPU and the
result comes back where the state came from.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _dispatch, _lib
from .convops_0d import ConvOperator, conv1d, host_taps


class ODEResidual:
    """``terms``: up to 6 ``(component, kernel, coeff)``; ``kernel`` a 1-D fp32 stencil of odd length <= 7 (tensor, array
    or sequence), ``coeff`` None (1) or a per-step row of Nt values."""

    def __init__(self, terms):
        terms = list(terms)
        if not 1 <= len(terms) <= _lib.PRE_ODE_MAX_TERMS:
            raise ValueError(f"an ODE residual has 1 to {_lib.PRE_ODE_MAX_TERMS} terms, got {len(terms)}")
        self.terms = []
        for term in terms:
            if len(term) != 3:
                raise ValueError("a term is (component, kernel, coeff)")
            comp, kernel, coeff = term
            if isinstance(comp, bool) or not isinstance(comp, (int, np.integer)) or comp < 0:
                raise IndexError(f"a term's component must be a non-negative int, got {comp!r}")
            k = kernel if isinstance(kernel, torch.Tensor) else torch.as_tensor(np.asarray(kernel, dtype=np.float32))
            k = k.detach().to(torch.float32)
            if k.dim() != 1 or k.numel() % 2 == 0 or k.numel() > _lib.PRE_ODE_MAX_TAPS:
                raise ValueError(f"a term's kernel is 1-D with an odd length <= {_lib.PRE_ODE_MAX_TAPS}, got shape "
                                 f"{tuple(k.shape)}")
            c = None
            if coeff is not None:
                c = coeff if isinstance(coeff, torch.Tensor) else torch.as_tensor(np.asarray(coeff, dtype=np.float32))
                c = c.detach().to(torch.float32).reshape(-1)
            self.terms.append((int(comp), k.cpu(), host_taps(k.cpu()), c))
        self._rows = {}                                     # (term, device) -> dense device coefficient row

    def _coeff(self, i, device, nt):
        c = self.terms[i][3]
        if c is None:
            return None
        if c.numel() != nt:
            raise ValueError(f"term {i}: the coefficient row has {c.numel()} values, the state has Nt = {nt}")
        key = (i, str(device))
        row = self._rows.get(key)
        if row is None:
            row = self._rows[key] = c.to(device).contiguous()
        return row

    @staticmethod
    def _fields(state):
        """(list of [BS,Nt] fp32 views, to numpy?, as a list?)"""
        is_np = isinstance(state, np.ndarray)
        if isinstance(state, (list, tuple)):
            fs = [torch.as_tensor(f) if isinstance(f, np.ndarray) else f for f in state]
            return fs, isinstance(state[0], np.ndarray) if len(state) else False, True
        t = torch.as_tensor(state) if is_np else state
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError("the state is a [BS,Nt,S] tensor or a list of [BS,Nt] fields")
        return [t[..., s] for s in range(t.shape[-1])], is_np, False

    def _select(self, fields):
        n = len(fields)
        for comp, *_ in self.terms:
            if comp >= n:
                raise IndexError(f"component {comp} is out of range for a state of {n} components")
        for f in fields:
            _dispatch._check_field(f)
            if f.dim() != 2 or f.shape != fields[0].shape:
                raise ValueError(f"every field of the state is [BS,Nt] of one shape, got {tuple(f.shape)}")

    def residual(self, state, absolute=False, out=None):
        """The residual [BS,Nt] (``absolute``: its |.|, the marginal score).  ``out``: an fp32 device [BS,Nt] tensor to write
        into, any non-overlapping strides (``pipeline.row_padded((BS,), (Nt,))`` included)."""
        fields, to_np, _ = self._fields(state)
        self._select(fields)
        bs, nt = fields[0].shape
        on_host = not fields[0].is_cuda
        if on_host:
            _lib.require_gpu()
        src = state if isinstance(state, torch.Tensor) else None
        if src is not None and on_host:
            dev_state = src.cuda()
            devs = [dev_state[..., s] for s in range(dev_state.shape[-1])]
        else:
            devs = [f if f.is_cuda else f.cuda() for f in fields]
        device = devs[0].device
        if out is None:
            res = torch.empty((bs, nt), dtype=torch.float32, device=device)
        else:
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (bs, nt)):
                raise ValueError("out must be an fp32 device tensor of shape [BS,Nt]")
            res = out

        def fused():
            if res.numel():
                arr = (_lib.PreOdeTerm * len(self.terms))()
                for i, (comp, _, taps, _c) in enumerate(self.terms):
                    f = devs[comp]
                    row = self._coeff(i, device, nt)
                    arr[i].x, arr[i].sB, arr[i].sT = f.data_ptr(), f.stride(0), f.stride(1)
                    arr[i].c = row.data_ptr() if row is not None else None
                    arr[i].k = len(taps)
                    for j, w in enumerate(taps):
                        arr[i].taps[j] = float(w)
                with torch.cuda.device(device):
                    rc = _lib.load_ode().pre_ode_residual_f32(arr, len(self.terms), _lib.ptr(res), _lib.iarr64(res.stride()),
                                                              bs, nt, _lib.PRE_ODE_FLAG_ABS if absolute else 0, _lib.stream())
                _lib.check(rc, "pre_ode_residual_f32")
            return res

        grads = [f for f in fields if isinstance(f, torch.Tensor)]
        if src is not None:
            grads = [src]
        r = _dispatch.fused_or_composed(fused, lambda *ts: self._composed(ts, absolute), *grads)
        if on_host and out is None:
            r = r.to(fields[0].device)
        return r.numpy() if to_np else r

    def _composed(self, ts, absolute):
        """The same sum term by term (HIP stencil per term, torch ops for the scaling and the sum), differentiable: what
        a backward through the fused pass recomputes."""
        fields = [ts[0][..., s] for s in range(ts[0].shape[-1])] if len(ts) == 1 and ts[0].dim() == 3 else list(ts)
        acc = None
        for i, (comp, kernel, _, _c) in enumerate(self.terms):
            f = fields[comp]
            f = f if f.is_cuda else f.cuda()
            y = conv1d(f, kernel)
            row = self._coeff(i, f.device, f.shape[1])
            if row is not None:
                y = row * y
            acc = y if acc is None else acc + y
        return acc.abs() if absolute else acc

    def composed(self, state, absolute=False):
        """The term-by-term route on its own (one stencil pass per term plus elementwise passes), for comparison."""
        fields, to_np, _ = self._fields(state)
        self._select(fields)
        r = self._composed(fields, absolute)
        if not fields[0].is_cuda:
            r = r.to(fields[0].device)
        return r.numpy() if to_np else r


# ---------------------------------------------------------------- the scripts' operators
def _ops():
    """``D_t``, ``D_tt`` and ``D_identity`` as the DHO / SHO scripts construct them (DHO_NODE.py:475-478)."""
    D_t = ConvOperator(order=1)
    D_tt = ConvOperator(order=2)
    D_identity = ConvOperator(order=0)
    D_identity.kernel = torch.tensor([0.0, 1.0, 0.0])
    return D_t, D_tt, D_identity


def SHO(omega, dt):
    """``m*D_tt.kernel + dt**2*k*D_identity.kernel`` on x (SHO_node_test.py:342) with m = 1, k = omega**2."""
    _, D_tt, D_identity = _ops()
    m, k = 1.0, omega ** 2
    return ODEResidual([(0, m * D_tt.kernel + dt ** 2 * k * D_identity.kernel, None)])


def DHO(m, c, k, dt, split=False):
    """Combined (DHO_NODE.py:482): ``2*m*D_tt + dt*c*D_t + 2*dt**2*k*I`` on x.  ``split=True`` (:509-515): ``D_R1(v) +
    D_R2(x)`` with ``D_R1 = m*D_t + 2*dt*c*I`` and ``D_R2 = 2*dt*k*I``."""
    D_t, D_tt, D_identity = _ops()
    if not split:
        return ODEResidual([(0, 2 * m * D_tt.kernel + dt * c * D_t.kernel + 2 * dt ** 2 * k * D_identity.kernel, None)])
    r1 = m * D_t.kernel + 2 * dt * c * D_identity.kernel
    r2 = 2 * dt * k * D_identity.kernel
    return ODEResidual([(1, r1, None), (0, r2, None)])


def DHO_kinematic(dt):
    """``- D_R4(v) + D_R3(x)`` (DHO_NODE.py:559-565): ``D_R3 = D_t`` on x, ``D_R4 = 2*dt*I`` on v (negated taps)."""
    D_t, _, D_identity = _ops()
    r3 = D_t.kernel
    r4 = 2 * dt * D_identity.kernel
    return ODEResidual([(1, -r4, None), (0, r3, None)])


def Bessel(x, n, dx):
    """``x^2*y'' + x*y' + (x^2 - n^2)*y`` on y (component 0), the loop of Bessel_NODE.py:502-516 as three terms: the
    central differences ``(y[i+1] - 2y[i] + y[i-1]) / dx**2`` and ``(y[i+1] - y[i-1]) / (2*dx)`` as scaled taps, and
    ``x**2``, ``x``, ``x**2 - n**2`` as coefficient rows.

    Difference from the loop: the loop leaves the two end points, and every point with ``|x| < 1e-6``, at 0; the fused
    form computes them like any other point (zero padding past the ends).  Compare on the interior with x != 0."""
    xs = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1)
    d_xx = torch.tensor([1.0, -2.0, 1.0], dtype=torch.float32) / (dx ** 2)
    d_x = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float32) / (2 * dx)
    ident = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32)
    return ODEResidual([(0, d_xx, xs ** 2), (0, d_x, xs), (0, ident, xs ** 2 - n ** 2)])
