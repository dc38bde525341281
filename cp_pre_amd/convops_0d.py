"""``ConvOperator`` for [BS,Nt] ODE trajectories: drop-in for ``Utils/ConvOps_0d.py:21-288``.

``convolution`` runs ``pre_ode_stencil_f32`` (``libcp_pre_ode.so``, ``include/cp_pre_ode.h``) instead of ``F.conv1d``
(``Utils/ConvOps_0d.py:103``): the field is read where it lies, so a component view ``sol[..., s]`` of a [BS,Nt,S] state
tensor costs no copy.  The spectral family stays on ``torch.fft`` (hipFFT underneath; ``libcp_pre_fft.so`` has no 1-D
plan), composed exactly as the reference composes it.

Reference behaviours kept on purpose (golden-tested, ``tests/golden/convops_0d.npz``):
  * ``get_stencil`` raises ``ValueError`` for any pair outside its table (``:47``);
  * a constructor that cannot build a kernel - ``order=None``, the default - swallows the error in a bare ``except``
    and leaves the operator without ``.kernel`` (``:66-75``); only a bad ``conv`` raises ``ValueError`` (``:77-82``);
  * ``requires_grad=True`` sets an ATTRIBUTE ``kernel.requires_grad_ = True`` (``:71-72``), it does not make the kernel
    require grad (as ``convops_2d.py`` mirrors for ``Utils/ConvOps_2d.py``);
  * a call with a kernel REPLACES ``self.kernel`` (``:95-96``, ``:121-122``, ``:144-145``, ``:193-194``);
  * ``differentiate`` zero-pads by ``k//2`` (``:151-152``), ``integrate`` does NOT: its ``padded_field`` is reassigned
    to the unpadded field (``:201-202``), yet ``slice_pad=True`` still crops ``Nt - k + 1`` samples (``:225-231``);
  * a [BS,Nt] field gets the channel axis added and squeezed off again (``:99-103``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn.functional as F
from torch.fft import irfftn, rfftn

from . import _dispatch, _lib

# Utils/ConvOps_0d.py:33-44, keyed (deriv_order, taylor_order); deriv_order 0 ignores the Taylor order
_STENCILS = {
    (1, 2): (-1., 0., 1.),
    (1, 4): (1 / 12, -2 / 3, 0, 2 / 3, -1 / 12),
    (2, 2): (1., -2., 1.),
    (2, 4): (-1 / 12, 4 / 3, -5 / 2, 4 / 3, -1 / 12),
    (2, 6): (1 / 90, -3 / 20, 3 / 2, -49 / 18, 3 / 2, -3 / 20, 1 / 90),
}


def get_stencil(deriv_order, taylor_order=2):
    """``Utils/ConvOps_0d.py:21-47``: fp32 stencil of a temporal derivative."""
    if deriv_order == 0:
        return torch.tensor([0., 1., 0.], dtype=torch.float32)
    for (d, t), row in _STENCILS.items():
        if deriv_order == d and taylor_order == t:
            return torch.tensor(row, dtype=torch.float32)
    raise ValueError("Invalid stencil parameters")


def host_taps(kernel):
    """fp32 numpy taps of a 1-D operator kernel; ``NotImplementedError`` for the extents the library does not serve
    (the messages of ``_dispatch.taps_of``)."""
    k = _dispatch.host_kernel(kernel)
    if k.ndim != 1:
        raise RuntimeError(f"expected a 1-D kernel, got shape {tuple(k.shape)}")
    if k.shape[0] % 2 == 0:
        raise NotImplementedError("even kernel extents change the output shape in the reference; not supported")
    if k.shape[0] > _lib.PRE_ODE_MAX_TAPS:
        raise NotImplementedError("kernel extents above 7 are not supported")
    return k


def _as_rows(field):
    """[BS,Nt] view of a [BS,Nt] or [BS,1,Nt] field (the reference's conv1d input after ``unsqueeze(1)``)."""
    _dispatch._check_field(field)
    if field.dim() == 3:
        if field.shape[1] != 1:
            raise RuntimeError("expected a single-channel [BS,1,Nt] field")
        return field[:, 0]
    if field.dim() != 2:
        raise RuntimeError(f"expected a [BS,Nt] field, got shape {tuple(field.shape)}")
    return field


def _dense_out(rows):
    return torch.empty(rows.shape, dtype=torch.float32, device=rows.device)


def stencil(field, taps, flags=0, out=None):
    """``out[b,t] = sum_j taps[j] * field[b, t + j - k//2]`` (zeros outside [0, Nt)) in one HIP pass, no autograd.
    ``field``: fp32 [BS,Nt] or [BS,1,Nt], any strides, CPU (staged through the GPU) or device; ``taps``: fp32 numpy."""
    rows = _as_rows(field)
    origin = None
    if not rows.is_cuda:
        _lib.require_gpu()
        rows, origin = rows.cuda(), rows.device
    dev = rows
    if out is None:
        out = _dense_out(dev)
    elif not (out.is_cuda and tuple(out.shape) == tuple(dev.shape) and out.dtype == torch.float32):
        raise ValueError("out must be an fp32 device tensor of the field's [BS,Nt] shape")
    if out.numel():
        t = np.ascontiguousarray(taps, dtype=np.float32)
        with torch.cuda.device(dev.device):
            rc = _lib.load_ode().pre_ode_stencil_f32(_lib.ptr(dev), _lib.iarr64(dev.stride()), _lib.ptr(out),
                                                     _lib.iarr64(out.stride()), dev.shape[0], dev.shape[1],
                                                     t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(t), flags,
                                                     _lib.stream())
        _lib.check(rc, "pre_ode_stencil_f32")
    return _dispatch.from_device(out, origin)


def wgrad(x, g, k):
    """``dK[j] = sum_{b,t} g[b,t] * x[b, t + j - k//2]`` on the device (``pre_ode_wgrad_f32``: fp64 partials in a fixed
    order, the same bits on every run); fp32 [k] on x's device."""
    work = torch.empty(_lib.PRE_ODE_WGRAD_BLOCKS * k, dtype=torch.float64, device=x.device)
    dk = torch.empty(k, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load_ode().pre_ode_wgrad_f32(_lib.ptr(x), _lib.iarr64(x.stride()), _lib.ptr(g), _lib.iarr64(g.stride()),
                                              x.shape[0], x.shape[1], k, _lib.ptr(work), _lib.ptr(dk), _lib.stream())
    _lib.check(rc, "pre_ode_wgrad_f32")
    return dk


class _Stencil0dFn(torch.autograd.Function):
    """Autograd of the zero-padded 1-D cross-correlation: the field gradient is the same HIP stencil with mirrored taps,
    the kernel gradient one deterministic ``pre_ode_wgrad_f32`` pass."""

    @staticmethod
    def forward(ctx, field, kernel):
        taps = host_taps(kernel)
        ctx.save_for_backward(field, kernel)
        ctx.taps = taps
        return stencil(field, taps)

    @staticmethod
    def backward(ctx, gout):
        field, kernel = ctx.saved_tensors
        gf = gk = None
        rows = _as_rows(field)
        if ctx.needs_input_grad[0]:
            gf = stencil(gout, np.ascontiguousarray(ctx.taps[::-1])).to(field.device).reshape(field.shape)
        if ctx.needs_input_grad[1]:
            x = rows if rows.is_cuda else rows.cuda()
            g = gout.to(x.device)
            gk = wgrad(x, g, len(ctx.taps)).to(kernel.device)
        return gf, gk


def conv1d(field, kernel):
    """``F.conv1d(field[:,None], kernel[None,None], padding=k//2).squeeze(1)`` on the HIP path, differentiable with
    respect to the field and the kernel."""
    if _dispatch.needs_grad(field, kernel):
        return _Stencil0dFn.apply(field, kernel)
    return stencil(field, host_taps(kernel))


def _integrate(field, kernel, correlation, slice_pad, eps):
    """``Utils/ConvOps_0d.py:175-233`` on the device with torch.fft: NO zero padding of the field (``:202``), the
    kernel spectrum zero-extended to Nt, 1/(K^ + eps), optional conjugate, crop ``Nt - k + 1`` when ``slice_pad``."""
    _dispatch._check_field(field)
    dev, origin = _dispatch.to_device(field)
    x = dev.unsqueeze(1) if dev.dim() == 2 else dev
    dims = tuple(range(2, x.ndim))
    field_fft = rfftn(x, dim=dims)
    # The kernel spectrum is taken where the kernel lives, as the reference takes it (a CPU kernel: on the CPU), and only
    # then moved: a difference stencil's K^ is 0 up to round-off at DC, so 1/(K^ + eps) amplifies that round-off 10^6
    # times, and another FFT's round-off there would shift the whole result by a few 1e-3.
    k = kernel.unsqueeze(0).unsqueeze(0)
    grow = [p for i in reversed(range(2, x.ndim)) for p in (0, x.size(i) - k.size(i))]
    kernel_fft = rfftn(F.pad(k, grow), dim=dims)
    inv = 1 / (kernel_fft + eps)
    if correlation:
        inv = torch.conj(inv)
    out = irfftn(field_fft * inv.to(dev.device), dim=dims)
    if slice_pad:
        keep = (slice(None), slice(None)) + tuple(slice(0, x.size(i) - k.size(i) + 1) for i in range(2, x.ndim))
        out = out[keep].contiguous()
    return _dispatch.from_device(out.squeeze(1), origin)


class ConvOperator:
    """Temporal finite-difference operator on [BS,Nt] fields (``Utils/ConvOps_0d.py:51-288``)."""

    def __init__(self, order=None, scale=1.0, taylor_order=2, conv='direct', device='cpu', requires_grad=False):
        try:
            self.order = order
            self.stencil = get_stencil(self.order, taylor_order)
            self.kernel = (scale * self.stencil).to(device)
            if requires_grad:
                self.kernel.requires_grad_ = True          # an attribute, as in the reference (:71-72)
        except Exception:                                  # bare except in the reference (:74-75)
            pass

        if conv == 'direct':
            self.conv = self.convolution
        elif conv == 'spectral':
            self.conv = self.spectral_convolution
        else:
            raise ValueError("Unknown Convolution Method")

    def convolution(self, field, kernel=None):
        """``F.conv1d(field[:,None], K[None,None], padding=k//2).squeeze(1)`` (``:85-106``) on the HIP path."""
        if kernel is not None:
            self.kernel = kernel
        return conv1d(field, self.kernel)

    def spectral_convolution(self, field, kernel=None):
        """``fft_conv(field, K, padding=k//2)`` (``:109-131``)."""
        from . import _spectral
        if kernel is not None:
            self.kernel = kernel
        return _spectral._torch_fft_xcorr(field, self.kernel)

    def differentiate(self, field, kernel=None, correlation=False, slice_pad=True):
        """``:134-172``: zero-pad by k//2, multiply by K^ (its conjugate when ``correlation``), crop when ``slice_pad``."""
        from . import _spectral
        if kernel is not None:
            self.kernel = kernel
        return _spectral._torch_differentiate(field, self.kernel, correlation, slice_pad)

    def integrate(self, field, kernel=None, correlation=False, slice_pad=True, eps=1e-6):
        """``:175-233``: divide by K^ + eps WITHOUT padding the field first (see the module docstring)."""
        if kernel is not None:
            self.kernel = kernel
        return _integrate(field, self.kernel, correlation, slice_pad, eps)

    def forward(self, field):
        return self.conv(field, self.kernel)

    def __call__(self, inputs):
        return self.forward(inputs)
