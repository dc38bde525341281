"""PRE set propagation: bounds on ODE residuals to bounds on solutions (``Inverted_bounds/SHO.py:350-407``,
``Inverse_residuals/Python/pre_set_prop.py:29-91``, ``Inverted_bounds/intervalFFT.py``).

The reference pushes a set in residual space (an interval per step) through the inverse of the ODE operator with zonotopes:
an interval DFT, a complex product with the inverse spectrum ``H``, an inverse interval DFT and the real-part interval hull.
Every step is linear, so for the set ``[c_j - r_j, c_j + r_j]``, ``j < N``, the result has a closed form::

    centre_k = sum_j c_j g[(k - j) mod N],   g = Re(ifft_N(H))
    radius_k = sum_j r_j a[(k - j) mod N],   a[m] = (1/N) sum_h |Re(H_h w^(h m))|,  w = exp(2 pi i / N)

(``hull='interval_fft'``, the reference's hull).  Because the zonotope pipeline treats the frequencies as independent it
over-approximates; ``hull='exact'`` takes ``a = |g|``, the exact interval hull of the same linear map, which is never wider
and still contains every image of the residual box.  The tables depend only on (kernel, N, eps, correlation, hull); they are
built once in float64 on the host, cached by value and uploaded.  On the device the two circulant products run in
``libcp_pre_setprop.so`` (``include/cp_pre_setprop.h``); host inputs take the same closed form in numpy.

The reference recipe (``set_pre_bounds``, ``set_PRE``) is kept step by step, quirks included:
  * the field is padded as ``[0, field, 0]`` (N = Nt + 2) and convolved circularly with the kernel zero-padded at the END
    (the kernel starts at index 0, it is not centred), in float64 from the float32 values;
  * convolved indices 1..3 are points whatever the kernel length, 4..N-2 symmetric ``[-|x|, |x|]``, N-1 a point, and
    index 0 is dropped, so the set has N' = Nt + 1 entries;
  * the interval DFT runs at size N' but ``H`` is the size-N spectrum truncated to its first N' entries (the ``zip`` of
    ``SHO.py:400``); this mismatch is the reference's and is kept.
Deviations: Nt < 3, where the reference's slices overlap, raises ``ValueError``, as does a kernel longer than Nt + 2, where
its ``np.zeros(N_pad)`` fails.  A non-finite field value makes its whole row NaN (in the reference the FFT spreads it).

Calibrated mode (``radius=qhat``, not in the reference): the interior radii ``|x|`` are replaced with conformal q-hat values
indexed like the residuals of ``ConvOperator`` (``calibrate(|D(cal)|, ...)``).  Convolved index n is the residual at step
``t = n - (k+1)/2`` for a symmetric k-tap kernel without correlation and at ``t = n + (k-3)/2`` for any k-tap kernel with
it; an even kernel, or an asymmetric one without correlation, has no such mapping and raises ``ValueError``.  An interior
index whose step falls outside ``[0, Nt)`` keeps ``|x|``, and the edge points stay as they are.  q-hat is read as fp32.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib

HULLS = ("interval_fft", "exact")


# ---------------------------------------------------------------- tables (host, float64)
def _host_taps(kernel):
    """float64 taps of a kernel given as a tensor, an array, a list or an object with ``.kernel`` (a ConvOperator)."""
    if hasattr(kernel, "kernel") and not isinstance(kernel, (np.ndarray, torch.Tensor)):
        kernel = kernel.kernel
    if isinstance(kernel, torch.Tensor):
        kernel = kernel.detach().cpu().numpy()
    k = np.asarray(kernel, dtype=np.float64)
    if k.ndim != 1 or k.size < 1:
        raise ValueError(f"expected a 1-D kernel, got shape {k.shape}")
    return k


def inverse_spectrum(kernel, n, eps=1e-6, correlation=False):
    """``1 / (fft(kernel zero-padded at the END to n) + eps)`` in complex128, the spectrum conjugated first when
    ``correlation`` (``SHO.py:360-374``)."""
    taps = _host_taps(kernel)
    if taps.size > n:
        raise ValueError(f"a {taps.size}-tap kernel does not fit a length-{n} signal")
    kp = np.zeros(n)
    kp[:taps.size] = taps
    K = np.fft.fft(kp)
    if correlation:
        K = np.conj(K)
    return 1.0 / (K + eps)


def _check_hull(hull):
    if hull not in HULLS:
        raise ValueError(f"hull must be one of {HULLS}, got {hull!r}")


def _tables_from_spectrum(H, hull):
    N = H.size
    g = np.fft.ifft(H).real.copy()
    if hull == "exact":
        return g, np.abs(g)
    q = np.arange(N)
    cos_t, sin_t = np.cos(2 * np.pi * q / N), np.sin(2 * np.pi * q / N)
    a = np.empty(N)
    rows = max(1, (1 << 22) // N)
    for m0 in range(0, N, rows):
        m = np.arange(m0, min(N, m0 + rows))
        ph = np.outer(m, q) % N                            # h * m mod N
        a[m] = np.abs(H.real * cos_t[ph] - H.imag * sin_t[ph]).sum(axis=1) / N
    return g, a


@functools.lru_cache(maxsize=64)
def _tables_cached(key, hull):
    kind = key[0]
    if kind == "recipe":
        _, taps, nt, eps, correlation = key
        H = inverse_spectrum(np.array(taps), nt + 2, eps, correlation)[:nt + 1]
    else:
        H = np.frombuffer(key[1], dtype=np.complex128)
    g, a = _tables_from_spectrum(H, hull)
    g.setflags(write=False)
    a.setflags(write=False)
    return g, a


_DEVICE_TABLES = {}


def _device_tables(key, hull, device):
    dkey = (key, hull, str(device))
    t = _DEVICE_TABLES.get(dkey)
    if t is None:
        g, a = _tables_cached(key, hull)
        t = (torch.from_numpy(g.copy()).to(device), torch.from_numpy(a.copy()).to(device))
        if len(_DEVICE_TABLES) >= 64:
            _DEVICE_TABLES.pop(next(iter(_DEVICE_TABLES)))
        _DEVICE_TABLES[dkey] = t
    return t


def recipe_key(kernel, nt, eps=1e-6, correlation=False):
    """The value key of the recipe's tables: kernel taps, Nt, eps and correlation (never a tensor's identity)."""
    return ("recipe", tuple(float(v) for v in _host_taps(kernel)), int(nt), float(eps), bool(correlation))


def tables(H_or_key, hull="interval_fft"):
    """(g, a) float64 for an inverse spectrum ``H`` (length N) or a ``recipe_key``; read-only, cached by value."""
    _check_hull(hull)
    if isinstance(H_or_key, tuple):
        return _tables_cached(H_or_key, hull)
    H = np.ascontiguousarray(np.asarray(H_or_key, dtype=np.complex128).reshape(-1))
    return _tables_cached(("spectrum", H.tobytes()), hull)


# ---------------------------------------------------------------- closed form on the host
def _circulant(t):
    N = t.size
    j, k = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return t[(k - j) % N]                                 # [j, k]


def _bounds_host(c, r, g, a, bad=None):
    with np.errstate(invalid="ignore", over="ignore"):          # non-finite rows become NaN below
        cen = c @ _circulant(g)
        rad = r @ _circulant(a)
        lo, hi = cen - rad, cen + rad
    ok = np.isfinite(cen) & np.isfinite(rad)
    ok &= np.isfinite(c).all(axis=1, keepdims=True) & np.isfinite(r).all(axis=1, keepdims=True)
    if bad is not None:
        ok &= ~bad[:, None]
    lo[~ok] = np.nan
    hi[~ok] = np.nan
    return lo, hi


def _to_host64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


# ---------------------------------------------------------------- general form
def propagate(centre, radius, H, hull="interval_fft"):
    """Solution bounds ``(lower, upper)``, fp64 ``[B, N]``, of the residual-space sets ``[centre - radius, centre + radius]``
    (``[B, N]`` fp32 or fp64, device or host, any strides; a 1-D row gives 1-D bounds) through the inverse spectrum ``H``
    (length N).  Device inputs run ``pre_setprop_bounds_f64``; host inputs the same closed form in numpy."""
    _check_hull(hull)
    H = np.asarray(H.detach().cpu().numpy() if isinstance(H, torch.Tensor) else H, dtype=np.complex128).reshape(-1)
    one = (centre.dim() if isinstance(centre, torch.Tensor) else np.ndim(centre)) == 1
    if isinstance(centre, torch.Tensor) and centre.is_cuda:
        if not isinstance(radius, torch.Tensor) or radius.device != centre.device:
            raise ValueError("centre and radius must be on the same device")
        c, r = (centre[None], radius[None]) if one else (centre, radius)
        _check_rows(c, r, H.size)
        if c.dtype not in (torch.float32, torch.float64) or r.dtype not in (torch.float32, torch.float64):
            raise TypeError("centre and radius must be float32 or float64")
        if c.dtype != r.dtype:
            c, r = c.double(), r.double()
        if bool((r < 0).any()):
            raise ValueError("radius must be >= 0")
        lo, hi = _bounds_device(c, r, ("spectrum", np.ascontiguousarray(H).tobytes()), hull)
    else:
        c, r = _to_host64(centre), _to_host64(radius)
        if one:
            c, r = c[None], r[None]
        _check_rows(c, r, H.size)
        if (r < 0).any():
            raise ValueError("radius must be >= 0")
        g, a = tables(H, hull)
        lo, hi = _bounds_host(c, r, g, a)
    return (lo[0], hi[0]) if one else (lo, hi)


def _check_rows(c, r, n):
    if len(c.shape) != 2 or tuple(c.shape) != tuple(r.shape):
        raise ValueError(f"centre and radius must both be [B, N], got {tuple(c.shape)} and {tuple(r.shape)}")
    if c.shape[1] != n:
        raise ValueError(f"rows have {c.shape[1]} entries but the spectrum has {n}")
    if n < 1:
        raise ValueError("N must be >= 1")


def _bounds_device(c, r, key, hull):
    _lib.require_gpu()
    lib = _lib.load_setprop()
    B, N = c.shape
    lo = torch.empty((B, N), dtype=torch.float64, device=c.device)
    hi = torch.empty_like(lo)
    if B == 0:
        return lo, hi
    with torch.cuda.device(c.device):
        g, a = _device_tables(key, hull, c.device)
        flags = _lib.PRE_SETPROP_FLAG_F64 if c.dtype == torch.float64 else 0
        rc = lib.pre_setprop_bounds_f64(_lib.ptr(c), _lib.iarr64(c.stride()), _lib.ptr(r), _lib.iarr64(r.stride()), B, N,
                                        _lib.ptr(g), _lib.ptr(a), _lib.ptr(lo), _lib.ptr(hi), flags, _lib.stream())
    _lib.check(rc, "pre_setprop_bounds_f64")
    return lo, hi


# ---------------------------------------------------------------- the reference recipe
def qhat_shift(k, correlation):
    """Convolved index n of the recipe is the ConvOperator residual at step ``t = n + qhat_shift(k, correlation)``
    (derived for odd k; without correlation only for a symmetric kernel, which the caller checks)."""
    return (k - 3) // 2 if correlation else -(k + 1) // 2


def _check_recipe(taps, nt, radius, correlation):
    if nt < 3:
        raise ValueError(f"set propagation needs Nt >= 3 steps (the reference's edge slices overlap below), got {nt}")
    if taps.size > nt + 2:
        raise ValueError(f"a {taps.size}-tap kernel does not fit the padded length-{nt + 2} signal")
    if radius is not None:
        if taps.size % 2 == 0:
            raise ValueError("radius=qhat needs an odd kernel: the residual index of an even one is not derived")
        if not correlation and not np.array_equal(taps, taps[::-1]):
            raise ValueError("radius=qhat without correlation needs a symmetric kernel: the residual index of an asymmetric "
                             "one is not derived")


def _qhat_rows(radius, B, nt):
    """q-hat as an fp32 tensor broadcastable to [B, Nt] (0-d, [Nt] or [B, Nt])."""
    q = radius if isinstance(radius, torch.Tensor) else torch.as_tensor(np.asarray(radius, dtype=np.float32))
    q = q.detach().to(torch.float32)
    if q.dim() > 2 or (q.dim() >= 1 and q.shape[-1] != nt) or (q.dim() == 2 and q.shape[0] != B):
        raise ValueError(f"radius must be a scalar, [Nt] or [B, Nt] with Nt = {nt} and B = {B}, got {tuple(q.shape)}")
    if bool((q < 0).any()):
        raise ValueError("radius must be >= 0")
    return q


def recipe_sets_host(fields, kernel, correlation=False, radius=None):
    """The residual-space set of the recipe on the host: ``(c, r, bad)``, c and r fp64 [B, Nt + 1], bad a [B] mask of rows
    with a non-finite convolved value."""
    taps = _host_taps(kernel)
    x = _to_host64(fields)
    B, nt = x.shape
    _check_recipe(taps, nt, radius, correlation)
    Ns = nt + 2
    s = np.zeros((B, Ns))
    s[:, 1:nt + 1] = x
    conv = np.zeros((B, Ns))
    for i, w in enumerate(taps):
        conv += w * np.roll(s, -i if correlation else i, axis=1)      # roll(s, i)[n] = s[n - i]
    bad = ~np.isfinite(conv[:, 1:]).all(axis=1)
    N = nt + 1
    c = np.zeros((B, N))
    r = np.zeros((B, N))
    c[:, 0:3] = conv[:, 1:4]
    c[:, N - 1] = conv[:, Ns - 1]
    r[:, 3:N - 1] = np.abs(conv[:, 4:Ns - 1])
    if radius is not None:
        q = np.broadcast_to(_qhat_rows(radius, B, nt).cpu().numpy().astype(np.float64), (B, nt))
        n = np.arange(4, Ns - 1)
        t = n + qhat_shift(taps.size, correlation)
        inside = (t >= 0) & (t < nt)
        r[:, n[inside] - 1] = q[:, t[inside]]
    return c, r, bad


def set_pre_bounds(fields, D_or_kernel, correlation=False, eps=1e-6, radius=None, hull="interval_fft"):
    """Solution bounds ``(lower, upper)``, fp64 ``[B, Nt + 1]``, of ``SHO.py:set_PRE`` for every row of ``fields`` ([B, Nt],
    e.g. the component view ``sol[..., 0]`` of a [B, Nt, S] state, read where it lies; a 1-D field gives 1-D bounds).
    Callers take ``[..., 1:-1]`` as the scripts do.  ``D_or_kernel``: a ConvOperator or its taps.  ``radius``: q-hat (a
    scalar, [Nt] or [B, Nt]) in place of the interior radii (calibrated mode).  cuda fields (fp32) run
    ``pre_setprop_recipe_f32``; host fields the same closed form in numpy."""
    _check_hull(hull)
    taps = _host_taps(D_or_kernel)
    one = (fields.dim() if isinstance(fields, torch.Tensor) else np.ndim(fields)) == 1
    x = fields[None] if one else fields
    if len(x.shape) != 2:
        raise ValueError(f"fields must be [B, Nt], got {tuple(x.shape)}")
    B, nt = x.shape
    _check_recipe(taps, nt, radius, correlation)
    key = recipe_key(taps, nt, eps, correlation)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        lo, hi = _recipe_device(x, taps, radius, correlation, key, hull)
    else:
        c, r, bad = recipe_sets_host(x, taps, correlation, radius)
        g, a = tables(key, hull)
        lo, hi = _bounds_host(c, r, g, a, bad)
    return (lo[0], hi[0]) if one else (lo, hi)


def _recipe_device(x, taps, radius, correlation, key, hull):
    _lib.require_gpu()
    if x.dtype != torch.float32:
        raise TypeError(f"the device recipe reads fp32 fields (the reference's set_PRE takes a float32 tensor), got {x.dtype}")
    if taps.size > _lib.PRE_SETPROP_MAX_TAPS:
        raise ValueError(f"the device recipe serves kernels of at most {_lib.PRE_SETPROP_MAX_TAPS} taps, got {taps.size}")
    lib = _lib.load_setprop()
    B, nt = x.shape
    lo = torch.empty((B, nt + 1), dtype=torch.float64, device=x.device)
    hi = torch.empty_like(lo)
    q, qs = None, (0, 0)
    if radius is not None:
        q = _qhat_rows(radius, B, nt).to(x.device)
        qs = (0, 0) if q.dim() == 0 else (0, q.stride(0)) if q.dim() == 1 else tuple(q.stride())
    if B == 0:
        return lo, hi
    flags = _lib.PRE_SETPROP_FLAG_CORRELATION if correlation else 0
    with torch.cuda.device(x.device):
        g, a = _device_tables(key, hull, x.device)
        rc = lib.pre_setprop_recipe_f32(_lib.ptr(x), _lib.iarr64(x.stride()), B, nt, (ctypes.c_double * taps.size)(*taps),
                                        taps.size, _lib.ptr(q), _lib.iarr64(qs), _lib.ptr(g), _lib.ptr(a), _lib.ptr(lo),
                                        _lib.ptr(hi), flags, _lib.stream())
    _lib.check(rc, "pre_setprop_recipe_f32")
    return lo, hi


# ---------------------------------------------------------------- drop-in for the scripts
class Interval:
    """What the scripts use of an interval (``SHO.py:423-440``): ``.inf``, ``.sup`` and ``x in iv``."""
    __slots__ = ("inf", "sup")

    def __init__(self, inf, sup):
        self.inf = float(inf)
        self.sup = float(sup)

    def __contains__(self, x):
        return self.inf <= float(x) <= self.sup

    def __repr__(self):
        return f"Interval({self.inf!r}, {self.sup!r})"


def _intervals(lo, hi):
    lo = lo.cpu().numpy() if isinstance(lo, torch.Tensor) else lo
    hi = hi.cpu().numpy() if isinstance(hi, torch.Tensor) else hi
    return [Interval(a, b) for a, b in zip(lo.tolist(), hi.tolist())]


def set_PRE(field, D, correlation=False, eps=1e-6):
    """Drop-in for ``Inverted_bounds/SHO.py:350``: a list of Nt + 1 ``Interval`` on the solution of one trajectory
    ``field`` ([Nt]); the scripts keep ``[1:-1]``."""
    return _intervals(*set_pre_bounds(field, D, correlation=correlation, eps=eps))
