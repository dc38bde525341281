"""Split-conformal calibration on the MI355X: the functions the reference imports from
``Neural_PDE.UQ.inductive_cp`` (``Marginal/NS_Residuals_CP.py:58``), same names and call
signatures: ``calibrate``, ``modulation_func``, ``ncf_metric_joint``, ``emp_cov``,
``emp_cov_joint`` (+ ``filter_sims_joint``, ``Joint/Burgers_Residuals_CP.py:298-300``).

That module is an un-vendored, un-pinned submodule absent from the reference snapshot.
``modulation_func``, ``ncf_metric_joint`` and joint coverage are pinned to vectors produced by
executing the reference's in-tree restatement (``Tests/test_advection_inv_sampling_marginal.py:428,
430-431,464-465`` -> ``tests/golden/conformal_ref.npz``); ``calibrate`` has no source or restatement
anywhere in the reference (PARITY UNPINNED, permanently): it is the standard split-CP quantile
inferred from the call sites, tested against numpy.

    calibrate(scores, n, alpha)        = np.quantile(scores, ceil((n+1)(1-alpha))/n, axis=0, method='higher')
    modulation_func(a, b)              = np.std(a - b, axis=0)
    ncf_metric_joint(a, b, modulation) = np.max(np.abs(a - b)/modulation, axis=(1..))
    emp_cov(sets, y)                   = ((y >= lo) & (y <= hi)).mean()
    emp_cov_joint(sets, y)             = ((y >= lo).all(1..) & (y <= hi).all(1..)).mean()

numpy arrays in -> numpy out (what the reference scripts pass); torch tensors in -> torch
out on the same device.  The arithmetic runs in ``libcp_pre_hip.so`` either way (radix
select, sequential-order std, max-reduce); q-hat is bit-for-bit one of the input scores.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _dispatch, _lib


# ------------------------------------------------------------------ marshalling
def canon(d):
    """(contiguous view [n, *cells in MEMORY order], order) of a dense tensor whose cell axes are
    permuted in memory (e.g. a residual computed in the surrogate's [BS,Nx,Ny,Nt] layout): the
    calibration kernels only need "n rows of M cells", so they run on the data where it lies.
    ``order`` is None for an already-contiguous tensor; non-dense views are copied."""
    if d.is_contiguous():
        return d, None
    if d.dim() >= 3:
        order = sorted(range(1, d.dim()), key=lambda k: (-d.stride(k), k))
        v = d.permute(0, *order)
        if v.is_contiguous():
            return v, order
    return d.contiguous(), None


def canon_cells(m, order):
    """A per-cell array (no batch axis) in the memory order ``order`` chosen by :func:`canon`."""
    return m.contiguous() if order is None else m.permute(*[o - 1 for o in order]).contiguous()


def uncanon(r, order, lead):
    """Inverse of the cell permutation on a result with ``lead`` leading non-cell axes."""
    if order is None:
        return r
    inv = [0] * len(order)
    for pos, o in enumerate(order):
        inv[o - 1] = pos
    return r.permute(*range(lead), *[lead + i for i in inv])


# (why and when score rows are padded: _lib.wants_row_pad)
wants_row_pad, PAD = _lib.wants_row_pad, _lib.PAD


def upload_rows(host, device=None):
    """Device copy [n, *cells] of a host fp32 tensor for a per-cell select: row-padded (``pipeline.row_padded``'s layout)
    when the row length asks for it - the H2D transfer happens anyway, into the strided view instead of a dense one."""
    n = host.shape[0] if host.dim() >= 2 else 0
    M = host[0].numel() if n else 0
    if not (host.dim() >= 2 and wants_row_pad(n, M)):
        return host.to(device or "cuda")
    buf = torch.empty(n * (M + PAD), dtype=torch.float32, device=device or "cuda")
    view = buf.as_strided((n, M), (M + PAD, 1))
    flat = host.reshape(n, M)
    # (torch stages a host -> strided-device copy through a dense device temporary of the copy's size: row blocks of at
    # most 1 GiB keep that temporary small whatever the matrix - a 100 GB score matrix must not need 200 GB for a moment)
    rows = max(1, (1 << 28) // M)
    for r0 in range(0, n, rows):
        view[r0:r0 + rows].copy_(flat[r0:r0 + rows])
    strides, acc = [], 1
    for d in reversed(host.shape[1:]):
        strides.append(acc)
        acc *= d
    return buf.as_strided(tuple(host.shape), (M + PAD,) + tuple(reversed(strides)))


def _dev(x, like=None, rows=False):
    """fp32 device tensor (layout untouched) + a function that converts results back.  ``rows``: the tensor is a score
    matrix about to be selected along axis 0 - a HOST input is uploaded row-padded when that pays (``upload_rows``); a
    device tensor is the caller's and is selected where it lies."""
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32:
            raise RuntimeError("cp_pre_amd.inductive_cp works on float32 tensors")
        if rows and not x.is_cuda and x.dim() >= 2:
            _lib.require_gpu()
            origin = x.device
            return upload_rows(x.contiguous()), (lambda r: _dispatch.from_device(r, origin))
        d, origin = _dispatch.to_device(x)
        return d, (lambda r: _dispatch.from_device(r, origin))
    arr = np.asarray(x)
    if arr.dtype != np.float32:
        arr = arr.astype(np.float32)
    _lib.require_gpu()
    host = torch.from_numpy(np.ascontiguousarray(arr))
    return (upload_rows(host) if rows else host.cuda()), (lambda r: r.cpu().numpy())


def _is_zero_like(b):
    """``np.zeros(res.shape)`` is how the scripts say 'no second argument' (Joint/Burgers_..:274)."""
    if b is None:
        return True
    if isinstance(b, np.ndarray):
        return not b.any()
    return False


# ------------------------------------------------------------------ ranks
def quantile_level(n, alpha):
    return math.ceil((n + 1) * (1 - alpha)) / n


def kth_index(n_rows, n, alpha):
    """0-based sorted index numpy's ``method='higher'`` selects: ceil(q*(n_rows-1)), float64."""
    q = np.ceil((n + 1) * (1 - alpha)) / n
    if not (0.0 <= q <= 1.0):
        raise ValueError("Quantiles must be in the range [0, 1]")
    return int(np.ceil((n_rows - 1) * q))


def rows_where_they_lie(scores):
    """(view [n, *cells in MEMORY order], row pitch or None, cell order or None) of a score tensor whose rows can be
    selected in place: dense, or dense rows a fixed pitch >= their length apart (``pipeline.row_padded``; a driver pads
    its residual buffer so that the rows of a cell's column are not a power of two apart), with the cell axes in any
    order in memory (a residual computed in the surrogate's [BS,Nx,Ny,Nt] layout).  Anything else: None (copied)."""
    if scores.is_contiguous():
        return scores, None, None
    if scores.dim() < 2:
        return None
    order = sorted(range(1, scores.dim()), key=lambda k: (-scores.stride(k), k))
    v = scores.permute(0, *order)
    M = v[0].numel()
    if not v[0].is_contiguous() or not (v.shape[0] == 1 or v.stride(0) >= M):
        return None
    pitch = v.stride(0) if (v.shape[0] > 1 and v.stride(0) != M) else None
    return v, pitch, (None if order == list(range(1, scores.dim())) else order)


def kth_axis0(scores, ks):
    """Order statistics ``ks`` (0-based ranks, any order) along axis 0 of a device tensor
    [n, ...] -> [len(ks), ...].  1-D scores use the scalar radix select."""
    lib = _lib.load()
    lie = rows_where_they_lie(scores)
    if lie is not None:
        scores, pitch, cell_order = lie
    else:
        pitch = None
        scores, cell_order = canon(scores)
    n = scores.shape[0]
    with torch.cuda.device(scores.device):
        if scores.dim() == 1:
            order = sorted(range(len(ks)), key=lambda i: ks[i])     # the scalar select wants ascending ranks
            sk = [int(ks[i]) for i in order]
            out = torch.empty(len(sk), dtype=torch.float32, device=scores.device)
            _lib.check(lib.pre_kth_f32(_lib.ptr(scores), n, _lib.iarr64(sk), len(sk), _lib.ptr(out), _lib.stream()),
                       "pre_kth_f32")
            inv = [0] * len(ks)
            for pos, i in enumerate(order):
                inv[i] = pos
            if inv != list(range(len(ks))):      # device-only reorder (no index upload: stays HIP-graph capturable)
                out = out.flip(0) if inv == list(range(len(ks) - 1, -1, -1)) else torch.stack([out[i] for i in inv])
        else:
            M = scores[0].numel()
            out = torch.empty((len(ks),) + tuple(scores.shape[1:]), dtype=torch.float32, device=scores.device)
            _lib.check(lib.pre_kth_axis0_strided_f32(_lib.ptr(scores), pitch or M, n, M, _lib.iarr32([int(k) for k in ks]), len(ks),
                                                     _lib.ptr(out), _lib.stream()), "pre_kth_axis0_strided_f32")   # (out[j] <-> ks[j])
    return uncanon(out, cell_order, 1)


# ------------------------------------------------------------------ the five functions
def calibrate(scores, n, alpha):
    """q-hat over axis 0; array of shape ``scores.shape[1:]`` (scalar for 1-D scores)."""
    d, back = _dev(scores, rows=True)
    k = kth_index(d.shape[0], n, alpha)
    res = back(kth_axis0(d, [k])[0])
    if d.dim() == 1 and not isinstance(scores, torch.Tensor):
        return res[()]                                       # numpy scalar, like np.quantile
    return res


def calibrate_multi(scores, n, alphas):
    """All levels in ONE radix sweep (the reference loops ``calibrate`` over 10 alphas,
    Marginal/Wave_Residuals_CP.py:284-288).  Returns [len(alphas), ...]."""
    d, back = _dev(scores, rows=True)
    ks = [kth_index(d.shape[0], n, a) for a in alphas]
    return back(kth_axis0(d, ks))


def _same_layout(t, order):
    """``t`` ([n, *cells]) as a contiguous tensor in the memory order ``order`` of its partner."""
    return t.contiguous() if order is None else t.permute(0, *order).contiguous()


def _wide(*xs):
    """numpy promotes float32 - float64 to float64 (``modulation_func(res, np.zeros(res.shape))``,
    Joint/Burgers_Residuals_CP.py:274): such calls get the fp64-accumulated route and a float64 result."""
    return any(isinstance(x, np.ndarray) and x.dtype == np.float64 for x in xs)


def modulation_func(a, b=None, eps=0.0):
    """Per-cell population std of (a-b) over axis 0.

    float32 inputs: float32 sequential accumulation in numpy's own operation order
    (bit-identical to ``np.std(a-b, axis=0)`` on float32).  If an argument is a float64 numpy
    array (numpy would then compute in float64) the sums are accumulated in fp64 on the device."""
    da, back = _dev(a)
    da, order = canon(da)
    db = None if _is_zero_like(b) else _same_layout(_dev(b)[0], order)
    n, M = da.shape[0], da.numel() // da.shape[0]
    mod = torch.empty(da.shape[1:], dtype=torch.float32, device=da.device)
    lib = _lib.load()
    with torch.cuda.device(da.device):
        if _wide(a, b):
            mom = torch.zeros(2, M, dtype=torch.float64, device=da.device)
            _lib.check(lib.pre_moments_axis0_f64(_lib.ptr(da), _lib.ptr(db), n, M, M, _lib.ptr(mom[0]), _lib.ptr(mom[1]),
                                                 _lib.stream()), "pre_moments_axis0_f64")
            _lib.check(lib.pre_std_from_moments_f32(_lib.ptr(mom[0]), _lib.ptr(mom[1]), n, M, float(eps), _lib.ptr(mod),
                                                    _lib.stream()), "pre_std_from_moments_f32")
            return back(uncanon(mod, order, 0)).astype(np.float64)
        _lib.check(lib.pre_std_axis0_f32(_lib.ptr(da), _lib.ptr(db), n, M, float(eps), _lib.ptr(mod), _lib.stream()),
                   "pre_std_axis0_f32")
    return back(uncanon(mod, order, 0))


def ncf_metric_joint(a, b, modulation, crop=0):
    """Per-sample max over cells of |a-b|/modulation -> [n].  ``crop`` > 0 restricts the max to
    the interior of the last three axes of UNCROPPED [n,T,X,Y] inputs (fusing the reference's
    ``[...,1:-1,1:-1,1:-1]``)."""
    da, back = _dev(a)
    da, order = canon(da)
    db = None if _is_zero_like(b) else _same_layout(_dev(b)[0], order)
    dm = canon_cells(_dev(modulation)[0], order)
    n = da.shape[0]
    if crop:
        if da.dim() != 4:
            raise ValueError("crop needs [n,T,X,Y] inputs")
        T, X, Y = da.shape[1:]                      # extents in memory order; the crop is the same on each axis
        ct = cx = cy = int(crop)
    else:
        # no crop: any rows x columns factorisation of the cells will do; one row of M cells would leave a single
        # workgroup per sample (measured 0.16 TB/s at n = 100) and a short innermost axis (the surrogate's Nt) would
        # defeat the float4 path: rows of the largest power of two that divides M
        M = da.numel() // n
        # (not longer than 512 either: a block takes 32 rows, and n x M / (32 x 4096) blocks left a calibration set
        # of n = 100 with two workgroups per CU - 2.4 TB/s against 5 with 512-cell rows)
        Y = next((c for c in (512, 256, 128, 64, 32, 16, 8, 4) if M % c == 0), da.shape[-1])
        T, X, ct, cx, cy = 1, M // Y, 0, 0, 0
    scores = torch.zeros(n, dtype=torch.float32, device=da.device)
    with torch.cuda.device(da.device):
        _lib.check(_lib.load().pre_joint_score_f32(_lib.ptr(da), _lib.ptr(db), _lib.ptr(dm), n, T, X, Y, ct, cx, cy,
                                                   _lib.ptr(scores), _lib.stream()), "pre_joint_score_f32")
    res = back(scores)
    return res.astype(np.float64) if _wide(a, b, modulation) else res


def _directed_f32(a, up):
    """float64 bound -> float32 rounded towards +inf (``up``) or -inf, so that comparing a float32
    sample with the float32 bound decides exactly like numpy's float64 comparison
    (``y >= lo64``  <=>  ``y >= ceil32(lo64)``;  ``y <= hi64``  <=>  ``y <= floor32(hi64)``)."""
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64) and not isinstance(a, float):
        return a
    a64 = np.asarray(a, np.float64)
    a32 = a64.astype(np.float32)
    wrong = (a32 < a64) if up else (a32 > a64)
    fixed = np.nextafter(a32, np.float32(np.inf if up else -np.inf), dtype=np.float32)
    return np.where(wrong, fixed, a32).astype(np.float32)


def _bounds(pred_sets, y, outside=False):
    """y as [n, M] rows in MEMORY order (no copy for dense permuted layouts, e.g. the surrogate's Nt-fastest
    one) and the two bounds laid out the same way, per cell ([M]) or per sample and cell ([n, M])."""
    ydev = _dev(y)[0]
    logical = tuple(ydev.shape)                             # [n, *cells] as the caller sees it
    dy, order = canon(ydev)
    n, M = dy.shape[0], dy.numel() // dy.shape[0]

    def lay(t):
        # inside test: y >= lo & y <= hi; outside test: y <= lo | y >= hi  (opposite rounding directions)
        if t.numel() == M and t.dim() >= 1:
            return canon_cells(t.reshape(logical[1:]), order), 0
        if t.numel() == n * M:
            return _same_layout(t.reshape(logical), order), 1
        return None, -1                                      # scalar / other broadcast: materialise below
    lo_t = _dev(_directed_f32(pred_sets[0], up=not outside))[0]
    hi_t = _dev(_directed_f32(pred_sets[1], up=outside))[0]
    (lo, pl), (hi, ph) = lay(lo_t), lay(hi_t)
    if pl != ph or pl < 0:
        ps = 1 if 1 in (pl, ph) else 0
        shape = logical if ps else logical[1:]
        lo = lay(lo_t.expand(shape).contiguous())[0]
        hi = lay(hi_t.expand(shape).contiguous())[0]
    else:
        ps = pl
    return dy, lo, hi, n, M, ps


def emp_cov(pred_sets, y):
    """Fraction of all cells of all samples inside [lo, hi]."""
    dy, lo, hi, n, M, ps = _bounds(pred_sets, y)
    count = torch.zeros(1, dtype=torch.int64, device=dy.device)
    with torch.cuda.device(dy.device):
        _lib.check(_lib.load().pre_cov_count_f32(_lib.ptr(dy), _lib.ptr(lo), _lib.ptr(hi), n, M, ps, _lib.ptr(count),
                                                 _lib.stream()), "pre_cov_count_f32")
    return float(count.item()) / float(n * M)


def filter_sims_joint(pred_sets, y):
    """Per-sample 'every cell inside the band' flags (bool [n])."""
    dy, lo, hi, n, M, ps = _bounds(pred_sets, y)
    inside = torch.ones(n, dtype=torch.uint8, device=dy.device)
    with torch.cuda.device(dy.device):
        _lib.check(_lib.load().pre_cov_joint_f32(_lib.ptr(dy), _lib.ptr(lo), _lib.ptr(hi), n, M, ps, _lib.ptr(inside),
                                                 _lib.stream()), "pre_cov_joint_f32")
    flags = inside.bool()
    return flags if isinstance(y, torch.Tensor) else flags.cpu().numpy()


def filter_sims_within_bounds(lower_bound, upper_bound, samples, threshold, within=False):
    """``Active_Learning/Advection_AL_Marginal.py:169-198``: bool [n], True where at least
    ``threshold`` of a sample's cells lie inside [lo,hi] (``within``) or on/outside the bounds."""
    dy, lo, hi, n, M, ps = _bounds([lower_bound, upper_bound], samples, outside=not within)
    counts = torch.zeros(n, dtype=torch.int32, device=dy.device)
    with torch.cuda.device(dy.device):
        _lib.check(_lib.load().pre_cov_rowcount_f32(_lib.ptr(dy), _lib.ptr(lo), _lib.ptr(hi), n, M, ps, 0 if within else 1,
                                                    _lib.ptr(counts), _lib.stream()), "pre_cov_rowcount_f32")
    flags = (counts.double() / float(M)) >= threshold          # numpy: mean of bools in float64
    return flags if isinstance(samples, torch.Tensor) else flags.cpu().numpy()


def emp_cov_joint(pred_sets, y):
    f = filter_sims_joint(pred_sets, y)
    return float(f.sum().item()) / f.numel() if isinstance(f, torch.Tensor) else float(f.mean())     # count / n in float64, as numpy


ALPHA_LEVELS = np.arange(0.05, 0.95 + 0.1, 0.1)     # Marginal/Wave_Residuals_CP.py:284


# ------------------------------------------------------------------ coverage at every level in one pass
# The reference's `for alpha in alphas: qhat = calibrate(...); emp_cov(...)` loop (Marginal/Wave_Residuals_CP.py:284-290)
# reads the test residual once per level; libcp_pre_cov.so (include/cp_pre_cov.h) reads it once for all of them, where it
# lies.  fp32 levels (what calibrate_multi returns) take that pass; float64 ones (Python floats, np.float64) make numpy
# compute float64 bounds and take the per-level functions above, which round those bounds exactly (_directed_f32).

def _merge_cells(shape, strides_list):
    """Cell axes (memory order) of one or two strided operands merged where every operand allows it and padded to three:
    ([A, B, C], [[sA, sB, sC] per operand]) or None when the innermost axis is not dense or more than three remain."""
    axes = [(d, [s[i] for s in strides_list]) for i, d in enumerate(shape) if d != 1]
    merged = []
    for d, st in axes:
        if merged and all(ps == s * d for ps, s in zip(merged[-1][1], st)):
            merged[-1] = (merged[-1][0] * d, st)
        else:
            merged.append((d, st))
    if not merged:
        merged = [(1, [1] * len(strides_list))]
    if len(merged) > 3 or any(s != 1 for s in merged[-1][1]):
        return None
    merged = [(1, [0] * len(strides_list))] * (3 - len(merged)) + merged
    return [d for d, _ in merged], [[st[i] for _, st in merged] for i in range(len(strides_list))]


def cov_operands(y, centre=None):
    """How ``libcp_pre_cov.so`` reads a device test residual ``y`` [n, *cells] and a centre laid out like it: (y view, centre
    view or None, (A, B, C), strides of y, strides of the centre, cell order).  The cell axes are relabelled into y's memory
    order (``canon``'s order, a view) and adjacent ones merged, so a cropped view (``res[:, 1:-1, 1:-1, 1:-1]``), the
    surrogate's Nt-fastest layout and ``pipeline.row_padded`` / ``time_major`` buffers are read where they lie; y is copied
    only if its innermost memory axis is not dense or more than three cell axes remain.  A centre that does not fit y's
    cell order is copied into it (``_same_layout``).  Strides: (sample, A, B) in elements.  The per-cell operands (q, m)
    follow the flat cell order of the result: ``cov_cells``."""
    d = y.dim()
    order = sorted(range(1, d), key=lambda k: (-y.stride(k), k)) if d > 1 else []
    yv = y.permute(0, *order)
    cv = centre.permute(0, *order) if centre is not None else None
    ops = [yv] + ([cv] if cv is not None else [])
    got = _merge_cells(tuple(yv.shape[1:]), [t.stride()[1:] for t in ops])
    if got is None and cv is not None and _merge_cells(tuple(yv.shape[1:]), [yv.stride()[1:]]) is not None:
        cv = _same_layout(centre, order)                 # the centre alone does not fit: into y's order
        ops[1] = cv
        got = _merge_cells(tuple(yv.shape[1:]), [t.stride()[1:] for t in ops])
    if got is None:                                      # y itself is not streamable: a dense copy in logical order
        order = list(range(1, d))
        yv = y.contiguous()
        cv = centre.contiguous() if centre is not None else None
        ops = [yv] + ([cv] if cv is not None else [])
        got = _merge_cells(tuple(yv.shape[1:]), [t.stride()[1:] for t in ops])
    ext, st = got
    ys = (yv.stride(0), st[0][0], st[0][1])
    cs = (cv.stride(0), st[1][0], st[1][1]) if cv is not None else (0, 0, 0)
    return yv, cv, tuple(ext), ys, cs, order


def cov_cells(t, order, lead):
    """A per-cell operand (``lead`` leading non-cell axes) as a dense tensor in the cell order ``order`` of
    :func:`cov_operands`, cells flattened."""
    v = t.permute(*range(lead), *[lead + o - 1 for o in order])
    return v.reshape(*t.shape[:lead], -1).contiguous()


def cov_levels_launch(y, q, centre=None, modulation=None, count=None, inside=None):
    """One pass of ``pre_cov_levels_f32`` over device fp32 ``y`` [n, *cells]: ``q`` [nk] (one half-width per level) or
    [nk, *cells], optional ``centre`` [n, *cells] and ``modulation`` [*cells].  Marginal: ``count`` int64 [nk] += cells
    inside; joint: ``inside`` bool [nk, >= n] cleared where a sample has a cell outside.  Asynchronous, no host sync."""
    n = y.shape[0]
    nk = q.shape[0]
    yv, cv, (A, B, C), ys, cs, order = cov_operands(y, centre)
    per_cell = q.dim() > 1
    qd = cov_cells(q, order, 1) if per_cell else q.contiguous()
    md = cov_cells(modulation, order, 0) if modulation is not None else None
    with torch.cuda.device(y.device):
        _lib.check(_lib.load_cov().pre_cov_levels_f32(
            _lib.ptr(yv), ys[0], ys[1], ys[2], _lib.ptr(cv), cs[0], cs[1], cs[2], n, A, B, C,
            _lib.ptr(qd), A * B * C if per_cell else 0, _lib.ptr(md), nk, _lib.ptr(count), _lib.ptr(inside),
            inside.stride(0) if inside is not None else 0, _lib.stream()), "pre_cov_levels_f32")


def _f64(x):
    """Would numpy (or torch) compute the bounds in float64?  (np.float64 is a Python float.)"""
    if isinstance(x, torch.Tensor):
        return x.dtype == torch.float64
    return isinstance(x, float) or (isinstance(x, np.ndarray) and x.dtype == np.float64)


def _levels(qhats):
    """The levels as given (a list / tuple / array / tensor with the level axis first)."""
    if isinstance(qhats, (list, tuple)):
        if any(_f64(q) for q in qhats):
            return list(qhats), True
        qhats = np.stack([np.asarray(q, np.float32) for q in qhats])
    return qhats, _f64(qhats)


def _loop_sets(q, centre, modulation):
    hw = q if modulation is None else q * modulation
    return [-hw, hw] if centre is None else [centre - hw, centre + hw]


def _levels_pass(qhats, y, centre, modulation, joint):
    """CoverageLevels over the whole of ``y`` on its device: (curve, inside or None, device)."""
    from . import pipeline
    ydev, back = _dev(y)
    if ydev.dim() < 1 or ydev.numel() == 0:
        raise ValueError("coverage of an empty test set")
    q = _dev(qhats)[0]
    c = _dev(centre)[0] if centre is not None else None
    m = _dev(modulation)[0] if modulation is not None else None
    cov = pipeline.CoverageLevels(ydev.shape[0], q.shape[0], ydev.device, joint=joint)
    cov.add_slab(ydev, q, centre=c, modulation=m)
    return cov, back


def emp_cov_levels(qhats, y, centre=None):
    """``[emp_cov([c - q[k], c + q[k]], y) for k]`` (no centre: ``[-q[k], q[k]]``) -> np.float64 [nk], in ONE pass over
    ``y`` and one device-to-host copy.  ``qhats``: ``calibrate_multi``'s [nk, *cells] (or [nk])."""
    qs, wide = _levels(qhats)
    if wide or _f64(centre):
        return np.array([emp_cov(_loop_sets(q, centre, None), y) for q in qs], np.float64)
    cov, _ = _levels_pass(qs, y, centre, None, joint=False)
    return cov.finish()


def emp_cov_joint_levels(qhats, y, modulation, centre=None):
    """``[emp_cov_joint([c - q[k]*m, c + q[k]*m], y) for k]`` (no centre: ``[-q[k]*m, q[k]*m]``) -> np.float64 [nk], in
    ONE pass over ``y``.  ``qhats``: the joint q-hats [nk] (fp32, as ``calibrate`` returns them)."""
    qs, wide = _levels(qhats)
    if wide or _f64(centre) or _f64(modulation):
        return np.array([emp_cov_joint(_loop_sets(q, centre, modulation), y) for q in qs], np.float64)
    cov, _ = _levels_pass(qs, y, centre, modulation, joint=True)
    return cov.finish()


def filter_sims_joint_levels(qhats, y, modulation, centre=None):
    """``filter_sims_joint`` at every level: bool [nk, n] (torch in -> torch out on y's device, numpy in -> numpy out)."""
    qs, wide = _levels(qhats)
    if wide or _f64(centre) or _f64(modulation):
        rows = [filter_sims_joint(_loop_sets(q, centre, modulation), y) for q in qs]
        return torch.stack(rows) if isinstance(y, torch.Tensor) else np.stack(rows)
    cov, back = _levels_pass(qs, y, centre, modulation, joint=True)
    return back(cov.inside) if isinstance(y, torch.Tensor) else cov.inside.cpu().numpy()
