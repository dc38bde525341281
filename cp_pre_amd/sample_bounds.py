"""Bounds on the solution u by sample acceptance: the inverse-sampling step of CP-PRE for PDE fields.

The reference's recipe (``Tests/test_advection_inv_sampling_marginal.py:312-359, 363-387, 476-491``; the active-learning
scripts ``Active_Learning/Advection_AL_Marginal.py:169-198``, ``Burgers_AL_Joint.py:332-338``): take candidate fields
``u_s``, compute their residuals ``r_s = D(u_s)``, keep the samples whose residual lies inside the calibrated set and
report the per-cell envelope of the kept ones::

    lo, hi, count = sample_envelope(u, accept)      # accept bool [nk, n] (or [n]): lo / hi [nk, *cells], count int64 [nk]
    lo, hi, count = sample_bounds(u, res, qhats, rule="joint", modulation=None, centre=None)
    lo, hi, count = sample_bounds(u, res, qhats, rule="threshold", threshold=0.9, modulation=None, centre=None)
    lo, hi, count = sample_bounds(u, res, qhats, rule="cellwise", modulation=None, centre=None)   # count int32 [nk, *cells]

Rules (level k: hw = q_k, times the modulation m when given; the set is [c - hw, c + hw], no centre: [-hw, hw]):
  * ``joint``: a sample is kept iff every residual cell is inside - decided by ``pipeline.CoverageLevels(joint=True)``,
    i.e. exactly as ``filter_sims_joint[_levels]`` decides (``:476-491``);
  * ``threshold``: kept iff the fraction of inside cells, in float64 as numpy's mean, is >= ``threshold``: the
    ``filter_sims_within_bounds(..., within=True)`` selection (``:312-359``) at every level, from ONE pass over ``res``
    that counts the inside cells of every (level, sample) (``pre_bounds_rowcount_f32``);
  * ``cellwise``: the per-cell rule (``:363-387``): cell j of sample s counts at level k iff r[s, j] is inside; lo / hi
    are over the counting samples of each cell and ``count`` is per cell.  ``res`` must have ``u``'s cell shape.
For ``joint`` and ``threshold`` the residual may have other cells than ``u`` (the reference tests the interior
``res[:, 1:-1, 1:-1]`` and takes the envelope of the whole field).  A centre is per cell (it broadcasts over the samples:
the reference centres its sets on one prediction's residual, ``prediction_sets[0][0]``) or, for ``joint`` and
``threshold``, laid out like ``res``.

Levels are taken as ``emp_cov_joint_levels`` takes them: fp32 levels (``calibrate`` returns fp32) take the one-pass
routes; float64 levels (Python floats) - or a float64 centre / modulation - make numpy's float64 bounds: acceptance then
comes from the per-level ``filter_sims_joint`` / ``filter_sims_within_bounds``, which round those bounds exactly, and the
cellwise bounds are rounded inwards to fp32 (``inductive_cp._directed_f32``); the envelope stays one pass either way.

Semantics (``include/cp_pre_bounds.h``): every result equals numpy's ``u[kept].min(0)`` / ``.max(0)`` (no rounding
anywhere; ``np.array_equal``, a zero's sign aside); a NaN in a kept sample makes that cell's bound NaN, as numpy; a
level that keeps nothing gives lo = +inf, hi = -inf and count 0 where numpy would raise on the empty reduction.

Reference bugs that are not reproduced (the intended recipe is computed):
  * ``:482`` tests the upper side with ``in_bounds_lower`` again: the upper bound is tested here;
  * ``:490`` indexes the samples with ``in_bounds`` instead of ``in_bounds_joint``: the joint flags select here;
  * ``:385-386`` swap the labels of ``Bounds_physical[0]`` and ``[1]``: lo is the minimum, hi the maximum here;
  * ``:377`` scrambles the axes with a reshape: the per-cell results keep ``u``'s cell axes here.

Streaming and sharding: :class:`SampleBounds` accumulates slabs of samples (``add_slab`` neither synchronises nor
communicates: it can be captured in a HIP graph) and its ``finish`` merges the ranks of ``group`` with two all-reduces
whose sizes follow from nk and the cell shape alone.  A C3-style job whose residual does not fit beside the fields runs in
two phases - acceptance over x-slabs of the residual, then the envelope over sample slabs of ``u``::

    cov = pipeline.CoverageLevels(n_local, nk, dev, joint=True, group=group)
    for x0, x1 in x_slabs:                                   # phase 1: every cell of every local sample, slab by slab
        cov.add_slab(residual(u_x_slab(x0, x1))[:, 1:-1, 1:-1, 1:-1], qhats, modulation=mod[..., x0:x1, :])
    sb = SampleBounds(nk, u_cells, dev, group=group)
    for s0, s1 in sample_slabs:                              # phase 2: the envelope of the kept samples
        sb.add_slab(u[s0:s1], cov.inside[:, s0:s1])
    lo, hi, count = sb.finish()
"""
from __future__ import annotations

from ctypes import byref, c_int64

import numpy as np
import torch

from . import _lib
from . import inductive_cp as icp

RULES = ("joint", "threshold", "cellwise")


# ------------------------------------------------------------------ operands
def _order(t):
    """The cell axes of ``t`` [n, *cells] in memory order (``canon``'s relabelling)."""
    return sorted(range(1, t.dim()), key=lambda k: (-t.stride(k), k))


def _operands(ts, order):
    """Views of ``ts`` (each [n, *cells], one cell shape) with the cell axes in ``order``, merged where every view allows:
    (views, (A, B, C), [(sN, sA, sB)] per view).  A view that cannot be streamed is copied into that order."""
    vs = [t.permute(0, *order) for t in ts]
    shape = tuple(vs[0].shape[1:])
    got = icp._merge_cells(shape, [v.stride()[1:] for v in vs])
    if got is None:
        vs = [v if icp._merge_cells(shape, [v.stride()[1:]]) is not None else v.contiguous() for v in vs]
        got = icp._merge_cells(shape, [v.stride()[1:] for v in vs])
    if got is None:
        vs = [v.contiguous() for v in vs]
        got = icp._merge_cells(shape, [v.stride()[1:] for v in vs])
    ext, st = got
    return vs, tuple(ext), [(v.stride(0), s[0], s[1]) for v, s in zip(vs, st)]


def _flat_cells(t, order, lead):
    """A per-cell operand ([*lead axes, *cells]) dense in the flat cell order of ``order``."""
    return icp.cov_cells(t, order, lead)


def _unflat(t, cells, order):
    """[nk, M] in the flat order of ``order`` -> [nk, *cells] in the logical order (contiguous)."""
    perm = [cells[o - 1] for o in order]
    return icp.uncanon(t.reshape(t.shape[0], *perm), order, 1).contiguous()


def centre_like(c, r):
    """A per-cell centre ``c`` [*cells] as a sample-stride-0 view [n, *cells] over ``r``'s samples, its cells laid out in
    ``r``'s memory order (a dense copy of the small per-cell array at most).  ``inductive_cp.cov_operands`` then reads it
    beside ``r`` where it lies: a centre in another order would be copied there into a full [n, *cells] buffer."""
    order = _order(r)
    dense = c.permute(*[o - 1 for o in order]).contiguous()
    return icp.uncanon(dense.unsqueeze(0), order, 1)[0].expand(r.shape)


def _workspace(fn, n, ext, nk, device):
    b = c_int64(0)
    _lib.check(fn(n, ext[0], ext[1], ext[2], nk, byref(b)), fn.__name__)
    return torch.empty(max(b.value, 1), dtype=torch.uint8, device=device), b.value


def _on_device(what, *ts):
    """Every operand a kernel reads or writes must be a tensor on the first one's HIP device: a host pointer handed to a
    kernel faults the GPU.  Raises TypeError before any launch."""
    dev = ts[0].device if isinstance(ts[0], torch.Tensor) else None
    for t in ts:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
            where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
            raise TypeError(f"{what}: every operand must be a tensor on the HIP device {dev} (got one on {where})")


# ------------------------------------------------------------------ launches (asynchronous, device fp32)
def envelope_launch(u, accept, order, lo, hi, count):
    """One pass of ``pre_bounds_envelope_f32``: ``lo`` / ``hi`` fp32 [nk, M] (flat cell order of ``order``) and ``count``
    int64 [nk] accumulate the envelope of the samples of ``u`` [n, *cells] accepted per level by ``accept`` (bool / uint8
    [nk, n]).  Every operand is on u's HIP device (TypeError otherwise)."""
    _on_device("envelope_launch", u, accept, lo, hi, count)
    n, nk = u.shape[0], accept.shape[0]
    (uv,), ext, ((sN, sA, sB),) = _operands([u], order)
    acc = accept.contiguous()
    acc = acc.view(torch.uint8) if acc.dtype == torch.bool else acc
    lib = _lib.load_bounds()
    work, wb = _workspace(lib.pre_bounds_envelope_workspace, n, ext, nk, u.device)
    with torch.cuda.device(u.device):
        _lib.check(lib.pre_bounds_envelope_f32(_lib.ptr(uv), sN, sA, sB, n, ext[0], ext[1], ext[2], _lib.ptr(acc),
                                               acc.stride(0), nk, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(count),
                                               _lib.ptr(work), wb, _lib.stream()), "pre_bounds_envelope_f32")


def rowcount_launch(r, q, centre, modulation, counts):
    """``counts`` int32 [nk, n] += inside cells of every (level, sample) of ``r`` [n, *cells]; ``q`` [nk] or [nk, *cells],
    ``centre`` [*cells] or laid out like ``r``, ``modulation`` [*cells]; every operand on r's HIP device."""
    _on_device("rowcount_launch", r, q, centre, modulation, counts)
    n, nk = r.shape[0], q.shape[0]
    order = _order(r)
    per_sample_c = centre is not None and centre.dim() == r.dim()
    vs, ext, st = _operands([r, centre] if per_sample_c else [r], order)
    A, B, C = ext
    if per_sample_c:
        cv, cs = vs[1], st[1]
    elif centre is not None:
        cv, cs = _flat_cells(centre, order, 0), (0, B * C, C)
    else:
        cv, cs = None, (0, 0, 0)
    per_cell_q = q.dim() > 1
    qd = _flat_cells(q, order, 1) if per_cell_q else q.contiguous()
    md = _flat_cells(modulation, order, 0) if modulation is not None else None
    rs = st[0]
    with torch.cuda.device(r.device):
        _lib.check(_lib.load_bounds().pre_bounds_rowcount_f32(
            _lib.ptr(vs[0]), rs[0], rs[1], rs[2], _lib.ptr(cv), cs[0], cs[1], cs[2], n, A, B, C,
            _lib.ptr(qd), A * B * C if per_cell_q else 0, _lib.ptr(md), nk, _lib.ptr(counts), counts.stride(0),
            _lib.stream()), "pre_bounds_rowcount_f32")


def cellwise_launch(u, r, order, lo, hi, count, q=None, modulation=None, centre=None, blo=None, bhi=None):
    """One pass of ``pre_bounds_cellwise_f32`` over ``u`` and ``r`` (one cell shape): fp32 ``q`` [nk] / [nk, *cells] with
    optional ``modulation`` / ``centre`` [*cells], or the bounds ``blo`` / ``bhi`` [nk, *cells] outright.  ``lo`` / ``hi``
    fp32 and ``count`` int32 [nk, M] in the flat cell order of ``order`` accumulate; every operand on u's HIP device."""
    _on_device("cellwise_launch", u, r, lo, hi, count, q, modulation, centre, blo, bhi)
    n = u.shape[0]
    (uv, rv), ext, (us, rs) = _operands([u, r], order)
    M = ext[0] * ext[1] * ext[2]
    if blo is not None:
        nk = blo.shape[0]
        qd = md = cd = None
        bl, bh = _flat_cells(blo, order, 1), _flat_cells(bhi, order, 1)
    else:
        nk = q.shape[0]
        qd = _flat_cells(q, order, 1) if q.dim() > 1 else q.contiguous()
        md = _flat_cells(modulation, order, 0) if modulation is not None else None
        cd = _flat_cells(centre, order, 0) if centre is not None else None
        bl = bh = None
    lib = _lib.load_bounds()
    work, wb = _workspace(lib.pre_bounds_cellwise_workspace, n, ext, nk, u.device)
    with torch.cuda.device(u.device):
        _lib.check(lib.pre_bounds_cellwise_f32(
            _lib.ptr(uv), us[0], us[1], us[2], _lib.ptr(rv), rs[0], rs[1], rs[2], n, ext[0], ext[1], ext[2],
            _lib.ptr(qd), M if (qd is not None and q.dim() > 1) else 0, _lib.ptr(md), _lib.ptr(cd), _lib.ptr(bl),
            _lib.ptr(bh), nk, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(count), _lib.ptr(work), wb, _lib.stream()),
            "pre_bounds_cellwise_f32")


# ------------------------------------------------------------------ argument handling
def _as_device(x, name):
    """fp32 device tensor of ``u`` / ``res`` and a function that converts results back (torch -> its device, numpy ->
    numpy).  Raises TypeError for another dtype."""
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32:
            raise TypeError(f"{name} must be float32 (got {x.dtype})")
        if x.is_cuda:
            return x, (lambda t: t)
        _lib.require_gpu()
        origin = x.device
        return x.cuda(), (lambda t: t.to(origin))
    arr = np.asarray(x)
    if arr.dtype != np.float32:
        raise TypeError(f"{name} must be float32 (got {arr.dtype})")
    _lib.require_gpu()
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda(), (lambda t: t.cpu().numpy())


def _shape(x):
    return tuple(x.shape)


def _check_samples(u, name="u"):
    s = _shape(u)
    if len(s) < 2 or s[0] == 0 or any(d == 0 for d in s[1:]):
        raise ValueError(f"{name} must be [n >= 1, *cells] with cells (got shape {s})")


def _accept_rows(accept, n):
    """(accept as bool [nk, n] without a device, squeeze): the level axis is added for a 1-D mask."""
    a = accept if isinstance(accept, torch.Tensor) else torch.from_numpy(np.asarray(accept))
    squeeze = a.dim() == 1
    if squeeze:
        a = a.unsqueeze(0)
    if a.dim() != 2 or a.shape[1] != n:
        raise ValueError(f"accept must be [nk, n] or [n] with n = {n} (got {tuple(a.shape)})")
    if a.shape[0] == 0:
        raise ValueError("accept has no level (nk == 0)")
    if a.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"accept must be bool (got {a.dtype})")
    return a, squeeze


def level_route(qhats, centre=None, modulation=None):
    """(levels, route): "f32" for the one-pass routes, "f64" when numpy would build the bounds in float64 (Python-float /
    float64 levels, a float64 centre or modulation).  Raises for an empty level list."""
    if isinstance(qhats, (list, tuple)) and len(qhats) == 0:
        raise ValueError("no level (nk == 0)")
    qs, wide = icp._levels(qhats)
    if not isinstance(qs, list) and (np.ndim(qs) == 0 or len(qs) == 0):
        raise ValueError("qhats must have a level axis with nk >= 1")
    return qs, "f64" if (wide or icp._f64(centre) or icp._f64(modulation)) else "f32"


def _dev_opt(x, device):
    """An optional per-cell / per-sample fp32 operand on ``device``."""
    if x is None:
        return None
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
    return t.to(device=device, dtype=torch.float32)


# ------------------------------------------------------------------ public API
def sample_envelope(u, accept):
    """Per level k: lo[k] = min, hi[k] = max over the samples s with accept[k, s] of u[s] (per cell), and count[k] the
    number of accepted samples.  ``u`` fp32 [n, *cells] (torch: any layout with a dense innermost memory axis is read where
    it lies; numpy: uploaded), ``accept`` bool [nk, n] (-> lo / hi [nk, *cells], count int64 [nk]) or [n] (no level axis)."""
    _check_samples(u)
    acc, squeeze = _accept_rows(accept, _shape(u)[0])
    ud, back = _as_device(u, "u")
    lo, hi, count = _envelope(ud, acc.to(ud.device))
    if squeeze:
        lo, hi, count = lo[0], hi[0], count[0]
    return back(lo), back(hi), back(count)


def _envelope(ud, acc):
    nk, cells = acc.shape[0], tuple(ud.shape[1:])
    order = _order(ud)
    M = int(np.prod(cells))
    lo = torch.full((nk, M), float("inf"), dtype=torch.float32, device=ud.device)
    hi = torch.full((nk, M), float("-inf"), dtype=torch.float32, device=ud.device)
    count = torch.zeros(nk, dtype=torch.int64, device=ud.device)
    envelope_launch(ud, acc, order, lo, hi, count)
    return _unflat(lo, cells, order), _unflat(hi, cells, order), count


def sample_bounds(u, res, qhats, rule="joint", threshold=0.9, modulation=None, centre=None):
    """Solution bounds from the calibrated residual sets at every level of ``qhats`` (see the module docstring for the
    rules): (lo, hi [nk, *u cells], count - int64 [nk] for ``joint`` / ``threshold``, int32 [nk, *cells] for
    ``cellwise``).  torch in -> torch out on u's device, numpy in -> numpy out."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES} (got {rule!r})")
    _check_samples(u)
    _check_samples(res, "res")
    if _shape(u)[0] != _shape(res)[0]:
        raise ValueError(f"u has {_shape(u)[0]} samples, res {_shape(res)[0]}")
    if rule == "cellwise" and _shape(u)[1:] != _shape(res)[1:]:
        raise ValueError(f"cellwise: res must have u's cells ({_shape(res)[1:]} vs {_shape(u)[1:]})")
    qs, route = level_route(qhats, centre, modulation)
    rcells = _shape(res)[1:]
    if modulation is not None and _shape(modulation) != rcells:
        raise ValueError(f"the modulation has the residual's cell shape {rcells} (got {_shape(modulation)})")
    if centre is not None and _shape(centre) not in (rcells, _shape(res)):
        raise ValueError(f"the centre is per cell {rcells} or laid out like res (got {_shape(centre)})")
    if rule == "cellwise" and centre is not None and _shape(centre) != rcells:
        raise ValueError("cellwise: the centre is per cell")
    if rule == "threshold" and not (0.0 <= float(threshold) <= 1.0):
        raise ValueError(f"threshold must lie in [0, 1] (got {threshold})")
    ud, back = _as_device(u, "u")
    if route == "f64":
        return _bounds_f64(ud, back, res, qs, rule, threshold, modulation, centre)
    rd, _ = _as_device(res, "res")
    q = _dev_opt(qs, ud.device)
    if q.dim() > 1 and tuple(q.shape[1:]) != rcells:
        raise ValueError(f"per-cell q-hats of shape {tuple(q.shape)} for residual cells {rcells}")
    m, c = _dev_opt(modulation, ud.device), _dev_opt(centre, ud.device)
    if rule == "cellwise":
        return _cellwise(ud, rd, back, q=q, modulation=m, centre=c)
    if rule == "joint":
        from . import pipeline
        cov = pipeline.CoverageLevels(rd.shape[0], q.shape[0], ud.device, joint=True)
        cov.add_slab(rd, q, centre=centre_like(c, rd) if c is not None and c.dim() < rd.dim() else c, modulation=m)
        acc = cov.inside
    else:
        counts = torch.zeros(q.shape[0], rd.shape[0], dtype=torch.int32, device=ud.device)
        rowcount_launch(rd, q, c, m, counts)
        acc = (counts.double() / float(np.prod(rcells))) >= float(threshold)      # numpy: mean of bools in float64
    lo, hi, count = _envelope(ud, acc)
    return back(lo), back(hi), back(count)


def _cellwise(ud, rd, back, **kw):
    cells = tuple(ud.shape[1:])
    nk = (kw["blo"] if kw.get("blo") is not None else kw["q"]).shape[0]
    order = _order(ud)
    M = int(np.prod(cells))
    lo = torch.full((nk, M), float("inf"), dtype=torch.float32, device=ud.device)
    hi = torch.full((nk, M), float("-inf"), dtype=torch.float32, device=ud.device)
    count = torch.zeros(nk, M, dtype=torch.int32, device=ud.device)
    cellwise_launch(ud, rd, order, lo, hi, count, **kw)
    return back(_unflat(lo, cells, order)), back(_unflat(hi, cells, order)), back(_unflat(count, cells, order))


def _bounds_f64(ud, back, res, qs, rule, threshold, modulation, centre):
    """float64 bounds, as numpy builds them: per-level acceptance (or inward-rounded cellwise bounds), one envelope."""
    if rule == "cellwise":
        rd, _ = _as_device(res, "res")
        blo, bhi = [], []
        for q in qs:
            lo64, hi64 = icp._loop_sets(_np64(q), _np64(centre), _np64(modulation))
            shape = _shape(res)[1:]
            blo.append(np.broadcast_to(icp._directed_f32(np.asarray(lo64, np.float64), up=True), shape))
            bhi.append(np.broadcast_to(icp._directed_f32(np.asarray(hi64, np.float64), up=False), shape))
        blo = torch.from_numpy(np.ascontiguousarray(np.stack(blo), np.float32)).to(ud.device)
        bhi = torch.from_numpy(np.ascontiguousarray(np.stack(bhi), np.float32)).to(ud.device)
        return _cellwise(ud, rd, back, blo=blo, bhi=bhi)
    rows = []
    for q in qs:
        sets = icp._loop_sets(q, centre, modulation)
        if rule == "joint":
            f = icp.filter_sims_joint(sets, res)
        else:
            f = icp.filter_sims_within_bounds(sets[0], sets[1], res, threshold, within=True)
        rows.append(f if isinstance(f, torch.Tensor) else torch.from_numpy(np.asarray(f)))
    acc = torch.stack([r.to(ud.device) for r in rows])
    lo, hi, count = _envelope(ud, acc)
    return back(lo), back(hi), back(count)


def _np64(x):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return x


# ------------------------------------------------------------------ streamed and sharded
class HipBoundsOps:
    """Device back end of :class:`SampleBounds` (one ``libcp_pre_bounds.so`` pass per slab)."""

    @staticmethod
    def zeros_bounds(nk, M, device):
        """lo = +inf, hi = -inf fp32 [nk, M]; count int64 [nk] = 0."""
        return (torch.full((nk, M), float("inf"), dtype=torch.float32, device=device),
                torch.full((nk, M), float("-inf"), dtype=torch.float32, device=device),
                torch.zeros(nk, dtype=torch.int64, device=device))

    @staticmethod
    def envelope(u, accept, order, lo, hi, count):
        envelope_launch(u, accept, order, lo, hi, count)


class SampleBounds:
    """The envelope of accepted samples, streamed over slabs of samples and sharded over the ranks of ``group`` (each
    rank its own samples, any number, none included).  ``add_slab(u_slab, accept_slab)``: ``u_slab`` fp32 [n_slab,
    *cell_shape] on ``device`` (any layout; a slab elsewhere is refused with a TypeError), ``accept_slab`` bool [nk,
    n_slab] (``CoverageLevels.inside[:, s0:s1]``; a numpy or host mask is copied to the slab's device first, which
    synchronises).  With a device mask it launches one pass and neither synchronises nor communicates: it can be captured
    in a HIP graph.  ``finish()`` returns new tensors (lo, hi [nk, *cell_shape], count int64 [nk]) - later slabs do not
    change them - over the group's samples, the same on every rank, after at most
    two collectives: a MIN all-reduce of [lo, -hi] (fp32, NaN replaced) and a SUM all-reduce of int64 [nk + nk*M] (the
    counts and a per-cell NaN flag that restores the NaN a backend's MIN may not propagate).  Their sizes follow from nk
    and the cell shape alone."""

    def __init__(self, nk, cell_shape, device, group=None, ops=None):
        cell_shape = tuple(int(d) for d in cell_shape)
        if nk < 1 or not cell_shape or any(d < 1 for d in cell_shape):
            raise ValueError(f"SampleBounds needs nk >= 1 and a cell shape (got {nk}, {cell_shape})")
        self.ops = ops or HipBoundsOps
        self.nk, self.cells, self.device, self.group = nk, cell_shape, device, group
        self.M = int(np.prod(cell_shape))
        self.lo, self.hi, self.count = self.ops.zeros_bounds(nk, self.M, device)
        self.order = None                    # flat cell order of lo / hi: the first slab's memory order

    def add_slab(self, u_slab, accept_slab):
        if not isinstance(u_slab, torch.Tensor) or u_slab.dtype != torch.float32:
            raise TypeError("u_slab must be a float32 tensor")
        if tuple(u_slab.shape[1:]) != self.cells or u_slab.shape[0] == 0:
            raise ValueError(f"slab of shape {tuple(u_slab.shape)}, expected [n >= 1, *{self.cells}]")
        acc, _ = _accept_rows(accept_slab, u_slab.shape[0])
        if acc.shape[0] != self.nk:
            raise ValueError(f"accept_slab has {acc.shape[0]} levels, expected {self.nk}")
        if u_slab.device != self.lo.device:
            raise TypeError(f"u_slab is on {u_slab.device}, this SampleBounds accumulates on {self.lo.device}")
        if self.ops is HipBoundsOps and not u_slab.is_cuda:
            raise TypeError("u_slab must be on the HIP device")
        acc = acc.to(u_slab.device)                  # (a host mask: one copy; a device mask: no-op)
        if self.order is None:
            self.order = _order(u_slab) if u_slab.dim() > 1 else []
        self.ops.envelope(u_slab, acc, self.order, self.lo, self.hi, self.count)

    def finish(self):
        order = self.order or list(range(1, len(self.cells) + 1))
        lo = _unflat(self.lo, self.cells, order).reshape(self.nk, -1)
        hi = _unflat(self.hi, self.cells, order).reshape(self.nk, -1)
        count = self.count
        if self.group is not None:
            nan = torch.isnan(lo)                                     # (hi is NaN exactly where lo is: one sample set)
            packed = torch.stack([lo, -hi]).masked_fill_(nan.unsqueeze(0).expand(2, -1, -1), float("inf"))
            ints = torch.cat([count, nan.reshape(-1).to(torch.int64)])
            torch.distributed.all_reduce(packed, op=torch.distributed.ReduceOp.MIN, group=self.group)
            torch.distributed.all_reduce(ints, group=self.group)
            count = ints[:self.nk].clone()
            nan = ints[self.nk:].reshape(self.nk, -1) > 0
            lo = packed[0].masked_fill(nan, float("nan"))
            hi = (-packed[1]).masked_fill(nan, float("nan"))
        else:                                        # (new tensors, not views of the accumulators)
            lo, hi, count = lo.clone(), hi.clone(), count.clone()
        return lo.reshape(self.nk, *self.cells), hi.reshape(self.nk, *self.cells), count
