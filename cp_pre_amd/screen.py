"""Screen predictions against calibrated sets without storing the residual.

What a calibrated joint set is used for afterwards (``Joint/NS_Residuals_CP.py:328-329,350-352,502-503``,
``Joint/MHD_Residuals_CP.py:409-410``, ``Active_Learning/Burgers_AL_Joint.py:305-379``,
``Other_UQ/Evaluation/Eval.py:287-288``) is to ask of each new prediction whether its residual lies inside the set::

    ns = NavierStokes(dt, dx, dy)
    s = screen(ns.residual_momentum, vars, qhats, modulation)     # one launch, no residual tensor
    s.score                 # fp32 [n]      max over the counted cells of |r| / m   (ncf_metric_joint(..., crop=1))
    s.inside                # int64 [nk, n] counted cells with |r| <= q_k * m
    s.accept()              # bool [nk, n]  filter_sims_joint at every level
    s.coverage_joint()      # float64 [nk]  emp_cov_joint at every level
    s.coverage_marginal()   # float64 [nk]  emp_cov at every level, bounds +-q_k * m
    s.within(0.95)          # bool [nk, n]  filter_sims_within_bounds

Fused route (``libcp_pre_screen.so``, ``include/cp_pre_screen.h``): the march of the residual passes evaluates the residual
in registers and reduces it per sample - a maximum and nk integer counts - so the three launches and the residual buffer of
the route a user writes today (residual, ``ncf_metric_joint``, ``CoverageLevels``) become one launch that stores nothing.
Fused kinds: ``stencil3d`` (a ``ConvOperator`` of ``convops_2d``, ``PRE_Wave``), ``linear2`` (NS continuity, MHD gauss),
``ns_momentum``, ``mhd_continuity`` / ``mhd_momentum`` / ``mhd_energy`` / ``mhd_induction`` and, opt-in, ``jorek_continuity``
/ ``jorek_temperature`` (below).  Everything else takes that three-pass route (residual, ``ncf_metric_joint``, then
``CoverageLevels`` once per sample) and returns the same ``Screened``: views without unit stride on their last axis, row
widths that are no multiple of 4, inputs on the CPU (staged as elsewhere), ``minus=`` (unless ``pair=True``, below),
operator kernels off the 7-point star or requiring grad, ``fused=False``, float64 levels or modulation.  ``last_route()``
says which route the last call took.

The 1-D family on ``[BS,Nt,Nx]`` (a ``ConvOperator`` of ``convops_1d``, ``Advection.residual``, ``Burgers.residual``) has a
fused route of its own (``libcp_pre_screen1d.so``, ``include/cp_pre_screen1d.h``): the march above would run over the
batch, so there a workgroup owns one sample's ``[Nt,Nx]`` plane and marches over its rows, in either layout (Nx-fastest, or
the Nt-fastest ``u.permute(0,1,3,2)[:,0]`` of the active-learning scripts).  Routes ``fused:rows_stencil2d`` and
``fused:rows_burgers``; the three-pass route is kept for the reasons above, for a contiguous axis that is no multiple of 4
and for a ``[BS,1,Nt,Nx]`` input (screened as ``vars[:, 0]``).  ``halo_x`` raises for this family.

Nt-fastest views of the 2-D residuals - ``pred.permute(0,1,4,2,3)`` of the surrogate's native ``[BS,F,Nx,Ny,Nt]``, what
``Joint/NS_Residuals_CP.py:282-305`` and ``Joint/MHD_Residuals_CP.py:326-346`` pass - have a fused route as well
(``libcp_pre_screenflat.so``, ``include/cp_pre_screenflat.h``): the merged-row march of the residual pass's flat form with
the same end of a plane.  Routes ``fused:flat_<kind>``; taken when the rows are dense (``stride(Ny) == Nt``), ``Ny*Nt`` is a
multiple of 4 and ``Nt < FLAT_MAX_NT``, else the three-pass route says why.  ``halo_x`` on such a view behaves as before.

The reduced-MHD residuals (``JOREK.residual_continuity`` / ``residual_temperature``, ``Joint/JOREK_residuals_CP.py:210-243,
297-308``) are screened in one launch only where the caller asks for it: ``screen(..., jorek=True)`` /
``Screen.add_slab(..., jorek=True)`` (``libcp_pre_screenjorek.so``, ``include/cp_pre_screenjorek.h``: both marches above with
the functors of ``pre_residual_jorek_f32``).  ``vars`` is the script's ``[BS,F,Nx,Ny,Nt]``; every layout decision is taken on
its ``unstack_fields`` views ``[BS,Nt,Nx,Ny]``: the dense tensor the script holds is Nt-fastest (route
``fused:flat_jorek_<eq>``), a view of memory ``[BS,F,Nt,Nx,Ny]`` is Ny-fastest (``fused:jorek_<eq>``).  A bound method is
evaluated with ``norms=False``; ``norms=True`` of the continuity equation is handed over as in ``losses``:
``functools.partial(jorek.residual_continuity, norms=True)`` (no positional arguments, no other keyword; the scalars are
``JOREK._coef(eq, norms)``, the route names the same, and the three-pass route calls the partial, so both routes evaluate
the same form; without ``dx, dy, dt`` it raises the method's ``ValueError``, on the temperature equation the reference's
exception, before any launch).  ``halo_x`` raises, as for every method whose residual pass reads no halo.  Without the keyword JOREK keeps the three-pass
route (``fallback:no fused screen for JOREK``) and the library is never loaded.

The data-driven score ``d = r(vars) - r(minus)`` - what every ``Joint/`` script calibrates on first and then validates on
held-out pairs (``Joint/NS_Residuals_CP.py:289-290, 307-313``, the same lines of ``Joint/MHD_Residuals_CP.py``,
``Joint/Burgers_Residuals_CP.py:217-220``; ``Other_UQ/Evaluation/Eval.py:278-281``) - is screened in one launch only where
the caller asks for it: ``screen(..., minus=pred, pair=True)`` / ``Screen.add_slab(..., minus=, pair=True)``
(``libcp_pre_screenpair.so``, ``include/cp_pre_screenpair.h``: both marches above with the paired functor of
``libcp_pre_pair.so``).  Routes ``fused:pair_<kind>`` (Ny-fastest sets) and ``fused:flat_pair_<kind>`` (Nt-fastest sets) for
the kinds ``stencil3d``, ``linear2``, ``ns_momentum`` and ``mhd_continuity``; both sets must be on the device and in the same
layout, and each must meet the layout conditions above (a reason of the second set is reported as ``minus: <reason>``).
Everything else keeps the three-pass route and says why: ``no paired screen for <kind>`` (the other three MHD equations,
JOREK), ``no paired screen for the 1-D family`` (under ``pair=True``; below), ``field sets in different layouts``, and the reasons above.  Under
``halo_x`` both sets must be Ny-contiguous device views with rows -1 and X in memory.  Without ``pair=True`` a ``minus=``
call takes ``fallback:minus=`` as before and the library is never loaded; ``pair=True`` without ``minus`` has no effect.
What is computed is the three-pass route's answer: ``d = fl(fl(r(vars)) - fl(r(minus)))``, ``score = max |d| / m``,
``inside = #{|d| <= fl(q_k * m)}`` - the one-sided test on the difference, NOT the reference's two-sided form
``c - hw <= y <= c + hw`` on the two residual arrays; the two can differ in a cell that sits within rounding of the band.
``minus`` may be ``vars`` itself: every score is then exactly 0 and every counted cell inside wherever ``q_k * m >= 0``.

The 1-D family has a paired screen as well, asked for by ``pair="rows"`` (``Joint/Burgers_Residuals_CP.py:217-220, 250-259``,
``Joint/Advection_Residuals_CP.py`` and the ``Active_Learning/*_AL_Joint.py`` loops; ``libcp_pre_screen1dpair.so``,
``include/cp_pre_screen1dpair.h``: the row march of the rows route on two field sets, with the same paired functor).
``pair="rows"`` does everything ``pair=True`` does and, for ``rows_kind`` ``stencil2d`` and ``burgers``, takes routes
``fused:rows_pair_stencil2d`` / ``fused:rows_pair_burgers`` - as ``mhd="flat"`` stands next to ``mhd=True`` in ``losses``.
Both sets must be on the device with their unit stride on the same axis (Nx-fastest, or the Nt-fastest
``u.permute(0,1,3,2)[:,0]``; else ``field sets in different layouts``), each with its own sample and row pitch; the reasons of
the rows route above apply to both (``minus: <reason>`` for the second), the modulation is relabelled or copied as there, and
``halo_x`` raises.  The semantics are those of the paragraph above.  ``pair=True`` keeps ``no paired screen for the 1-D
family``, any other value of ``pair`` keeps its truthiness, and without ``pair="rows"`` the library is never loaded.

Per-cell (marginal) sets at ONE level - ``Other_UQ/Evaluation/Eval.py:286-288`` and the ``Marginal/`` validation at a fixed
alpha, where the calibration left a quantile per cell - need no entry of their own: pass the per-cell quantiles as the
modulation and one level of 1, ``screen(method, vars, torch.ones(1), modulation=qhat_cells, [minus=pred, pair=True])``.
``1.0f * m == m`` exactly, so ``inside[0]`` counts ``|d| <= qhat_cells`` exactly (``emp_cov_levels``'s count per sample).

Per-cell sets at SEVERAL levels - how every ``Marginal/*_Residuals_CP.py`` script ends (``Marginal/NS_Residuals_CP.py:307-337``,
``Marginal/MHD_Residuals_CP.py:408-418``, ``Marginal/Wave_Residuals_CP.py:284-288``): ``calibrate_multi`` leaves a quantile per
cell at ten alphas, and each is checked against the residual of every held-out prediction - have an entry of their own,
``screen_cells(method, vars, qcells, modulation=None)`` / ``ScreenCells`` (``libcp_pre_screencells.so``,
``include/cp_pre_screencells.h``): both marches above with nk level quads per cell and plane next to the field loads, the
samples taken in groups (``sample_group()``) so that a group shares its level quads in an XCD's L2.  ``inside[k, b]`` counts
``|r| <= qcells[k][cell]`` (``* modulation[cell]`` with one): ``emp_cov_levels``'s count with per-cell levels, per sample.
Routes ``fused:cells_<kind>`` / ``fused:flat_cells_<kind>`` for the kinds of the first paragraph; the 1-D family (without
``rows=True``, below), JOREK (without ``jorek=True``, further below), ``minus=`` (without ``pair=True``, further below) and every reason above keep the three-pass route (one ``CoverageLevels`` pass per
sample with the per-cell levels).  Without a call to these two the library is never loaded.

The 1-D family has per-cell screens as well, asked for by ``rows=True`` on ``screen_cells`` / ``ScreenCells.add_slab``
(``Active_Learning/Advection_AL_Marginal.py:169-198, 290-311`` keeps or rejects every candidate by ``within(threshold)`` on
per-cell sets; ``Marginal/Burgers_Residuals_CP.py:274-283`` and ``Marginal/Advection_Residuals_CP.py`` check ``±qhat[cell]``
at ten alphas; ``libcp_pre_screen1dcells.so``, ``include/cp_pre_screen1dcells.h``: the row march of the rows route with nk
level quads per cell and row, the samples in groups of ``sample_group_rows()``).  ``vars`` is ``[BS,Nt,Nx]`` in either layout,
``qcells`` fp32 ``[nk,Nt,Nx]`` (with ``boundary=False`` also the cropped ``[nk,Nt-2,Nx-2]``, padded once with NaN in the
fields' layout); levels and a modulation whose unit-stride axis is not the fields' are copied once.  Routes
``fused:rows_cells_stencil2d`` / ``fused:rows_cells_burgers``.  With ``minus=`` the paired entries run - the data-driven form
``|r(vars) - r(minus)| <= qcells[k][cell] (* m)`` of ``Marginal/Burgers_Residuals_CP.py:249-259``, the one-sided test of the
paragraphs above - with routes ``fused:rows_cells_pair_stencil2d`` / ``fused:rows_cells_pair_burgers``; both sets in the same
layout, each with its own pitches.  The reasons that keep the three-pass route are ``prepare_rows``', in its order (CPU
inputs, float64 levels, a ``[BS,1,Nt,Nx]`` input, no unit-stride axis, a contiguous axis that is no multiple of 4, sets in
different layouts, kernels off the star or requiring grad, ``declined by the library``); ``halo_x`` raises.  Row slabs with
crops compose to the bits of the whole plane.  Without ``rows=True`` the family keeps ``fallback:1-D family: the marched
axis is the batch`` and the library is never loaded; on a method outside the family the keyword has no effect.

Per-cell sets for the data-driven score of the 2-D residuals - how every ``Marginal/*_Residuals_CP.py`` script validates its
held-out pairs (``Marginal/NS_Residuals_CP.py:282-312``, ``Marginal/MHD_Residuals_CP.py:350-392``,
``Marginal/Wave_Residuals_CP.py:219-254``: a quantile per cell at ten alphas on ``|r(y) - r(y_hat)|``, then ``r(y)`` inside
``r(y_hat) ± qhat[k][cell]``) - are screened in one launch only where the caller asks for it: ``screen_cells(method, vars,
qcells, minus=pred, pair=True)`` / ``ScreenCells.add_slab(..., minus=, pair=True)`` (``libcp_pre_screencellspair.so``,
``include/cp_pre_screencellspair.h``: both marches above with the paired functor AND the level quads; the samples in groups of
``sample_group_pair()``).  Routes ``fused:cells_pair_<kind>`` / ``fused:flat_cells_pair_<kind>`` for the kinds of
``pair=True`` on ``screen``; the reasons that keep the three-pass route, their order, ``halo_x`` and the semantics (the
one-sided test on ``d``) are that paragraph's, the level fields' layout and rim this one's predecessor's.  Without
``pair=True`` a ``minus=`` call keeps ``fallback:minus=`` and the library is never loaded; ``pair=True`` without ``minus``
has no effect, and ``rows=True`` with ``minus=`` is as before.

Per-cell sets for the JOREK residuals - how ``Marginal/JOREK_residuals_CP.py:297-311`` ends: per-cell q-hats at ten alphas,
then which cells of ``residual_temperature(pred)`` lie inside ``[-qhat, +qhat]`` at each - are screened in one launch only
where the caller asks for it: ``screen_cells(method, vars, qcells, jorek=True)`` / ``ScreenCells.add_slab(..., jorek=True)``
(``libcp_pre_screenjorekcells.so``, ``include/cp_pre_screenjorekcells.h``: both marches above with the JOREK functors AND the
level quads; the samples in groups of ``sample_group_jorek()``).  ``vars`` is ``[BS,3,Nx,Ny,Nt]``, ``qcells`` ``[nk,Nt,Nx,Ny]``
(with ``boundary=False`` also the cropped ``[nk,Nt-2,Nx-2,Ny-2]``); levels and modulation are re-laid to the fields'
unit-stride axis.  Routes ``fused:flat_cells_jorek_<eq>`` (the dense tensor) and ``fused:cells_jorek_<eq>`` (Ny-fastest field
views); the reasons that keep the three-pass route are those of ``screen(..., jorek=True)``, ``len(R) != Ny`` and ``halo_x``
raise before any launch, and ``minus=`` keeps ``fallback:minus=`` (two temperature sets are 8 views against the march's 6).
The method may be the ``norms`` partial of the paragraph on JOREK above.  ``jorek=True`` on any other method is a
``TypeError``; without the keyword JOREK keeps ``fallback:no fused screen for JOREK`` and the library is never loaded.

Per-sample statistics of the residual - the 'PRE' acquisition of the active-learning loops, which orders the candidates by
``torch.sort(torch.mean(torch.abs(pred_residual), axis=...))`` (``Active_Learning/Wave_AL_Joint.py:403-408``,
``Active_Learning/Advection_AL_Joint.py:340-345``; the signed mean in ``Active_Learning/Burgers_AL_Joint.py:340-345``) - come
from ``screen_stats(method, vars, boundary=False)`` / ``ScreenStats`` (``libcp_pre_screenstats.so``,
``include/cp_pre_screenstats.h``): the three marches above with three float64 accumulators per thread in place of the counts,
no levels and no modulation.  One launch evaluates the residual and stores nothing but a workgroup's partial sums into a
cached per-device workspace; a second, tiny launch adds each sample's partials in a fixed order (no floating-point atomics:
the same inputs give the same bytes on every run).  The result is a ``SampleStats``: ``sum``, ``sum_abs``, ``sum_sq``
(float64 [n]), ``max_abs`` (float32 [n], bitwise the ``score`` of ``screen`` without a modulation), ``mean()``,
``mean_abs()``, ``mean_sq()``, ``rms()``, ``order(by="mean_abs")`` - the scripts' ``sort_index`` - and ``take(k)``.  Routes
``fused:stats_<kind>`` (Ny-fastest), ``fused:flat_stats_<kind>`` (Nt-fastest) and, for the 1-D family by default,
``fused:rows_stats_<rows_kind>``.  Everything else stores the residual by the existing pass and reduces its counted region in
float64, with ``fallback:<why>``: the reasons of the paragraphs above in their order (CPU inputs, no unit stride, widths that
are no multiple of 4, ``Nt >= 96`` or rows that are not dense on an Nt-fastest view, a ``[BS,1,Nt,Nx]`` input, spectral
operators, kernels off the star or requiring grad, ``fused=False``, fewer than six MHD channels, ``declined by the library``:
the general-star tap structure of the MHD momentum and energy equations, which does not fit the register file next to the
accumulators), and JOREK keeps ``fallback:no fused stats for JOREK``.  ``minus=`` is not accepted; ``halo_x`` raises where
``Screen.add_slab`` raises.  Without a call to these two the library is never loaded, and they load no other screen library.

Residuals under boundary conditions on the x-y rim (``bc=`` on the constructors of ``residuals``: ``r_bc(fields) =
r_zero_pad(pad(f) for f in fields)[..., :, 1:-1, 1:-1]``, the time axis zero-padded) are screened and reduced in one launch
only where the caller asks for it: ``screen(method, vars, qhats, modulation, bc=True)`` / ``Screen.add_slab(..., bc=True)`` /
``screen_stats(method, vars, bc=True)`` / ``ScreenStats.add_slab(..., bc=True)`` on a method of ``NavierStokes`` / ``PRE_NS``,
``MHD`` / ``PRE_MHD`` or ``PRE_Wave`` whose object was built with ``bc=`` (the object's condition is used, read anew on every
call; without one, or on JOREK, a ``TypeError``), and ``bc=<condition>`` - anything ``residuals._BC`` takes - on a bare
``convops_2d.ConvOperator``, where the screened quantity is ``residuals.apply_bc(D, field, bc)`` (any other value on a bound
method is a ``TypeError``).  ``libcp_pre_screenbc.so`` (``include/cp_pre_screenbc.h``): the Ny-fastest march above with the
halo row beyond the grid, the ghost row of a partial last tile and the cells beyond a row's ends read from the mapped
in-domain cell or taken as the side's constant.  With ``bc`` set, ``boundary=False`` of ``screen`` / ``screen_stats`` counts
``crop=(1, 0, 0)`` - the time rim only, as ``residual*(..., boundary=False)`` crops under ``bc`` - and ``boundary=True`` every
cell; ``add_slab`` keeps its explicit ``crop``; ``modulation`` keeps the uncropped extents.  Routes ``fused:bc_<kind>`` /
``fused:bc_stats_<kind>`` for the kinds ``stencil3d``, ``linear2``, ``ns_momentum``, ``mhd_<eq>``.  The three-pass route runs on
the bc residual (``_Spec.full`` calls the method with ``boundary=True``) for, in this order: ``minus=``, ``input on the CPU``,
float64 levels; ``no fused screen under bc for the 1-D family``; ``Nt-fastest view: the merged-row march has no BC form``; no
unit stride on Ny, a width that is no multiple of 4; ``fused=False``; what ``_BC.struct`` says of the condition (per-field
conditions, a mixed condition without a fused mapping); a kernel that requires grad or lies off the 7-point star; ``declined
by the library`` (the general stars of MHD momentum and energy).  A ``'free_slip'`` side - in the condition, or in any
member of a per-field list (``residuals._BC.free_slip``) - raises ``ValueError`` before any device work: the reference pads nothing there, so the residual under it has not the field's extents and neither a cell count
nor a modulation would fit it.  ``halo_x=True`` with ``bc`` raises ``ValueError``, as the residuals do; per-cell sets, ``pair=`` and the 1-D family
have no fused form under ``bc``.  Without the keyword an object with ``bc`` keeps ``fallback:bc= (...)`` and the library is never
loaded.

Sharding is by the batch axis: each rank screens its own samples, nothing is exchanged.

Host side: what a method is, what it reads and what declines a fused launch whatever the layout is resolved in
``_method.Method`` (shared with ``losses``); ``_Spec`` adds the kinds that have a fused screen, the order of the reasons of
``prepare`` / ``prepare_flat`` / ``prepare_rows`` and ONE launcher for all the libraries (``launch``, by ``form``, ``minus``
and ``cells``).
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _dispatch, _lib
from . import inductive_cp as icp
from . import residuals as R
from ._method import FLAT_MAX_NT, MHD_EQ, Method

_last_route = None


def last_route():
    """'fused:<kind>' or 'fallback:<why>' of the last ``screen`` / ``Screen.add_slab`` call."""
    return _last_route


# ------------------------------------------------------------------------------------------- the result
class Screened:
    """``score`` fp32 [n], ``inside`` int64 [nk, n], ``cells`` counted cells per sample (host int)."""

    def __init__(self, score, inside, cells):
        self.score, self.inside, self.cells = score, inside, int(cells)

    def accept(self):
        """bool [nk, n]: every counted cell of the sample inside the level's band (``filter_sims_joint`` per level)."""
        return self.inside == self.cells

    def _group_sum(self, t, group):
        if group is not None:
            torch.distributed.all_reduce(t, group=group)
        return t.cpu().numpy()

    def coverage_joint(self, group=None):
        """float64 [nk]: fraction of samples accepted (``emp_cov_joint`` per level: count / n in float64).  ``group``: the
        ranks that split the samples; one all-reduce of int64 [nk + 1]."""
        nk, n = self.inside.shape
        buf = torch.empty(nk + 1, dtype=torch.int64, device=self.inside.device)
        torch.sum(self.accept(), dim=1, out=buf[:nk])
        buf[nk] = n
        host = self._group_sum(buf, group)
        return np.array([float(c) / float(host[nk]) for c in host[:nk]], np.float64)

    def coverage_marginal(self, group=None):
        """float64 [nk]: fraction of all counted cells of all samples inside (``emp_cov`` per level, bounds +-q_k * m)."""
        nk, n = self.inside.shape
        buf = torch.empty(nk + 1, dtype=torch.int64, device=self.inside.device)
        torch.sum(self.inside, dim=1, out=buf[:nk])
        buf[nk] = n * self.cells
        host = self._group_sum(buf, group)
        return np.array([float(c) / float(host[nk]) for c in host[:nk]], np.float64)

    def within(self, threshold):
        """bool [nk, n]: at least ``threshold`` of the sample's counted cells inside, compared in float64
        (``filter_sims_within_bounds(..., within=True)``)."""
        return (self.inside.double() / float(self.cells)) >= threshold


# ------------------------------------------------------------------------------------------- what a method is
def _input_declined(x, minus, qhats, modulation, pair=False):
    """What keeps a call from every fused screen, whatever the method and the layout, or None.  ``pair``: the caller asked
    for the paired screens, which take ``minus``."""
    if minus is not None and not pair:
        return "minus="
    if not x.is_cuda or (minus is not None and not minus.is_cuda):
        return "input on the CPU"
    if qhats.dtype != torch.float32 or (modulation is not None and modulation.dtype != torch.float32):
        return "float64 levels or modulation"
    return None


# form of the fused screen -> (its loader in ``_lib``, the prefix of its entry points, the prefix of its route)
_FORMS = {"": ("load_screen", "pre_screen_", ""), "flat": ("load_screenflat", "pre_screenflat_", "flat_"),
          "rows": ("load_screen1d", "pre_screen1d_", "rows_")}
# the four MHD kinds share ONE entry point, pre_screen[flat]_mhd_f32: kind -> the ``eq`` it takes first
_MHD_EQ = {"mhd_" + e: i for i, e in enumerate(MHD_EQ)}
# the two JOREK kinds (opt-in) share the two entry points of a library of their own: kind -> ``eq``; form -> entry point
_JOREK_EQ = {"jorek_continuity": 0, "jorek_temperature": 1}
_JOREK_ENTRY = {"": "pre_screenjorek_f32", "flat": "pre_screenjorek_flat_f32"}
# the kinds with a paired screen (opt-in, ``pair=True`` with ``minus=``), a library of their own: form -> prefix of its entries
_PAIR_KINDS = ("stencil3d", "linear2", "ns_momentum", "mhd_continuity")
_PAIR_ENTRY = {"": "pre_screenpair_", "flat": "pre_screenpair_flat_"}
# the per-cell screens (``screen_cells`` / ``ScreenCells``), a library of their own: form -> prefix of its entries
_CELLS_ENTRY = {"": "pre_screencells_", "flat": "pre_screencells_flat_"}
# the paired screen of the 1-D family (opt-in, ``pair="rows"`` with ``minus=``), one more library: the prefix of its entries
_PAIR_ROWS_ENTRY = "pre_screen1dpair_"
# the per-cell screens of the 1-D family (opt-in, ``rows=True`` of ``screen_cells`` / ``ScreenCells``; with ``minus=`` its
# paired entries), one more library: the prefix of its entries
_CELLS_ROWS_ENTRY = "pre_screen1dcells_"
# the per-cell screens of the data-driven scores (opt-in, ``pair=True`` with ``minus=`` on ``screen_cells`` / ``ScreenCells``;
# the kinds of ``_PAIR_KINDS``), one more library: form -> prefix of its entries
_CELLS_PAIR_ENTRY = {"": "pre_screencellspair_", "flat": "pre_screencellspair_flat_"}
# the per-cell screens of the JOREK residuals (opt-in, ``jorek=True`` on ``screen_cells`` / ``ScreenCells``), one more library:
# form -> entry point
_JOREK_CELLS_ENTRY = {"": "pre_screenjorekcells_f32", "flat": "pre_screenjorekcells_flat_f32"}
# the per-sample statistics (``screen_stats`` / ``ScreenStats``), one more library for all three forms: the prefix of its
# entries, followed by the form's route prefix
_STATS_ENTRY = "pre_screenstats_"
# the screens and statistics under boundary conditions on the x-y rim (opt-in, ``bc=``), one more library, Ny-fastest views only
_BC_ENTRY = "pre_screenbc_"
_BC_HALO_X = "bc with halo_x=True: an x-slab with a wrapped x is not served under boundary conditions"


def _pair_mode(pair, minus):
    """``pair`` as the host side carries it: False without ``minus``, "rows" for ``pair="rows"`` (the paired screens and,
    for the 1-D family, the paired rows screen), else its truthiness."""
    if minus is None:
        return False
    return "rows" if isinstance(pair, str) and pair == "rows" else bool(pair)


class _Spec(Method):
    """One residual method, resolved (``_method.Method``) for the fused screens: ``kind`` (None: no fused screen of the
    2-D family), ``chan`` - the channels of a stacked ``[BS,F,...]`` input the residual reads (None: the input is the field
    itself), ``rows_kind`` - the fused screen of the 1-D family ('stencil2d', 'burgers'; None: none), which ``kind`` and
    ``why`` do not speak of; ``eq`` (the MHD and JOREK equations) and ``ratio`` (``linear2``) as the launches take them.
    ``jorek=True`` on a bound ``JOREK.residual_continuity`` / ``residual_temperature`` resolves the opt-in kinds
    ``jorek_continuity`` / ``jorek_temperature``: ``ops`` are the object's five operators, ``fields`` its ``unstack_fields``
    views; on anything else it is a ``TypeError``.  With it the method may also be ``functools.partial(<bound JOREK
    equation>, norms=<bool>)`` - the rule of ``losses``: no positional arguments, keywords within ``{"norms"}`` - and
    ``norms`` is what ``JOREK._coef`` folds into the scalars of the launch; ``method`` stays the partial, so the three-pass
    route evaluates the same form.  ``norms=True`` raises here what the equation itself would raise: without ``dx, dy, dt``
    its ``ValueError``, on the temperature equation the reference's exception.  Without ``jorek`` JOREK has no fused kind,
    as before."""
    KIND = {"op3d": "stencil3d", "wave": "stencil3d", "ns_momentum": "ns_momentum", "ns_continuity": "linear2",
            "mhd_gauss": "linear2", **{k: k for k in _MHD_EQ}}
    ROWS_KIND = {"op2d": "stencil2d", "advection": "stencil2d", "burgers": "burgers"}
    WHY = {"spectral": "spectral operator", "jorek": "no fused screen for JOREK",
           **dict.fromkeys(ROWS_KIND, "1-D family: the marched axis is the batch")}

    def __init__(self, method, jorek=False, bc=False):
        bound, self.norms = method, False
        if jorek and isinstance(method, functools.partial) and not method.args and set(method.keywords) <= {"norms"} and \
                isinstance(getattr(method.func, "__self__", None), R.JOREK):
            bound, self.norms = method.func, bool(method.keywords.get("norms", False))      # (the one keyword of the equations)
        super().__init__(bound)
        self.method = method
        if jorek:
            kind = "jorek_" + getattr(bound, "__name__", "")[len("residual_"):]
            if self.row != "jorek" or kind not in _JOREK_EQ:
                raise TypeError("jorek=True takes a bound JOREK.residual_continuity or JOREK.residual_temperature")
            self.kind, self.why, self.eq, self.ops = kind, None, _JOREK_EQ[kind], tuple(self.obj._ops())
            if self.norms and self.eq == 1:
                raise Exception("Norm not implemented yet")      # (as ``JOREK.residual_temperature`` and the reference)
            if self.norms and (self.obj.dx is None or self.obj.dy is None or self.obj.dt is None):
                raise ValueError("norms=True needs dx, dy, dt")  # (as ``JOREK.residual_continuity``)
        if self.kind == "linear2":
            self.ratio, = self.scalars()
        elif self.kind in _MHD_EQ:
            self.eq = _MHD_EQ[self.kind]
        # ``bc``: the opt-in screens of the residual under boundary conditions on the x-y rim.  None: not asked for (an
        # object with ``bc`` then keeps its three-pass route); else the ``residuals._BC`` the launches read, each time anew
        self.bc = None
        if bc is not False and bc is not None:
            if jorek or self.row in ("jorek", "jorek_any"):
                raise TypeError("bc= takes no JOREK method: its residuals have no boundary conditions on the x-y rim")
            if self.is_op:
                if bc is True or self.row == "spectral":
                    raise TypeError("bc=True takes a bound residual method of an object built with bc=; a bare ConvOperator "
                                    "takes the condition itself, bc=<condition> (residuals.apply_bc)")
                self.bc = R._BC(bc)
            else:
                if bc is not True:
                    raise TypeError("bc=<condition> takes a bare ConvOperator; a bound residual method takes bc=True and "
                                    "uses the condition of its object")
                if getattr(self.obj, "bc", None) is None:
                    raise TypeError(f"bc=True on a {type(self.obj).__name__} built without bc=")
                self.bc = self.obj.bc

    def fields(self, x):
        if self.kind in _JOREK_EQ:
            return R.JOREK.unstack_fields(x)[:2 + self.eq]
        return super().fields(x)

    def scalars(self):
        if self.kind in _JOREK_EQ:
            return (_lib.farr(self.obj._coef(self.eq, self.norms)),)   # (norms: a ``functools.partial``'s, else False)
        return super().scalars()

    def view(self, x):
        """What the layout of input ``x`` is decided on: ``x`` itself, or for JOREK's ``[BS,F,Nx,Ny,Nt]`` a field view."""
        return x[:, 0].permute(0, 3, 1, 2) if self.kind in _JOREK_EQ else x

    def reads_halo(self):
        """Does the method's own residual pass take ``halo_x``?  (A ``ConvOperator`` call, NS continuity and MHD gauss do
        not: their slabs would be evaluated against zero padding.)"""
        return not self.is_op and self.kind != "linear2" and isinstance(self.obj, (R.NavierStokes, R.MHD, R.PRE_Wave))

    def full(self, x, minus, halo_x):
        """The uncropped residual by the existing passes (what the fallback's first launch is)."""
        if halo_x and not self.reads_halo():
            raise RuntimeError("halo_x: only the fused screen reads the halo rows for this method, and it declined")
        if self.rows_kind is not None and x.dim() == 4:
            x, minus = x[:, 0], (minus[:, 0] if minus is not None else None)
        with torch.no_grad():
            kw = {} if minus is None else {"minus": minus}
            if halo_x:
                kw["halo_x"] = True
            if self.is_op:
                op = self.method if self.bc is None else (lambda f: R.apply_bc(self.method, f, self.bc))
                r = op(x)
                return r if minus is None else r - op(minus)
            return self.method(x, boundary=True, **kw)

    # -------- can a fused screen run?  input, then layout, then what declines whatever the layout, then the kernels
    def pair_declined(self, rows=False):
        """What keeps this method from the paired screens (``pair=True`` with ``minus=``) whatever the input, or None.
        ``rows``: the caller asked with ``pair="rows"``, which the 1-D family takes."""
        if self.rows_kind is not None:
            return None if rows else "no paired screen for the 1-D family"
        if self.kind is None:
            return self.why
        return None if self.kind in _PAIR_KINDS else "no paired screen for " + self.kind

    def _prepare(self, layout, kind, points, x, minus, qhats, modulation, pair=False):
        pair = _pair_mode(pair, minus)
        why = (self.pair_declined(pair == "rows") if pair else None) or _input_declined(x, minus, qhats, modulation, pair) or \
            layout(self.view(x))
        if why is None and pair:
            # the second set: in the other layout no march takes the two together; in the same one, its own reasons
            if self._other_layout(x, minus) if layout is self._layout_rows else self.nt_fastest(minus) != self.nt_fastest(x):
                why = "field sets in different layouts"
            else:
                why = layout(self.view(minus))
                why = why and "minus: " + why
        why = why or self.declined(x)
        if why is None and not pair and kind in _MHD_EQ and x.shape[1] < 6:
            why = "fewer than six MHD channels"                  # (pre_screen_mhd_f32 takes the six views)
        if why is None and kind in _JOREK_EQ and x.shape[1] != 3:
            why = "not three JOREK channels"                     # (the residual methods unstack exactly rho, phi, T)
        return (why, ()) if why is not None else self.star_kernels(kind, points)

    def declined(self, x, yy=None, kernel_trains=False):
        """``Method.declined``, under this spec's ``bc`` where one was asked for."""
        return super().declined(x, yy, kernel_trains, bc=self.bc)

    def prepare_bc(self, x, minus, qhats, modulation):
        """``prepare`` with ``bc`` asked for: (why, kernels), the reasons in the order of the module docstring."""
        # (before anything else, and before any device work: the reference pads nothing on a 'free_slip' side, so the residual
        # under it has not the field's extents - there is no rim to count, and no cell count or modulation that would fit)
        if self.bc.free_slip(self.nd):                           # (per-field conditions included)
            raise ValueError("bc= with a 'free_slip' side: it has no padding rule, the residual under it does not cover the "
                             "x-y plane and no screen of it is defined")
        why = _input_declined(x, minus, qhats, modulation)
        if why is None and (self.rows_kind is not None or self.nd == 2):
            why = "no fused screen under bc for the 1-D family"
        if why is None and self.nt_fastest(x):
            why = "Nt-fastest view: the merged-row march has no BC form"
        why = why or self._layout(self.view(x)) or self.declined(x)
        if why is None and self.kind in _MHD_EQ and x.shape[1] < 6:
            why = "fewer than six MHD channels"
        return (why, ()) if why is not None else self.star_kernels(self.kind, 7)

    def prepare(self, x, minus, qhats, modulation, pair=False):
        """(why, kernels): ``why`` is None if the fused screen can run; host checks and one download of the operator
        kernels (``_dispatch.host_kernel`` on every call: a screen applies the kernels its operators hold now).  ``pair``
        with a ``minus``: the same question of the paired screen, of both sets."""
        if self.bc is not None:
            return self.prepare_bc(x, minus, qhats, modulation)
        if self.kind is None:
            pair = _pair_mode(pair, minus)
            return (pair and self.pair_declined(pair == "rows")) or self.why, ()
        return self._prepare(self._layout, self.kind, 7, x, minus, qhats, modulation, pair)

    def prepare_flat(self, x, minus, qhats, modulation, pair=False):
        """``prepare`` for the fused screen of Nt-fastest views (``nt_fastest(x)``): (why, kernels)."""
        return self._prepare(self._layout_flat, self.kind, 7, x, minus, qhats, modulation, pair)

    def prepare_rows(self, x, minus, qhats, modulation, pair=False):
        """``prepare`` for the fused screen of the 1-D family (``rows_kind``): (why, kernels)."""
        return self._prepare(self._layout_rows, self.rows_kind, 5, x, minus, qhats, modulation, pair)

    @staticmethod
    def _layout(x):
        if x.stride(-1) != 1:
            return "no unit stride on the last axis"
        if x.shape[-1] % 4 != 0:
            return "row width not a multiple of 4"
        return None

    def nt_fastest(self, x):
        """Is ``x`` an Nt-fastest view of a 2-D residual's input (unit stride on Nt, not on Ny)?"""
        x = self.view(x)
        return self.kind is not None and x.dim() >= 4 and x.stride(-3) == 1 and x.stride(-1) != 1

    @staticmethod
    def _layout_flat(x):
        T, Y = x.shape[-3], x.shape[-1]
        if T >= FLAT_MAX_NT:
            return "Nt >= %d" % FLAT_MAX_NT                       # (the residual pass leaves its flat form there too)
        if (Y * T) % 4 != 0:
            return "merged row Ny*Nt not a multiple of 4"
        if Y <= 1 or x.stride(-1) != T:
            return "rows not dense"                               # (a t-slab of an Nt-fastest tensor)
        return None

    @staticmethod
    def _layout_rows(x):
        if x.dim() == 4:
            return "[BS,1,Nt,Nx] input"
        if x.stride(2) != 1 and x.stride(1) != 1:
            return "no unit-stride axis"
        if x.shape[2 if x.stride(2) == 1 else 1] % 4 != 0:
            return "contiguous-axis length not a multiple of 4"
        return None

    @staticmethod
    def _other_layout(x, minus):
        """Of two [BS,Nt,Nx] sets of the 1-D family, ``x`` past ``_layout_rows``: does ``minus`` have its unit stride on the
        other axis only?  (No unit-stride axis at all is a reason of its own, ``_layout_rows``'s.)"""
        ax = 2 if x.stride(2) == 1 else 1
        return minus.dim() == 3 and minus.stride(ax) != 1 and minus.stride(3 - ax) == 1

    # -------- the launches: one body, three forms ('': Ny-fastest views, 'flat': Nt-fastest views, 'rows': the 1-D family)
    def entry(self, form, pair=False, cells=False, stats=False):
        """The entry point of this method's fused screen in the library of ``form`` (``pair``: of its paired screen,
        ``cells``: of its per-cell screen; form 'rows' has both at once; ``stats``: of its per-sample statistics).  With
        ``bc`` asked for: of ``libcp_pre_screenbc.so``, form '' only."""
        if self.bc is not None:
            return _BC_ENTRY + ("stats_" if stats else "") + ("mhd" if self.kind in _MHD_EQ else self.kind) + "_f32"
        if stats:
            kind = self.rows_kind if form == "rows" else "mhd" if self.kind in _MHD_EQ else self.kind
            return _STATS_ENTRY + _FORMS[form][2] + kind + "_f32"
        if cells and form == "rows":
            return _CELLS_ROWS_ENTRY + ("pair_" if pair else "") + self.rows_kind + "_f32"
        if cells and pair:
            return _CELLS_PAIR_ENTRY[form] + self.kind + "_f32"
        if cells and self.kind in _JOREK_EQ:
            return _JOREK_CELLS_ENTRY[form]
        if cells:
            return _CELLS_ENTRY[form] + ("mhd" if self.kind in _MHD_EQ else self.kind) + "_f32"
        if pair:
            return _PAIR_ROWS_ENTRY + self.rows_kind + "_f32" if form == "rows" else _PAIR_ENTRY[form] + self.kind + "_f32"
        if self.kind in _JOREK_EQ and form != "rows":
            return _JOREK_ENTRY[form]
        kind = self.rows_kind if form == "rows" else "mhd" if self.kind in _MHD_EQ else self.kind
        return _FORMS[form][1] + kind + "_f32"

    def route(self, form, pair=False, cells=False, stats=False):
        if self.bc is not None:
            return "fused:bc_" + ("stats_" if stats else "") + self.kind
        if stats:
            return "fused:" + _FORMS[form][2] + "stats_" + (self.rows_kind if form == "rows" else self.kind)
        if cells and form == "rows":
            return "fused:rows_cells_" + ("pair_" if pair else "") + self.rows_kind
        if cells:
            return "fused:" + _FORMS[form][2] + "cells_" + ("pair_" if pair else "") + self.kind
        return "fused:" + _FORMS[form][2] + ("pair_" if pair else "") + (self.rows_kind if form == "rows" else self.kind)

    def launch(self, kernels, x, st, flags, form="", minus=None, cells=False, stats=False):
        """The fused launch of ``form`` on device views ``x`` ([BS,Nt,Nx] for 'rows'); returns the library's code.
        ``minus``: the paired screen of ``x`` and ``minus`` (``libcp_pre_screenpair.so`` for forms '' and 'flat',
        ``libcp_pre_screen1dpair.so`` for 'rows').  ``cells``: the per-cell screen (``libcp_pre_screencells.so`` for forms ''
        and 'flat', with ``minus`` ``libcp_pre_screencellspair.so``; ``libcp_pre_screen1dcells.so`` for 'rows', there with
        ``minus`` too, ``libcp_pre_screenjorekcells.so`` for the JOREK kinds; ``st`` is then its set descriptor).  ``stats``:
        the per-sample statistics (``libcp_pre_screenstats.so``, all three forms; ``st`` is its descriptor)."""
        assert form == "" or not flags & _lib.PRE_FLAG_HALO_X    # (only the Ny-fastest march reads halo rows)
        if minus is not None and form == "rows":
            sets = (_lib.ptr(x), _lib.iarr64(x.stride()), _lib.ptr(minus), _lib.iarr64(minus.stride()))
            if self.rows_kind.startswith("stencil"):
                kernels = _dispatch.tap_args(*kernels)
            fn = getattr(_lib.load_screen1dcells() if cells else _lib.load_screen1dpair(), self.entry(form, True, cells))
            return fn(*sets, *kernels, *self.scalars(), ctypes.byref(st), *x.shape, flags, _lib.stream())
        if minus is not None:
            fa, fb = self.fields(x), self.fields(minus)
            one = self.kind.startswith("stencil")                # (one view per set; else a pre_field_t[F] per set)
            views = [ctypes.byref(_lib.field(f[0])) if one else R._arr(f) for f in (fa, fb)]
            if one:
                kernels = _dispatch.tap_args(*kernels)
            # (the per-cell paired library by its row of ``_lib``'s loader table: loaded on this route only)
            fn = getattr(_lib._load("screencellspair") if cells else _lib.load_screenpair(), self.entry(form, True, cells))
            return fn(*views, *kernels, *self.scalars(), ctypes.byref(st), *fa[0].shape, flags, _lib.stream())
        kind = self.rows_kind if form == "rows" else self.kind
        tail = ()                                                # (what follows the set descriptor: under ``bc`` the conditions)
        if self.bc is not None:
            assert form == "" and not cells and not flags & _lib.PRE_FLAG_HALO_X
            lib = _lib.load_screenbc()                           # (loaded on this route only)
            tail = (ctypes.byref(self.bc.struct(3)[0]),)         # (``prepare_bc`` has found that the condition has one)
        elif stats:
            lib = _lib.load_screenstats()                        # (loaded on this route only)
        elif cells and form == "rows":
            lib = _lib.load_screen1dcells()
        elif cells and kind in _JOREK_EQ:
            lib = _lib.load_screenjorekcells()                   # (loaded on this route only)
        else:
            lib = _lib.load_screencells() if cells else getattr(_lib, "load_screenjorek" if kind in _JOREK_EQ else _FORMS[form][0])()
        if form == "rows":
            views, shape = (_lib.ptr(x), _lib.iarr64(x.stride())), x.shape
        else:
            fs = self.fields(x)
            shape = fs[0].shape
            if kind in _MHD_EQ:
                views = (self.eq, R._arr([x[:, i] for i in range(6)]))
            elif kind in _JOREK_EQ:
                Rb = self.obj._R_view(fs[0])                     # (raises before any launch if len(R) is not Ny)
                if Rb is None:
                    return _lib.PRE_E_UNSUPPORTED
                views = (self.eq, R._arr([fs[i] if i < len(fs) else fs[0] for i in range(3)]), ctypes.byref(_lib.field(Rb)))
            else:
                views = [ctypes.byref(_lib.field(f)) for f in fs]
        if kind.startswith("stencil"):
            kernels = _dispatch.tap_args(*kernels)
        return getattr(lib, self.entry(form, cells=cells, stats=stats))(*views, *kernels, *self.scalars(), ctypes.byref(st),
                                                                        *tail, *shape, flags, _lib.stream())

    def launch_flat(self, kernels, x, st, flags):
        return self.launch(kernels, x, st, flags, "flat")

    def launch_rows(self, kernels, x, st, flags):
        return self.launch(kernels, x, st, flags, "rows")


# ------------------------------------------------------------------------------------------- validation (host only)
def _check_inputs(spec, vars, qhats, modulation, minus, crop, nk=None):
    """Every shape, dtype and device error, raised before any device work.  Returns the residual's uncropped shape."""
    if not isinstance(vars, torch.Tensor):
        raise TypeError("vars must be a torch.Tensor")
    if vars.dtype != torch.float32:
        raise TypeError(f"vars has dtype {vars.dtype}: the screen takes float32 fields")
    shape = spec.field_shape(vars)
    if vars.numel() == 0:
        raise ValueError("screen of an empty batch")
    if not isinstance(qhats, torch.Tensor):
        raise TypeError("qhats must be a torch.Tensor [nk]")
    if qhats.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"qhats has dtype {qhats.dtype}: float32 levels (float64 ones take the fallback)")
    if qhats.dim() != 1 or not 1 <= qhats.shape[0] <= _lib.PRE_SCREEN_MAX_LEVELS:
        raise ValueError(f"qhats has shape {tuple(qhats.shape)}, expected [nk] with 1 <= nk <= {_lib.PRE_SCREEN_MAX_LEVELS}")
    if nk is not None and qhats.shape[0] != nk:
        raise ValueError(f"qhats has shape {tuple(qhats.shape)}, expected ({nk},)")
    if qhats.device != vars.device:
        raise ValueError(f"qhats is on {qhats.device}, vars on {vars.device}")
    if modulation is not None:
        if not isinstance(modulation, torch.Tensor):
            raise TypeError("modulation must be a torch.Tensor or None")
        if modulation.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"modulation has dtype {modulation.dtype}")
        if tuple(modulation.shape) != tuple(shape[1:]):
            raise ValueError(f"modulation has shape {tuple(modulation.shape)}, expected {tuple(shape[1:])}: the uncropped "
                             "extents of the residual")
        if modulation.device != vars.device:
            raise ValueError(f"modulation is on {modulation.device}, vars on {vars.device}")
    if minus is not None:
        R._check_minus(vars, minus)
    crop = tuple(int(c) for c in crop)
    if len(crop) != len(shape) - 1 or any(c < 0 for c in crop):
        raise ValueError(f"crop {crop}: one non-negative count per residual axis")
    if any(n - 2 * c <= 0 for n, c in zip(shape[1:], crop)):
        raise ValueError(f"crop {crop} leaves no cell of a {tuple(shape[1:])} residual")
    cells = 1
    for n, c in zip(shape[1:], crop):
        cells *= n - 2 * c
    if cells >= 1 << 32:
        raise ValueError("cells per sample >= 2^32: screen the grid in slabs")
    return shape, crop, cells


def _dev_key(d):
    d = torch.device(d)
    return d.type, (d.index or 0)


class Screen:
    """Accumulating screen of ``n_local`` samples at ``nk`` levels: ``add_slab`` once per slab of the grid (x-slabs with
    ``halo_x``, t-slabs with their halo planes, as ``JointCalibration.add_slab`` takes them), ``finish`` -> ``Screened``.
    Maximum and integer adds compose exactly: the slabs of a grid give the bits of the whole grid."""

    def __init__(self, n_local, nk, device):
        if n_local < 1 or not 1 <= nk <= _lib.PRE_SCREEN_MAX_LEVELS:
            raise ValueError(f"Screen needs n_local >= 1 and 1 <= nk <= {_lib.PRE_SCREEN_MAX_LEVELS} (got {n_local}, {nk})")
        self.n_local, self.nk, self.device = int(n_local), int(nk), torch.device(device)
        self.acc = None                # int32 [nk + 1, n_local]: row 0 the score's bits, rows 1.. the counts; made at the first slab
        self.cells = 0

    def _buffers(self, device):
        if self.acc is None:
            self.acc = torch.zeros(self.nk + 1, self.n_local, dtype=torch.int32, device=device)
        return self.acc

    def add_slab(self, method, vars_slab, qhats, modulation_slab=None, crop=(1, 1, 1), halo_x=False, minus=None, jorek=False,
                 pair=False, bc=False):
        """``vars_slab``: the method's input on a slab of the grid (all local samples); ``modulation_slab`` [T,X,Y] of the
        slab's uncropped residual extents, or None (m == 1); ``crop`` cells per side of each residual axis are left out
        (``JointCalibration.add_slab``'s meaning); ``halo_x``: the slab's rows -1 and X lie in the same memory; ``jorek``: the
        opt-in fused screen of the JOREK residuals (``_Spec``; a method given as a ``_Spec`` has decided already); ``pair``:
        the opt-in paired screen of ``vars_slab`` and ``minus`` (no effect without ``minus``; under ``halo_x`` both sets
        must be Ny-contiguous device views with rows -1 and X in memory); ``pair="rows"``: the same, and the paired rows
        screen for the 1-D family (module docstring); ``bc``: the opt-in screen of the residual under boundary conditions
        on the x-y rim (module docstring; ``crop`` stays the caller's: ``(ct, 0, 0)`` counts the whole plane)."""
        global _last_route
        spec = method if isinstance(method, _Spec) else _Spec(method, jorek, bc)
        if spec.bc is not None and halo_x:
            raise ValueError(_BC_HALO_X)
        pair = _pair_mode(pair, minus)
        shape, crop, cells = _check_inputs(spec, vars_slab, qhats, modulation_slab, minus, crop, self.nk)
        if shape[0] != self.n_local:
            raise ValueError(f"slab of {shape[0]} samples, expected n_local = {self.n_local}")
        if _dev_key(vars_slab.device) != _dev_key(self.device):
            raise ValueError(f"slab on {vars_slab.device}, this Screen was made for {self.device}")
        if halo_x and pair and vars_slab.is_cuda:
            R._check_minus(vars_slab, minus, device_view=True)
        why, kernels = spec.prepare(vars_slab, minus, qhats, modulation_slab, pair)
        if halo_x and spec.kind in _JOREK_EQ:
            why = why or "halo_x"                                 # (no pass of the JOREK residuals reads halo rows: raises below)
        if halo_x and not vars_slab.is_cuda:
            raise ValueError("halo_x needs a device-resident view of a larger grid (a staged copy has no halo rows)")
        if halo_x and why is not None and not spec.reads_halo():
            # (before any device work: this slab would be evaluated against zero padding and counted as if it were right)
            raise RuntimeError(f"halo_x: the fused screen cannot run ({why}) and no other pass of this method reads the halo rows")
        rows = spec.rows_kind is not None and spec.bc is None     # (the 1-D family: halo_x has raised above)
        if rows:
            why, kernels = spec.prepare_rows(vars_slab, minus, qhats, modulation_slab, pair)
        # Nt-fastest views of the 2-D residuals: the flat route (halo_x keeps the behaviour it had: the flat form pads x)
        flat = not rows and spec.bc is None and not halo_x and vars_slab.is_cuda and spec.nt_fastest(vars_slab)
        if flat:
            why, kernels = spec.prepare_flat(vars_slab, minus, qhats, modulation_slab, pair)
        if why is None:
            acc = self._buffers(vars_slab.device)
            mod = modulation_slab
            if rows:
                nt_fast = vars_slab.stride(2) != 1            # the modulation's unit-stride axis must be the field's
                if mod is not None and mod.stride(0 if nt_fast else 1) != 1:
                    mod = mod.t().contiguous().t() if nt_fast else mod.contiguous()
            elif flat:
                if mod is not None and (mod.stride(0) != 1 or mod.stride(2) != mod.shape[0]):
                    mod = mod.permute(1, 2, 0).contiguous().permute(2, 0, 1)       # (one sample-sized copy, memory [X,Y,T])
            elif mod is not None and mod.stride(-1) != 1:
                mod = mod.contiguous()
            q = qhats.contiguous()
            if flat:
                st = _lib.PreScreenFlat(_lib.ptr(q), self.nk, _lib.ptr(mod), *(mod.stride() if mod is not None else (0, 0, 0)),
                                        crop[0], crop[1], crop[2], ctypes.c_void_p(acc[0].data_ptr()),
                                        ctypes.c_void_p(acc[1].data_ptr()), acc.stride(0))
            else:
                st = _lib.PreScreen(_lib.ptr(q), self.nk, _lib.ptr(mod), mod.stride(0) if mod is not None else 0,
                                    mod.stride(1) if mod is not None else 0, crop[0], crop[1], 0 if rows else crop[2],
                                    ctypes.c_void_p(acc[0].data_ptr()), ctypes.c_void_p(acc[1].data_ptr()), acc.stride(0))
            form = "rows" if rows else "flat" if flat else ""
            with torch.no_grad(), torch.cuda.device(vars_slab.device):
                rc = spec.launch(kernels, vars_slab, st, _lib.PRE_FLAG_HALO_X if halo_x and form == "" else 0, form,
                                 minus if pair else None)
            if rc == _lib.PRE_E_UNSUPPORTED:
                why = "declined by the library"
                if halo_x and not spec.reads_halo():
                    raise RuntimeError("halo_x: the library declined and no other pass of this method reads the halo rows")
            else:
                _lib.check(rc, spec.entry(form, bool(pair)))
                _last_route = spec.route(form, bool(pair))
                self.cells += cells
                return
        _last_route = "fallback:" + why
        self._fallback(spec, vars_slab, qhats, modulation_slab, crop, halo_x, minus)
        self.cells += cells

    def _fallback(self, spec, vars, qhats, modulation, crop, halo_x, minus):
        """(``qhats``: [nk], or for ``ScreenCells`` the level fields [nk, *uncropped residual extents].)
        What a user writes today: the residual by the existing pass with ``boundary=True``, ``ncf_metric_joint`` over
        the cropped interior, ``CoverageLevels`` for the counts.  ``CoverageLevels`` counts over all the samples it is
        given, so the per-sample counts take one pass PER SAMPLE (n launches over a sample each; together they read the
        residual once): this route is for correctness where the fused launch cannot run, not for speed."""
        from . import pipeline
        res = spec.full(vars, minus, halo_x)
        res, _ = _dispatch.to_device(res)
        acc = self._buffers(res.device)
        wide = qhats.dtype == torch.float64 or (modulation is not None and modulation.dtype == torch.float64)
        q = qhats.to(res.device)
        mod = modulation.to(res.device) if modulation is not None else None
        sl = (slice(None),) + tuple(slice(c, n - c) for c, n in zip(crop, res.shape[1:]))
        if wide:
            # numpy would compute the score and the bounds in float64: so does this route (torch, on the device)
            r64 = res[sl].double().abs()
            m64 = mod[sl[1:]].double() if mod is not None else None
            s = (r64 / m64 if m64 is not None else r64).reshape(res.shape[0], -1)
            score = s.max(dim=1).values
            score = torch.where(torch.isnan(s).any(dim=1), torch.full_like(score, float("nan")), score).float()
            hw = q[(slice(None),) + sl[1:]].double() if q.dim() > 1 else q.double().reshape(-1, *([1] * (res.dim() - 1)))
            hw = hw * m64 if m64 is not None else hw
            counts = torch.stack([(r64 <= hw[k]).reshape(res.shape[0], -1).sum(dim=1) for k in range(self.nk)])
        else:
            ones = mod if mod is not None else torch.ones(res.shape[1:], dtype=torch.float32, device=res.device)
            if len(set(crop)) == 1 and res.dim() == 4:
                score = icp.ncf_metric_joint(res, None, ones, crop=crop[0])
            else:
                score = icp.ncf_metric_joint(res[sl].contiguous(), None, ones[sl[1:]].contiguous())
            # the counts per sample: a CoverageLevels pass per sample (its marginal count is a total over its samples)
            rows, mrows = res[sl], (mod[sl[1:]] if mod is not None else None)
            if q.dim() > 1:                                  # (per-cell levels, ``ScreenCells``: the counted cells' ones)
                q = q[(slice(None),) + sl[1:]]
            counts = torch.empty(self.nk, res.shape[0], dtype=torch.int64, device=res.device)
            cov = pipeline.CoverageLevels(1, self.nk, res.device)
            for i in range(res.shape[0]):
                cov.acc.zero_()
                cov.add_slab(rows[i:i + 1], q, modulation=mrows)
                counts[:, i] = cov.acc
        bits = score.contiguous().view(torch.int32)
        # unsigned maximum of the bit patterns (non-negative scores: the patterns are non-negative int32 too)
        torch.maximum(acc[0], bits, out=acc[0])
        acc[1:] += counts.to(torch.int32)

    def finish(self):
        if self.acc is None or self.cells == 0:
            raise ValueError("Screen.finish() before any slab")
        return Screened(self.acc[0].view(torch.float32).clone(), self.acc[1:].to(torch.int64) & 0xffffffff, self.cells)


def _whole_crop(spec, boundary):
    """The crop of ``screen`` / ``screen_stats``: nothing with ``boundary=True``; else one cell per side of every residual
    axis - with ``bc`` asked for of the time axis only, as ``residual*(..., boundary=False)`` crops under ``bc``."""
    if boundary:
        return (0,) * spec.nd
    return (1,) + (0,) * (spec.nd - 1) if spec.bc is not None else (1,) * spec.nd


def screen(residual_method, vars, qhats, modulation=None, boundary=False, minus=None, jorek=False, pair=False, bc=False):
    """Screen the predictions ``vars`` against the sets ``|r| <= qhats[k] * modulation``.  ``boundary=False``: the counted
    cells are the interior ``[1:-1]`` of every residual axis, as the reference crops its residuals (``modulation`` keeps
    the uncropped extents: its rim is never used); ``boundary=True``: every cell.  ``jorek=True``: the opt-in fused screen
    of ``JOREK.residual_continuity`` / ``residual_temperature`` (``vars`` [BS,F,Nx,Ny,Nt], ``modulation`` [Nt,Nx,Ny]; the
    equations with ``norms=False``).  ``minus``: the data-driven score, ``d = r(vars) - r(minus)`` in place of the residual;
    ``pair=True`` with it: the opt-in paired screen (one launch over both sets; module docstring), ``pair="rows"``: the
    same, and for the 1-D family its paired rows screen; without ``minus`` the keyword has no effect.  ``bc``: the opt-in
    screen of the residual under boundary conditions on the x-y rim (``True`` on a method of an object built with ``bc=``,
    the condition itself on a bare ``ConvOperator``); ``boundary=False`` then crops the time rim only.  Returns a
    :class:`Screened`."""
    spec = _Spec(residual_method, jorek, bc)
    crop = _whole_crop(spec, boundary)
    shape, _, _ = _check_inputs(spec, vars, qhats, modulation, minus, crop)
    s = Screen(shape[0], qhats.shape[0], vars.device)
    s.add_slab(spec, vars, qhats, modulation, crop=crop, minus=minus, pair=pair)
    out = s.finish()
    if not vars.is_cuda:                                     # (staged inputs: the verdicts come home, as elsewhere)
        out.score, out.inside = out.score.to(vars.device), out.inside.to(vars.device)
    return out


# ------------------------------------------------------------------------------------------- per-cell sets
def sample_group():
    """Samples per group in the block order of the per-cell screens (``pre_screencells_sample_group``): speed only."""
    return int(_lib.load_screencells().pre_screencells_sample_group())


def sample_group_rows():
    """Samples per group in the block order of the per-cell screens of the 1-D family
    (``pre_screen1dcells_sample_group``): speed only."""
    return int(_lib.load_screen1dcells().pre_screen1dcells_sample_group())


def sample_group_pair():
    """Samples per group in the block order of the per-cell screens of the data-driven scores
    (``pre_screencellspair_sample_group``): speed only."""
    return int(_lib._load("screencellspair").pre_screencellspair_sample_group())


def sample_group_jorek():
    """Samples per group in the block order of the per-cell screens of the JOREK residuals
    (``pre_screenjorekcells_sample_group``): speed only."""
    return int(_lib.load_screenjorekcells().pre_screenjorekcells_sample_group())


def _check_cells(spec, vars, qcells, modulation, minus, crop, nk=None):
    """``_check_inputs`` for level fields: every error before any device work.  Returns (uncropped residual shape, crop,
    counted cells per sample); ``qcells`` has the uncropped extents or (``cropped`` in the caller) the cropped ones."""
    if not isinstance(qcells, torch.Tensor):
        raise TypeError("qcells must be a torch.Tensor [nk, *residual extents]")
    if qcells.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"qcells has dtype {qcells.dtype}: float32 levels (float64 ones take the fallback)")
    if qcells.dim() < 2 or not 1 <= qcells.shape[0] <= _lib.PRE_SCREEN_MAX_LEVELS or qcells.numel() == 0:
        raise ValueError(f"qcells has shape {tuple(qcells.shape)}, expected [nk, *residual extents] with 1 <= nk <= "
                         f"{_lib.PRE_SCREEN_MAX_LEVELS}")
    # (the checks of vars, modulation, minus and crop, with one level value per k standing in for the [nk] levels)
    return _check_inputs(spec, vars, qcells[(slice(None),) + (0,) * (qcells.dim() - 1)], modulation, minus, crop, nk)


class ScreenCells(Screen):
    """``Screen`` against per-cell sets: ``add_slab`` takes the level fields of the slab in place of the nk levels.
    Accumulation, ``crop``, ``halo_x`` and ``finish`` are ``Screen``'s: slabs compose to the bits of the whole grid."""

    def add_slab(self, method, vars_slab, qcells_slab, modulation_slab=None, crop=(1, 1, 1), halo_x=False, minus=None,
                 jorek=False, rows=False, pair=False):
        """``qcells_slab``: fp32 [nk, *uncropped residual extents of the slab] on the slab's device, shared by all samples
        (its values outside the counted region are never used); the other arguments as ``Screen.add_slab`` takes them.
        Level fields whose unit-stride axis is not the fields' are copied once into the matching layout, as the
        modulation is.  ``minus`` keeps the three-pass route (``fallback:minus=``) unless ``pair=True``: the opt-in per-cell
        screen of the data-driven score ``r(vars_slab) - r(minus)`` for the 2-D kinds with a paired screen (no effect
        without ``minus``; under ``halo_x`` both sets must be Ny-contiguous device views with rows -1 and X in memory;
        module docstring).  ``rows=True``: the opt-in per-cell screen of the 1-D family (``crop`` of two axes; with
        ``minus`` its paired entries; module docstring); no effect on any other method.  ``jorek=True``: the opt-in per-cell
        screen of the JOREK residuals (``_Spec``; a method given as a ``_Spec`` has decided already): ``vars_slab``
        [BS,3,Nx,Ny,Nt], ``qcells_slab`` [nk,Nt,Nx,Ny]; ``halo_x`` raises and ``minus`` keeps the three-pass route."""
        global _last_route
        spec = method if isinstance(method, _Spec) else _Spec(method, jorek)
        if spec.bc is not None:
            raise TypeError("per-cell sets have no screen under bc: a _Spec made with bc= goes to Screen / ScreenStats")
        rows = bool(rows) and spec.rows_kind is not None
        # (the paired entries of the rows form take ``minus``; the 2-D kinds take it where the caller asks with ``pair=True``)
        pair = "rows" if rows and minus is not None else spec.rows_kind is None and minus is not None and bool(pair)
        shape, crop, cells = _check_cells(spec, vars_slab, qcells_slab, modulation_slab, minus, crop, self.nk)
        if tuple(qcells_slab.shape[1:]) != tuple(shape[1:]):
            raise ValueError(f"qcells has shape {tuple(qcells_slab.shape)}, expected {(self.nk,) + tuple(shape[1:])}: the "
                             "uncropped extents of the residual")
        if shape[0] != self.n_local:
            raise ValueError(f"slab of {shape[0]} samples, expected n_local = {self.n_local}")
        if _dev_key(vars_slab.device) != _dev_key(self.device):
            raise ValueError(f"slab on {vars_slab.device}, this Screen was made for {self.device}")
        if halo_x and pair is True and vars_slab.is_cuda:
            R._check_minus(vars_slab, minus, device_view=True)
        why, kernels = spec.prepare(vars_slab, minus, qcells_slab, modulation_slab, pair is True)
        if spec.kind in _JOREK_EQ and minus is not None:
            why = "minus="                                        # (two temperature sets are 8 views against the march's 6)
        if halo_x and spec.kind in _JOREK_EQ:
            why = why or "halo_x"                                 # (no pass of the JOREK residuals reads halo rows: raises below)
        if halo_x and not vars_slab.is_cuda:
            raise ValueError("halo_x needs a device-resident view of a larger grid (a staged copy has no halo rows)")
        if halo_x and why is not None and not spec.reads_halo():
            raise RuntimeError(f"halo_x: the fused screen cannot run ({why}) and no other pass of this method reads the halo rows")
        if rows:                                              # (the 1-D family: halo_x has raised above)
            why, kernels = spec.prepare_rows(vars_slab, minus, qcells_slab, modulation_slab, pair)
        flat = spec.kind is not None and not halo_x and vars_slab.is_cuda and spec.nt_fastest(vars_slab)
        if flat:
            why, kernels = spec.prepare_flat(vars_slab, minus, qcells_slab, modulation_slab, pair is True)
            if spec.kind in _JOREK_EQ and minus is not None:
                why = "minus="
        if why is None:
            acc = self._buffers(vars_slab.device)
            mod, lev = modulation_slab, qcells_slab
            if rows:
                nt_fast = vars_slab.stride(2) != 1            # the unit-stride axis of modulation and levels must be the field's
                if mod is not None and mod.stride(0 if nt_fast else 1) != 1:
                    mod = mod.t().contiguous().t() if nt_fast else mod.contiguous()
                if lev.stride(1 if nt_fast else 2) != 1:      # (nk of them, memory [nk,Nx,Nt] for Nt-fastest fields)
                    lev = lev.transpose(1, 2).contiguous().transpose(1, 2) if nt_fast else lev.contiguous()
                st = _lib.PreScreen1dCells(_lib.ptr(lev), self.nk, *lev.stride(), _lib.ptr(mod),
                                           *(mod.stride() if mod is not None else (0, 0)), crop[0], crop[1],
                                           ctypes.c_void_p(acc[0].data_ptr()), ctypes.c_void_p(acc[1].data_ptr()), acc.stride(0))
            elif flat:
                if mod is not None and (mod.stride(0) != 1 or mod.stride(2) != mod.shape[0]):
                    mod = mod.permute(1, 2, 0).contiguous().permute(2, 0, 1)       # (one sample-sized copy, memory [X,Y,T])
                if lev.stride(1) != 1 or lev.stride(3) != lev.shape[1]:
                    lev = lev.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # (nk of them, memory [nk,X,Y,T])
                st = _lib.PreScreenCellsFlat(_lib.ptr(lev), self.nk, *lev.stride(), _lib.ptr(mod),
                                             *(mod.stride() if mod is not None else (0, 0, 0)), crop[0], crop[1], crop[2],
                                             ctypes.c_void_p(acc[0].data_ptr()), ctypes.c_void_p(acc[1].data_ptr()), acc.stride(0))
            else:
                if mod is not None and mod.stride(-1) != 1:
                    mod = mod.contiguous()
                if lev.stride(-1) != 1:
                    lev = lev.contiguous()
                st = _lib.PreScreenCells(_lib.ptr(lev), self.nk, *lev.stride()[:3], _lib.ptr(mod),
                                         mod.stride(0) if mod is not None else 0, mod.stride(1) if mod is not None else 0,
                                         crop[0], crop[1], crop[2], ctypes.c_void_p(acc[0].data_ptr()),
                                         ctypes.c_void_p(acc[1].data_ptr()), acc.stride(0))
            form = "rows" if rows else "flat" if flat else ""
            with torch.no_grad(), torch.cuda.device(vars_slab.device):
                rc = spec.launch(kernels, vars_slab, st, _lib.PRE_FLAG_HALO_X if halo_x else 0, form,
                                 minus if pair else None, cells=True)
            if rc == _lib.PRE_E_UNSUPPORTED:
                why = "declined by the library"
                if halo_x and not spec.reads_halo():
                    raise RuntimeError("halo_x: the library declined and no other pass of this method reads the halo rows")
            else:
                _lib.check(rc, spec.entry(form, bool(pair), cells=True))
                _last_route = spec.route(form, bool(pair), cells=True)
                self.cells += cells
                return
        _last_route = "fallback:" + why
        self._fallback(spec, vars_slab, qcells_slab, modulation_slab, crop, halo_x, minus)
        self.cells += cells


def screen_cells(residual_method, vars, qcells, modulation=None, boundary=False, minus=None, jorek=False, rows=False,
                 pair=False):
    """Screen the predictions ``vars`` against the per-cell sets ``|r| <= qcells[k][cell]`` (``* modulation[cell]`` with a
    modulation) at every level k in one launch; the residual is never stored.  ``qcells``: fp32 ``[nk, *uncropped residual
    extents]`` on ``vars``' device, 1 <= nk <= 16.  ``boundary=False``: the counted cells are the interior ``[1:-1]`` of
    every residual axis, and ``qcells`` may instead have the CROPPED extents - what ``calibrate_multi`` returns for scores
    taken from ``res[..., 1:-1, 1:-1, 1:-1]``; it is then padded once with NaN to the uncropped extents (one copy of nk
    sample-sized fields, in the fields' layout).  ``boundary=True``: every cell, uncropped extents only.  Inside the counted
    region a NaN level or a NaN residual puts the cell outside at that level, a negative level puts it outside, ``+inf``
    puts it inside for every non-NaN residual.  ``minus`` (the data-driven score) keeps the three-pass route unless
    ``pair=True``: the opt-in per-cell screen of ``d = fl(fl(r(vars)) - fl(r(minus)))`` in one launch over both sets, for the
    kinds with a paired screen (routes ``fused:cells_pair_<kind>`` / ``fused:flat_cells_pair_<kind>``): ``score = max |d| /
    m``, ``inside[k] = #{|d| <= fl(qcells[k][cell] * m[cell])}`` - the one-sided test on the difference, NOT the reference's
    two-sided form ``fl(pred - q) <= y <= fl(pred + q)`` on the two residual arrays; the two can differ in a cell within
    rounding of the band's edge.  A caller who needs only the coverage totals keeps ``emp_cov_levels`` on the stored
    difference (below).  Without ``minus`` the keyword has no effect.
    ``rows=True``: the opt-in per-cell screen of the 1-D family (``vars`` [BS,Nt,Nx] in either layout, ``qcells``
    [nk,Nt,Nx] or the cropped [nk,Nt-2,Nx-2]; routes ``fused:rows_cells_<kind>``); ``minus`` with it takes the paired
    entries, the one-sided test ``|r(vars) - r(minus)| <= qcells[k][cell] (* m)`` (``fused:rows_cells_pair_<kind>``).
    Without it the 1-D family keeps the three-pass route; on any other method it has no effect.  Returns a
    :class:`Screened`: ``inside``, ``accept()``, ``coverage_marginal(group=)``, ``within()`` and ``score`` as for
    ``screen``; the samples may be sharded by the batch axis with nothing exchanged.

    Measured (nk = 10): this launch is SLOWER than the residual pass followed by ONE ``CoverageLevels`` pass
    with per-cell levels (``emp_cov_levels``) - 3.8 against 2.6 ms for the wave residual on [512,32,256,256], 69 against 34 ms
    for NS momentum on Nt-fastest [512,3,64,512,512].  That route gives the totals of the coverage curve only; who needs
    nothing else should keep it.  This one gives per-sample counts - ``accept``, ``within``, the score - stores no residual,
    takes slabs, and is 4-6 times faster than ten calls of the one-level trick, the other way to the same answer.
    The same holds for ``rows=True`` (Burgers on [8192,200,512], nk = 10): SLOWER than that route - 2.56
    against 2.06 ms Nx-fastest, 3.34 against 2.25 ms Nt-fastest, 4.63 against 3.07 ms for a pair - and 4.4-4.9 times faster
    than ten one-level calls of the joint rows screen.  And for ``minus=`` with ``pair=True`` (nk = 10): SLOWER
    than the paired residual pass followed by one ``CoverageLevels`` pass - 90.7 against 61.4 ms for NS momentum on two
    Nt-fastest [512,3,64,512,512] sets, 4.4 against 3.3 ms for the wave residual on two [512,32,256,256] sets - and 5.3-6.7
    times faster than ten one-level calls of the paired joint screen.
    ``jorek=True``: the opt-in per-cell screen of ``JOREK.residual_continuity`` / ``residual_temperature`` (or the ``norms``
    partial of either; ``vars`` [BS,3,Nx,Ny,Nt], ``qcells`` [nk,Nt,Nx,Ny] or the cropped [nk,Nt-2,Nx-2,Ny-2], ``modulation``
    [Nt,Nx,Ny]; routes ``fused:flat_cells_jorek_<eq>`` / ``fused:cells_jorek_<eq>``; ``minus=`` keeps ``fallback:minus=``); on
    any other method a ``TypeError``.  Measured ([96,3,256,256,40] dense, nk = 10): SLOWER than
    ``pre_residual_jorek_f32`` followed by one ``CoverageLevels`` pass - 1.57 against 1.27 ms for the temperature equation,
    1.45 against 1.09 ms for the continuity equation - and 6.6-6.7 times faster than ten one-level calls of ``screen(...,
    jorek=True)``; the library takes the level quads in batches of 4, 26-28 % faster than all 16 held across the functor."""
    spec = _Spec(residual_method, jorek)
    crop = (0,) * spec.nd if boundary else (1,) * spec.nd
    shape, _, _ = _check_cells(spec, vars, qcells, modulation, minus, crop)
    full, cropped = tuple(shape[1:]), tuple(n - 2 * c for n, c in zip(shape[1:], crop))
    if tuple(qcells.shape[1:]) != full:
        if boundary or tuple(qcells.shape[1:]) != cropped:
            raise ValueError(f"qcells has shape {tuple(qcells.shape)}, expected [nk, *{full}]" +
                             ("" if boundary else f" or the cropped [nk, *{cropped}]"))
        rows_nt = bool(rows) and spec.rows_kind is not None and vars.dim() == 3 and vars.stride(2) != 1 and vars.stride(1) == 1
        qcells = _pad_levels(qcells, full, vars.is_cuda and (rows_nt or spec.nt_fastest(vars)))
    s = ScreenCells(shape[0], qcells.shape[0], vars.device)
    s.add_slab(spec, vars, qcells, modulation, crop=crop, minus=minus, rows=rows, pair=pair)
    out = s.finish()
    if not vars.is_cuda:                                     # (staged inputs: the verdicts come home, as elsewhere)
        out.score, out.inside = out.score.to(vars.device), out.inside.to(vars.device)
    return out


def _pad_levels(qcells, full, nt_fastest):
    """Cropped level fields [nk, *cropped] inside NaN fields of the uncropped extents ``full`` (a NaN level is outside:
    the rim is never counted anyway); ``nt_fastest``: memory [nk,X,Y,T], the layout of an Nt-fastest view's fields (for the
    1-D family's [Nt,Nx] extents: memory [nk,Nx,Nt])."""
    nk = qcells.shape[0]
    if nt_fastest and len(full) == 2:
        out = torch.full((nk, full[1], full[0]), float("nan"), dtype=qcells.dtype, device=qcells.device).transpose(1, 2)
    elif nt_fastest and len(full) == 3:
        out = torch.full((nk, full[1], full[2], full[0]), float("nan"), dtype=qcells.dtype, device=qcells.device).permute(0, 3, 1, 2)
    else:
        out = torch.full((nk,) + tuple(full), float("nan"), dtype=qcells.dtype, device=qcells.device)
    out[(slice(None),) + (slice(1, -1),) * len(full)] = qcells
    return out


# ------------------------------------------------------------------------------------------- per-sample statistics
_STATS = ("mean", "mean_abs", "mean_sq", "rms", "max_abs", "sum", "sum_abs", "sum_sq")


class SampleStats:
    """Per-sample statistics of a residual over its counted cells: ``sum`` = sum r, ``sum_abs`` = sum |r|, ``sum_sq`` =
    sum r^2 (float64 [n]), ``max_abs`` = max |r| (float32 [n], NaN sticky), ``cells`` counted cells per sample (host int).
    All tensors are on the device of the input."""

    def __init__(self, sum, sum_abs, sum_sq, max_abs, cells):
        self.sum, self.sum_abs, self.sum_sq, self.max_abs, self.cells = sum, sum_abs, sum_sq, max_abs, int(cells)

    def mean(self):
        """float64 [n]: ``torch.mean(r, axis=...)`` per sample (the 'PRE' acquisition of ``Burgers_AL_Joint.py:340-345``)."""
        return self.sum / float(self.cells)

    def mean_abs(self):
        """float64 [n]: ``torch.mean(torch.abs(r), axis=...)`` per sample (``Wave_AL_Joint.py:403-408``,
        ``Advection_AL_Joint.py:340-345``)."""
        return self.sum_abs / float(self.cells)

    def mean_sq(self):
        """float64 [n]: the per-sample mean of r^2, the per-sample term of ``PI_loss``."""
        return self.sum_sq / float(self.cells)

    def rms(self):
        return torch.sqrt(self.mean_sq())

    def _stat(self, by):
        if by not in _STATS:
            raise ValueError(f"by={by!r}: one of {_STATS}")
        v = getattr(self, by)
        return v() if callable(v) else v

    def order(self, by="mean_abs", descending=False):
        """int64 [n]: the indices of ``torch.sort(<statistic>, stable=True)`` - the ``sort_index`` of the three scripts."""
        return torch.sort(self._stat(by), descending=descending, stable=True).indices

    def take(self, k, by="mean_abs", largest=False):
        """The first ``k`` of ``order(by, descending=largest)``."""
        k = int(k)
        if not 0 <= k <= self.sum.shape[0]:
            raise ValueError(f"k = {k} of {self.sum.shape[0]} samples")
        return self.order(by, descending=largest)[:k]


def _check_stats(spec, vars, crop):
    """Every shape, dtype and empty-batch error of a statistics call, raised before any device work (``_check_inputs``
    without levels, modulation and ``minus``).  Returns (uncropped residual shape, crop, counted cells per sample)."""
    if not isinstance(vars, torch.Tensor):
        raise TypeError("vars must be a torch.Tensor")
    if vars.dtype != torch.float32:
        raise TypeError(f"vars has dtype {vars.dtype}: the screen takes float32 fields")
    shape = spec.field_shape(vars)
    if vars.numel() == 0:
        raise ValueError("screen of an empty batch")
    crop = tuple(int(c) for c in crop)
    if len(crop) != len(shape) - 1 or any(c < 0 for c in crop):
        raise ValueError(f"crop {crop}: one non-negative count per residual axis")
    if any(n - 2 * c <= 0 for n, c in zip(shape[1:], crop)):
        raise ValueError(f"crop {crop} leaves no cell of a {tuple(shape[1:])} residual")
    cells = 1
    for n, c in zip(shape[1:], crop):
        cells *= n - 2 * c
    if cells >= 1 << 32:
        raise ValueError("cells per sample >= 2^32: screen the grid in slabs")
    return shape, crop, cells


# the workspace of the statistics launches: one float64 buffer per (device, stream), grown on demand, never handed out (its
# contents mean nothing between calls: every slot a launch reads it has written before)
_stats_ws = {}
_F32 = torch.empty(0, dtype=torch.float32)        # (stands in for the levels in ``_input_declined``: there are none)


def _stats_workspace(device, n):
    key = _dev_key(device) + (torch.cuda.current_stream(device).cuda_stream,)
    ws = _stats_ws.get(key)
    if ws is None or ws.numel() < n:
        ws = _stats_ws[key] = torch.empty(max(int(n), 1), dtype=torch.float64, device=device)
    return ws


class ScreenStats:
    """Accumulating per-sample statistics of ``n_local`` samples: ``add_slab`` once per slab of the grid (x-slabs with
    ``halo_x``, t-slabs with their halo planes, row slabs of the 1-D family - what slabs mean for ``Screen.add_slab``),
    ``finish`` -> ``SampleStats``.  The maximum composes exactly: the slabs of a grid give the bits of the whole grid's
    ``max_abs``; the float64 sums are those of the whole grid to the rounding of another order of the same terms."""

    def __init__(self, n_local, device):
        if n_local < 1:
            raise ValueError(f"ScreenStats needs n_local >= 1 (got {n_local})")
        self.n_local, self.device = int(n_local), torch.device(device)
        self.mx = self.sums = None     # int32 [n_local]: the bits of max |r|; float64 [3, n_local]; made at the first slab
        self.cells = 0

    def _buffers(self, device):
        if self.mx is None:
            self.mx = torch.zeros(self.n_local, dtype=torch.int32, device=device)
            self.sums = torch.zeros(3, self.n_local, dtype=torch.float64, device=device)
        return self.mx, self.sums

    def add_slab(self, method, vars_slab, crop=(1, 1, 1), halo_x=False, bc=False):
        """``vars_slab``: the method's input on a slab of the grid (all local samples); ``crop`` cells per side of each
        residual axis are left out (two axes for the 1-D family); ``halo_x``: the slab's rows -1 and X lie in the same
        memory (raises where ``Screen.add_slab`` raises); ``bc``: the opt-in statistics of the residual under boundary
        conditions on the x-y rim (module docstring).  There is no ``minus``: the 'PRE' acquisition has no paired form."""
        global _last_route
        spec = method if isinstance(method, _Spec) else _Spec(method, bc=bc)
        if spec.bc is not None and halo_x:
            raise ValueError(_BC_HALO_X)
        shape, crop, cells = _check_stats(spec, vars_slab, crop)
        if shape[0] != self.n_local:
            raise ValueError(f"slab of {shape[0]} samples, expected n_local = {self.n_local}")
        if _dev_key(vars_slab.device) != _dev_key(self.device):
            raise ValueError(f"slab on {vars_slab.device}, this ScreenStats was made for {self.device}")
        why, kernels = spec.prepare(vars_slab, None, _F32, None)
        if spec.row == "jorek":
            why = "no fused stats for JOREK"
        if halo_x and not vars_slab.is_cuda:
            raise ValueError("halo_x needs a device-resident view of a larger grid (a staged copy has no halo rows)")
        if halo_x and why is not None and not spec.reads_halo():
            # (before any device work: this slab would be evaluated against zero padding and counted as if it were right)
            raise RuntimeError(f"halo_x: the fused statistics cannot run ({why}) and no other pass of this method reads the halo rows")
        rows = spec.rows_kind is not None and spec.bc is None     # (the 1-D family: its rows route by default; halo_x has raised)
        if rows:
            why, kernels = spec.prepare_rows(vars_slab, None, _F32, None)
        flat = not rows and spec.bc is None and not halo_x and vars_slab.is_cuda and spec.nt_fastest(vars_slab)
        if flat:
            why, kernels = spec.prepare_flat(vars_slab, None, _F32, None)
        if why is None:
            mx, sums = self._buffers(vars_slab.device)
            form = "rows" if rows else "flat" if flat else ""
            with torch.no_grad(), torch.cuda.device(vars_slab.device):
                if spec.bc is not None:
                    need = int(_lib.load_screenbc().pre_screenbc_stats_workspace_len(*shape))
                else:
                    need = int(_lib.load_screenstats().pre_screenstats_workspace_len(
                        _lib.PRE_SCREENSTATS_FORM[form], *shape, *((1,) if rows else ())))
                ws = _stats_workspace(vars_slab.device, need)
                st = _lib.PreScreenStats(crop[0], crop[1], 0 if rows else crop[2], ctypes.c_void_p(mx.data_ptr()),
                                         ctypes.c_void_p(sums.data_ptr()), sums.stride(0), ctypes.c_void_p(ws.data_ptr()),
                                         ws.numel())
                rc = spec.launch(kernels, vars_slab, st, _lib.PRE_FLAG_HALO_X if halo_x and form == "" else 0, form, stats=True)
            if rc == _lib.PRE_E_UNSUPPORTED:
                why = "declined by the library"
                if halo_x and not spec.reads_halo():
                    raise RuntimeError("halo_x: the library declined and no other pass of this method reads the halo rows")
            else:
                _lib.check(rc, spec.entry(form, stats=True))
                _last_route = spec.route(form, stats=True)
                self.cells += cells
                return
        _last_route = "fallback:" + why
        self._fallback(spec, vars_slab, crop, halo_x)
        self.cells += cells

    def _fallback(self, spec, vars, crop, halo_x):
        """What a caller writes today: the stored residual by the existing pass with ``boundary=True``, then float64
        reductions of the counted region, where the residual lives."""
        res = spec.full(vars, None, halo_x)
        mx, sums = self._buffers(res.device)
        sl = (slice(None),) + tuple(slice(c, n - c) for c, n in zip(crop, res.shape[1:]))
        r32 = res[sl].reshape(res.shape[0], -1)
        r64 = r32.double()
        sums[0] += r64.sum(dim=1)
        sums[1] += r64.abs().sum(dim=1)
        sums[2] += (r64 * r64).sum(dim=1)
        a = r32.abs().max(dim=1).values
        a = torch.where(r32.isnan().any(dim=1), torch.full_like(a, float("nan")), a)
        # unsigned maximum of the bit patterns (non-negative values, the NaN pattern 0x7fc00000 above +inf)
        bits = torch.where(a.isnan(), torch.full_like(mx, 0x7fc00000), a.contiguous().view(torch.int32))
        torch.maximum(mx, bits, out=mx)

    def finish(self):
        if self.mx is None or self.cells == 0:
            raise ValueError("ScreenStats.finish() before any slab")
        return SampleStats(self.sums[0].clone(), self.sums[1].clone(), self.sums[2].clone(), self.mx.view(torch.float32).clone(),
                           self.cells)


def screen_stats(residual_method, vars, boundary=False, bc=False):
    """Per-sample statistics of the residual of ``vars`` - sum r, sum |r|, sum r^2 in float64 and max |r| - from ONE
    streaming launch that stores no residual (followed by a tiny launch that adds the workgroups' partial sums; no
    floating-point atomics: the same inputs give the same bytes on every run).  ``boundary=False``: the counted cells are
    the interior ``[1:-1]`` of every residual axis; ``boundary=True``: every cell.  Returns a :class:`SampleStats`:
    ``stats.order()`` is the ``sort_index`` of ``torch.sort(torch.mean(torch.abs(residual), axis=...))``,
    ``stats.order("mean")`` that of the signed form.  There is no ``minus=``: the 'PRE' acquisition has no paired form.
    ``bc``: as in ``screen`` (``boundary=False`` then crops the time rim only)."""
    spec = _Spec(residual_method, bc=bc)
    crop = _whole_crop(spec, boundary)
    shape, _, _ = _check_stats(spec, vars, crop)
    s = ScreenStats(shape[0], vars.device)
    s.add_slab(spec, vars, crop=crop)
    out = s.finish()
    if not vars.is_cuda:                                     # (staged inputs: the statistics come home, as elsewhere)
        out.sum, out.sum_abs, out.sum_sq, out.max_abs = (t.to(vars.device) for t in (out.sum, out.sum_abs, out.sum_sq, out.max_abs))
    return out
