"""Helpers shared by tests/test_screencells_cpu.py, tests/test_gpu_screencells.py and tests/test_gpu_screencells_flat.py:
the per-cell screen (``cp_pre_amd.screen.screen_cells`` / ``ScreenCells``, csrc/screen_cells.hip).

Reference: ``screen_helpers.Case`` for the fields, the modulation and the float64 oracle residual ``r_ref`` (uncropped),
``tau = 1e-5 * max |r_ref|``, ``s_ref`` and its slack ``tau / m_min``.  The per-cell levels of a case are order statistics
of the score ``|r_cal| / m`` (``m == 1`` without a modulation) of a synthetic calibration set of ``N_CAL`` = 12 samples drawn
with ANOTHER seed than the screened ones (a screened sample that is its own order statistic would be undecided by
construction): for nk = 10 the ranks ``ceil((1 - alpha) * 12) - 1`` at the reference's ten alphas 0.05 ... 0.95, for nk = 16
all twelve ranks and four midpoints of adjacent ranks, for nk = 1 the median.  They are float32 ``[nk,T,X,Y]`` with the
uncropped extents; ``count_ref[k, b] = #{|r_ref| <= q32_k * m32}`` over the counted cells in float64, a cell is undecided
at level k if ``||r_ref| - q_k m| <= tau``; a count may differ from ``count_ref`` by at most the undecided cells of that
(k, sample), whose share of the counted cells is at most ``SHARE_CAP`` - asserted on the CPU for every GPU case
(tests/test_screencells_cpu.py), so the reference alone is known to stay within it."""
import functools
import math

import numpy as np
import torch

import screen_helpers as sh
import screenflat_helpers as fh

N_CAL = 12
ALPHAS = tuple(round(0.05 + 0.1 * i, 2) for i in range(10))
SHARE_CAP = 0.01
# (nk, name of the shape in screen_helpers.SEAM_SHAPES) of the cases every kind runs, in both layouts
MAIN = ((10, "two_tseg"), (1, "rows2_narrow"), (16, "rows3_wide"))
SEAM_KINDS = ("ns_momentum", "lap", "mhd_momentum")
FLAT_SEAMS = ("straddle_10", "two_chunks", "chunk_seam", "widest_halo", "two_marches", "many_marches_last_one")
SLAB_SHAPE = (3, 12, 41, 64)      # the grid the slab tests cut
# (T, X, Y) of the sample-group cases, screened with boundary=True: cropped it has 60 counted cells, of which a single
# undecided one is 1.7 %; all 240 counted, the one undecided cell the reference has at some (level, sample) is 0.4 %
GROUP_TXY = (4, 5, 12)
GROUP_KINDS = ("ns_momentum", "wave")


def route(kind, flat=False):
    return "fused:" + ("flat_" if flat else "") + "cells_" + sh.FUSED_KIND[kind]


def ranks(nk):
    """Indices (and, for nk = 16, midpoints) into the 12 sorted calibration scores of a cell: a list of (i, j), level =
    (s[i] + s[j]) / 2."""
    if nk == 1:
        return [(5, 6)]
    r = [(i, i) for i in (math.ceil(round((1 - a) * N_CAL, 9)) - 1 for a in ALPHAS)]
    if nk == 10:
        return r
    assert nk == 16
    return [(i, i) for i in range(N_CAL)] + [(i, i + 1) for i in (1, 4, 7, 10)]


class CellCase:
    """One per-cell screening case: the inputs of ``screen_helpers.Case``, level fields and their float64 reference."""

    def __init__(self, kind, shape, boundary, with_mod, nk, seed=0, n=None):
        shape = tuple(shape) if n is None else (n,) + tuple(shape[1:])
        base = sh.Case(kind, shape, boundary, with_mod, 1, seed=seed)
        self.kind, self.shape, self.boundary, self.nk, self.crop = kind, shape, boundary, nk, base.crop
        self.x, self.mod, self.r_ref, self.tau = base.x, base.mod, base.r_ref, base.tau
        self.cells, self.s_ref, self.tol_s = base.cells, base.s_ref, base.tol_s
        cal = sh.oracle_residual(kind, sh.fields(kind, shape, seed + 200, n=N_CAL).double()).abs()
        m = self.mod.double() if with_mod else torch.ones(cal.shape[1:], dtype=torch.float64)
        s = torch.sort(cal / m, dim=0).values                                         # [12, T, X, Y]
        self.q = torch.stack([0.5 * (s[i] + s[j]) for i, j in ranks(nk)]).float()     # [nk, T, X, Y]
        reg = sh.region(shape, self.crop)
        self.reg = reg
        hw = (self.q.double() * m.float().double())[(slice(None),) + reg[1:]].reshape(nk, -1)      # [nk, cells]
        d = base.a[None] - hw[:, None]                                                # [nk, B, cells]
        self.count_ref = (d <= 0).sum(dim=2)
        self.undecided = (d.abs() <= self.tau).sum(dim=2)

    def q_cropped(self):
        return self.q[(slice(None),) + self.reg[1:]].contiguous()

    def caps(self):
        """(largest share of undecided cells over (level, sample), does a level split the cells of a sample)"""
        share = float(self.undecided.max()) / self.cells
        split = bool(((self.count_ref > 0) & (self.count_ref < self.cells)).any())
        return share, split


@functools.lru_cache(maxsize=None)
def case(kind, shape, boundary=False, with_mod=True, nk=10, n=None):
    return CellCase(kind, shape, boundary, with_mod, nk, seed=fh.SEEDS.get((kind, tuple(shape)), 0), n=n)


def gpu_cases():
    """(kind, shape, boundary, with_mod, nk, n) of every case the two GPU files check against the reference with the
    default sample count or a stated one (the sample-group cases are added by the caller, which knows G)."""
    out = []
    for nk, name in MAIN:
        for kind in sh.KINDS:
            for boundary in (False, True):
                for with_mod in (False, True):
                    out.append((kind, sh.SEAM_SHAPES[name], boundary, with_mod, nk, None))
    for name, shape in sh.SEAM_SHAPES.items():
        for kind in SEAM_KINDS:
            out.append((kind, shape, False, True, 10, None))
    for name in FLAT_SEAMS:
        for kind in fh.SEAM_KINDS:
            out.append((kind, fh.SEAM_SHAPES[name], False, True, 10, None))
    for kind in ("ns_momentum", "wave", "mhd_energy"):               # views, contracts, slabs, fallbacks
        out.append((kind, sh.SEAM_SHAPES["rows2_narrow"], False, True, 10, None))
    out.append(("ns_momentum", SLAB_SHAPE, False, True, 10, None))
    out.append(("ns_momentum", sh.ODD_SHAPES[0], False, True, 10, None))
    for shape in fh.FALLBACK_SHAPES:
        out.append(("ns_momentum", shape, False, True, 10, None))
    return out


def group_batches(G):
    """The batch sizes that cross the seam of a sample group of G: one past a group, one short of two groups."""
    return (3,) if G == 1 else tuple(sorted({G + 1, 2 * G - 1}))


def check(c, out, label=""):
    """Assert ``out`` (a ``Screened``) against the reference of case ``c``; prints the figures first."""
    score = out.score.double().cpu()
    inside = out.inside.cpu()
    ulp = torch.from_numpy(np.spacing(c.s_ref.float().numpy()).astype(np.float64))
    es = float(((score - c.s_ref).abs() - ulp).max())
    dc = (inside - c.count_ref).abs()
    print(f"{label} {c.kind} {c.shape} nk={c.nk}: score err {es:.3e} (tol {c.tol_s:.3e}), count diff max {int(dc.max())} "
          f"(undecided max {int(c.undecided.max())}), cells {c.cells}")
    assert out.cells == c.cells
    assert tuple(inside.shape) == (c.nk, c.shape[0])
    assert es <= c.tol_s, (es, c.tol_s)
    assert bool((dc <= c.undecided).all()), (inside, c.count_ref, c.undecided)
