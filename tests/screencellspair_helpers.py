"""Helpers shared by tests/test_screencellspair_cpu.py, tests/test_gpu_screencellspair.py and
tests/test_gpu_screencellspair_flat.py: the per-cell screen of the data-driven scores (``cp_pre_amd.screen.screen_cells`` /
``ScreenCells`` with ``minus=`` and ``pair=True``, csrc/screen_cells_pair.hip).

Nothing is restated here: the two field sets, the modulation, the float64 oracle difference ``d_ref = r_ref(a) - r_ref(b)``
and ``tau = 1e-5 * (max |r_ref(a)| + max |r_ref(b)|)`` are ``screenpair_helpers.PairCase``'s; the level fields, their
reference counts, the undecided cells, ``caps`` and ``check`` are ``screencells_helpers``' (``CellCase``'s methods, ``ranks``,
``N_CAL``, ``SHARE_CAP``), built here from ``|d_cal| / m`` of ``N_CAL`` = 12 calibration PAIRS drawn with other seeds (+200 the
truths, +250 the predictions) than the screened pair (0, +50) and the modulation's (+100, +150).  nk = 2, 5 and 9, which
``screencells_helpers.ranks`` does not have, take that many of the ten alphas' ranks.

A count may differ from ``count_ref`` by at most the cells with ``||d_ref| - hw| <= tau``; the score is within
``tau / m_min`` plus one fp32 ulp (``screencells_helpers.check``).  tests/test_screencellspair_cpu.py asserts, from the oracle
alone, for every case of ``gpu_cases``: the undecided share per (level, sample) is at most ``SHARE_CAP`` on regions of 100
cells and more, else at most one cell; the level fields have rank nk (at nk = 16, where four fields are means of two others
by construction: the twelve order statistics have rank 12 and all sixteen differ pairwise, ``CellPairCase.level_rank``); one
level splits the cells.  ``SEEDS`` holds the seed of a case that misses a cap at seed 0."""
import torch

import screen_helpers as sh
import screencells_helpers as ch
import screenflat_helpers as fh
import screenpair_helpers as sp

KINDS = sp.KINDS
# (nk, shape) of the cases every kind runs: all ten alphas; the first batch alone; sixteen levels (every later batch full);
# and a later batch with ONE live level for every pair of batch sizes the library is built with - nk = 2 (1 + 15: the NS
# momentum), 5 (4 + 12: the star operators), 9 (8 + 8: NS continuity / MHD gauss, the y-fixed MHD continuity)
ONE_LIVE = (2, 5, 9)
NY_MAIN = tuple((nk, sh.SEAM_SHAPES[name]) for nk, name in ch.MAIN) + tuple((nk, sh.SEAM_SHAPES["two_tseg"]) for nk in ONE_LIVE)
FLAT_MAIN = tuple((nk, sp.FLAT_BASE) for nk in (10, 1, 16) + ONE_LIVE)
FLAT_SEAMS = ch.FLAT_SEAMS
FLAT_SEAM_KINDS = sp.FLAT_SEAM_KINDS          # wave, NS momentum, MHD continuity
SLAB_SHAPE = ch.SLAB_SHAPE
GROUP_TXY, GROUP_KINDS = ch.GROUP_TXY, ch.GROUP_KINDS
VIEW_KINDS = ("ns_momentum", "wave", "mhd_continuity")
# the kinds whose functor is compiled per tap structure, and what the library builds of them: (kind, structure, form) -> built
TAP_KINDS = ("ns_momentum", "mhd_continuity")
BUILT = {("mhd_continuity", "yfix"): True, ("mhd_continuity", "general"): False, ("ns_momentum", "yfix"): False,
         ("ns_momentum", "general"): False}


def route(kind, flat=False):
    return "fused:" + ("flat_" if flat else "") + "cells_pair_" + sp.PAIR_KIND[kind]


def ranks(nk):
    """``screencells_helpers.ranks``, and for the nk it does not have a choice among the ten alphas' ranks"""
    if nk in ONE_LIVE:
        return {2: [(8, 8), (4, 4)], 5: ch.ranks(10)[::2], 9: ch.ranks(10)[:9]}[nk]
    return ch.ranks(nk)


class CellPairCase(ch.CellCase):
    """``screencells_helpers.CellCase`` (``q_cropped``, ``caps``; what ``screencells_helpers.check`` reads) for the
    difference of two residuals: ``x`` the truth, ``y`` the prediction, as ``screenpair_helpers.PairCase`` draws them."""

    def __init__(self, kind, shape, boundary, with_mod, nk, seed=0):
        base = sp.PairCase(kind, shape, boundary, with_mod, 1, seed=seed)
        self.kind, self.shape, self.boundary, self.nk, self.crop, self.seed = kind, tuple(shape), boundary, nk, base.crop, seed
        self.x, self.y, self.mod, self.r_ref, self.tau = base.x, base.y, base.mod, base.r_ref, base.tau
        self.cells, self.s_ref, self.tol_s = base.cells, base.s_ref, base.tol_s
        cal = (sh.oracle_residual(kind, sh.fields(kind, shape, seed + 200, n=ch.N_CAL).double()) -
               sh.oracle_residual(kind, sh.fields(kind, shape, seed + 250, n=ch.N_CAL).double())).abs()
        m = self.mod.double() if with_mod else torch.ones(cal.shape[1:], dtype=torch.float64)
        s = torch.sort(cal / m, dim=0).values                                         # [12, T, X, Y]
        self.q = torch.stack([0.5 * (s[i] + s[j]) for i, j in ranks(nk)]).float()     # [nk, T, X, Y]
        self.reg = sh.region(self.shape, self.crop)
        hw = (self.q.double() * m.float().double())[(slice(None),) + self.reg[1:]].reshape(nk, -1)
        d = base.a[None] - hw[:, None]                                                # [nk, B, cells]
        self.count_ref = (d <= 0).sum(dim=2)
        self.undecided = (d.abs() <= self.tau).sum(dim=2)

    def level_rank(self):
        """(rank of the level fields that are order statistics, their number, smallest share of cells in which two level
        fields differ).  The rank is what keeps a kernel that reads one level field for every k, or one level per k for every
        cell, from passing.  At nk = 16 the four midpoint fields are, cell by cell, the mean of two of the twelve order
        statistics: the sixteen fields have rank 12 by construction (what more a rank routine finds is the fp32 rounding of
        the means), so there the rank is asked of the twelve and each of the sixteen must differ from every other in most
        cells."""
        own = [k for k, (i, j) in enumerate(ranks(self.nk)) if i == j] or list(range(self.nk))      # (nk = 1: the median)
        rank = int(torch.linalg.matrix_rank(self.q[own].reshape(len(own), -1).double()))
        q = self.q.reshape(self.nk, -1)
        differ = min([float((q[a] != q[b]).double().mean()) for a in range(self.nk) for b in range(a)], default=1.0)
        return rank, len(own), differ

    def caps_hold(self):
        """(do the caps hold, (undecided cells at the worst (level, sample), counted cells, ``level_rank()``, does a level
        split the cells))"""
        _, split = self.caps()
        worst = int(self.undecided.max())
        rank, want, differ = self.level_rank()
        allowed = int(ch.SHARE_CAP * self.cells) if self.cells >= 100 else 1
        return worst <= allowed and rank == want and differ > 0.5 and split, (worst, self.cells, (rank, want, differ), split)


# (kind, shape, boundary, with_mod, nk) -> the seed for which the oracle meets the caps (default 0).  Chosen by hand as
# ``screenpair_helpers.SEEDS`` was: every case of ``gpu_cases`` was built at seeds 0, 1, ... and the first seed at which
# ``caps_hold`` is true was taken.  tests/test_screencellspair_cpu.py asserts the caps at the seed tabulated here and that no
# entry names a case no test uses; it does not search.
SEEDS = {
}

_cache = {}


def case(kind, shape, boundary=False, with_mod=True, nk=10, n=None):
    """The case of (kind, shape, boundary, with_mod, nk), built once and shared: the tests read it and leave it unchanged.
    ``n``: that many samples in place of ``shape[0]``."""
    shape = tuple(shape) if n is None else (n,) + tuple(shape[1:])
    key = (kind, shape, bool(boundary), bool(with_mod), nk)
    if key not in _cache:
        _cache[key] = CellPairCase(kind, shape, boundary, with_mod, nk, seed=SEEDS.get(key, 0))
    return _cache[key]


def gpu_cases(G):
    """Every (kind, shape, boundary, with_mod, nk) the two GPU files compare with the reference; ``G``: the library's sample
    group, which sizes the sample-group cases."""
    out = []
    for main in (NY_MAIN, FLAT_MAIN):                              # every kind x boundary x modulation
        for nk, shape in main:
            for kind in KINDS:
                for boundary in (False, True):
                    for with_mod in (False, True):
                        out.append((kind, shape, boundary, with_mod, nk))
    for name in FLAT_SEAMS:                                        # the flat seams
        for kind in FLAT_SEAM_KINDS:
            out.append((kind, fh.SEAM_SHAPES[name], False, True, 10))
    for kind in GROUP_KINDS:                                       # the sample group
        for B in ch.group_batches(G):
            out.append((kind, (B,) + GROUP_TXY, True, True, 10))
    for kind in VIEW_KINDS:                                        # views, contracts
        out.append((kind, sh.SEAM_SHAPES["rows2_narrow"], False, True, 10))
    out.append(("ns_momentum", SLAB_SHAPE, False, True, 10))       # slabs
    out.append(("ns_momentum", sp.ODD_NY, False, True, 10))        # the fallbacks by shape
    out.append(("ns_momentum", sp.ODD_FLAT, False, True, 10))
    return sorted(set(out), key=repr)


check = ch.check
group_batches = ch.group_batches


# ------------------------------------------------------------------ what the two GPU files share
def put(t, flat, device):
    """``t`` ([B,F,T,X,Y], [B,T,X,Y], level fields [nk,T,X,Y] or a modulation [T,X,Y]) on ``device``, Ny-fastest or
    (``flat``) as ``screenflat_helpers.to_layout`` lays it out"""
    if t is None:
        return None
    return fh.to_layout(t, device) if flat else t.to(device)


def run(c, device, flat, x=None, y=None, q=None, mod=None, method=None, pair=True, **kw):
    """``screen_cells(..., minus=, pair=)`` on case ``c``; a tensor given by keyword is taken as it is"""
    from cp_pre_amd import screen
    xd = put(c.x, flat, device) if x is None else x
    yd = put(c.y, flat, device) if y is None else y
    qd = put(c.q, flat, device) if q is None else q
    md = put(c.mod, flat, device) if mod is None else mod
    return screen.screen_cells(method or sh.method_of(c.kind, device), xd, qd, md, boundary=c.boundary, minus=yd, pair=pair, **kw)


def same(a, b):
    import stencil_guards as sg
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside)


def check_routes_agree(c, s, other, what):
    """Two routes on the same inputs, each within ``check``'s bounds of the reference: the scores within ``2 tau / m_min``
    plus an ulp of each other, a count apart by at most the undecided cells of its (level, sample)."""
    err = (s.score.double() - other.score.double()).abs().cpu()
    dcount = (s.inside - other.inside).abs().cpu()
    print(f"{what}: score diff {float(err.max()):.3e} (allowed {2 * c.tol_s:.3e} + ulp), count diff max {int(dcount.max())}, "
          f"bit-identical: {same(s, other)}")
    assert s.cells == other.cells
    assert bool((err <= 2 * c.tol_s + 1.2e-7 * other.score.double().abs().cpu()).all()), (what, err)
    assert bool((dcount <= c.undecided).all()), (what, dcount, c.undecided)


def check_against_stored_difference(c, s, method, xd, yd, flat, what):
    """``s`` against the difference the package's own paired residual pass STORES with the same operators (the oracle has
    the reference's operators only).  The bounds are worked out for these operators from the stored fp32 residuals: each
    half is within tau_h = 1e-5 max |r_h| of the truth, so the stored difference and the one the screen
    holds in registers are each within tau = tau_a + tau_b of it and within 2 tau of each other: the score within
    2 tau / m_min (and one rounding of the divide), a count off by no more than the cells whose stored |d| lies within 2 tau
    of that level's edge."""
    device = xd.device
    ra, rb = method(xd, boundary=True), method(yd, boundary=True)
    tau = 1e-5 * (float(ra.abs().max()) + float(rb.abs().max()))
    d = method(xd, boundary=True, minus=yd)[c.reg].abs().double().flatten(1)          # [B, cells]
    m = (c.mod.to(device) if c.mod is not None else torch.ones(c.shape[1:], device=device))[c.reg[1:]].double().flatten()
    tol = 2 * tau / float(m.min())
    want = (d / m).max(dim=1).values
    hw = c.q.to(device).double()[(slice(None),) + c.reg[1:]].flatten(1) * m[None]     # [nk, cells]
    gap = d[None] - hw[:, None]
    und = (gap.abs() <= 2 * tau).sum(dim=2)
    err = (s.score.double() - want).abs()
    dcount = (s.inside - (gap <= 0).sum(dim=2)).abs()
    print(f"{what}: score diff {float(err.max()):.3e} (allowed {tol:.3e} + ulp), count diff max {int(dcount.max())} "
          f"(within 2 tau of an edge: max {int(und.max())} of {m.numel()} cells)")
    assert s.cells == m.numel() and tuple(s.inside.shape) == (c.nk, c.shape[0])
    assert bool((err <= tol + 1.2e-7 * want).all()), (what, err, tol)
    assert bool((dcount <= und).all()), (what, dcount, und)
