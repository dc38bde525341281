"""Helpers shared by tests/test_screenjorekcells_cpu.py and tests/test_gpu_screenjorekcells.py: the opt-in per-cell screen
of the JOREK residuals (``cp_pre_amd.screen.screen_cells`` / ``ScreenCells`` with ``jorek=True``,
csrc/screen_jorek_cells.hip), and ``norms=True`` of the continuity equation through ``functools.partial`` on both JOREK
screens.

Cases are ``screencells_helpers.CellCase`` built inside ``screenjorek_helpers._jorek_case(mode)``: the fields, ``R =
linspace(1, 2, Ny)``, the float64 oracle and the staged modes are those of tests/screenjorek_helpers.py; the level fields are
order statistics of a 12-sample calibration set drawn with another seed, as tests/screencells_helpers.py builds them.
Tolerances are the project's: tau = 1e-5 max |r_ref|; score within tau / m_min + one fp32 ulp; a count may differ from the
float64 count by at most the undecided cells of that (level, sample).

Seed: per case the first of 0..5 for which the undecided share is at most ``SHARE_CAP`` = 1 % of the counted cells and one
level splits a sample's cells (``case`` raises if there is none; tests/test_screenjorekcells_cpu.py runs every case the GPU
file uses).

``norms=True``: the reference is ``oracle.residuals.jorek_continuity(..., norms=True, dx=, dy=, dt=)`` with ``NORMS``, three
grid steps off 1 and unlike each other, so that a launch that took the scalars of ``norms=False`` is far outside every
bound."""
import contextlib
import functools

import screen_helpers as sh
import screencells_helpers as sc
import screenflat_helpers as sf
import screenjorek_helpers as sj
from oracle import residuals as orr

KINDS, EQS, MODES = sj.KINDS, sj.EQS, sj.MODES
FLAT_BASE, NY_BASE = sj.FLAT_BASE, sj.NY_BASE
FLAT_SEAMS = {k: sf.SEAM_SHAPES[k] for k in sc.FLAT_SEAMS}
NY_SEAMS = dict(sj.NY_SEAMS)
SLAB_SHAPE = sc.SLAB_SHAPE
SMALLEST_Y = sf.SMALLEST_Y
STAGED = {"flat": ((3, 10, 5, 12), (3, 95, 5, 12)), "ny": ((3, 4, 33, 16),)}
GROUP_TXY = sc.GROUP_TXY
FALLBACK_SHAPES = dict(sj.FALLBACK_SHAPES)
SHARE_CAP = sc.SHARE_CAP
NORMS = {"dx": 0.5, "dy": 0.25, "dt": 0.125}
NKS = (1, 10, 16)


def route(kind, form):
    return "fused:" + ("flat_" if form == "flat" else "") + "cells_" + kind


@contextlib.contextmanager
def _norms_case():
    """``sj._jorek_case`` with the oracle of ``norms=True`` (continuity only)"""
    with sj._jorek_case(None):
        def residual(kind, x):
            assert kind == "jorek_continuity"
            with sh.oracle_fp64():
                return orr.jorek_continuity(sj.to_vars(x), sj.radius(x.shape[-1]).double(), boundary=True, norms=True, **NORMS)
        sh.oracle_residual = residual
        yield


_cases = {}


def _first_seed(key, build, holds):
    if key not in _cases:
        for seed in range(6):
            c = build(seed)
            if holds(c):
                c.seed = seed
                _cases[key] = c
                break
        else:
            raise AssertionError(f"no seed in 0..5 meets the caps for {key}")
    return _cases[key]


def caps_hold(c):
    share, split = c.caps()
    return share <= SHARE_CAP and split


def case(kind, shape, boundary=False, with_mod=True, nk=10, mode=None, n=None, norms=False):
    """The per-cell case (computed once per key and left unchanged); ``case.seed`` is the seed taken.  ``n``: another sample
    count than ``shape[0]`` (the sample-group cases)."""
    key = ("cells", kind, tuple(shape), boundary, with_mod, nk, mode, n, norms)

    def build(seed):
        with (_norms_case() if norms else sj._jorek_case(mode)):
            return sc.CellCase(kind, shape, boundary, with_mod, nk, seed=seed, n=n)
    return _first_seed(key, build, caps_hold)


def joint_norms_case(shape, boundary=False, with_mod=True, nk=10):
    """``screen_helpers.Case`` (nk scalar levels) of the continuity equation with ``norms=True``: for ``screen(...,
    jorek=True)`` through the partial; the caps are tests/screenjorek_helpers.py's."""
    key = ("joint", tuple(shape), boundary, with_mod, nk)

    def build(seed):
        with _norms_case():
            return sh.Case("jorek_continuity", shape, boundary, with_mod, nk, seed=seed)
    return _first_seed(key, build, sj.caps_hold)


def norms_method(device="cpu", ny=12, norms=True, kind="jorek_continuity", steps=True):
    """``functools.partial(<bound equation>, norms=)`` on a ``JOREK`` that holds ``NORMS`` (``steps=False``: no grid steps)"""
    j = sj.jorek_of(None, device, ny, coef=NORMS if steps else None)
    return functools.partial(getattr(j, "residual_" + kind[len("jorek_"):]), norms=norms)


def group_batches(G):
    return sc.group_batches(G)


def gpu_cases(G=16):
    """Every (kind, shape, boundary, with_mod, nk, mode, n) tests/test_gpu_screenjorekcells.py compares with the float64
    reference (``G``: the library's sample group; the CPU test takes the default of the build, 16)."""
    for kind in KINDS:
        for base in (FLAT_BASE, NY_BASE):
            for boundary in (False, True):
                for with_mod in (False, True):
                    for nk in NKS:
                        yield kind, base, boundary, with_mod, nk, None, None
        for shape in list(FLAT_SEAMS.values()) + list(NY_SEAMS.values()):
            for boundary in (False, True):
                yield kind, shape, boundary, True, 10, None, None
        yield kind, SMALLEST_Y, True, True, 10, None, None
        for mode in MODES:
            for shape in STAGED["flat"] + STAGED["ny"]:
                yield kind, shape, False, True, 10, mode, None
        for B in sorted(set(group_batches(G)) | {3}):
            yield kind, (3,) + GROUP_TXY, True, True, 10, None, B
        yield kind, SLAB_SHAPE, False, True, 10, None, None
        for shape in FALLBACK_SHAPES:
            yield kind, shape, False, True, 10, None, None


check = sc.check
