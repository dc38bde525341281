"""Helpers shared by tests/test_screenjorek_cpu.py and tests/test_gpu_screenjorek.py: the opt-in fused screen of the JOREK
residuals (cp_pre_amd.screen with ``jorek=True``, csrc/screen_jorek.hip).

Cases are ``screen_helpers.Case``: the same float64 reference and tolerances (tau = 1e-5 max |r_ref|, the tolerance the
JOREK residual pass is already held to; score within tau / m_min + one fp32 ulp; counts within the undecided cells; accept
exact).  Inputs: the three positive channels of ``screen_helpers.fields("ns_momentum", shape, seed)`` on the logical
(B, T, X, Y), handed to the package as ``vars = x.permute(0,1,3,4,2)`` ([BS,F,Nx,Ny,Nt]), and ``R = linspace(1, 2, Ny)`` in
float32.  Reference: ``oracle.residuals.jorek_continuity`` / ``jorek_temperature(vars, R.double(), boundary=True)`` under
``screen_helpers.oracle_fp64()``; ``ops=`` hands the oracle other operators (the staged modes).

Seed: per case the first of 0..5 for which the undecided share is at most 1 % of the counted cells, every level lies
further than tau / m_min from every per-sample score and one level splits the samples (``case`` raises if there is none;
tests/test_screenjorek_cpu.py runs every case the GPU file uses)."""
import contextlib

import torch

import screen_helpers as sh
import screenflat_helpers as sf
from oracle import residuals as orr

EQS = ("continuity", "temperature")
KINDS = tuple("jorek_" + e for e in EQS)
FLAT_BASE, NY_BASE = (3, 10, 5, 12), (3, 5, 9, 12)
FLAT_SEAMS = {k: sf.SEAM_SHAPES[k] for k in ("straddle_10", "straddle_30", "whole_rows", "two_chunks", "chunk_seam",
                                             "one_counted_plane", "two_marches", "many_marches_last_one")}
NY_SEAMS = {k: sh.SEAM_SHAPES[k] for k in ("two_tseg", "three_tseg_last_one", "rows2_narrow", "rows3_mid", "rows3_wide",
                                           "cols2_wide")}
STAGED_FLAT = {"straddle_10": sf.SEAM_SHAPES["straddle_10"], "widest_halo": sf.SEAM_SHAPES["widest_halo"]}
STAGED_NY = {"rows2_narrow": sh.SEAM_SHAPES["rows2_narrow"]}
MODES = ("yfix", "general")                  # the staged tap structures: <4> / <2> in the flat form, <1> / <2> Ny-fastest
FALLBACK_SHAPES = {(3, 96, 5, 12): "Nt >= 96", (3, 10, 5, 13): "merged row Ny*Nt not a multiple of 4"}
X_STAR = 0.25                                # the weight the 'general' mode puts on D_R's t and y neighbours


def radius(ny):
    return torch.linspace(1, 2, ny, dtype=torch.float32)


def to_vars(x):
    """the logical [B,3,T,X,Y] as the script's ``vars`` [BS,F,Nx,Ny,Nt] (a view)"""
    return x.permute(0, 1, 3, 4, 2)


def general_kernel(k):
    """``D_R``'s kernel with weight on all three axes: the general star"""
    k = k.clone()
    k[0, 1, 1], k[1, 1, 2] = X_STAR, -X_STAR
    return k


def oracle_ops(mode, coef=None, rescale=None):
    """The oracle's five operators for a staged mode (None: the script's).  ``coef``: a dict of ``JOREK``'s constructor
    scalars off their defaults (``lap_scale`` and ``gamma`` reach the operators); ``rescale``: operator name -> the factor
    its kernel is multiplied by after construction."""
    if mode is None and not coef and not rescale:
        return None
    coef = coef or {}
    o = orr.OpsJorek(lap_scale=coef.get("lap_scale"), gamma=coef.get("gamma", 5 / 3))
    if mode == "yfix":                       # the taps of the 'y' operators moved from Nt to the true Ny axis
        for op in (o.D_Z, o.D_ZZ):
            op.kernel = op.kernel.permute(2, 1, 0).contiguous()
    elif mode == "general":
        o.D_R.kernel = general_kernel(o.D_R.kernel)
    for a, s in (rescale or {}).items():
        getattr(o, a).kernel = getattr(o, a).kernel * s
    return o


def jorek_of(mode=None, device="cpu", ny=12, fused=True, coef=None, rescale=None):
    """The package's ``JOREK`` with the operators of ``mode``; ``coef`` / ``rescale`` as ``oracle_ops`` takes them (``coef``
    may hold any constructor scalar: D, K, gamma, lap_scale, dx, dy, dt)."""
    from cp_pre_amd import residuals as R
    j = R.JOREK(radius(ny), device=device, fused=fused, y_axis_fix=(mode == "yfix"), **(coef or {}))
    if mode == "general":
        j.D_R.kernel = general_kernel(j.D_R.kernel)
    for a, s in (rescale or {}).items():
        getattr(j, a).kernel = getattr(j, a).kernel * s
    return j


def method_of(kind, mode=None, device="cpu", ny=12, fused=True, coef=None, rescale=None):
    return getattr(jorek_of(mode, device, ny, fused, coef, rescale), "residual_" + kind[len("jorek_"):])


def oracle_residual(kind, x, mode=None, coef=None, rescale=None):
    """The uncropped residual [B,T,X,Y] of the logical float64 fields ``x`` [B,3,T,X,Y] by the oracle."""
    kw = {}
    if coef:
        names = ("D",) if kind == "jorek_continuity" else ("K", "gamma")
        kw = {k: coef[k] for k in names if k in coef}
    with sh.oracle_fp64():
        return getattr(orr, kind)(to_vars(x), radius(x.shape[-1]).double(), boundary=True,
                                  ops=oracle_ops(mode, coef, rescale), **kw)


@contextlib.contextmanager
def _jorek_case(mode, coef=None, rescale=None, rho0=False):
    """``screen_helpers.Case`` builds its inputs and reference through ``sh.fields`` / ``sh.oracle_residual``: swapped for
    the JOREK kinds while a case is built.  ``rho0``: every field set (the calibration set of the modulation too) with
    ``rho = 0`` exactly - the input on which the temperature residual is ``a3*Y(T)`` and nothing else."""
    fields, residual = sh.fields, sh.oracle_residual

    def jorek_fields(kind, shape, seed=0, n=None):
        x = fields("ns_momentum", shape, seed, n)
        if rho0:
            x[:, 0] = 0.0
        return x
    sh.fields = jorek_fields
    sh.oracle_residual = lambda kind, x: oracle_residual(kind, x, mode, coef, rescale)
    try:
        yield
    finally:
        sh.fields, sh.oracle_residual = fields, residual


def caps_hold(c):
    share, dist, split = c.caps()
    return c.m_min > 0 and share <= 0.01 and dist > 1.0 and split


_cases = {}


def case(kind, shape, boundary=False, with_mod=True, nk=10, mode=None, coef=None, rescale=None, rho0=False):
    """(computed once per key and left unchanged)  ``case.seed`` is the seed taken.  ``coef`` / ``rescale`` / ``rho0``:
    optional, as ``jorek_of`` and ``_jorek_case`` take them; absent, the key and the case are what they were."""
    key = (kind, tuple(shape), boundary, with_mod, nk, mode)
    if coef or rescale or rho0:
        key += (tuple(sorted((coef or {}).items())), tuple(sorted((rescale or {}).items())), bool(rho0))
    if key not in _cases:
        for seed in range(6):
            with _jorek_case(mode, coef, rescale, rho0):
                c = sh.Case(kind, shape, boundary, with_mod, nk, seed=seed)
            if caps_hold(c):
                c.seed = seed
                _cases[key] = c
                break
        else:
            raise AssertionError(f"no seed in 0..5 meets the caps for {key}")
    return _cases[key]


def gpu_cases():
    """Every (kind, shape, boundary, with_mod, nk, mode) tests/test_gpu_screenjorek.py builds."""
    for kind in KINDS:
        for base in (FLAT_BASE, NY_BASE):
            for boundary in (False, True):
                for with_mod in (False, True):
                    for nk in (1, 10, 16):
                        yield kind, base, boundary, with_mod, nk, None
        for shape in list(FLAT_SEAMS.values()) + list(NY_SEAMS.values()):
            for boundary in (False, True):
                yield kind, shape, boundary, True, 10, None
        yield kind, sf.SMALLEST_Y, True, True, 10, None
        for mode in MODES:
            for shape in list(STAGED_FLAT.values()) + list(STAGED_NY.values()):
                yield kind, shape, False, True, 10, mode
        for shape in FALLBACK_SHAPES:
            yield kind, shape, False, True, 10, None
