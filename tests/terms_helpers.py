"""Helpers shared by tests/test_terms_cpu.py and tests/test_gpu_terms.py: the fused residuals term by term and off their
default coefficients (tests/TERMS_TESTS.md).

For ``ns_momentum``, ``mhd_energy``, ``jorek_continuity`` (``norms`` False and True) and ``jorek_temperature`` a ``*_terms``
function returns the UNCROPPED residual as a dict of named terms, restated from the lines ``oracle/residuals.py`` cites with
the oracle's own operators and every coefficient an argument; the three parts of ``a3*Y(T)`` are entries of their own.
Their sum is the oracle's function (tests/test_terms_cpu.py, fp64, ``rtol 1e-12``).  ``MUTANTS`` lists, per equation, wrong
versions of the same expression, each a callable on the reference's inputs: a coefficient at its default, in another's slot
or folded wrongly, a term dropped, a ``Y`` part dropped, ``Y`` reading ``rho``, ``R`` where ``1/R`` belongs.  A mutant is
VISIBLE on an input if ``rel_err(mutant, reference) >= VISIBLE = 100 * RES_TOL``: the condition the CPU file asserts for every
input family the GPU file uses, so that a kernel or host entry with that mistake cannot pass the GPU file's ``RES_TOL``.

Coefficients, all off the defaults (``COEF``): NS ``dt, dx, dy, nu = 0.01, 1/64, 1/48, 0.02``; MHD ``gamma = 1.4``; JOREK
``D = 1.7``, ``K = jorekvjp_helpers.K_BIG``, ``gamma = 1.4``, ``lap_scale = 0.625``, and for ``norms=True``
``jorekvjp_helpers.NORM_DX / NORM_DY / NORM_DT``; the operator set 'rescaled' multiplies the five JOREK kernels by
``jorekvjp_helpers.RESCALE`` after construction.

The isolating input of the default-``K`` path: ordinary fields with ``rho = 0`` exactly.  Every other term of the temperature
residual carries a factor ``rho`` or a derivative of ``rho``, so the residual IS ``a3*Y(T)`` and ``rel_err``'s denominator
the term's own maximum."""
import numpy as np
import torch

import jorekvjp_helpers as jh
import screen_helpers as sh
import screenflat_helpers as sf
import screenjorek_helpers as sj
import screenpair_helpers as sp
from oracle import residuals as orr

RES_TOL = 1e-5
VISIBLE = 100 * RES_TOL

NS = dict(dt=0.01, dx=1 / 64, dy=1 / 48, nu=0.02)
NS_DEFAULT = dict(nu=0.001)
MHD = dict(gamma=1.4)
MHD_DEFAULT = dict(gamma=5 / 3)
JOREK = dict(D=1.7, K=jh.K_BIG, gamma=1.4, lap_scale=0.625)
JOREK_DEFAULT = dict(D=3.4, K=2.25 * 1e-7, gamma=5 / 3, lap_scale=None)
NORMS = dict(dx=jh.NORM_DX, dy=jh.NORM_DY, dt=jh.NORM_DT)
COEF = {"ns_momentum": NS, "mhd_energy": MHD, "jorek_continuity": JOREK, "jorek_temperature": JOREK}
OPSETS = ("default", "rescaled", "yfix", "general")

# the shapes of tests/test_gpu_terms.py
NY_SHAPES = [(2, 5, 10, 64), (2, 3, 7, 66)]              # [B,T,X,Y] of test_ns_residuals_in_a_poisoned_allocation
JOREK_SHAPES = [(2, 40, 12), (3, 64, 10)]                # (B, N, Nt): vars [B,3,N,N,Nt]
SCREEN2D = {"march": [sh.SEAM_SHAPES["two_tseg"], sh.SEAM_SHAPES["rows2_narrow"]],       # sp.NY_BASE and one seam
            "flat": [sf.BASE, sf.SEAM_SHAPES["two_marches"]]}
SCREEN_KINDS = ("ns_momentum", "mhd_energy")
SCREEN_JOREK = {"flat": [sj.FLAT_BASE, sj.FLAT_SEAMS["two_marches"]], "ny": [sj.NY_BASE, sj.NY_SEAMS["rows2_narrow"]]}
STAGED_JOREK = {"flat": sj.STAGED_FLAT["straddle_10"], "ny": sj.STAGED_NY["rows2_narrow"]}


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def total(terms, drop=()):
    """The sum of the named terms, without those in ``drop``."""
    drop = (drop,) if isinstance(drop, str) else tuple(drop)
    assert all(d in terms for d in drop), drop
    out = None
    for name, t in terms.items():
        if name not in drop:
            out = t if out is None else out + t
    return out


# ------------------------------------------------------------------------------------------------ Navier-Stokes momentum
def ns_momentum_terms(vars, dt, dx, dy, nu, ops=None):
    """Marginal/NS_Residuals_CP.py:231-240 (``oracle.residuals.ns_momentum``), uncropped."""
    o = ops or orr.Ops2D()
    D_t, D_x, D_y, L = o.D_t, o.D_x, o.D_y, o.D_xx_yy
    u, v, p = vars[:, 0], vars[:, 1], vars[:, 2]
    return {"x:Dt(u)dxdy": D_t(u)*dx*dy, "x:uDx(u)dtdy": u*D_x(u)*dt*dy, "x:vDy(u)dtdx": v*D_y(u)*dt*dx,
            "x:-nuL(u)dt": -nu*L(u)*dt, "x:Dx(p)dtdy": D_x(p)*dt*dy,
            "y:Dt(v)dxdy": D_t(v)*dx*dy, "y:uDx(v)dtdx": u*D_x(v)*dt*dx, "y:vDy(v)dtdy": v*D_y(v)*dt*dy,
            "y:-nuL(v)dt": -nu*L(v)*dt, "y:Dy(p)dtdx": D_y(p)*dt*dx}


def ns_momentum_ref(vars, coef=NS):
    return orr.ns_momentum(vars, coef["dt"], coef["dx"], coef["dy"], coef["nu"], boundary=True)


def _ns_mutants():
    c = NS
    out = [("nu at its default", lambda v: total(ns_momentum_terms(v, **{**c, **NS_DEFAULT}))),
           ("dx and dy swapped", lambda v: total(ns_momentum_terms(v, c["dt"], c["dy"], c["dx"], c["nu"]))),
           ("nu*dx in place of nu*dt", lambda v: total({**ns_momentum_terms(v, **c), **{
               k: t * (c["dx"] / c["dt"]) for k, t in ns_momentum_terms(v, **c).items() if "nuL" in k}}))]
    names = list(ns_momentum_terms(torch.zeros(1, 3, 3, 3, 4), **c))
    out += [("dropped " + n, lambda v, n=n: total(ns_momentum_terms(v, **c), n)) for n in names]
    return out


# ------------------------------------------------------------------------------------------------ MHD energy
def mhd_energy_terms(vars, gamma, gm2=None, ops=None):
    """Marginal/MHD_Residuals_CP.py:247-256 (``oracle.residuals.mhd_energy``), uncropped.  ``gm2``: the factor ``gamma - 2``
    (the kernels fold it on the host), by default from ``gamma``."""
    o = ops or orr.Ops2D()
    D_t, D_x, D_y = o.D_t, o.D_x, o.D_y
    rho, u, v, p, Bx, By = (vars[:, i] for i in range(6))
    gm2 = gamma - 2 if gm2 is None else gm2
    p_gas = p - 0.5*(Bx**2 + By**2)
    return {"Dt(rho)": D_t(rho), "uDx(p)": u*D_x(p), "vDy(p)": v*D_y(p),
            "(gamma-2)(uBx+vBy)divB": gm2*(u*Bx+v*By)*(D_x(Bx) + D_y(By)),
            "gamma p_gas Dx(u)": gamma*p_gas*D_x(u), "By^2 Dx(u)": By**2*D_x(u),
            "gamma p_gas Dy(v)": gamma*p_gas*D_y(v), "Bx^2 Dy(v)": Bx**2*D_y(v),
            "-BxBy(Dy(u)+Dx(v))": -Bx*By*(D_y(u) + D_x(v))}


def mhd_energy_ref(vars, coef=MHD):
    return orr.mhd_energy(vars, gamma=coef["gamma"], boundary=True)


def _mhd_mutants():
    g, g0 = MHD["gamma"], MHD_DEFAULT["gamma"]
    out = [("gamma at its default", lambda v: total(mhd_energy_terms(v, g0))),
           ("gamma - 2 from the default gamma", lambda v: total(mhd_energy_terms(v, g, gm2=g0 - 2))),
           ("gamma at its default, gamma - 2 right", lambda v: total(mhd_energy_terms(v, g0, gm2=g - 2))),
           ("gamma in the slot of gamma - 2", lambda v: total(mhd_energy_terms(v, g, gm2=g)))]
    names = list(mhd_energy_terms(torch.zeros(1, 6, 3, 3, 4), g))
    out += [("dropped " + n, lambda v, n=n: total(mhd_energy_terms(v, g), n)) for n in names]
    return out


# ------------------------------------------------------------------------------------------------ JOREK
def jorek_ops(opset="default", coef=JOREK, rescale=None):
    """The oracle's five operators for ``coef`` (``lap_scale``, ``gamma``) with the tap structure of ``opset``; 'rescaled'
    (or ``rescale``, a dict) multiplies the kernels after construction, as a caller replaces ``.kernel``."""
    o = orr.OpsJorek(lap_scale=coef.get("lap_scale"), gamma=coef.get("gamma", 5 / 3))
    if opset == "yfix":
        for op in (o.D_Z, o.D_ZZ):
            op.kernel = op.kernel.permute(2, 1, 0).contiguous()
    elif opset == "general":
        o.D_R.kernel = sj.general_kernel(o.D_R.kernel)
    rescale = jh.RESCALE if (rescale is None and opset == "rescaled") else rescale
    for a, s in (rescale or {}).items():
        getattr(o, a).kernel = getattr(o, a).kernel * s
    return o


def y_parts(f, R, c, o, radial="1/R"):
    """The three parts of ``c * (D_RR(f) + (1/R) D_R(f) + D_ZZ(f))``; ``radial='R'``: the mistake ``R`` for ``1/R``."""
    return {"c D_RR": c * o.D_RR(f), "(c/R) D_R": c * ((1/R if radial == "1/R" else R) * o.D_R(f)), "c D_ZZ": c * o.D_ZZ(f)}


def jorek_continuity_terms(vars, R, D, ops, norms=False, dx=None, dy=None, dt=None, radial="1/R"):
    """Marginal/JOREK_residuals_CP.py:207-221 (``oracle.residuals.jorek_continuity``), uncropped."""
    o = ops
    rho, phi, _ = orr.jorek_unstack(vars)
    D = f32(D)
    a0, a1, a2, a3 = (2*dx*dy, dt, (2*dt*dy)*2, (4*dt)*D) if norms else (1.0, 1.0, 2.0, D)
    out = {"a0 Dt(rho)": a0*o.D_t(rho), "-a1 R DR(rho)DZ(phi)": -(a1*R*(o.D_R(rho)*o.D_Z(phi))),
           "+a1 R DR(phi)DZ(rho)": a1*R*(o.D_R(phi)*o.D_Z(rho)), "-a2 rho DZ(phi)": -(a2*rho*o.D_Z(phi))}
    out.update({"-" + k.replace("c", "a3"): -t for k, t in y_parts(rho, R, a3, o, radial).items()})
    return out


def jorek_temperature_terms(vars, R, K, gamma, ops, y_of="T", radial="1/R"):
    """Marginal/JOREK_residuals_CP.py:224-243 (``oracle.residuals.jorek_temperature``), uncropped.  ``y_of='rho'``: the
    mistake of ``Y`` reading ``rho``."""
    o = ops
    rho, phi, T = orr.jorek_unstack(vars)
    K, gamma = f32(K), f32(gamma)
    out = {"T Dt(rho)": T*o.D_t(rho), "rho Dt(T)": rho*o.D_t(T), "-rho R DR(T)DZ(phi)": -(rho*R*(o.D_R(T)*o.D_Z(phi))),
           "+rho R DR(phi)DZ(T)": rho*R*(o.D_R(phi)*o.D_Z(T)), "+T R DR(rho)DZ(phi)": T*R*(o.D_R(rho)*o.D_Z(phi)),
           "-T R DR(phi)DZ(rho)": -(T*R*(o.D_R(phi)*o.D_Z(rho))), "2 gamma rho T DZ(phi)": 2*gamma*rho*T*o.D_Z(phi)}
    out.update({k.replace("c", "K"): t for k, t in y_parts(T if y_of == "T" else rho, R, K, o, radial).items()})
    return out


Y_PARTS = ("K D_RR", "(K/R) D_R", "K D_ZZ")


def jorek_ref(kind, vars, R, opset="default", coef=JOREK, norms=False, rescale=None):
    """The oracle's uncropped residual of ``vars`` [BS,3,Nx,Ny,Nt] with ``coef`` on the operators of ``opset``."""
    o = jorek_ops(opset, coef, rescale)
    if kind == "jorek_continuity":
        kw = {k: f32(v) for k, v in NORMS.items()} if norms else {}
        return orr.jorek_continuity(vars, R, coef.get("D", 3.4), boundary=True, norms=norms, ops=o, **kw)
    return orr.jorek_temperature(vars, R, coef.get("K", 2.25 * 1e-7), coef.get("gamma", 5 / 3), boundary=True, ops=o)


def _jorek_terms(kind, v, R, opset, coef=JOREK, norms=False, rescale=None, **kw):
    o = jorek_ops(opset, coef, rescale)
    if kind == "jorek_continuity":
        n = {k: f32(x) for k, x in NORMS.items()} if norms else {}
        return jorek_continuity_terms(v, R, coef["D"], o, norms, **n, **kw)
    return jorek_temperature_terms(v, R, coef["K"], coef["gamma"], o, **kw)


def _jorek_mutants(kind, norms=False):
    """Callables ``(vars, R, opset)``.  The coefficients ``lap_scale`` / ``gamma`` reach the continuity equation only
    through the operators (``lap_scale=None`` is the ``gamma`` the object was given)."""
    c = JOREK
    T = lambda **kw: (lambda v, R, opset: total(_jorek_terms(kind, v, R, opset, norms=norms, **kw)))      # noqa: E731
    out = [("lap_scale at its default", T(coef={**c, "lap_scale": None})),
           ("1/R replaced by R", T(radial="R"))]
    out += [("kernel of %s not rescaled" % a, (lambda v, R, opset, a=a: total(_jorek_terms(
        kind, v, R, opset, norms=norms, rescale={k: s for k, s in jh.RESCALE.items() if k != a})))) for a in jh.RESCALE]
    if kind == "jorek_continuity":
        out.append(("D at its default", T(coef={**c, "D": JOREK_DEFAULT["D"]})))
        out.append(("K in the slot of D", T(coef={**c, "D": c["K"]})))
        if norms:
            n = {k: f32(x) for k, x in NORMS.items()}
            for a, b in (("dx", "dy"), ("dy", "dt"), ("dx", "dt")):
                sw = {**n, a: n[b], b: n[a]}
                out.append(("%s and %s swapped" % (a, b), lambda v, R, opset, sw=sw: total(jorek_continuity_terms(
                    v, R, c["D"], jorek_ops(opset), True, **sw))))
            out.append(("norms ignored", lambda v, R, opset: total(_jorek_terms(kind, v, R, opset, norms=False))))
    else:
        out.append(("K at its default", T(coef={**c, "K": JOREK_DEFAULT["K"]})))
        out.append(("gamma at its default", T(coef={**c, "gamma": JOREK_DEFAULT["gamma"]})))
        out.append(("D in the slot of K", T(coef={**c, "K": c["D"]})))
        out.append(("2 gamma in the slot of K (coef[0] for coef[3])", T(coef={**c, "K": 2 * c["gamma"]})))
        out.append(("Y reads rho", T(y_of="rho")))
    v0, R0 = torch.zeros(1, 3, 3, 4, 3), torch.ones(4)
    for n in _jorek_terms(kind, v0, R0, "default", norms=norms):
        out.append(("dropped " + n, lambda v, R, opset, n=n: total(_jorek_terms(kind, v, R, opset, norms=norms), n)))
    return out


def rescale_applies(name, opset):
    """The mutants 'kernel of X not rescaled' are mistakes of the rescaled operator set only."""
    return opset == "rescaled" or "not rescaled" not in name


MUTANTS = {"ns_momentum": _ns_mutants(), "mhd_energy": _mhd_mutants(),
           "jorek_continuity": _jorek_mutants("jorek_continuity"),
           "jorek_continuity_norms": _jorek_mutants("jorek_continuity", True),
           "jorek_temperature": _jorek_mutants("jorek_temperature")}


def y_mutants(coef=JOREK_DEFAULT):
    """The mutants of ``a3*Y(T)`` alone, for the ``rho = 0`` input at ``coef`` (the defaults): callables (vars, R, opset)."""
    T = lambda drop=(), **kw: (lambda v, R, opset: total(_jorek_terms("jorek_temperature", v, R, opset, coef=coef, **kw), drop))      # noqa: E731
    out = [("dropped " + n, T(drop=n)) for n in Y_PARTS]
    out += [("Y reads rho", T(y_of="rho")), ("1/R replaced by R", T(radial="R")),
            ("K = 0", lambda v, R, opset: total(_jorek_terms("jorek_temperature", v, R, opset, coef={**coef, "K": 0.0}))),
            ("2 gamma in the slot of K", lambda v, R, opset: total(_jorek_terms(
                "jorek_temperature", v, R, opset, coef={**coef, "K": 2 * coef["gamma"]}))),
            ("lap_scale 1 in place of gamma", lambda v, R, opset: total(_jorek_terms(
                "jorek_temperature", v, R, opset, coef={**coef, "lap_scale": 1.0})))]
    return out


# ------------------------------------------------------------------------------------------------ inputs
def rel_err(a, b):
    """``conftest.rel_err`` for tensors: max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (d if d > 0 else 1.0))


def fields2d(nchan, shape, seed=0):
    """``rand + 0.5`` [B,F,T,X,Y] float32 (the inputs of the parity tests)."""
    B, T, X, Y = shape
    return torch.rand(B, nchan, T, X, Y, generator=torch.Generator().manual_seed(1000 * seed + sum(shape) + nchan)) + 0.5


def jorek_vars(shape, seed=0, rho0=False):
    """``rand + 0.5`` ``vars`` [B,3,N,N,Nt] float32 for (B, N, Nt); ``rho0``: with ``rho = 0`` exactly."""
    B, N, Nt = shape
    v = torch.rand(B, 3, N, N, Nt, generator=torch.Generator().manual_seed(1000 * seed + sum(shape))) + 0.5
    if rho0:
        v[:, 0] = 0.0
    return v


def zero_rho(x):
    """The logical [B,3,T,X,Y] fields with ``rho = 0`` exactly (a copy)."""
    x = x.clone()
    x[:, 0] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ the screen cases
def _first_seed(key, build, holds):
    """The case of ``key`` at the first seed of 0..5 that meets its caps (as ``screenjorek_helpers.case`` takes its seed):
    built once, shared, left unchanged."""
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


def screen2d_case(kind, shape, boundary):
    """The 2-D screen case of ``kind`` at ``COEF[kind]``: ``screen_helpers.Case`` under the caps of tests/test_screen_cpu.py."""
    return _first_seed(("2d", kind, tuple(shape), boundary),
                       lambda seed: sh.Case(kind, shape, boundary, True, 10, seed=seed, coef=COEF[kind]), sj.caps_hold)


def pair_case(kind, form, boundary):
    """The data-driven case of ``kind`` at ``COEF[kind]``: ``screenpair_helpers.PairCase`` under its own caps."""
    shape = sp.NY_BASE if form == "ny" else sp.FLAT_BASE
    return _first_seed(("pair", kind, shape, boundary), lambda seed: sp.PairCase(
        kind, shape, boundary, True, sp.NK[form], seed=seed, coef=COEF[kind]), lambda c: c.caps_hold()[0])


def jorek_screen_case(kind, shape, boundary, mode=None, rho0=False):
    """The JOREK screen case: ordinary fields at ``JOREK``, or ``rho = 0`` at the default coefficients."""
    return sj.case(kind, shape, boundary, mode=mode, **(dict(rho0=True) if rho0 else dict(coef=JOREK)))


def jorek_screen_cases():
    """Every (kind, form, shape, boundary, mode, rho0) tests/test_gpu_terms.py screens."""
    for form, shapes in SCREEN_JOREK.items():
        for shape in shapes:
            for boundary in (False, True):
                for kind in sj.KINDS:
                    yield kind, form, shape, boundary, None, False
                yield "jorek_temperature", form, shape, boundary, None, True
        for mode in sj.MODES:
            yield "jorek_temperature", form, STAGED_JOREK[form], False, mode, False
            yield "jorek_temperature", form, STAGED_JOREK[form], False, mode, True


def screen2d_cases():
    """Every (kind, form, shape, boundary) of the 2-D screens tests/test_gpu_terms.py runs."""
    for kind in SCREEN_KINDS:
        for form, shapes in SCREEN2D.items():
            for shape in shapes:
                for boundary in (False, True):
                    yield kind, form, shape, boundary


_cases = {}


# ------------------------------------------------------------------------------------------------ the backward cases
VJP_NY_SHAPE = (2, 17, 5, 12)                # losses_helpers.SEAM_SHAPES["tseg"][0]: two marches of the Ny-fastest kernels
VJP_FLAT_SHAPE = (2, 10, 5, 6)               # vjpflat_helpers.SEAM_SHAPES["straddle_10"]: row ends inside quads


def vjp_route(name, chosen=True):
    """The existing route object of a backward case - ``losses_helpers.Route('ns_momentum')``, ``mhdvjp_helpers.MHDRoute(
    'energy')``, ``jorekvjp_helpers.JorekRoute('continuity', 6)`` - with its package object's coefficients set to this
    file's (``chosen=False``: left at the defaults the existing tests run).  Their fp64 references read the coefficients
    from that object, as the package does."""
    from losses_helpers import Route
    from mhdvjp_helpers import MHDRoute
    if name == "ns_momentum":
        r, coef = Route("ns_momentum"), NS
    elif name == "mhd_energy":
        r, coef = MHDRoute("energy"), MHD
    else:
        r, coef = jh.JorekRoute("continuity", VJP_FLAT_SHAPE[3]), {"D": JOREK["D"]}
    if chosen:
        for k, v in coef.items():
            assert hasattr(r.obj, k), k
            setattr(r.obj, k, v)
    return r


VJP_ROUTES = ("ns_momentum", "mhd_energy", "jorek_continuity")
