"""The fused residuals term by term and off their default coefficients, on the GPU (pytest -m gpu; tests/TERMS_TESTS.md).

Reference: the oracle in float64 (``terms_helpers``, ``screen_helpers.oracle_fp64``).  Tolerance: the project's
``RES_TOL = 1e-5`` on ``rel_err = max |got - want| / max |want|``; the screens keep the assertions of their own files (score
within tau / m_min + one ulp, counts within the undecided cells, accept exact), the backward cases the fp64 references and
TOL of their helpers.  tests/test_terms_cpu.py shows, from the oracle alone, that at the coefficients and on the inputs used
here every mistake of ``terms_helpers.MUTANTS`` - a coefficient at its default or in another's slot, a term dropped, ``Y``
reading ``rho``, ``R`` for ``1/R`` - moves the residual by at least 100 x RES_TOL; and that on the ``rho = 0`` input the
temperature residual is ``a3*Y(T)`` alone, so that at the default ``K`` the metric is on that term's own scale.

Every fused row is the fused kernel: the entry points are counted with their return codes (a decline would compose)."""
import numpy as np
import pytest
import torch

import jorekvjp_helpers as jh
import screen_helpers as sh
import screenflat_helpers as sf
import screenjorek_helpers as sj
import screenpair_helpers as sp
import terms_helpers as th
import vjpflat_helpers as vf
import vjpflatmhd_helpers as fh
from losses_helpers import channel_errs, ref_vjp, seam_inputs
from test_gpu_pair import _scaled_err
from test_gpu_screenjorek import check_against_ref, route_of as jorek_route, run as run_jorek_screen

pytestmark = pytest.mark.gpu
RES_TOL = th.RES_TOL
_refs, _worst = {}, {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def held(group, err, what):
    """assert ``err <= RES_TOL``; keep and print the group's largest"""
    _worst[group] = max(_worst.get(group, 0.0), err)
    print(f"{what}: rel_err {err:.3e}   [largest of '{group}': {_worst[group] / RES_TOL:.3f} x RES_TOL]")
    assert err <= RES_TOL, (group, what, err)


def counted(monkeypatch, lib, name):
    """The return codes of every call of entry ``name`` of the loaded library ``lib`` from here on."""
    codes, real = [], getattr(lib, name)
    monkeypatch.setattr(lib, name, lambda *a: (codes.append(real(*a)), codes[-1])[1])
    return codes


def ny_fastest(v):
    """the dense ``vars`` [B,3,Nx,Ny,Nt] as a view of memory [B,3,Nt,Nx,Ny]: Ny-fastest field views"""
    out = v.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
    assert out.stride(3) == 1 and torch.equal(out, v)
    return out


# ------------------------------------------------------------------ 1, 2. the JOREK residual pass, every forward route
def jorek_object(ny, opset, coef, norms, device, fused=True):
    c = dict(coef, **th.NORMS) if norms else dict(coef)
    mode = opset if opset in sj.MODES else None
    return sj.jorek_of(mode, device, ny, fused, coef=c, rescale=jh.RESCALE if opset == "rescaled" else None)


def jorek_reference(kind, shape, seed, rho0, opset, coef, norms):
    key = (kind, shape, seed, rho0, opset, tuple(coef.items()), norms)
    if key not in _refs:
        v = th.jorek_vars(shape, seed, rho0).double()
        with sh.oracle_fp64():
            _refs[key] = th.jorek_ref(kind, v, sj.radius(shape[1]).double(), opset, coef, norms).numpy()
    return _refs[key]


def jorek_routes(gpu, monkeypatch, kind, norms, coef, rho0, group):
    from cp_pre_amd import _lib
    codes = counted(monkeypatch, _lib.load(), "pre_residual_jorek_f32")
    crop = (slice(None),) + (slice(1, -1),) * 3
    fused_calls = 0

    def call(j, x, **kw):
        if norms:
            kw["norms"] = True
        return getattr(j, "residual_" + kind[len("jorek_"):])(x, **kw)
    for i, shape in enumerate(th.JOREK_SHAPES):
        B, N, Nt = shape
        v, w = th.jorek_vars(shape, 0, rho0), th.jorek_vars(shape, 1, rho0)
        layouts = {"Nt-fastest": (v.to(gpu), w.to(gpu)), "Ny-fastest": (ny_fastest(v.to(gpu)), ny_fastest(w.to(gpu)))}
        assert layouts["Nt-fastest"][0].is_contiguous() and bool(v[:, 0].any()) != rho0
        for opset in (th.OPSETS if i == 0 else ("default",)):
            ra = jorek_reference(kind, shape, 0, rho0, opset, coef, norms)
            assert ra.shape == (B, Nt, N, N) and np.abs(ra).max() > 0
            j = jorek_object(N, opset, coef, norms, gpu)
            for name, (x, xm) in layouts.items():
                what = f"{kind} norms={norms} {shape} {opset} {name}"
                got = call(j, x, boundary=True)
                assert got.is_cuda and tuple(got.shape) == ra.shape
                held(group, th.rel_err(got.cpu().numpy(), ra), what + " boundary=True")
                fused_calls += 1
                if opset != "default":
                    continue
                got = call(j, x)
                assert tuple(got.shape) == ra[crop].shape
                held(group, th.rel_err(got.cpu().numpy(), ra[crop]), what + " boundary=False")
                got = call(j, x, boundary=True, absolute=True)
                assert bool((got >= 0).all())
                held(group, th.rel_err(got.cpu().numpy(), np.abs(ra)), what + " absolute")
                rb = jorek_reference(kind, shape, 1, rho0, opset, coef, norms)
                got = call(j, x, boundary=True, minus=xm)
                held(group, _scaled_err(got.cpu().numpy(), ra, rb), what + " minus= (scaled as test_gpu_pair)")
                fused_calls += 4
            if opset == "default":
                before = len(codes)
                got = call(jorek_object(N, opset, coef, norms, gpu, fused=False), layouts["Nt-fastest"][0], boundary=True)
                assert len(codes) == before
                held(group, th.rel_err(got.cpu().numpy(), ra), f"{kind} norms={norms} {shape} fused=False")
    assert len(codes) == fused_calls and not any(codes), codes      # every fused row WAS the fused kernel (PRE_OK)


@pytest.mark.parametrize("scenario", ["off_defaults", "rho0_at_the_default_K"])
def test_jorek_temperature_every_forward_route(gpu, monkeypatch, scenario):
    """``K = K_BIG`` with the whole coefficient set, and the isolating input ``rho = 0`` at the default ``K`` (the residual
    is ``a3*Y(T)``, 1e-6 in size: ``rel_err`` is on that term's own scale)"""
    if scenario == "off_defaults":
        jorek_routes(gpu, monkeypatch, "jorek_temperature", False, th.JOREK, False, "JOREK temperature, off the defaults")
    else:
        jorek_routes(gpu, monkeypatch, "jorek_temperature", False, th.JOREK_DEFAULT, True, "JOREK temperature, rho = 0 at the default K")


@pytest.mark.parametrize("norms", [False, True])
def test_jorek_continuity_every_forward_route(gpu, monkeypatch, norms):
    jorek_routes(gpu, monkeypatch, "jorek_continuity", norms, th.JOREK, False, "JOREK continuity%s, off the defaults" % (" norms" if norms else ""))


# ------------------------------------------------------------------ 3. screen(..., jorek=True), both forms
@pytest.mark.parametrize("which", ["off_defaults", "rho0_at_the_default_K"])
@pytest.mark.parametrize("form", ["flat", "ny"])
def test_screenjorek_off_the_defaults_and_on_the_k_term_alone(gpu, form, which):
    """``pre_screenjorek_flat_f32`` ('flat') and ``pre_screenjorek_f32`` ('ny') with the coefficient set, and with ``rho = 0``
    at the default ``K``: there tau = 1e-5 max |r_ref| is 1e-5 of the K term."""
    from cp_pre_amd import screen
    n = 0
    for kind, f, shape, boundary, mode, rho0 in th.jorek_screen_cases():
        if f != form or rho0 != (which != "off_defaults"):
            continue
        case = th.jorek_screen_case(kind, shape, boundary, mode, rho0)
        method = sj.method_of(kind, mode, gpu, ny=shape[3], coef=None if rho0 else th.JOREK)
        s = run_jorek_screen(case, gpu, form, method=method)
        assert screen.last_route() == jorek_route(kind, form)
        check_against_ref(case, s, f"{kind} {form} {shape} boundary={boundary} mode={mode} rho0={rho0} (seed {case.seed})")
        n += 1
    assert n == (10 if which == "off_defaults" else 6)


# ------------------------------------------------------------------ 4. NS momentum and MHD energy off their defaults
KINDS_2D = {"ns_momentum": (3, "residual_momentum", "pre_residual_ns_momentum_f32", th.ns_momentum_ref),
            "mhd_energy": (6, "residual_energy", "pre_residual_mhd_f32", th.mhd_energy_ref)}


def reference_2d(kind, shape, seed):
    key = (kind, shape, seed)
    if key not in _refs:
        with sh.oracle_fp64():
            _refs[key] = KINDS_2D[kind][3](th.fields2d(KINDS_2D[kind][0], shape, seed).double()).numpy()
    return _refs[key]


@pytest.mark.parametrize("kind", list(KINDS_2D))
def test_2d_residual_and_paired_pass_off_the_defaults(gpu, monkeypatch, kind):
    """``nu = 0.02`` (with dt, dx, dy all different) / ``gamma = 1.4`` through the residual pass - Ny-fastest, Nt-fastest, an
    x-slab with ``halo_x``, ``out=`` - and ``minus=`` (NS: one launch of ``pre_pair_ns_momentum_f32``; MHD energy: two
    passes).  The 66-wide shape streams in no whole quads: both layouts compose there, with the same scalars."""
    from cp_pre_amd import _lib
    nchan, mname, entry, _ = KINDS_2D[kind]
    group = kind + " residual pass, off the defaults"
    single = counted(monkeypatch, _lib.load(), entry)
    paired = counted(monkeypatch, _lib.load_pair(), "pre_pair_ns_momentum_f32")
    m = sh.method_of(kind, gpu, coef=th.COEF[kind])
    assert m.__name__ == mname
    for shape in th.NY_SHAPES:
        B, T, X, Y = shape
        v, w = th.fields2d(nchan, shape), th.fields2d(nchan, shape, seed=1)
        ra, rb = reference_2d(kind, shape, 0), reference_2d(kind, shape, 1)
        n_single, n_paired, want_single, want_paired = len(single), len(paired), 0, 0
        for name, x, xm in (("Ny-fastest", v.to(gpu), w.to(gpu)), ("Nt-fastest", vf.nt_fastest(v, gpu), vf.nt_fastest(w, gpu))):
            assert (x.stride(-1) == 1) == (name == "Ny-fastest") and (x.stride(2) == 1) == (name == "Nt-fastest")
            what = f"{kind} {shape} {name}"
            held(group, th.rel_err(m(x, boundary=True).cpu().numpy(), ra), what + " boundary=True")
            held(group, th.rel_err(m(x).cpu().numpy(), ra[:, 1:-1, 1:-1, 1:-1]), what + " boundary=False")
            held(group, th.rel_err(m(x, boundary=True, absolute=True).cpu().numpy(), np.abs(ra)), what + " absolute")
            held(group, _scaled_err(m(x, boundary=True, minus=xm).cpu().numpy(), ra, rb), what + " minus=")
            want_single += 3 + (2 if kind == "mhd_energy" else 0)
            want_paired += kind == "ns_momentum"
        if Y % 4 != 0:
            # no whole quads to stream: every entry was asked and declined, the rows above are the composed route's
            assert single[n_single:] and all(c == _lib.PRE_E_UNSUPPORTED for c in single[n_single:] + paired[n_paired:])
            continue
        x = v.to(gpu)
        out = torch.full((B, T, X, Y), float("nan"), device=gpu)
        got = m(x, boundary=True, out=out)
        assert got.data_ptr() == out.data_ptr()
        held(group, th.rel_err(out.cpu().numpy(), ra), f"{kind} {shape} out=")
        x0, x1 = 3, 8
        got = m(x[:, :, :, x0:x1], boundary=True, halo_x=True)
        held(group, th.rel_err(got.cpu().numpy(), ra[:, :, x0:x1]), f"{kind} {shape} halo_x slab [{x0}:{x1}]")
        # every row of this shape WAS the fused kernel: the entries' counts and their return codes (PRE_OK)
        assert single[n_single:] == [0] * (want_single + 2), (single[n_single:], want_single)
        assert paired[n_paired:] == [0] * want_paired, (paired[n_paired:], want_paired)


def test_gamma_reaches_the_energy_equation_alone(gpu):
    """the other three equations of ``pre_residual_mhd_f32`` take ``gamma`` and must not use it: bit for bit the default's"""
    from cp_pre_amd import residuals as R
    x = th.fields2d(6, th.NY_SHAPES[0]).to(gpu)
    a, b = R.MHD(gamma=th.MHD["gamma"], device=gpu), R.MHD(device=gpu)
    for eq in ("continuity", "momentum", "induction"):
        assert torch.equal(getattr(a, "residual_" + eq)(x, True), getattr(b, "residual_" + eq)(x, True)), eq
    assert not torch.equal(a.residual_energy(x, True), b.residual_energy(x, True))


def put(t, form, device):
    return sf.to_layout(t, device) if form == "flat" else t.to(device)


@pytest.mark.parametrize("form", ["march", "flat"])
@pytest.mark.parametrize("kind", th.SCREEN_KINDS)
def test_2d_screens_off_the_defaults(gpu, kind, form):
    """``pre_screen_*`` (Ny-fastest: the march) and ``pre_screenflat_*`` (Nt-fastest) with the scalars of ``_method``"""
    from cp_pre_amd import screen
    for shape in th.SCREEN2D[form]:
        for boundary in (False, True):
            case = th.screen2d_case(kind, shape, boundary)
            s = screen.screen(sh.method_of(kind, gpu, coef=th.COEF[kind]), put(case.x, form, gpu), case.q.to(gpu),
                              put(case.mod, form, gpu), boundary=boundary)
            assert screen.last_route() == "fused:" + ("flat_" if form == "flat" else "") + sh.FUSED_KIND[kind]
            check_against_ref(case, s, f"{kind} {form} {shape} boundary={boundary} (seed {case.seed})")


@pytest.mark.parametrize("form", ["ny", "flat"])
@pytest.mark.parametrize("kind", th.SCREEN_KINDS)
def test_data_driven_screens_off_the_defaults(gpu, kind, form):
    """``pair=True``: NS momentum in one launch of ``pre_screenpair[_flat]_ns_momentum_f32``; MHD energy has no paired screen
    and says so - its three passes carry ``gamma`` through the two-pass residual"""
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = th.pair_case(kind, form, boundary)
        s = screen.screen(sh.method_of(kind, gpu, coef=th.COEF[kind]), put(case.x, form, gpu), case.q.to(gpu),
                          put(case.mod, form, gpu), boundary=boundary, minus=put(case.y, form, gpu), pair=True)
        assert screen.last_route() == (sp.route(kind, form) if kind in sp.KINDS else "fallback:" + sp.UNPAIRED[kind])
        check_against_ref(case, s, f"{kind} pair {form} boundary={boundary} (seed {case.seed})")


# ------------------------------------------------------------------ 5. backward, one case each
def vjp_held(route, got, want, what):
    errs = channel_errs(got, want)
    print(f"{route.name} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= jh.TOL, (route.name, what, k, v)
    _worst["backward"] = max(_worst.get("backward", 0.0), max(errs.values()))
    print(f"   [largest of 'backward': {_worst['backward'] / jh.TOL:.3f} x TOL]")


@pytest.mark.parametrize("boundary", [False, True])
def test_backward_off_the_defaults(gpu, boundary):
    """The NS loss VJP (nu = 0.02, dt, dx, dy of ``terms_helpers.NS``) and the MHD-energy VJP (gamma = 1.4) in both layouts,
    the JOREK continuity VJP (D = 1.7): the helpers' fp64 autograd references, which read the coefficients off the package
    object, and their TOL"""
    from cp_pre_amd import losses
    for name, kw, kind in (("ns_momentum", {}, "ns_momentum"), ("mhd_energy", {"mhd": True}, "mhd_energy")):
        route = th.vjp_route(name)
        x, g = seam_inputs(route, th.VJP_NY_SHAPE, boundary)
        want = ref_vjp(route, x.double(), g.double(), boundary)
        got = losses.residual_vjp(route.method, x.to(gpu), g.to(gpu), boundary=boundary, **kw)
        assert losses.last_route() == "fused:" + kind, losses.last_route()
        vjp_held(route, got, want, f"Ny-fastest {th.VJP_NY_SHAPE} boundary={boundary}")
        x, g = seam_inputs(route, th.VJP_FLAT_SHAPE, boundary)
        want = ref_vjp(route, x.double(), g.double(), boundary)
        xd = fh.nt_fastest_exact(x, gpu)
        got = losses.residual_vjp(route.method, xd, g.to(gpu), boundary=boundary, **({"mhd": "flat"} if kw else {"flat": True}))
        assert losses.last_route() == "fused:flat_" + kind, losses.last_route()
        vjp_held(route, got, want, f"Nt-fastest {th.VJP_FLAT_SHAPE} boundary={boundary}")
    route = th.vjp_route("jorek_continuity")
    assert route.coef()[3] == float(th.f32(th.JOREK["D"]))
    x, g = seam_inputs(route, th.VJP_FLAT_SHAPE, boundary)
    want = ref_vjp(route, x.double(), g.double(), boundary)
    got = losses.residual_vjp(route.method, jh.vars_on(x, gpu), g.to(gpu), boundary=boundary, jorek=True)
    assert losses.last_route() == "fused:flat_jorek_continuity", losses.last_route()
    vjp_held(route, jh.to_logical(got), want, f"{th.VJP_FLAT_SHAPE} boundary={boundary}")
