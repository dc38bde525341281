"""The conditions tests/test_gpu_terms.py rests on, from the oracle alone (no GPU; tests/TERMS_TESTS.md):
  * the per-term restatements of ``terms_helpers`` sum to ``oracle.residuals``' functions (fp64);
  * every mutant - a coefficient at its default or in another's slot, a term dropped, a ``Y`` part dropped, ``Y`` reading
    ``rho``, ``R`` for ``1/R`` - moves the residual by ``rel_err >= 1e-3 = 100 * RES_TOL`` on every input family the GPU
    file uses, at the coefficients it uses: a kernel or host entry with that mistake cannot meet ``RES_TOL`` there;
  * why the suite was blind before: at the default ``K`` on the parity test's inputs, ``K = 0`` stays under ``RES_TOL``;
  * every screen case of the GPU file meets the caps its tolerances rest on."""
import inspect

import numpy as np
import pytest
import torch

import screen_helpers as sh
import screenjorek_helpers as sj
import terms_helpers as th
from oracle import residuals as orr


def _close(got, want, scale):
    """``rtol 1e-12``, and ``1e-12`` of the largest term for the cells where the terms cancel: a sum of a dozen fp64 terms
    of size ``scale`` carries a rounding of a few 1e-16 * scale whatever its own size."""
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-12 * scale)


def _scale(terms):
    return max(float(t.abs().max()) for t in terms.values())


def _visible(name, mutant, ref, seen):
    e = th.rel_err(mutant, ref)
    seen[name] = min(seen.get(name, np.inf), e)
    assert e >= th.VISIBLE, (name, e)


def _report(title, seen):
    print(title)
    for name, e in seen.items():
        print(f"  {name:55s} {e:.3g}")


# ------------------------------------------------------------------ the defaults are the package's
def test_the_defaults_the_mutants_fall_back_to_are_the_constructors():
    from cp_pre_amd import residuals as R
    sig = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items()}      # noqa: E731
    assert sig(R.NavierStokes.__init__)["nu"] == th.NS_DEFAULT["nu"] == sh.NS_NU
    assert sig(R.MHD.__init__)["gamma"] == th.MHD_DEFAULT["gamma"]
    j = sig(R.JOREK.__init__)
    assert {k: j[k] for k in th.JOREK_DEFAULT} == th.JOREK_DEFAULT and (j["alpha"], j["beta"]) == (1, 1)
    o = sig(orr.jorek_continuity), sig(orr.jorek_temperature)
    assert (o[0]["D"], o[1]["K"], o[1]["gamma"]) == tuple(th.JOREK_DEFAULT[k] for k in ("D", "K", "gamma"))
    # every chosen coefficient that has a default is off it, and no two NS / norms scalars share a value
    for chosen, default in ((th.NS, th.NS_DEFAULT), (th.MHD, th.MHD_DEFAULT), (th.JOREK, th.JOREK_DEFAULT)):
        assert all(chosen[k] != default[k] for k in default)
    assert len(set(th.NS.values())) == 4 and len(set(th.NORMS.values())) == 3 and th.JOREK["lap_scale"] != th.JOREK["gamma"]


# ------------------------------------------------------------------ the term sums
@pytest.mark.parametrize("shape", th.NY_SHAPES)
def test_ns_and_mhd_terms_sum_to_the_oracle(shape):
    with sh.oracle_fp64():
        v = th.fields2d(3, shape).double()
        for coef in (th.NS, {**th.NS, **th.NS_DEFAULT}):
            t = th.ns_momentum_terms(v, **coef)
            assert len(t) == 10
            _close(th.total(t), th.ns_momentum_ref(v, coef), _scale(t))
        v = th.fields2d(6, shape).double()
        for coef in (th.MHD, th.MHD_DEFAULT):
            t = th.mhd_energy_terms(v, **coef)
            _close(th.total(t), th.mhd_energy_ref(v, coef), _scale(t))


@pytest.mark.parametrize("opset", th.OPSETS)
def test_jorek_terms_sum_to_the_oracle(opset):
    shape = th.JOREK_SHAPES[0]
    R = sj.radius(shape[1]).double()
    with sh.oracle_fp64():
        for rho0 in (False, True):
            v = th.jorek_vars(shape, rho0=rho0).double()
            for coef in (th.JOREK, th.JOREK_DEFAULT):
                for kind, norms in (("jorek_continuity", False), ("jorek_continuity", True), ("jorek_temperature", False)):
                    t = th._jorek_terms(kind, v, R, opset, coef=coef, norms=norms)
                    assert set(th.Y_PARTS) <= set(t) or kind == "jorek_continuity"
                    _close(th.total(t), th.jorek_ref(kind, v, R, opset, coef, norms), _scale(t))
                # rho = 0: the temperature residual is a3*Y(T) and nothing else, the continuity residual exactly 0
                if rho0:
                    t = th._jorek_terms("jorek_temperature", v, R, opset, coef=coef)
                    assert all(not bool(x.any()) for k, x in t.items() if k not in th.Y_PARTS)
                    assert bool(th.total(t).any())
                    assert not bool(th.jorek_ref("jorek_continuity", v, R, opset, coef).any())


def test_rho_zero_isolates_the_k_term_in_the_fp32_oracle_bit_for_bit():
    """at the default K, in the oracle's own fp32: the residual of the rho = 0 input is K*(D_RR(T) + (1/R) D_R(T) + D_ZZ(T))
    to the bit, 1.7e-6 at its largest on (2, 12, 10)"""
    v = th.jorek_vars((2, 12, 10), rho0=True)
    R = sj.radius(12)
    o = orr.OpsJorek()
    T = orr.jorek_unstack(v)[2]
    want = th.f32(2.25 * 1e-7) * (o.D_RR(T) + (1/R)*o.D_R(T) + o.D_ZZ(T))
    got = orr.jorek_temperature(v, R, boundary=True)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert 1e-6 < float(got.abs().max()) < 3e-6


# ------------------------------------------------------------------ visibility: a condition, not a measurement
def _inputs_2d(kind, nchan):
    """name -> float64 [B,F,T,X,Y]: every input family tests/test_gpu_terms.py hands ``kind``"""
    out = {f"rand+0.5 {s}": th.fields2d(nchan, s).double() for s in th.NY_SHAPES}
    out.update({f"rand+0.5 second set {s}": th.fields2d(nchan, s, seed=1).double() for s in th.NY_SHAPES})
    for _, form, shape, boundary in (c for c in th.screen2d_cases() if c[0] == kind):
        out[f"screen {form} {shape} boundary={boundary}"] = th.screen2d_case(kind, shape, boundary).x.double()
    for form in ("ny", "flat"):
        for boundary in (False, True):
            c = th.pair_case(kind, form, boundary)
            out[f"pair {form} boundary={boundary} truth"], out[f"pair {form} boundary={boundary} prediction"] = c.x.double(), c.y.double()
    return out


@pytest.mark.parametrize("kind,nchan,ref", [("ns_momentum", 3, th.ns_momentum_ref), ("mhd_energy", 6, th.mhd_energy_ref)])
def test_2d_mutants_are_visible_on_every_input_family(kind, nchan, ref):
    seen = {}
    with sh.oracle_fp64():
        for what, v in _inputs_2d(kind, nchan).items():
            want = ref(v)
            for name, mutant in th.MUTANTS[kind]:
                _visible(name, mutant(v), want, seen)
    _report(f"{kind}: smallest rel_err of each mutant over the input families", seen)
    assert len(seen) == len(th.MUTANTS[kind]) >= 12


def _inputs_jorek(kinds, rho0):
    """(name, vars float64 [B,3,Nx,Ny,Nt], opset): every input family and operator set of the GPU file"""
    for i, s in enumerate(th.JOREK_SHAPES):
        for seed in (0, 1):                                  # (seed 1: the second set of minus=)
            v = th.jorek_vars(s, seed, rho0).double()
            for opset in (th.OPSETS if i == 0 else ("default",)):
                yield f"rand+0.5 {s} seed {seed}", v, opset
    done = set()
    for kind, form, shape, boundary, mode, r0 in th.jorek_screen_cases():
        if kind in kinds and r0 == rho0 and (kind, shape, boundary, mode) not in done:
            done.add((kind, shape, boundary, mode))
            c = th.jorek_screen_case(kind, shape, boundary, mode, rho0)
            yield f"screen {kind} {shape} boundary={boundary} mode={mode}", sj.to_vars(c.x.double()), mode or "default"


@pytest.mark.parametrize("key", ["jorek_continuity", "jorek_continuity_norms", "jorek_temperature"])
def test_jorek_mutants_are_visible_on_every_input_family(key):
    kind, norms = key.replace("_norms", ""), key.endswith("_norms")
    seen = {}
    with sh.oracle_fp64():
        for what, v, opset in _inputs_jorek((kind,), False):
            if norms and what.startswith("screen"):
                continue                                     # (the screens evaluate norms=False)
            R = sj.radius(v.shape[3]).double()
            want = th.jorek_ref(kind, v, R, opset, norms=norms)
            for name, mutant in th.MUTANTS[key]:
                if th.rescale_applies(name, opset):
                    _visible(name, mutant(v, R, opset), want, seen)
    _report(f"{key}: smallest rel_err of each mutant over the input families", seen)
    assert len(seen) == len(th.MUTANTS[key])


def test_y_mutants_are_visible_on_the_rho_zero_input_at_the_default_k():
    seen = {}
    with sh.oracle_fp64():
        for what, v, opset in _inputs_jorek(("jorek_temperature",), True):
            assert not bool(v[:, 0].any())
            R = sj.radius(v.shape[3]).double()
            want = th.jorek_ref("jorek_temperature", v, R, opset, th.JOREK_DEFAULT)
            for name, mutant in th.y_mutants():
                _visible(name, mutant(v, R, opset), want, seen)
    _report("a3*Y(T) on rho = 0 at the default K: smallest rel_err of each mutant", seen)


@pytest.mark.parametrize("name,attr,default", [("ns_momentum", "nu", th.NS_DEFAULT["nu"]), ("mhd_energy", "gamma", th.MHD_DEFAULT["gamma"]),
                                               ("jorek_continuity", "D", th.JOREK_DEFAULT["D"])])
def test_backward_references_move_with_the_coefficient(name, attr, default):
    """the fp64 gradients the backward cases are held to: with the one coefficient back at its default they differ by at
    least 100 x TOL on the cases' own inputs"""
    from losses_helpers import channel_errs, ref_vjp, seam_inputs
    chosen, mutant = th.vjp_route(name), th.vjp_route(name)
    assert getattr(chosen.obj, attr) != default
    setattr(mutant.obj, attr, default)
    for shape in ((th.VJP_FLAT_SHAPE,) if name == "jorek_continuity" else (th.VJP_NY_SHAPE, th.VJP_FLAT_SHAPE)):
        for boundary in (False, True):
            x, g = seam_inputs(chosen, shape, boundary)
            errs = channel_errs(ref_vjp(mutant, x.double(), g.double(), boundary), ref_vjp(chosen, x.double(), g.double(), boundary))
            print(name, shape, boundary, {k: f"{v:.3g}" for k, v in errs.items()})
            assert errs["all"] >= th.VISIBLE


# ------------------------------------------------------------------ why the suite was blind
def test_at_the_default_k_the_parity_inputs_hide_the_whole_k_term():
    """The inputs of test_jorek_streaming_sizes_and_layouts_vs_oracle (its first shape): each part of a3*Y(T) is under 1e-7
    of max |res|, and K = 0 moves the residual by 1.1e-7 - a hundredth of RES_TOL."""
    g = torch.Generator().manual_seed(23)
    v = (torch.rand(3, 3, 64, 64, 10, generator=g) + 0.5).double()
    R = (torch.linspace(1.0, 2.0, 64) + 0.01 * torch.rand(64, generator=g)).double()
    with sh.oracle_fp64():
        want = orr.jorek_temperature(v, R, boundary=True)
        t = th.jorek_temperature_terms(v, R, th.JOREK_DEFAULT["K"], th.JOREK_DEFAULT["gamma"], orr.OpsJorek())
        blind = th.rel_err(orr.jorek_temperature(v, R, K=0.0, boundary=True), want)
    shares = {k: float(t[k].abs().max() / want.abs().max()) for k in th.Y_PARTS}
    print("shares of max|res|:", {k: f"{s:.2g}" for k, s in shares.items()}, f"K = 0: rel_err {blind:.2g}")
    assert all(s < 1e-7 for s in shares.values()) and blind < th.RES_TOL / 50
    others = {k: float(x.abs().max() / want.abs().max()) for k, x in t.items() if k not in th.Y_PARTS}
    assert min(others.values()) > th.VISIBLE


# ------------------------------------------------------------------ the caps of the screen cases
def test_every_screen_case_meets_the_caps():
    n = 0
    for kind, form, shape, boundary in th.screen2d_cases():
        c = th.screen2d_case(kind, shape, boundary)
        assert sj.caps_hold(c) and 0 <= c.seed <= 5 and c.coef == th.COEF[kind], (kind, shape, boundary, c.caps())
        n += 1
    for kind in th.SCREEN_KINDS:
        for form in ("ny", "flat"):
            for boundary in (False, True):
                c = th.pair_case(kind, form, boundary)
                ok, figures = c.caps_hold()
                assert ok and 0 <= c.seed <= 5, (kind, form, boundary, figures)
                n += 1
    for kind, form, shape, boundary, mode, rho0 in th.jorek_screen_cases():
        c = th.jorek_screen_case(kind, shape, boundary, mode, rho0)
        assert sj.caps_hold(c) and 0 <= c.seed <= 5, (kind, shape, boundary, mode, rho0, c.caps())
        assert bool(c.x[:, 0].any()) != rho0
        if rho0:                                              # the tolerance is on the K term's own scale
            assert c.tau < 1e-5 * 1e-5 and float(c.r_ref.abs().max()) > 0
        n += 1
    print(n, "screen cases")
    # the optional arguments change nothing where they are absent: the key and the case of an existing call
    a = sj.case("jorek_temperature", sj.FLAT_BASE)
    b = sj.case("jorek_temperature", sj.FLAT_BASE, coef=th.JOREK)
    assert a is sj.case("jorek_temperature", sj.FLAT_BASE) and a is not b and not torch.equal(a.r_ref, b.r_ref)
    assert torch.equal(sh.Case("mhd_energy", sj.NY_BASE, False, True, 10).r_ref,
                       sh.Case("mhd_energy", sj.NY_BASE, False, True, 10, coef=th.MHD_DEFAULT).r_ref)
