"""The opt-in paired screen of the data-driven scores (cp_pre_amd.screen with ``minus=`` and ``pair=True``,
csrc/screen_pair.hip) on the GPU, against float64 (pytest -m gpu).

Reference, tolerances and cases: tests/screenpair_helpers.py (the oracle in float64 on both sets, d_ref = r_ref(a) - r_ref(b);
tau = 1e-5 (max |r_ref(a)| + max |r_ref(b)|); score within tau / m_min + one ulp; counts within the undecided cells; accept
exact).  Shapes are the logical (B, T, X, Y), all B = 3; the Nt-fastest form is ``screenflat_helpers.to_layout`` of both
sets.  tests/test_screenpair_cpu.py shows, with the oracle alone, that every case compared with the reference here meets
the caps the tolerances rest on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import screen_helpers as sh
import screenflat_helpers as sf
import screenpair_helpers as sp
import stencil_guards as sg

pytestmark = pytest.mark.gpu
FORMS = ("ny", "flat")
BASE = {"ny": sp.NY_BASE, "flat": sp.FLAT_BASE}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def put(t, form, device):
    if t is None:
        return None
    return sf.to_layout(t, device) if form == "flat" else t.to(device)


def run(case, gpu, form, x=None, y=None, mod="native", method=None, pair=True, q=None):
    from cp_pre_amd import screen
    xd = put(case.x, form, gpu) if x is None else x
    yd = put(case.y, form, gpu) if y is None else y
    md = put(case.mod, form, gpu) if isinstance(mod, str) else mod
    method = method or sh.method_of(case.kind, gpu)
    return screen.screen(method, xd, case.q.to(gpu) if q is None else q, md, boundary=case.boundary, minus=yd, pair=pair)


def check_against_ref(case, s, what):
    score = s.score.cpu().double()
    inside = s.inside.cpu()
    ulp = np.spacing(case.s_ref.float().numpy()).astype(np.float64)
    err = (score - case.s_ref).abs()
    dcount = (inside - case.count_ref).abs()
    print(f"{what}: score err {float(err.max()):.3e} (allowed {case.tol_s:.3e} + ulp), count diff max {int(dcount.max())} "
          f"(undecided max {int(case.undecided.max())} of {case.cells} cells)")
    assert s.cells == case.cells
    assert s.score.dtype == torch.float32 and s.inside.dtype == torch.int64 and tuple(s.inside.shape) == (case.nk, case.shape[0])
    assert bool((err <= case.tol_s + torch.from_numpy(ulp)).all()), (what, err, case.tol_s)
    assert bool((dcount <= case.undecided).all()), (what, dcount, case.undecided)
    assert torch.equal(s.accept().cpu(), case.accept_ref), what


def same(a, b):
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside)


def check_against_route(case, s, other, what):
    """``s`` against the result ``other`` of another route on the same inputs, within the bounds ``check_against_ref`` holds
    each to the reference with: the score within tau / m_min plus one ulp, the counts within the undecided cells of that
    (level, sample), accept equal"""
    a, b = s.score.cpu().double(), other.score.cpu().double()
    ulp = torch.from_numpy(np.spacing(other.score.cpu().numpy()).astype(np.float64))
    err, dcount = (a - b).abs(), (s.inside.cpu() - other.inside.cpu()).abs()
    print(f"{what}: score diff {float(err.max()):.3e} (allowed {case.tol_s:.3e} + ulp), count diff max {int(dcount.max())}, "
          f"bit-identical: {same(s, other)}")
    assert s.cells == other.cells
    assert bool((err <= case.tol_s + ulp).all()), (what, err, case.tol_s)
    assert bool((dcount <= case.undecided).all()), (what, dcount, case.undecided)
    assert torch.equal(s.accept(), other.accept()), what


# ------------------------------------------------------------------ 1. every kind, both forms, against fp64 and the three passes
@pytest.mark.parametrize("with_mod", [False, True])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", sp.KINDS)
def test_screenpair_every_kind_against_fp64_and_three_pass(gpu, kind, form, boundary, with_mod):
    from cp_pre_amd import screen
    case = sp.case(kind, BASE[form], boundary, with_mod, form=form)
    xd, yd, md = put(case.x, form, gpu), put(case.y, form, gpu), put(case.mod, form, gpu)
    assert (xd.stride(-3) == 1) == (form == "flat") and (xd.stride(-1) == 1) == (form == "ny")
    s = run(case, gpu, form, x=xd, y=yd, mod=md)
    assert screen.last_route() == sp.route(kind, form)
    check_against_ref(case, s, f"{kind} {form} boundary={boundary} mod={with_mod}")
    s3 = run(case, gpu, form, x=xd, y=yd, mod=md, pair=False)
    assert screen.last_route() == "fallback:minus="
    check_against_ref(case, s3, "  three-pass")
    check_against_route(case, s, s3, "  fused against three-pass")


# ------------------------------------------------------------------ 2. the seams of both marches
@pytest.mark.parametrize("name", list(sh.SEAM_SHAPES))
@pytest.mark.parametrize("kind", sp.NY_SEAM_KINDS)
def test_screenpair_ny_fastest_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        for with_mod in (False, True):
            case = sp.case(kind, sh.SEAM_SHAPES[name], boundary, with_mod, form="ny")
            s = run(case, gpu, "ny")
            assert screen.last_route() == sp.route(kind, "ny")
            check_against_ref(case, s, f"{kind} {name} boundary={boundary} mod={with_mod} (seed {case.seed})")


@pytest.mark.parametrize("name", list(sf.SEAM_SHAPES) + ["smallest_y"])
@pytest.mark.parametrize("kind", sp.FLAT_SEAM_KINDS)
def test_screenpair_flat_at_the_seams(gpu, kind, name):
    """``smallest_y``: two columns, every cell on the y rim (boundary=True only; cropped, no cell would be left)"""
    from cp_pre_amd import screen
    shape = sf.SMALLEST_Y if name == "smallest_y" else sf.SEAM_SHAPES[name]
    for boundary in ((True,) if name == "smallest_y" else (False, True)):
        for with_mod in (False, True):
            case = sp.case(kind, shape, boundary, with_mod, form="flat")
            s = run(case, gpu, "flat")
            assert screen.last_route() == sp.route(kind, "flat")
            check_against_ref(case, s, f"{kind} {name} boundary={boundary} mod={with_mod} (seed {case.seed})")


# ------------------------------------------------------------------ 3. minus = vars: exactly zero
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", sp.KINDS)
def test_screenpair_minus_equal_to_vars_gives_exactly_zero(gpu, kind, form):
    """the same tensor and an equal copy: both halves of the paired functor round alike, so d is +-0 in every cell - score
    bits exactly 0 and every counted cell inside at every level (q_k * m >= 0)"""
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = sp.case(kind, BASE[form], boundary, True, form=form)
        xd = put(case.x, form, gpu)
        for yd in (xd, xd.clone(memory_format=torch.preserve_format)):
            s = run(case, gpu, form, x=xd, y=yd)
            assert screen.last_route() == sp.route(kind, form)
            assert bool((sg.bits(s.score) == 0).all()), (kind, form, s.score)
            assert bool((s.inside == s.cells).all()) and s.cells == case.cells and bool(s.accept().all())


# ------------------------------------------------------------------ 4. views in poisoned memory, non-finite values
def _embedded(t, form, gpu, nch_extra=2):
    """(allocation, view holding ``t``): channels [1:1+F] of a larger stacked tensor ([B,F,...] inputs) or the field in a
    guarded allocation, laid out for ``form``"""
    n = t.dim()
    order = None if form == "ny" else tuple(range(n - 3)) + (n - 2, n - 1, n - 3)
    if n == 5:
        big = torch.zeros(t.shape[0], t.shape[1] + nch_extra, *t.shape[2:])
        big[:, 1:1 + t.shape[1]] = t
        alloc, view = sg.embed(big, order, None, 0, gpu)
        return alloc, view[:, 1:1 + t.shape[1]]
    return sg.embed(t, order, None, 0, gpu)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", sp.KINDS)
def test_screenpair_views_in_poisoned_memory(gpu, kind, form):
    """``vars[:, i]`` / ``minus[:, i]`` of larger storages filled with NaN, 0 and 1e30 around the views: the bits of the
    dense run, and nothing written"""
    from cp_pre_amd import screen
    case = sp.case(kind, BASE[form], False, True, form=form)
    dense = run(case, gpu, form)
    assert screen.last_route() == sp.route(kind, form)
    xa, xd = _embedded(case.x, form, gpu)
    ya, yd = _embedded(case.y, form, gpu, nch_extra=3)
    ma, md = sg.embed(case.mod, (1, 2, 0) if form == "flat" else None, None, 0, gpu)
    masks = [sg.outside_mask(a, v) for a, v in ((xa, xd), (ya, yd), (ma, md))]
    for value in sg.POISONS:
        for a, m in zip((xa, ya, ma), masks):
            sg.poison(a, m, value)
        before = [a.clone() for a in (xa, ya, ma)]
        got = run(case, gpu, form, x=xd, y=yd, mod=md)
        assert screen.last_route() == sp.route(kind, form), screen.last_route()
        assert same(got, dense), (kind, form, value)
        assert all(torch.equal(sg.bits(a), sg.bits(b)) for a, b in zip((xa, ya, ma), before))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", sp.KINDS)
def test_screenpair_non_finite_values(gpu, kind, form):
    """NaN and inf in the cropped rim of either set change nothing; a NaN in ONE counted cell of the prediction only makes
    that sample's score NaN and the cell outside at every level"""
    from cp_pre_amd import screen
    case = sp.case(kind, BASE[form], False, True, form=form)
    clean = run(case, gpu, form)
    B, T, X, Y = case.shape
    for which in ("x", "y"):
        t = getattr(case, which).clone()
        # corners of the rim: no counted cell's star reaches them
        t[..., 0, 0, :], t[..., -1, :, 0] = float("nan"), float("inf")
        t[..., :, 0, 0], t[..., -1, -1, :] = float("inf"), float("nan")
        got = run(case, gpu, form, **{which: put(t, form, gpu)})
        assert screen.last_route() == sp.route(kind, form)
        assert same(got, clean), (kind, form, which)
    # one counted cell of sample 1 of the prediction (every channel of it): NaN there and at most in the cells whose star
    # reaches it, all counted (the cell lies two cells inside the counted region along t and y, in its middle row)
    yp = case.y.clone()
    yp[(1,) + ((slice(None),) if yp.dim() == 5 else ()) + (T // 2, X // 2, Y // 2)] = float("nan")
    got = run(case, gpu, form, y=put(yp, form, gpu))
    assert screen.last_route() == sp.route(kind, form)
    score = got.score.cpu()
    assert bool(torch.isnan(score[1])) and not bool(torch.isnan(score[[0, 2]]).any())
    assert torch.equal(sg.bits(got.score[[0, 2]]), sg.bits(clean.score[[0, 2]]))
    assert torch.equal(got.inside[:, [0, 2]], clean.inside[:, [0, 2]])
    top = got.inside[-1, 1].item()                       # the level above every score: every cell but the NaN ones
    assert clean.inside[-1, 1].item() == case.cells and case.cells - 7 <= top <= case.cells - 1
    assert bool((got.inside[:, 1] <= clean.inside[:, 1]).all())
    assert not bool(got.accept()[:, 1].any())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["mhd_continuity", "ns_momentum"])
def test_screenpair_y_fixed_tap_structure_on_two_distinct_sets(gpu, kind, form):
    """``y_axis_fix=True`` puts D_y's taps on the true Ny axis: the y-fixed instantiations (<1> Ny-fastest, <4> Nt-fastest)
    on two DISTINCT sets, against the stored difference of the same operators and against the three-pass route, within
    bounds worked out for these operators below (the levels are the default operators' case's: what they split does not
    matter here) - and not the default operators' answer.  The paired NS
    momentum is not built in that tap structure on Nt-fastest sets: the library declines."""
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    obj = (R.MHD(device=gpu, y_axis_fix=True) if kind == "mhd_continuity" else
           R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, device=gpu, y_axis_fix=True))
    method = getattr(obj, "residual_" + kind.split("_", 1)[1])
    for boundary in (False, True):
        case = sp.case(kind, BASE[form], boundary, True, form=form)
        s = run(case, gpu, form, method=method)
        built = not (kind == "ns_momentum" and form == "flat")
        assert screen.last_route() == (sp.route(kind, form) if built else "fallback:declined by the library")
        s3 = run(case, gpu, form, method=method, pair=False)
        assert screen.last_route() == "fallback:minus="
        assert not same(s, run(case, gpu, form))             # the y-fixed operators were applied
        # The bounds, for THESE operators, from the stored fp32 residuals (each within tau of the truth):
        # tau from both halves; a cell on which two routes can disagree lies within tau of the level's edge in truth,
        # so within 2 tau of it by the stored difference; accept is compared where the level is further than
        # 2 tau / m_min from the score.
        xd, yd = put(case.x, form, gpu), put(case.y, form, gpu)
        reg = sh.region(case.shape, case.crop)
        ra, rb = method(xd, boundary=True), method(yd, boundary=True)
        tau = 1e-5 * (float(ra.abs().max()) + float(rb.abs().max()))
        d = method(xd, boundary=True, minus=yd)[reg].abs().double().flatten(1)            # [B, cells]
        m = case.mod.to(gpu)[reg[1:]].double().flatten()
        tol = tau / float(m.min())
        want = (d / m).max(dim=1).values
        hw = case.q.to(gpu).double()[:, None] * m[None]
        und = ((d[None] - hw[:, None]).abs() <= 2 * tau).sum(dim=2)
        for got, what in ((s, "fused"), (s3, "three-pass")):
            err = (got.score.double() - want).abs()
            print(f"{kind} {form} y-fixed boundary={boundary} {what}: score err {float(err.max()):.3e} (allowed {tol:.3e} + ulp)")
            assert bool((err <= tol + 1.2e-7 * want).all()), (what, err, tol)
            assert bool(((got.inside - (d[None] <= hw[:, None]).sum(dim=2)).abs() <= und).all()), what
        assert bool(((s.inside - s3.inside).abs() <= und).all())
        far = (want[None] - case.q.to(gpu).double()[:, None]).abs() > 2 * tol
        assert torch.equal(s.accept()[far], s3.accept()[far])
        print(f"  fused and three-pass bit-identical: {same(s, s3)}")


# ------------------------------------------------------------------ 5. composition: slabs equal the one-shot screen exactly
@pytest.mark.parametrize("kind", ["ns_momentum", "wave", "mhd_continuity"])
def test_screenpair_x_slabs_with_halo_and_t_slabs_equal_the_whole_grid(gpu, kind):
    from cp_pre_amd import screen
    shape = sh.SEAM_SHAPES["rows2_narrow"]                   # (3, 4, 33, 16)
    case = sp.case(kind, shape, False, True, form="ny")
    whole = run(case, gpu, "ny")
    assert screen.last_route() == sp.route(kind, "ny")
    assert same(run(case, gpu, "ny"), whole)                 # two runs: identical bytes
    method = sh.method_of(kind, gpu)
    xd, yd, md, q = case.x.to(gpu), case.y.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    X = shape[2]
    # two x-slabs of unequal length with their halo rows, the rim rows left out by the cut itself
    s = screen.Screen(shape[0], case.nk, gpu)
    for x0, x1 in ((1, 10), (10, X - 1)):
        s.add_slab(method, xd[..., x0:x1, :], q, md[:, x0:x1], crop=(1, 0, 1), halo_x=True, minus=yd[..., x0:x1, :], pair=True)
        assert screen.last_route() == sp.route(kind, "ny")
    got = s.finish()
    assert got.cells == whole.cells and same(got, whole)
    # two t-slabs with their halo planes
    tcase = sp.case(kind, sh.SEAM_SHAPES["two_tseg"], False, True, form="ny")
    twhole = run(tcase, gpu, "ny")
    xd, yd, md, q = tcase.x.to(gpu), tcase.y.to(gpu), tcase.mod.to(gpu), tcase.q.to(gpu)
    s = screen.Screen(3, tcase.nk, gpu)
    for t0, t1 in ((0, 9), (7, 17)):
        s.add_slab(method, xd[..., t0:t1, :, :], q, md[t0:t1], minus=yd[..., t0:t1, :, :], pair=True)
        assert screen.last_route() == sp.route(kind, "ny")
    got = s.finish()
    assert got.cells == twhole.cells and same(got, twhole)


@pytest.mark.parametrize("kind", ["ns_momentum", "mhd_continuity"])
def test_screenpair_flat_slabs_along_x_equal_the_whole_grid(gpu, kind):
    """the merged-row march composes along its marched axis (logical x: slabs with their halo rows and crop 1) and over
    batch halves"""
    from cp_pre_amd import screen
    case = sp.case(kind, sf.SEAM_SHAPES["two_marches"], False, True, form="flat")
    whole = run(case, gpu, "flat")
    assert screen.last_route() == sp.route(kind, "flat")
    method = sh.method_of(kind, gpu)
    xd, yd, md, q = put(case.x, "flat", gpu), put(case.y, "flat", gpu), put(case.mod, "flat", gpu), case.q.to(gpu)
    s = screen.Screen(3, case.nk, gpu)
    for x0, x1 in ((0, 9), (7, 17)):
        s.add_slab(method, xd[..., x0:x1, :], q, md[:, x0:x1], minus=yd[..., x0:x1, :], pair=True)
        assert screen.last_route() == sp.route(kind, "flat")
    got = s.finish()
    assert got.cells == whole.cells and same(got, whole)
    parts = []
    for a, b in ((0, 2), (2, 3)):
        s = screen.Screen(b - a, case.nk, gpu)
        s.add_slab(method, xd[a:b], q, md, minus=yd[a:b], pair=True)
        parts.append(s.finish())
    assert torch.equal(sg.bits(torch.cat([p.score for p in parts])), sg.bits(whole.score))
    assert torch.equal(torch.cat([p.inside for p in parts], dim=1), whole.inside)


# ------------------------------------------------------------------ 6. every named fallback says why and agrees
def test_screenpair_fallbacks_say_why_and_agree(gpu):
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    kind = "ns_momentum"
    case = sp.case(kind, sp.NY_BASE, False, True, form="ny")
    fused = run(case, gpu, "ny")
    assert screen.last_route() == sp.route(kind, "ny")
    xd, yd, md, q = case.x.to(gpu), case.y.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    # no paired screen for the kind
    for other, why in sp.UNPAIRED.items():
        c = sp.case(other, sp.NY_BASE, False, True, form="ny")
        s = run(c, gpu, "ny")
        assert screen.last_route() == "fallback:" + why
        check_against_ref(c, s, why)
    # input on the CPU (both sets staged); float64 levels, float64 modulation
    s = screen.screen(sh.method_of(kind), case.x, case.q, case.mod, minus=case.y, pair=True)
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    check_against_ref(case, s, "CPU inputs")
    np.testing.assert_array_equal(fused.accept().cpu().numpy(), s.accept().numpy())
    s = run(case, gpu, "ny", q=q.double())
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, s, "float64 levels")
    s = run(case, gpu, "ny", mod=md.double())
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, s, "float64 modulation")
    # the layout of vars; the same of minus; one set in each layout
    for k in ("ns_momentum", "wave"):
        oc = sp.case(k, sp.ODD_NY, False, True, form="ny")
        s = run(oc, gpu, "ny")
        assert screen.last_route() == "fallback:row width not a multiple of 4"
        check_against_ref(oc, s, f"{k} Ny = 13")
        oc = sp.case(k, sp.ODD_FLAT, False, True, form="flat")
        s = run(oc, gpu, "flat")
        assert screen.last_route() == "fallback:merged row Ny*Nt not a multiple of 4"
        check_against_ref(oc, s, f"{k} flat Ny = 13")
        shape, why = next(iter(sf.FALLBACK_SHAPES.items()))
        oc = sp.case(k, shape, False, True, form="flat")
        s = run(oc, gpu, "flat")
        assert screen.last_route() == why
        check_against_ref(oc, s, f"{k} {why}")
    wide = torch.zeros(*case.y.shape[:-1], 2 * case.y.shape[-1], device=gpu)
    wide[..., ::2] = yd
    s = run(case, gpu, "ny", y=wide[..., ::2])
    assert screen.last_route() == "fallback:minus: no unit stride on the last axis"
    check_against_ref(case, s, "strided minus")
    s = run(case, gpu, "ny", y=sf.to_layout(case.y, gpu))
    assert screen.last_route() == "fallback:field sets in different layouts"
    check_against_ref(case, s, "Ny-fastest vars, Nt-fastest minus")
    fc = sp.case(kind, sp.FLAT_BASE, False, True, form="flat")
    s = run(fc, gpu, "flat", y=fc.y.to(gpu))
    assert screen.last_route() == "fallback:field sets in different layouts"
    check_against_ref(fc, s, "Nt-fastest vars, Ny-fastest minus")
    big = torch.full((3, 3, 16, 5, 12), 7.0)
    big[:, :, 2:12] = fc.y
    s = run(fc, gpu, "flat", y=sf.to_layout(big, gpu)[:, :, 2:12])
    assert screen.last_route() == "fallback:minus: rows not dense"
    check_against_ref(fc, s, "t-slab of an Nt-fastest minus")
    # fused=False, a kernel that requires grad, a kernel off the star
    ns = lambda **kw: R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, device=gpu, **kw)
    s = run(case, gpu, "ny", method=ns(fused=False).residual_momentum)
    assert screen.last_route() == "fallback:fused=False"
    check_against_ref(case, s, "fused=False")
    live = ns()
    live.D_x.kernel.requires_grad_(True)
    s = run(case, gpu, "ny", method=live.residual_momentum)
    assert screen.last_route() == "fallback:operator kernel requires grad"
    check_against_ref(case, s, "requires grad")
    box = ns()
    box.D_y.kernel.data[0, 0, 0] = 0.5
    a = run(case, gpu, "ny", method=box.residual_momentum)
    assert screen.last_route() == "fallback:operator kernel off the 7-point star"
    b = run(case, gpu, "ny", method=box.residual_momentum, pair=False)
    assert screen.last_route() == "fallback:minus=" and same(a, b) and not same(a, fused)
    # declined by the library: a D_x with weight on all three axes is a star, but the paired general star is not built
    gen = ns()
    gen.D_x.kernel.data[0, 1, 1] = 0.25
    gen.D_x.kernel.data[1, 1, 0] = 0.25
    a = run(case, gpu, "ny", method=gen.residual_momentum)
    assert screen.last_route() == "fallback:declined by the library"
    b = run(case, gpu, "ny", method=gen.residual_momentum, pair=False)
    assert screen.last_route() == "fallback:minus=" and same(a, b)
    # ... nor is the y-fixed tap structure of the paired NS momentum on Nt-fastest sets (it would not fit the registers);
    # on Ny-fastest sets it is
    fix = ns(y_axis_fix=True)
    a = run(fc, gpu, "flat", method=fix.residual_momentum)
    assert screen.last_route() == "fallback:declined by the library"
    b = run(fc, gpu, "flat", method=fix.residual_momentum, pair=False)
    assert screen.last_route() == "fallback:minus=" and same(a, b)
    a = run(case, gpu, "ny", method=fix.residual_momentum)
    assert screen.last_route() == "fused:pair_ns_momentum"
    b = run(case, gpu, "ny", method=fix.residual_momentum, pair=False)
    assert torch.equal(a.accept(), b.accept()) and not same(a, fused)
    # the 1-D family
    bu = R.Burgers(0.02, 0.01, 0.01, device=gpu)
    u, v = torch.rand(3, 12, 16, device=gpu) + 0.5, torch.rand(3, 12, 16, device=gpu) + 0.5
    a = screen.screen(bu.residual, u, torch.tensor([0.5, 50.0], device=gpu), minus=v, pair=True)
    assert screen.last_route() == "fallback:no paired screen for the 1-D family"
    b = screen.screen(bu.residual, u, torch.tensor([0.5, 50.0], device=gpu), minus=v)
    assert screen.last_route() == "fallback:minus=" and same(a, b)


def test_screenpair_halo_x_rules(gpu):
    """under halo_x both sets must be Ny-contiguous device views; the flat form is not offered; a declined fused launch
    raises where no other pass reads the halo rows"""
    from cp_pre_amd import screen
    case = sp.case("ns_continuity", sh.SEAM_SHAPES["rows2_narrow"], False, True, form="ny")
    xd, yd, md, q = case.x.to(gpu), case.y.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    method = sh.method_of("ns_continuity", gpu)
    kw = dict(crop=(1, 0, 1), halo_x=True, pair=True)
    whole = run(case, gpu, "ny")
    s = screen.Screen(3, case.nk, gpu)
    for x0, x1 in ((1, 20), (20, 32)):
        s.add_slab(method, xd[..., x0:x1, :], q, md[:, x0:x1], minus=yd[..., x0:x1, :], **kw)
        assert screen.last_route() == "fused:pair_linear2"
    assert same(s.finish(), whole)
    s = screen.Screen(3, case.nk, gpu)
    with pytest.raises(ValueError, match="Ny-contiguous device views"):
        s.add_slab(method, xd[..., 1:20, :], q, md[:, 1:20], minus=sf.to_layout(case.y, gpu)[..., 1:20, :], **kw)
    # NS continuity's own pass reads no halo: a fused launch that cannot run raises instead of counting zero padding
    with pytest.raises(RuntimeError, match="halo_x"):
        s.add_slab(method, xd[..., 1:20, :], q.double(), md[:, 1:20], minus=yd[..., 1:20, :], **kw)
    with pytest.raises(RuntimeError, match="halo_x"):
        s.add_slab(method, xd[..., 1:20, :], q, md[:, 1:20], minus=yd[..., 1:20, :], crop=(1, 0, 1), halo_x=True)
    assert s.cells == 0 and (s.acc is None or not bool(s.acc.any()))


# ------------------------------------------------------------------ 7. the default is unchanged
def test_screenpair_default_route_is_unchanged_and_the_library_is_not_loaded(gpu):
    """``minus=`` without ``pair`` in a fresh interpreter: ``fallback:minus=`` and ``_lib._screenpair`` stays None; ``pair=True``
    without ``minus`` takes the single-set fused screen"""
    code = (
        "import sys, torch\n"
        "sys.path[:0] = [%r, %r]\n"
        "import screen_helpers as sh, screenpair_helpers as sp\n"
        "from cp_pre_amd import screen, _lib\n"
        "c = sp.case('ns_momentum', sp.NY_BASE)\n"
        "d = torch.device('cuda:0')\n"
        "m = sh.method_of('ns_momentum', d)\n"
        "a = screen.screen(m, c.x.to(d), c.q.to(d), c.mod.to(d), minus=c.y.to(d))\n"
        "assert screen.last_route() == 'fallback:minus=', screen.last_route()\n"
        "b = screen.screen(m, c.x.to(d), c.q.to(d), c.mod.to(d), pair=True)\n"
        "assert screen.last_route() == 'fused:ns_momentum', screen.last_route()\n"
        "e = screen.screen(m, c.x.to(d), c.q.to(d), c.mod.to(d))\n"
        "assert torch.equal(b.inside, e.inside) and torch.equal(b.score.view(torch.int32), e.score.view(torch.int32))\n"
        "assert _lib._screenpair is None\n"
        "f = screen.screen(m, c.x.to(d), c.q.to(d), c.mod.to(d), minus=c.y.to(d), pair=True)\n"
        "assert screen.last_route() == 'fused:pair_ns_momentum' and _lib._screenpair is not None\n"
        "assert torch.equal(a.accept(), f.accept())\n"
        "print('default unchanged')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                           os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "default unchanged" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ 8. the C client
def test_screenpair_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screenpair_check.c on the device, as a child process under a time limit: the paired star in both layouts
    against plain C loops, two t-slabs, b == a for every entry, and the argument errors of the header."""
    from test_screenpair_cpu import c_client_command
    exe = tmp_path / "screenpair_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") == 37, out.stdout


# ------------------------------------------------------------------ 9. per-cell (marginal) sets at one level
@pytest.mark.parametrize("form", FORMS)
def test_screenpair_one_level_marginal_idiom_counts_as_emp_cov_levels(gpu, form):
    """``screen(method, vars, ones(1), modulation=qhat_cells, minus=pred, pair=True)`` counts |d| <= qhat_cells exactly
    (1.0f * m == m): the counts of ``emp_cov_levels`` on the stored difference, in total and per sample"""
    from cp_pre_amd import inductive_cp as icp
    from cp_pre_amd import screen
    kind = "ns_momentum"
    case = sp.case(kind, BASE[form], True, True, form=form)
    method = sh.method_of(kind, gpu)
    xd, yd = put(case.x, form, gpu), put(case.y, form, gpu)
    d = method(xd, boundary=True, minus=yd).contiguous()                    # the stored difference, as the three passes see it
    qhat_cells = torch.quantile(d.abs().flatten(1).T.contiguous(), 0.6, dim=1).reshape(d.shape[1:]).contiguous()
    one = torch.ones(1, device=gpu)
    s = screen.screen(method, xd, one, put(qhat_cells.cpu(), form, gpu), boundary=True, minus=yd, pair=True)
    assert screen.last_route() == sp.route(kind, form)
    want = (d.abs() <= qhat_cells[None]).flatten(1).sum(dim=1)
    assert torch.equal(s.inside[0], want)
    cov = icp.emp_cov_levels(qhat_cells[None], d)
    assert cov.shape == (1,) and round(float(cov[0]) * d.numel()) == int(want.sum())
    assert float(s.coverage_marginal()[0]) == float(int(want.sum())) / float(d.numel())
    # the single-set form of the idiom
    r = method(xd, boundary=True).contiguous()
    s1 = screen.screen(method, xd, one, put(qhat_cells.cpu(), form, gpu), boundary=True)
    assert torch.equal(s1.inside[0], (r.abs() <= qhat_cells[None]).flatten(1).sum(dim=1))
