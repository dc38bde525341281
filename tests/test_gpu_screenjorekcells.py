"""The opt-in per-cell screen of the JOREK residuals (``cp_pre_amd.screen.screen_cells`` / ``ScreenCells`` with ``jorek=True``,
csrc/screen_jorek_cells.hip) and ``norms=True`` through ``functools.partial`` on both JOREK screens, on the GPU, against
float64 (pytest -m gpu).

Reference, level fields, tolerances and cases: tests/screenjorekcells_helpers.py (the oracle in float64; tau = 1e-5 max
|r_ref|; score within tau / m_min + one ulp; a count within the undecided cells of its (level, sample)).  Shapes are the
logical (B, T, X, Y); ``vars`` is [BS,F,Nx,Ny,Nt] - dense for the flat form (Nt-fastest field views), a view of memory
[BS,F,Nt,Nx,Ny] for the Ny-fastest form.  tests/test_screenjorekcells_cpu.py shows, with the oracle alone, that every case
compared with the reference here meets the caps those bounds rest on; tests/SCREENJOREKCELLS_TESTS.md says which test reaches
which branch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import screen_helpers as sh
import screenflat_helpers as sf
import screenjorek_helpers as sj
import screenjorekcells_helpers as jc
import stencil_guards as sg
from oracle import residuals as orr

pytestmark = pytest.mark.gpu
FORMS = ("flat", "ny")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def vars_of(x, form, device):
    """The logical CPU fields ``x`` [B,3,T,X,Y] as ``vars`` [BS,F,Nx,Ny,Nt] on ``device``: dense ('flat': the script's
    tensor, Nt-fastest field views) or a view of memory [BS,F,Nt,Nx,Ny] ('ny': Ny-fastest field views)."""
    v = sj.to_vars(x.to(device))
    return v.contiguous() if form == "flat" else v


def laid(t, ntfast, device):
    """``t`` (a modulation [T,X,Y] or level fields [nk,T,X,Y]) on ``device``, Nt-fastest in memory or contiguous"""
    if t is None:
        return None
    return sf.to_layout(t, device) if ntfast else t.to(device)


def run(c, gpu, form, x=None, q=None, mod="native", method=None, mode=None, **kw):
    """``screen_cells`` on case ``c``; ``mod``: 'none', 'native' (the fields' layout), 'other', or a tensor"""
    from cp_pre_amd import screen
    xd = vars_of(c.x, form, gpu) if x is None else x
    if isinstance(mod, str):
        mod = None if mod == "none" or c.mod is None else laid(c.mod, (form == "flat") == (mod == "native"), gpu)
    qd = laid(c.q, form == "flat", gpu) if q is None else q
    method = method or sj.method_of(c.kind, mode, gpu, ny=c.shape[3])
    kw.setdefault("jorek", True)
    return screen.screen_cells(method, xd, qd, mod, boundary=c.boundary, **kw)


def same(a, b):
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside) and a.cells == b.cells


# ------------------------------------------------------------------ 1. both equations against fp64 and the three-pass route
@pytest.mark.parametrize("mod", ["none", "native", "other"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_both_equations_against_fp64_and_three_pass(gpu, kind, form, boundary, mod):
    """nk = 1 (one live level of the first batch), 10, 16 (every batch full)"""
    from cp_pre_amd import screen
    for nk in jc.NKS:
        c = jc.case(kind, jc.FLAT_BASE if form == "flat" else jc.NY_BASE, boundary, mod != "none", nk)
        xd = vars_of(c.x, form, gpu)
        f0 = xd[:, 0].permute(0, 3, 1, 2)
        assert (f0.stride(1) == 1 and f0.stride(3) == f0.shape[1]) if form == "flat" else f0[0].is_contiguous()
        s = run(c, gpu, form, x=xd, mod=mod)
        assert screen.last_route() == jc.route(kind, form)
        jc.check(c, s, f"fused {form} boundary={boundary} mod={mod}")
        s3 = run(c, gpu, form, x=xd, mod=mod, jorek=False)
        assert screen.last_route() == "fallback:no fused screen for JOREK"
        jc.check(c, s3, "  three-pass")
        print(f"  fused and three-pass bit-identical: {same(s, s3)}")


# ------------------------------------------------------------------ 2. the seams of both marches
@pytest.mark.parametrize("name", list(jc.FLAT_SEAMS))
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_flat_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        c = jc.case(kind, jc.FLAT_SEAMS[name], boundary)
        s = run(c, gpu, "flat")
        assert screen.last_route() == jc.route(kind, "flat")
        jc.check(c, s, f"{name} boundary={boundary} (seed {c.seed})")


@pytest.mark.parametrize("name", list(jc.NY_SEAMS))
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_ny_fastest_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        c = jc.case(kind, jc.NY_SEAMS[name], boundary)
        s = run(c, gpu, "ny")
        assert screen.last_route() == jc.route(kind, "ny")
        jc.check(c, s, f"{name} boundary={boundary} (seed {c.seed})")


@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_flat_smallest_y(gpu, kind):
    """two columns: every cell lies on the y rim (boundary=True; cropped, no cell would be left)"""
    from cp_pre_amd import screen
    c = jc.case(kind, jc.SMALLEST_Y, True)
    s = run(c, gpu, "flat")
    assert screen.last_route() == jc.route(kind, "flat")
    jc.check(c, s, f"{jc.SMALLEST_Y}")


# ------------------------------------------------------------------ 3. the staged modes: every tap structure built is launched
@pytest.mark.parametrize("mode", jc.MODES)
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_staged_modes(gpu, kind, mode):
    """``y_axis_fix=True`` puts the taps of D_Z / D_ZZ on the true Ny axis (<4> in the flat form, <1> Ny-fastest); a D_R with
    weight on all three axes is the general star (<2>): both stage fields through LDS.  The reference is the oracle with the
    same operators; <3> and <0> are the tap structures of every other test here."""
    from cp_pre_amd import screen
    for form in FORMS:
        for shape in jc.STAGED[form]:
            c = jc.case(kind, shape, mode=mode)
            s = run(c, gpu, form, mode=mode)
            assert screen.last_route() == jc.route(kind, form)
            jc.check(c, s, f"{mode} {form}")
            assert not torch.equal(c.r_ref, sj.oracle_residual(kind, c.x.double()))     # the staged kernels were applied


# ------------------------------------------------------------------ 4. the sample group
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_across_the_sample_group(gpu, kind, form):
    """B = G + 1 and B = 2G - 1: a group with one sample and a group one short, next to whole ones; G from the library.
    The samples of the partial group have the bits they have in a run of three samples of the same data."""
    from cp_pre_amd import screen
    G = screen.sample_group_jorek()
    assert G >= 1
    for B in jc.group_batches(G):
        c = jc.case(kind, (3,) + jc.GROUP_TXY, True, True, 10, n=B)
        xd = vars_of(c.x, form, gpu)
        s = run(c, gpu, form, x=xd)
        assert screen.last_route() == jc.route(kind, form)
        jc.check(c, s, f"G={G} B={B} {form}")
        first = (B - 1) // G * G                                   # the partial group: samples [first, B)
        assert 0 < B - first < G or G == 1
        lo = max(first, B - 3)
        last3 = xd[B - 3:]
        small = run(c, gpu, form, x=last3 if form == "ny" else last3.contiguous())
        assert screen.last_route() == jc.route(kind, form) and small.inside.shape[1] == 3
        assert torch.equal(sg.bits(s.score[lo:]), sg.bits(small.score[lo - (B - 3):]))
        assert torch.equal(s.inside[:, lo:], small.inside[:, lo - (B - 3):])


# ------------------------------------------------------------------ 5. exact contracts
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_level_extremes_and_nan(gpu, kind, form):
    from cp_pre_amd import screen
    c = jc.case(kind, jc.FLAT_BASE if form == "flat" else jc.NY_BASE)
    base = run(c, gpu, form)
    assert screen.last_route() == jc.route(kind, form)
    ones = torch.ones_like(c.q)
    allin = run(c, gpu, form, q=laid(ones * float("inf"), form == "flat", gpu))
    assert bool((allin.inside == c.cells).all()) and torch.equal(sg.bits(allin.score), sg.bits(base.score))
    for v in (-1.0, float("nan")):
        none = run(c, gpu, form, q=laid(ones * v, form == "flat", gpu))
        assert bool((none.inside == 0).all()) and torch.equal(sg.bits(none.score), sg.bits(base.score))
    # a NaN in one field cell (phi of sample 1, an interior cell): its stencil footprint is outside at every level, +inf
    # included, and the sample's score is NaN; the other samples do not move
    x = c.x.clone()
    x[1, 1, 2, 2, 5] = float("nan")
    xd = vars_of(x, form, gpu)
    stored = sj.method_of(kind, None, gpu, ny=c.shape[3])(xd, boundary=True)
    nbad = int(torch.isnan(stored[c.reg][1]).sum())
    assert 1 <= nbad <= 27 and not bool(torch.isnan(stored[c.reg][[0, 2]]).any())
    got = run(c, gpu, form, x=xd, q=laid(ones * float("inf"), form == "flat", gpu))
    assert screen.last_route() == jc.route(kind, form)
    assert bool(torch.isnan(got.score[1])) and torch.equal(sg.bits(got.score[[0, 2]]), sg.bits(base.score[[0, 2]]))
    assert bool((got.inside[:, 1] == c.cells - nbad).all()) and bool((got.inside[:, [0, 2]] == c.cells).all())
    got = run(c, gpu, form, x=xd)
    assert bool((got.inside[:, 1] <= c.cells - nbad).all()) and torch.equal(got.inside[:, [0, 2]], base.inside[:, [0, 2]])


@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_constant_level_fields_give_the_bits_of_the_joint_screen(gpu, kind, form, with_mod):
    from cp_pre_amd import screen
    shape = jc.FLAT_BASE if form == "flat" else jc.NY_BASE
    for boundary in (False, True):
        c = jc.case(kind, shape, boundary, with_mod)
        q = sj.case(kind, shape, boundary, with_mod, nk=6).q                           # six scalar levels of the joint case
        xd, md = vars_of(c.x, form, gpu), laid(c.mod, form == "flat", gpu)
        method = sj.method_of(kind, None, gpu)
        joint = screen.screen(method, xd, q.to(gpu), md, boundary=boundary, jorek=True)
        assert screen.last_route() == "fused:" + ("flat_" if form == "flat" else "") + kind
        qc = q[:, None, None, None].expand(6, *c.shape[1:]).contiguous()
        got = run(c, gpu, form, x=xd, q=laid(qc, form == "flat", gpu), mod=md)
        assert screen.last_route() == jc.route(kind, form)
        assert same(got, joint)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_cropped_levels_layouts_and_two_runs(gpu, kind, form):
    from cp_pre_amd import screen
    c = jc.case(kind, jc.FLAT_BASE if form == "flat" else jc.NY_BASE)
    base = run(c, gpu, form)
    assert same(run(c, gpu, form), base)                                             # two runs: the same bytes
    # cropped level fields and their NaN-padded form agree, whatever the rim of the uncropped ones holds
    got = run(c, gpu, form, q=c.q_cropped().to(gpu))
    assert screen.last_route() == jc.route(kind, form) and same(got, base)
    padded = screen._pad_levels(c.q_cropped().to(gpu), tuple(c.shape[1:]), form == "flat")
    assert bool(torch.isnan(padded[:, 0]).all()) and same(run(c, gpu, form, q=padded), base)
    # level fields in the other layout are re-laid once: same bits
    other = laid(c.q, form != "flat", gpu)
    assert (other.stride(-1) == 1) == (form == "flat")
    assert same(run(c, gpu, form, q=other), base) and screen.last_route() == jc.route(kind, form)
    # a permutation of the levels permutes the rows of the counts and keeps the score
    perm = torch.tensor([3, 0, 9, 1, 7, 2, 8, 4, 6, 5])
    got = run(c, gpu, form, q=laid(c.q[perm], form == "flat", gpu))
    assert torch.equal(got.inside, base.inside[perm.to(gpu)]) and torch.equal(sg.bits(got.score), sg.bits(base.score))


# ------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_slabs_compose_bit_for_bit(gpu, kind, form):
    """x-slabs that overlap by their crop rows and t-slabs that overlap by their crop planes (the JOREK passes read no halo
    rows: a slab carries its neighbours' rows itself and crops them) give the bits of the whole grid; t-slabs of the dense
    tensor are copied, a view of them has no dense rows"""
    from cp_pre_amd import screen
    shape = jc.SLAB_SHAPE
    c = jc.case(kind, shape)
    whole = run(c, gpu, form)
    assert screen.last_route() == jc.route(kind, form)
    jc.check(c, whole, f"whole grid {form}")
    method = sj.method_of(kind, None, gpu, ny=shape[3])
    xd, q, md = vars_of(c.x, form, gpu), laid(c.q, form == "flat", gpu), laid(c.mod, form == "flat", gpu)
    X, T = shape[2], shape[1]
    for order in (((0, 11), (9, 34), (32, X)), ((32, X), (0, 11), (9, 34))):
        s = screen.ScreenCells(shape[0], c.nk, gpu)
        for x0, x1 in order:
            s.add_slab(method, xd[:, :, x0:x1], q[:, :, x0:x1], md[:, x0:x1], jorek=True)
            assert screen.last_route() == jc.route(kind, form)
        assert same(s.finish(), whole)
    for order in (((0, 8), (6, T)), ((6, T), (0, 8))):
        s = screen.ScreenCells(shape[0], c.nk, gpu)
        for t0, t1 in order:
            slab = xd[..., t0:t1]
            s.add_slab(method, slab.contiguous() if form == "flat" else slab, q[:, t0:t1], md[t0:t1], jorek=True)
            assert screen.last_route() == jc.route(kind, form)
        assert same(s.finish(), whole)
    # twice without zeroing: the counts double, the score stays
    s = screen.ScreenCells(shape[0], c.nk, gpu)
    s.add_slab(method, xd, q, md, jorek=True)
    once = s.acc.clone()
    s.add_slab(method, xd, q, md, jorek=True)
    assert torch.equal(s.acc[0], once[0]) and torch.equal(s.acc[1:], 2 * once[1:])
    assert torch.equal(sg.bits(once[0].view(torch.float32)), sg.bits(whole.score))


# ------------------------------------------------------------------ 7. norms=True through the partial, on both JOREK screens
@pytest.mark.parametrize("form", FORMS)
def test_screenjorek_norms_through_the_partial_on_both_screens(gpu, form):
    from cp_pre_amd import screen
    kind, shape = "jorek_continuity", jc.FLAT_BASE if form == "flat" else jc.NY_BASE
    part = jc.norms_method(gpu)
    assert all(v != 1 for v in jc.NORMS.values())
    # the per-cell screen
    c, plain = jc.case(kind, shape, norms=True), jc.case(kind, shape)
    xd = vars_of(c.x, form, gpu)
    assert torch.equal(c.x, plain.x)
    s = run(c, gpu, form, x=xd, method=part)
    assert screen.last_route() == jc.route(kind, form)
    jc.check(c, s, f"norms=True, per-cell, {form}")
    s3 = run(c, gpu, form, x=xd, method=part, q=laid(c.q, form == "flat", gpu).double())      # the fallback calls the partial
    assert screen.last_route() == "fallback:float64 levels or modulation"
    jc.check(c, s3, "  three-pass")
    # without the partial the result is that of norms=False: the bits of the bound method of an object without grid steps
    a = run(c, gpu, form, x=xd, method=part.func)
    b = run(c, gpu, form, x=xd, method=jc.norms_method(gpu, norms=False))
    d = run(c, gpu, form, x=xd)
    assert same(a, b) and same(a, d) and not same(a, s)
    # the joint screen
    j = jc.joint_norms_case(shape)
    md = laid(j.mod, form == "flat", gpu)
    got = screen.screen(part, vars_of(j.x, form, gpu), j.q.to(gpu), md, jorek=True)
    assert screen.last_route() == "fused:" + ("flat_" if form == "flat" else "") + kind
    score, inside = got.score.cpu().double(), got.inside.cpu()
    ulp = torch.from_numpy(np.spacing(j.s_ref.float().numpy()).astype(np.float64))
    print(f"norms=True, joint, {form}: score err {float((score - j.s_ref).abs().max()):.3e} (allowed {j.tol_s:.3e} + ulp), count "
          f"diff max {int((inside - j.count_ref).abs().max())} (undecided max {int(j.undecided.max())})")
    assert got.cells == j.cells and bool(((score - j.s_ref).abs() <= j.tol_s + ulp).all())
    assert bool(((inside - j.count_ref).abs() <= j.undecided).all()) and torch.equal(got.accept().cpu(), j.accept_ref)
    plain_joint = screen.screen(part.func, vars_of(j.x, form, gpu), j.q.to(gpu), md, jorek=True)
    assert not torch.equal(sg.bits(plain_joint.score), sg.bits(got.score))
    # the stored residual of the partial is the reference's form too
    r = part(xd, boundary=True)
    assert float((r.cpu().double() - c.r_ref).abs().max()) <= c.tau


def test_screenjorek_norms_refusals(gpu):
    from cp_pre_amd import screen
    c = jc.case("jorek_continuity", jc.FLAT_BASE)
    xd, q = vars_of(c.x, "flat", gpu), laid(c.q, True, gpu)
    with pytest.raises(ValueError, match="norms=True needs dx, dy, dt"):
        screen.screen_cells(jc.norms_method(gpu, steps=False), xd, q, jorek=True)
    with pytest.raises(ValueError, match="norms=True needs dx, dy, dt"):
        screen.screen(jc.norms_method(gpu, steps=False), xd, q[:, 0, 0, 0].contiguous(), jorek=True)
    for fn in (lambda m: screen.screen_cells(m, xd, q, jorek=True), lambda m: screen.screen(m, xd, q[:, 0, 0, 0].contiguous(), jorek=True)):
        with pytest.raises(Exception, match="Norm not implemented yet"):
            fn(jc.norms_method(gpu, kind="jorek_temperature"))
    with pytest.raises(TypeError):
        screen.screen_cells(jc.norms_method(gpu), xd, q)                             # the partial without the keyword


# ------------------------------------------------------------------ 8. declines and errors
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_fallbacks_say_why_and_agree(gpu, kind):
    from cp_pre_amd import screen
    for shape, why in jc.FALLBACK_SHAPES.items():
        c = jc.case(kind, shape)
        s = run(c, gpu, "flat")
        assert screen.last_route() == "fallback:" + why
        jc.check(c, s, f"{shape} ({why})")
    c = jc.case(kind, jc.FLAT_BASE)
    fused = run(c, gpu, "flat")
    assert screen.last_route() == jc.route(kind, "flat")
    s = run(c, gpu, "flat", method=sj.method_of(kind, None, gpu, fused=False))
    assert screen.last_route() == "fallback:fused=False"
    jc.check(c, s, "fused=False")
    live = sj.jorek_of(None, gpu)
    live.D_R.kernel.requires_grad_(True)
    run(c, gpu, "flat", method=getattr(live, "residual_" + kind[6:]))
    assert screen.last_route() == "fallback:operator kernel requires grad"
    box = sj.jorek_of(None, gpu)
    box.D_Z.kernel.data[0, 0, 0] = 0.5
    run(c, gpu, "flat", method=getattr(box, "residual_" + kind[6:]))
    assert screen.last_route() == "fallback:operator kernel off the 7-point star"
    xd, q, md = vars_of(c.x, "flat", gpu), laid(c.q, True, gpu), laid(c.mod, True, gpu)
    s = run(c, gpu, "flat", q=q.double())
    assert screen.last_route() == "fallback:float64 levels or modulation"
    jc.check(c, s, "float64 levels")
    # minus= keeps the three-pass route, with or without pair=True
    method = sj.method_of(kind, None, gpu)
    a = screen.screen_cells(method, xd, q, md, minus=torch.zeros_like(xd), jorek=True)
    assert screen.last_route() == "fallback:minus="
    b = screen.screen_cells(method, xd, q, md, minus=torch.zeros_like(xd), jorek=True, pair=True)
    assert screen.last_route().startswith("fallback:") and same(a, b)
    # four channels: declined, and the method itself unstacks exactly three; CPU tensors, staged
    with pytest.raises(ValueError):
        run(c, gpu, "flat", x=torch.cat([xd, xd[:, :1]], dim=1))
    assert screen.last_route() == "fallback:not three JOREK channels"
    s = screen.screen_cells(sj.method_of(kind), vars_of(c.x, "flat", "cpu"), c.q_cropped(), c.mod, jorek=True)
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    jc.check(c, s, "CPU inputs, cropped levels")
    assert torch.equal(fused.accept().cpu(), s.accept())
    # a t-slab of the dense tensor: rows not dense; an Ny-fastest view whose rows are no multiple of 4
    big = torch.full((3, 3, 5, 12, 16), 7.0)
    big[..., 2:12] = sj.to_vars(c.x)
    s = run(c, gpu, "flat", x=big.to(gpu)[..., 2:12])
    assert screen.last_route() == "fallback:rows not dense"
    jc.check(c, s, "t-slab")
    oc = jc.case(kind, (3, 10, 5, 13))
    s = run(oc, gpu, "ny")
    assert screen.last_route() == "fallback:row width not a multiple of 4"
    jc.check(oc, s, "Ny = 13")


def test_screenjorekcells_refusals_raise_before_any_launch_and_leave_the_accumulators(gpu):
    from cp_pre_amd import screen
    c = jc.case("jorek_temperature", jc.FLAT_BASE)
    for form in FORMS:
        xd, q, md = vars_of(c.x, form, gpu), laid(c.q, form == "flat", gpu), laid(c.mod, form == "flat", gpu)
        method = sj.method_of(c.kind, None, gpu)
        s = screen.ScreenCells(3, c.nk, gpu)
        s.add_slab(method, xd, q, md, jorek=True)
        before, cells = s.acc.clone(), s.cells
        # len(R) != Ny: the residual pass's error
        with pytest.raises(RuntimeError, match="R has 8 points"):
            s.add_slab(sj.method_of(c.kind, None, gpu, ny=8), xd, q, md, jorek=True)
        # halo_x: no pass of the JOREK residuals reads halo rows
        with pytest.raises(RuntimeError, match="halo_x"):
            s.add_slab(method, xd[:, :, 1:-1], q[:, :, 1:-1], md[:, 1:-1], crop=(1, 0, 1), halo_x=True, jorek=True)
        for bad in (lambda: s.add_slab(method, xd, q[:3], md, jorek=True), lambda: s.add_slab(method, xd, q[:, 1:], md, jorek=True),
                    lambda: s.add_slab(method, xd, q, md[1:], jorek=True), lambda: s.add_slab(method, xd[:2], q, md, jorek=True),
                    lambda: s.add_slab(method, xd, c.q_cropped().to(gpu), md, jorek=True)):
            with pytest.raises(ValueError):
                bad()
        # the keyword on another method is an error
        with pytest.raises(TypeError, match="jorek=True"):
            s.add_slab(sh.method_of("ns_momentum", gpu), torch.rand(3, 3, 10, 5, 12, device=gpu), q, md, jorek=True)
        torch.cuda.synchronize()
        assert torch.equal(s.acc, before) and s.cells == cells
    with pytest.raises(TypeError, match="jorek=True"):
        screen.screen_cells(sh.method_of("ns_momentum", gpu), torch.rand(3, 3, 10, 5, 12, device=gpu), q, jorek=True)


def test_screenjorekcells_default_route_is_unchanged_and_the_library_is_not_loaded(gpu):
    """without the keyword, in a fresh interpreter: ``fallback:no fused screen for JOREK`` and the library stays unloaded
    through the joint JOREK screen and the per-cell screen of another method; with the keyword it is loaded"""
    code = (
        "import sys, torch\n"
        "sys.path[:0] = [%r, %r]\n"
        "import screen_helpers as sh, screenjorek_helpers as sj, screenjorekcells_helpers as jc\n"
        "from cp_pre_amd import screen, _lib\n"
        "c = jc.case('jorek_continuity', jc.FLAT_BASE)\n"
        "d = torch.device('cuda:0')\n"
        "m = sj.method_of(c.kind, None, d)\n"
        "x, q, mod = sj.to_vars(c.x.to(d)).contiguous(), c.q.to(d), c.mod.to(d)\n"
        "a = screen.screen_cells(m, x, q, mod)\n"
        "assert screen.last_route() == 'fallback:no fused screen for JOREK', screen.last_route()\n"
        "screen.screen(m, x, q[:, 0, 0, 0].contiguous(), mod, jorek=True)\n"
        "assert screen.last_route() == 'fused:flat_jorek_continuity', screen.last_route()\n"
        "w = sh.fields('wave', (3, 4, 33, 16)).to(d)\n"
        "screen.screen_cells(sh.method_of('wave', d), w, torch.ones(2, 4, 33, 16, device=d))\n"
        "assert screen.last_route() == 'fused:cells_stencil3d', screen.last_route()\n"
        "assert _lib._screenjorekcells is None\n"
        "f = screen.screen_cells(m, x, q, mod, jorek=True)\n"
        "assert screen.last_route() == 'fused:flat_cells_jorek_continuity' and _lib._screenjorekcells is not None\n"
        "jc.check(c, a, 'three-pass'); jc.check(c, f, 'fused')\n"
        "print('default unchanged')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                           os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "default unchanged" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ 9. the C client
def client_reference():
    """The inputs of tests/c_abi/screenjorekcells_check.c rebuilt bit for bit (its header states the closed forms) and, per
    equation, what the float64 oracle gives on them with crop 1: B scores, NK x B counts, NK x B undecided cells."""
    B, T, X, Y, NK = 2, 6, 5, 12, 3
    cells = T * X * Y
    state = [5]

    def stream(n):
        out = np.empty(n, np.float64)
        for i in range(n):
            state[0] = (state[0] * 1664525 + 1013904223) & 0xffffffff
            out[i] = (state[0] >> 16) / 65536.0
        return out
    f = np.stack([1.0 + 0.125 * ch + 0.25 * (stream(B * cells) - 0.5) for ch in range(3)])
    x = torch.from_numpy(f.reshape(3, B, T, X, Y)).permute(1, 0, 2, 3, 4).contiguous()          # [B,3,T,X,Y], exact in fp32
    assert torch.equal(x.float().double(), x)
    m = torch.from_numpy(0.75 + 0.5 * stream(cells)).reshape(T, X, Y)
    lv = torch.stack([torch.from_numpy(level * (0.75 + 0.5 * stream(cells))).reshape(T, X, Y) for level in (0.25, 1.0, 1048576.0)])
    R = (np.float32(1) + np.arange(Y, dtype=np.float32) / np.float32(Y - 1)).astype(np.float32)
    args = []
    reg = (slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
    for fn in (orr.jorek_continuity, orr.jorek_temperature):
        with sh.oracle_fp64():
            r = fn(sj.to_vars(x), torch.from_numpy(R).double(), boundary=True)
        tau = 1e-5 * float(r.abs().max())
        a, mm = r[reg].abs().flatten(1), m[reg[1:]].flatten()
        gap = a[None] - (lv[(slice(None),) + reg[1:]].flatten(1) * mm)[:, None]                  # [NK, B, cells]
        args += [float(v) for v in (a / mm).max(dim=1).values]
        args += [int(v) for v in (gap <= 0).sum(dim=2).flatten()] + [int(v) for v in (gap.abs() <= tau).sum(dim=2).flatten()]
    assert len(args) == 2 * (B + 2 * NK * B)
    return args


def test_screenjorekcells_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screenjorekcells_check.c on the device, as a child process under a time limit: both equations in both
    layouts against plain C loops AND against the float64 oracle's values on the same inputs, handed over as arguments;
    accumulation over two calls, and the argument errors of the header."""
    from test_screenjorekcells_cpu import c_client_command
    exe = tmp_path / "screenjorekcells_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)] + [repr(v) for v in client_reference()], capture_output=True, text=True, timeout=120)
    print(out.stdout[-8000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") == 38, out.stdout
    assert out.stdout.count("the caller's score") == 8
