"""The opt-in fused screen of the JOREK residuals (cp_pre_amd.screen with ``jorek=True``, csrc/screen_jorek.hip) on the GPU,
against float64 (pytest -m gpu).

Reference, tolerances and cases: tests/screen_helpers.py and tests/screenjorek_helpers.py (the oracle in float64; tau = 1e-5
max |r_ref|, the tolerance the JOREK residual pass is held to; score within tau / m_min + one ulp; counts within the undecided
cells; accept exact).  Shapes are the logical (B, T, X, Y); ``vars`` is [BS,F,Nx,Ny,Nt] - dense for the flat form (Nt-fastest
field views), a view of memory [BS,F,Nt,Nx,Ny] for the Ny-fastest form.  tests/test_screenjorek_cpu.py shows, with the oracle
alone, that every case used here meets the caps the tolerances rest on."""
import subprocess

import numpy as np
import pytest
import torch

import screen_helpers as sh
import screenflat_helpers as sf
import screenjorek_helpers as sj
import stencil_guards as sg

pytestmark = pytest.mark.gpu


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


def mod_of(case, how, device):
    if case.mod is None or how == "none":
        return None
    return sf.to_layout(case.mod, device) if how == "ntfast" else case.mod.to(device)


def route_of(kind, form):
    return "fused:" + ("flat_" if form == "flat" else "") + kind


def run(case, gpu, form, x=None, mod="native", method=None, mode=None, jorek=True):
    from cp_pre_amd import screen
    xd = vars_of(case.x, form, gpu) if x is None else x
    md = mod_of(case, ("ntfast" if form == "flat" else "contiguous") if mod == "native" else mod, gpu) if isinstance(mod, str) else mod
    method = method or sj.method_of(case.kind, mode, gpu, ny=case.shape[3])
    return screen.screen(method, xd, case.q.to(gpu), md, boundary=case.boundary, jorek=jorek)


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


# ------------------------------------------------------------------ 1. every kind against the reference
@pytest.mark.parametrize("mod", ["none", "ntfast", "contiguous"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("form", ["flat", "ny"])
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_every_kind_against_fp64_and_three_pass(gpu, kind, form, boundary, mod):
    from cp_pre_amd import screen
    for nk in (1, 10, 16):
        case = sj.case(kind, sj.FLAT_BASE if form == "flat" else sj.NY_BASE, boundary, mod != "none", nk)
        md = mod_of(case, mod, gpu)
        assert md is None or (md.stride(0) == 1) == (mod == "ntfast")
        xd = vars_of(case.x, form, gpu)
        f0 = xd[:, 0].permute(0, 3, 1, 2)
        assert (f0.stride(1) == 1 and f0.stride(3) == f0.shape[1]) if form == "flat" else f0[0].is_contiguous()
        s = run(case, gpu, form, x=xd, mod=md)
        assert screen.last_route() == route_of(kind, form)
        check_against_ref(case, s, f"{kind} {form} boundary={boundary} mod={mod} nk={nk}")
        s3 = run(case, gpu, form, x=xd, mod=md, jorek=False)
        assert screen.last_route() == "fallback:no fused screen for JOREK"
        check_against_ref(case, s3, "  three-pass")
        print(f"  fused and three-pass bit-identical: {same(s, s3)}")


# ------------------------------------------------------------------ 2. the seams of both marches
@pytest.mark.parametrize("name", list(sj.FLAT_SEAMS))
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_flat_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = sj.case(kind, sj.FLAT_SEAMS[name], boundary)
        s = run(case, gpu, "flat")
        assert screen.last_route() == route_of(kind, "flat")
        check_against_ref(case, s, f"{kind} {name} boundary={boundary} (seed {case.seed})")


@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_flat_smallest_y(gpu, kind):
    """two columns: every cell lies on the y rim (boundary=True; cropped, no cell would be left)"""
    from cp_pre_amd import screen
    case = sj.case(kind, sf.SMALLEST_Y, True)
    s = run(case, gpu, "flat")
    assert screen.last_route() == route_of(kind, "flat")
    check_against_ref(case, s, f"{kind} {sf.SMALLEST_Y}")


@pytest.mark.parametrize("name", list(sj.NY_SEAMS))
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_ny_fastest_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = sj.case(kind, sj.NY_SEAMS[name], boundary)
        s = run(case, gpu, "ny")
        assert screen.last_route() == route_of(kind, "ny")
        check_against_ref(case, s, f"{kind} {name} boundary={boundary} (seed {case.seed})")


# ------------------------------------------------------------------ 3. the staged modes
@pytest.mark.parametrize("mode", sj.MODES)
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_staged_modes(gpu, kind, mode):
    """``y_axis_fix=True`` puts the taps of D_Z / D_ZZ on the true Ny axis (<4> in the flat form, <1> Ny-fastest); a D_R with
    weight on all three axes is the general star (<2>): both stage fields through LDS.  The reference is the oracle with the
    same operators."""
    from cp_pre_amd import screen
    for form, shapes in (("flat", sj.STAGED_FLAT), ("ny", sj.STAGED_NY)):
        for name, shape in shapes.items():
            case = sj.case(kind, shape, mode=mode)
            s = run(case, gpu, form, mode=mode)
            assert screen.last_route() == route_of(kind, form)
            check_against_ref(case, s, f"{kind} {mode} {form} {name}")
            # not the default operators' answer: the staged kernels were applied
            assert not torch.equal(case.r_ref, sj.oracle_residual(kind, case.x.double()))


# ------------------------------------------------------------------ 4. views in poisoned allocations
def _views(case, form, gpu):
    """name -> (allocation, vars view [BS,3,Nx,Ny,Nt] holding case.x): channels [:, 1:4] of a five-channel tensor, an
    x-range slice [:, :, 2:-2] of a longer grid"""
    v = sj.to_vars(case.x)                                   # [B,3,X,Y,T], logical values
    B, F, X, Y, T = v.shape
    order = (0, 1, 2, 3, 4) if form == "flat" else (0, 1, 4, 2, 3)
    out = {}
    big = torch.zeros(B, F + 2, X, Y, T)
    big[:, 1:4] = v
    alloc, view = sg.embed(big, order, None, 0, gpu)
    out["channels"] = (alloc, view[:, 1:4])
    big = torch.zeros(B, F, X + 4, Y, T)
    big[:, :, 2:-2] = v
    alloc, view = sg.embed(big, order, None, 0, gpu)
    out["x_slice"] = (alloc, view[:, :, 2:-2])
    return out


@pytest.mark.parametrize("form", ["flat", "ny"])
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_views_in_poisoned_memory(gpu, kind, form):
    from cp_pre_amd import screen
    case = sj.case(kind, sj.FLAT_BASE if form == "flat" else sj.NY_BASE)
    dense = run(case, gpu, form)
    assert screen.last_route() == route_of(kind, form)
    malloc, md = sg.embed(case.mod, (1, 2, 0) if form == "flat" else None, None, 1, gpu)
    mmask = sg.outside_mask(malloc, md)
    for name, (alloc, xd) in _views(case, form, gpu).items():
        assert name != "x_slice" or xd.stride(1) > xd[0, 0].numel()
        mask = sg.outside_mask(alloc, xd)
        for value in sg.POISONS:
            sg.poison(alloc, mask, value)
            sg.poison(malloc, mmask, value)
            before = [alloc.clone(), malloc.clone()]
            got = run(case, gpu, form, x=xd, mod=md)
            assert screen.last_route() == route_of(kind, form), (name, screen.last_route())
            assert same(got, dense), (name, value)
            assert torch.equal(sg.bits(alloc), sg.bits(before[0])) and torch.equal(sg.bits(malloc), sg.bits(before[1]))


# ------------------------------------------------------------------ 5. fallbacks and refusals
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_fallbacks_say_why_and_agree(gpu, kind):
    from cp_pre_amd import screen
    for shape, why in sj.FALLBACK_SHAPES.items():
        case = sj.case(kind, shape)
        s = run(case, gpu, "flat")
        assert screen.last_route() == "fallback:" + why
        check_against_ref(case, s, f"{kind} {shape} ({why})")
    case = sj.case(kind, sj.FLAT_BASE)
    fused = run(case, gpu, "flat")
    assert screen.last_route() == route_of(kind, "flat")
    # fused=False, a kernel that requires grad, float64 levels, minus=: the existing reasons, and the reference is met
    s = run(case, gpu, "flat", method=sj.method_of(kind, None, gpu, fused=False))
    assert screen.last_route() == "fallback:fused=False"
    check_against_ref(case, s, "fused=False")
    live = sj.jorek_of(None, gpu)
    live.D_R.kernel.requires_grad_(True)
    s = run(case, gpu, "flat", method=getattr(live, "residual_" + kind[6:]))
    assert screen.last_route() == "fallback:operator kernel requires grad"
    check_against_ref(case, s, "requires grad")
    box = sj.jorek_of(None, gpu)
    box.D_Z.kernel.data[0, 0, 0] = 0.5
    run(case, gpu, "flat", method=getattr(box, "residual_" + kind[6:]))
    assert screen.last_route() == "fallback:operator kernel off the 7-point star"
    xd, q, md = vars_of(case.x, "flat", gpu), case.q.to(gpu), mod_of(case, "ntfast", gpu)
    method = sj.method_of(kind, None, gpu)
    s = screen.screen(method, xd, q.double(), md, jorek=True)
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, s, "float64 levels")
    screen.screen(method, xd, q, md, minus=torch.zeros_like(xd), jorek=True)
    assert screen.last_route() == "fallback:minus="
    # CPU tensors are staged and take the three-pass route; the verdicts are the fused ones
    s = screen.screen(sj.method_of(kind), vars_of(case.x, "flat", "cpu"), case.q, case.mod, jorek=True)
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    check_against_ref(case, s, "CPU inputs")
    np.testing.assert_array_equal(fused.accept().cpu().numpy(), s.accept().numpy())
    # a t-slab of the dense tensor: rows not dense; an Ny-fastest view whose rows are no multiple of 4
    big = torch.full((3, 3, 5, 12, 16), 7.0)
    big[..., 2:12] = sj.to_vars(case.x)
    s = run(case, gpu, "flat", x=big.to(gpu)[..., 2:12])
    assert screen.last_route() == "fallback:rows not dense"
    check_against_ref(case, s, "t-slab")
    ocase = sj.case(kind, (3, 10, 5, 13))
    s = run(ocase, gpu, "ny")
    assert screen.last_route() == "fallback:row width not a multiple of 4"
    check_against_ref(ocase, s, "Ny = 13")


def test_screenjorek_refusals_raise_before_any_launch(gpu):
    from cp_pre_amd import screen
    case = sj.case("jorek_temperature", sj.FLAT_BASE)
    q, md = case.q.to(gpu), mod_of(case, "ntfast", gpu)
    for form in ("flat", "ny"):
        xd = vars_of(case.x, form, gpu)
        # len(R) != Ny: the residual pass's error
        short = sj.method_of(case.kind, None, gpu, ny=8)
        s = screen.Screen(3, case.nk, gpu)
        with pytest.raises(RuntimeError, match="R has 8 points"):
            s.add_slab(short, xd, q, md, jorek=True)
        assert s.cells == 0 and (s.acc is None or not bool(s.acc.any()))
        # halo_x: no pass of the JOREK residuals reads halo rows
        s = screen.Screen(3, case.nk, gpu)
        with pytest.raises(RuntimeError, match="halo_x"):
            s.add_slab(sj.method_of(case.kind, None, gpu), xd[:, :, 1:-1], q, md[:, 1:-1], crop=(1, 0, 1), halo_x=True, jorek=True)
        assert s.cells == 0 and s.acc is None
    # the keyword on another method is an error
    with pytest.raises(TypeError, match="jorek=True"):
        screen.screen(sh.method_of("ns_momentum", gpu), torch.rand(3, 3, 10, 5, 12, device=gpu), q, jorek=True)


# ------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("form", ["flat", "ny"])
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_composition(gpu, kind, form):
    from cp_pre_amd import screen
    case = sj.case(kind, sj.FLAT_SEAMS["two_marches"] if form == "flat" else sj.NY_SEAMS["two_tseg"])
    whole = run(case, gpu, form)
    # two identical runs: the same bytes
    assert same(run(case, gpu, form), whole)
    method = sj.method_of(kind, None, gpu)
    xd, q = vars_of(case.x, form, gpu), case.q.to(gpu)
    md = mod_of(case, "ntfast" if form == "flat" else "contiguous", gpu)
    # twice without zeroing: the counts double, the score stays
    s = screen.Screen(case.shape[0], case.nk, gpu)
    s.add_slab(method, xd, q, md, jorek=True)
    once = s.acc.clone()
    s.add_slab(method, xd, q, md, jorek=True)
    assert screen.last_route() == route_of(kind, form)
    assert torch.equal(s.acc[0], once[0]) and torch.equal(s.acc[1:], 2 * once[1:])
    assert torch.equal(sg.bits(once[0].view(torch.float32)), sg.bits(whole.score))
    # two batch halves equal the whole, bit for bit
    parts = []
    for a, b in ((0, 2), (2, 3)):
        s = screen.Screen(b - a, case.nk, gpu)
        s.add_slab(method, xd[a:b], q, md, jorek=True)
        parts.append(s.finish())
    assert torch.equal(sg.bits(torch.cat([p.score for p in parts])), sg.bits(whole.score))
    assert torch.equal(torch.cat([p.inside for p in parts], dim=1), whole.inside) and parts[0].cells == whole.cells


def test_screenjorek_default_route_is_unchanged_and_the_residual_pass_agrees(gpu):
    """without the keyword: the three-pass route, as before; and the residual methods, whose R view and scalars now come
    from the two lifted methods, still give the oracle's residual in both layouts"""
    from cp_pre_amd import screen
    for kind in sj.KINDS:
        case = sj.case(kind, sj.FLAT_BASE)
        for form in ("flat", "ny"):
            xd = vars_of(case.x, form, gpu)
            s = screen.screen(sj.method_of(kind, None, gpu), xd, case.q.to(gpu), mod_of(case, "contiguous", gpu))
            assert screen.last_route() == "fallback:no fused screen for JOREK"
            check_against_ref(case, s, f"{kind} {form} default")
            r = sj.method_of(kind, None, gpu)(xd, boundary=True)
            assert float((r.cpu().double() - case.r_ref).abs().max()) <= case.tau


# ------------------------------------------------------------------ 7. the C client
def test_screenjorek_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screenjorek_check.c on the device, as a child process under a time limit: both equations in both layouts
    against plain C loops, accumulation over two calls, and the argument errors of the header."""
    from test_screenjorek_cpu import c_client_command
    exe = tmp_path / "screenjorek_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") == 32, out.stdout
