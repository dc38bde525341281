"""The fused screen of Nt-fastest views of the 2-D residuals (cp_pre_amd.screen's flat route, csrc/screen_flat.hip) on the
GPU, against float64 (pytest -m gpu).

Reference, tolerances and cases: tests/screen_helpers.py and tests/screenflat_helpers.py (the oracle in float64; tau = 1e-5
max |r_ref|; score within tau / m_min + one ulp; counts within the undecided cells; accept exact).  Shapes are the logical
(B, T, X, Y); memory is [B,(F),X,Y,T].  tests/test_screenflat_cpu.py shows, with the oracle alone, that every case used here
keeps its undecided cells under 1 % and every level further than tau / m_min from every per-sample score, and that the
seam shapes cross the seams of the kernel's split rule."""
import subprocess

import numpy as np
import pytest
import torch

import screen_helpers as sh
import screenflat_helpers as sf
import stencil_guards as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


_cases = {}


def case_of(kind, shape, boundary=False, with_mod=True, nk=10):
    """(computed once per key and left unchanged)"""
    key = (kind, tuple(shape), boundary, with_mod, nk)
    if key not in _cases:
        _cases[key] = sf.case(kind, shape, boundary, with_mod, nk)
    return _cases[key]


def run(case, gpu, x=None, mod=None, method=None):
    from cp_pre_amd import screen
    xd = sf.to_layout(case.x, gpu) if x is None else x
    md = (sf.to_layout(case.mod, gpu) if case.mod is not None else None) if mod is None else mod
    return screen.screen(method or sh.method_of(case.kind, gpu), xd, case.q.to(gpu), md, boundary=case.boundary)


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


def three_pass(case, gpu):
    """The package's own three-pass route on the same Nt-fastest views: ``fused=False`` on the method."""
    from cp_pre_amd import screen
    method = sh.method_of(case.kind, gpu)
    obj = method if case.kind == "lap" else method.__self__
    obj.fused = False
    s = run(case, gpu, method=method)
    assert screen.last_route() == "fallback:fused=False"
    return s


def same(a, b):
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside)


# ------------------------------------------------------------------ 1. every kind against the reference
@pytest.mark.parametrize("mod", ["none", "ntfast", "contiguous"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", sf.KINDS)
def test_screenflat_every_kind_against_fp64_and_three_pass(gpu, kind, boundary, mod):
    from cp_pre_amd import screen
    for nk in (1, 10, 16):
        case = case_of(kind, sf.BASE, boundary, mod != "none", nk)
        md = None if mod == "none" else (case.mod.to(gpu) if mod == "contiguous" else sf.to_layout(case.mod, gpu))
        assert md is None or (md.stride(0) == 1) == (mod == "ntfast")
        s = run(case, gpu, mod=md)
        assert screen.last_route() == sf.ROUTE[kind]
        check_against_ref(case, s, f"{kind} boundary={boundary} mod={mod} nk={nk}")
        s3 = three_pass(case, gpu)
        check_against_ref(case, s3, "  three-pass")
        print(f"  fused and three-pass bit-identical: {same(s, s3)}")


# ------------------------------------------------------------------ 2. the seams of the split rule
@pytest.mark.parametrize("name", list(sf.SEAM_SHAPES))
@pytest.mark.parametrize("kind", sf.SEAM_KINDS)
def test_screenflat_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = case_of(kind, sf.SEAM_SHAPES[name], boundary)
        s = run(case, gpu)
        assert screen.last_route() == sf.ROUTE[kind]
        check_against_ref(case, s, f"{kind} {name} boundary={boundary}")


@pytest.mark.parametrize("kind", sf.SEAM_KINDS)
def test_screenflat_smallest_y(gpu, kind):
    """two columns: every cell lies on the y rim (boundary=True; cropped, no cell would be left)"""
    from cp_pre_amd import screen
    case = case_of(kind, sf.SMALLEST_Y, True)
    s = run(case, gpu)
    assert screen.last_route() == sf.ROUTE[kind]
    check_against_ref(case, s, f"{kind} {sf.SMALLEST_Y}")


@pytest.mark.parametrize("kind", sf.SEAM_KINDS)
def test_screenflat_shapes_outside_the_layout_take_the_three_pass_route(gpu, kind):
    from cp_pre_amd import screen
    for shape, route in sf.FALLBACK_SHAPES.items():
        case = case_of(kind, shape)
        s = run(case, gpu)
        assert screen.last_route() == route
        check_against_ref(case, s, f"{kind} {shape} ({route})")
    # a t-slab [:, :, 2:8] of an Nt-fastest tensor: its rows are not dense
    (B, T, X, Y), sl = sf.SLAB
    case = case_of(kind, (B, sl.stop - sl.start, X, Y))
    big = torch.full((B,) + tuple(case.x.shape[1:-3]) + (T, X, Y), 7.0)
    big[..., sl, :, :] = case.x
    xd = sf.to_layout(big, gpu)[..., sl, :, :]
    assert xd.stride(-3) == 1 and xd.stride(-1) == T
    s = run(case, gpu, x=xd)
    assert screen.last_route() == "fallback:rows not dense"
    check_against_ref(case, s, f"{kind} t-slab")


# ------------------------------------------------------------------ 3. views in poisoned allocations
def _views(case, gpu):
    """name -> (allocation, Nt-fastest view holding case.x): channel views of a stacked tensor with two more channels, an
    x-range slice [..., 2:-2, :] of a longer grid (pitched sample stride, base offset), a base misaligned by one float"""
    x = case.x if case.x.dim() == 5 else case.x[:, None]
    B, F, T, X, Y = x.shape
    order = (0, 1, 3, 4, 2)                                   # memory [B,F,X,Y,T]
    out = {}
    big = torch.zeros(B, F + 2, T, X, Y)
    big[:, 1:-1] = x
    alloc, view = sg.embed(big, order, None, 0, gpu)
    out["channels"] = (alloc, view[:, 1:-1])
    big = torch.zeros(B, F, T, X + 4, Y)
    big[:, :, :, 2:-2] = x
    alloc, view = sg.embed(big, order, None, 0, gpu)
    out["x_slice"] = (alloc, view[..., 2:-2, :])
    alloc, view = sg.embed(x, order, None, 1, gpu)
    out["misaligned"] = (alloc, view)
    return {k: (a, v if case.x.dim() == 5 else v[:, 0]) for k, (a, v) in out.items()}


@pytest.mark.parametrize("kind", ["ns_momentum", "wave", "mhd_energy"])
def test_screenflat_views_in_poisoned_memory(gpu, kind):
    from cp_pre_amd import screen
    case = case_of(kind, sf.BASE)
    dense = run(case, gpu)
    malloc, md = sg.embed(case.mod, (1, 2, 0), None, 1, gpu)
    mmask = sg.outside_mask(malloc, md)
    for name, (alloc, xd) in _views(case, gpu).items():
        assert xd.stride(-3) == 1 and xd.stride(-1) == xd.shape[-3], name
        assert name != "x_slice" or xd.stride(0) > xd[0].numel()
        mask = sg.outside_mask(alloc, xd)
        for value in sg.POISONS:
            sg.poison(alloc, mask, value)
            sg.poison(malloc, mmask, value)
            before = [alloc.clone(), malloc.clone()]
            got = run(case, gpu, xd, md)
            assert screen.last_route() == sf.ROUTE[kind]
            assert same(got, dense), (name, value)
            assert torch.equal(sg.bits(alloc), sg.bits(before[0])) and torch.equal(sg.bits(malloc), sg.bits(before[1]))


# ------------------------------------------------------------------ 4. the non-finite contract
def test_screenflat_non_finite_contract(gpu):
    case = case_of("ns_momentum", sf.BASE)
    base = run(case, gpu)
    B, T, X, Y = case.shape
    nan, inf = float("nan"), float("inf")
    # NaN in every rim of the modulation changes nothing
    mod = case.mod.clone()
    mod[0], mod[-1], mod[:, 0], mod[:, -1], mod[:, :, 0], mod[:, :, -1] = [nan] * 6
    assert same(run(case, gpu, mod=sf.to_layout(mod, gpu)), base)
    # NaN and inf in every rim (t, x, y) of the fields, at cells no counted cell's star reaches (the edges where two rims
    # meet), change nothing
    x = case.x.clone()
    x[:, :, 0, 0, :], x[:, :, -1, :, 0], x[:, :, :, -1, -1] = nan, inf, -inf
    x[:, :, -1, -1, :], x[:, :, 0, :, -1], x[:, :, :, 0, 0] = inf, nan, nan
    assert same(run(case, gpu, x=sf.to_layout(x, gpu)), base)
    # a NaN in one counted cell: that sample's score is NaN, the cells it reaches are outside at every level, no other
    # sample differs (how many cells it reaches: from the package's own residual pass - the same functor)
    x = case.x.clone()
    x[1, 0, T // 2, X // 2, Y // 2] = nan
    xd = sf.to_layout(x, gpu)
    got = run(case, gpu, x=xd)
    r = sh.method_of("ns_momentum", gpu)(xd, boundary=True)
    nbad = int(torch.isnan(r[sh.region(case.shape, case.crop)][1]).sum())
    assert 1 <= nbad <= 27
    assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
    others = [0, 2]
    assert torch.equal(sg.bits(got.score[others]), sg.bits(base.score[others])) and torch.equal(got.inside[:, others], base.inside[:, others])
    top = case.q.argmax()                                    # the level above every score: everything finite is inside
    assert int(got.inside[top, 1]) == case.cells - nbad
    assert bool((got.inside[:, 1] <= base.inside[:, 1]).all())
    # one whole sample NaN: the others are bit-identical
    x = case.x.clone()
    x[1] = nan
    got = run(case, gpu, x=sf.to_layout(x, gpu))
    assert bool(torch.isnan(got.score[1])) and int(got.inside[:, 1].sum()) == 0
    assert torch.equal(sg.bits(got.score[others]), sg.bits(base.score[others])) and torch.equal(got.inside[:, others], base.inside[:, others])
    # m = 0 with r != 0: an inf score and the cell outside; r = 0 over m = 0: NaN, as numpy's 0/0
    mod = case.mod.clone()
    mod[T // 2, X // 2, Y // 2] = 0.0
    md = sf.to_layout(mod, gpu)
    got = run(case, gpu, mod=md)
    assert bool(torch.isinf(got.score).all()) and bool((got.inside[top] == case.cells - 1).all())
    got = run(case, gpu, x=sf.to_layout(torch.zeros_like(case.x), gpu), mod=md)
    assert bool(torch.isnan(got.score).all())


# ------------------------------------------------------------------ 5. composition
@pytest.mark.parametrize("kind", ["ns_momentum", "mhd_induction"])
def test_screenflat_composition(gpu, kind):
    from cp_pre_amd import screen
    case = case_of(kind, sf.SEAM_SHAPES["two_marches"])
    whole = run(case, gpu)
    method = sh.method_of(kind, gpu)
    xd, md, q = sf.to_layout(case.x, gpu), sf.to_layout(case.mod, gpu), case.q.to(gpu)
    # two batch halves through Screen.add_slab equal the whole, bit for bit
    parts = []
    for a, b in ((0, 2), (2, 3)):
        s = screen.Screen(b - a, case.nk, gpu)
        s.add_slab(method, xd[a:b], q, md)
        assert screen.last_route() == sf.ROUTE[kind]
        parts.append(s.finish())
    assert torch.equal(sg.bits(torch.cat([p.score for p in parts])), sg.bits(whole.score))
    assert torch.equal(torch.cat([p.inside for p in parts], dim=1), whole.inside) and parts[0].cells == whole.cells
    # the same call twice into zeroed buffers: identical bytes
    assert same(run(case, gpu), whole)
    # twice without zeroing: the counts double, the score stays
    s = screen.Screen(case.shape[0], case.nk, gpu)
    s.add_slab(method, xd, q, md)
    once = s.acc.clone()
    s.add_slab(method, xd, q, md)
    assert screen.last_route() == sf.ROUTE[kind]
    assert torch.equal(s.acc[0], once[0]) and torch.equal(s.acc[1:], 2 * once[1:])
    assert torch.equal(sg.bits(once[0].view(torch.float32)), sg.bits(whole.score))


# ------------------------------------------------------------------ 6. live kernels, refusals, declining library
def test_screenflat_refused_calls_launch_nothing_and_live_kernels_are_seen(gpu):
    from cp_pre_amd import screen
    case = case_of("ns_momentum", sf.BASE)
    method = sh.method_of("ns_momentum", gpu)
    xd, md, q = sf.to_layout(case.x, gpu), sf.to_layout(case.mod, gpu), case.q.to(gpu)
    s = screen.Screen(case.shape[0], case.nk, gpu)
    s.add_slab(method, xd, q, md)
    assert screen.last_route() == "fused:flat_ns_momentum"
    before = s.acc.clone()
    for bad in (lambda: s.add_slab(method, xd, q[:3], md), lambda: s.add_slab(method, xd, q, md[1:]),
                lambda: s.add_slab(method, xd[:2], q, md), lambda: s.add_slab(method, xd, q, md, crop=(9, 1, 1)),
                lambda: s.add_slab(method, xd, q, md, crop=(1, 1))):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(s.acc, before) and s.cells == case.cells
    # a kernel mutated through .data between two calls is seen by the second
    a = screen.screen(method, xd, q, md)
    method.__self__.D_t.kernel.data.mul_(2.0)
    b = screen.screen(method, xd, q, md)
    method.__self__.D_t.kernel.data.mul_(0.5)
    c = screen.screen(method, xd, q, md)
    assert screen.last_route() == "fused:flat_ns_momentum"
    assert not torch.equal(sg.bits(a.score), sg.bits(b.score)) and same(a, c)
    # the live kernel is applied, not only noticed: D_t doubled is the oracle's answer for it on the three-pass route too
    method.__self__.D_t.kernel.data.mul_(2.0)
    method.__self__.fused = False
    b3 = screen.screen(method, xd, q, md)
    assert screen.last_route() == "fallback:fused=False"
    np.testing.assert_allclose(b.score.cpu().numpy(), b3.score.cpu().numpy(), rtol=1e-4)


def test_screenflat_fallbacks_say_why_and_agree(gpu):
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    case = case_of("ns_momentum", sf.BASE)
    fused = run(case, gpu)
    xd, md, q = sf.to_layout(case.x, gpu), sf.to_layout(case.mod, gpu), case.q.to(gpu)
    meth = sh.method_of("ns_momentum", gpu)
    got = screen.screen(meth, xd, q.double(), md)
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, got, "float64 levels")
    got = screen.screen(meth, xd, q, md, minus=torch.zeros_like(xd))
    assert screen.last_route() == "fallback:minus="
    got = screen.screen(sh.method_of("ns_momentum"), sf.to_layout(case.x, "cpu"), case.q, case.mod)
    assert screen.last_route() == "fallback:input on the CPU"
    check_against_ref(case, got, "CPU inputs")
    np.testing.assert_array_equal(fused.accept().cpu().numpy(), got.accept().cpu().numpy())
    live = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, device=gpu)
    live.D_x.kernel.requires_grad_(True)
    got = screen.screen(live.residual_momentum, xd, q, md)
    assert screen.last_route() == "fallback:operator kernel requires grad"
    check_against_ref(case, got, "requires grad")
    mcase = case_of("mhd_continuity", sf.BASE)
    got = screen.screen(sh.method_of("mhd_continuity", gpu), sf.to_layout(mcase.x[:, :3].contiguous(), gpu), mcase.q.to(gpu),
                        sf.to_layout(mcase.mod, gpu))
    assert screen.last_route() == "fallback:fewer than six MHD channels"
    check_against_ref(mcase, got, "three-channel MHD continuity")
    wcase = case_of("wave", sf.BASE)
    two = torch.stack([wcase.x, wcase.x], dim=1)
    got = screen.screen(sh.method_of("wave", gpu), sf.to_layout(two, gpu), wcase.q.to(gpu), sf.to_layout(wcase.mod, gpu))
    assert screen.last_route() == "fallback:multi-channel wave input"
    # a declining library: MHD momentum whose D_t also has a tap along x is the general-star tap structure, which is not
    # built for that equation; the three-pass route applies that kernel
    pcase = case_of("mhd_momentum", sf.BASE)
    pm = sh.method_of("mhd_momentum", gpu)
    plain = run(pcase, gpu, method=pm)
    assert screen.last_route() == "fused:flat_mhd_momentum"
    pm.__self__.D_t.kernel.data[1, 0, 1] = 0.25
    odd = run(pcase, gpu, method=pm)
    assert screen.last_route() == "fallback:declined by the library"
    assert not torch.equal(sg.bits(odd.score), sg.bits(plain.score))
    # halo_x on an Nt-fastest view behaves as it did: the three-pass route with the method's own halo pass, or an error
    s = screen.Screen(case.shape[0], case.nk, gpu)
    try:
        s.add_slab(meth, xd[..., 1:-1, :], q, md[:, 1:-1], crop=(1, 0, 1), halo_x=True)
        assert screen.last_route() == "fallback:no unit stride on the last axis"
    except (RuntimeError, ValueError) as e:
        print("halo_x raises:", e)
        assert s.cells == 0


# ------------------------------------------------------------------ 7. memory
def test_screenflat_ns_momentum_memory(gpu):
    """one screen of NS momentum on memory [8,3,256,256,32] allocates less than one field beyond its inputs"""
    from cp_pre_amd import screen
    method = sh.method_of("ns_momentum", gpu)
    x = (torch.rand(8, 3, 256, 256, 32, device=gpu) + 0.5).permute(0, 1, 4, 2, 3)
    mod = (torch.rand(256, 256, 32, device=gpu) + 0.5).permute(2, 0, 1)
    q = torch.linspace(0.1, 2.0, 10, device=gpu)
    screen.screen(method, x[:1], q, mod)                      # (library load, occupancy query)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    s = screen.screen(method, x, q, mod)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert screen.last_route() == "fused:flat_ns_momentum"
    field = 8 * 32 * 256 * 256 * 4
    print(f"peak beyond the inputs: {extra} bytes (one field: {field})")
    assert extra < field
    assert s.cells == 30 * 254 * 254


def test_screenflat_reference_script_shapes_take_the_fused_route(gpu):
    """the Nt-fastest calls of Joint/NS_Residuals_CP.py and Joint/MHD_Residuals_CP.py: [BS,F,Nx,Ny,T_out] surrogate output
    seen through permute(0,1,4,2,3), 64 x 64 and 128 x 128 grids"""
    from cp_pre_amd import screen
    q = torch.linspace(0.1, 2.0, 10, device=gpu)
    for kind, F, shape in (("ns_momentum", 3, (4, 64, 64, 10)), ("mhd_continuity", 6, (4, 128, 128, 10)),
                           ("mhd_momentum", 6, (4, 128, 128, 10)), ("mhd_energy", 6, (4, 128, 128, 10)),
                           ("mhd_induction", 6, (4, 128, 128, 10)), ("mhd_gauss", 6, (4, 128, 128, 10))):
        B, X, Y, T = shape
        pred = torch.rand(B, F, X, Y, T, device=gpu) + 0.5
        s = screen.screen(sh.method_of(kind, gpu), pred.permute(0, 1, 4, 2, 3), q)
        assert screen.last_route() == sf.ROUTE[kind]
        assert s.cells == (T - 2) * (X - 2) * (Y - 2) and bool(torch.isfinite(s.score).all())


# ------------------------------------------------------------------ 8. the C client
def test_screenflat_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screenflat_check.c on the device, as a child process under a time limit: a star, NS momentum and MHD
    continuity against plain C loops, accumulation over two calls, and the argument errors of the header."""
    from test_screenflat_cpu import c_client_command
    exe = tmp_path / "screenflat_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-4000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") >= 35, out.stdout


# ------------------------------------------------------------------ the tap structures beside the reference's
@pytest.mark.parametrize("structure", sh.TAP_STRUCTURES)
@pytest.mark.parametrize("kind", sh.TAP_KINDS)
def test_screenflat_other_tap_structures_against_the_stored_residual(gpu, kind, structure):
    """The y-fixed (<4>) and general-star (<2>) instantiations of every functor compiled per tap structure, which the
    default operators never reach, against the residual stored with the same operators on the same Nt-fastest views
    (``sh.check_against_stored`` has the bounds; the levels are the default operators' case's) - and not the default
    operators' answer.  The general star of the MHD momentum is not built: the library declines."""
    from cp_pre_amd import screen
    case = case_of(kind, sf.SEAM_SHAPES["straddle_10"])
    method = sh.method_with_taps(kind, structure, gpu)
    xd = sf.to_layout(case.x, gpu)
    s = run(case, gpu, x=xd, method=method)
    built = (kind, structure) != ("mhd_momentum", "general")
    assert screen.last_route() == (sf.ROUTE[kind] if built else "fallback:declined by the library")
    assert not same(s, run(case, gpu, x=xd))
    sh.check_against_stored(case, s, method(xd, boundary=True), case.q, f"{kind} {structure} flat")
