"""The fused screen (cp_pre_amd.screen, csrc/screen_march.hip) on the GPU, against float64 (pytest -m gpu).

Reference, tolerances and cases: tests/screen_helpers.py (the oracle in float64; tau = 1e-5 max |r_ref|; score within
tau / m_min + one ulp; counts within the undecided cells; accept exact).  tests/test_screen_cpu.py shows, with the oracle
alone, that every case used here keeps its undecided cells below 1 % and every level further than tau / m_min from every
per-sample score."""
import numpy as np
import pytest
import torch

import screen_helpers as sh
import stencil_guards as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(case, gpu, x=None, mod=None, method=None):
    from cp_pre_amd import screen
    xd = case.x.to(gpu) if x is None else x
    md = (case.mod.to(gpu) if case.mod is not None else None) if mod is None else mod
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
    """The package's own three-pass route: the same functions the fallback calls."""
    from cp_pre_amd import inductive_cp as icp
    from cp_pre_amd import pipeline
    method = sh.method_of(case.kind, gpu)
    xd = case.x.to(gpu)
    res = method(xd) if case.kind == "lap" else method(xd, boundary=True)
    reg = sh.region(case.shape, case.crop)
    mod = case.mod.to(gpu) if case.mod is not None else torch.ones(case.shape[1:], device=gpu)
    if case.boundary:
        score = icp.ncf_metric_joint(res, None, mod)
    else:
        score = icp.ncf_metric_joint(res, None, mod, crop=1)
    q = case.q.to(gpu)
    counts = torch.empty(case.nk, case.shape[0], dtype=torch.int64, device=gpu)
    cov = pipeline.CoverageLevels(1, case.nk, gpu)
    for i in range(case.shape[0]):
        cov.acc.zero_()
        cov.add_slab(res[reg][i:i + 1], q, modulation=mod[reg[1:]] if case.mod is not None else None)
        counts[:, i] = cov.acc
    return score, counts


@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", sh.KINDS)
def test_screen_every_kind_against_fp64_and_three_pass(gpu, kind, boundary, with_mod):
    from cp_pre_amd import screen
    for nk, shape in ((10, sh.SEAM_SHAPES["two_tseg"]), (1, sh.SEAM_SHAPES["rows2_narrow"]), (16, sh.SEAM_SHAPES["rows3_wide"])):
        case = sh.Case(kind, shape, boundary, with_mod, nk)
        s = run(case, gpu)
        assert screen.last_route() == "fused:" + sh.FUSED_KIND[kind]
        check_against_ref(case, s, f"{kind} {shape} boundary={boundary} mod={with_mod} nk={nk}")
        score3, counts3 = three_pass(case, gpu)
        s3 = screen.Screened(score3, counts3, case.cells)
        check_against_ref(case, s3, "  three-pass")
        same = torch.equal(sg.bits(s.score), sg.bits(score3)) and torch.equal(s.inside, counts3)
        print(f"  fused and three-pass bit-identical: {same}")


@pytest.mark.parametrize("name", list(sh.SEAM_SHAPES))
@pytest.mark.parametrize("kind", ["ns_momentum", "lap", "mhd_momentum"])
def test_screen_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = sh.Case(kind, sh.SEAM_SHAPES[name], boundary, True, 10)
        s = run(case, gpu)
        assert screen.last_route() == "fused:" + sh.FUSED_KIND[kind]
        check_against_ref(case, s, f"{kind} {name} boundary={boundary}")


@pytest.mark.parametrize("shape", sh.ODD_SHAPES)
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_screen_odd_widths_give_the_same_answers_by_their_route(gpu, kind, shape):
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = sh.Case(kind, shape, boundary, True, 10)
        s = run(case, gpu)
        print(kind, shape, screen.last_route())
        assert screen.last_route().startswith(("fused:", "fallback:"))
        check_against_ref(case, s, f"{kind} {shape} boundary={boundary} ({screen.last_route()})")


def _embed(case, gpu, offset, pitch):
    """``vars[:, i]`` views of a stacked tensor with two more channels, rows ``pitch`` floats further apart than they are
    long, the base ``offset`` floats off the allocation's 16-byte boundary, in a guarded allocation."""
    x = case.x
    if sh.NCHAN[case.kind] is None:
        big = torch.zeros((x.shape[0], 3) + tuple(x.shape[1:]))
        big[:, 1] = x
    else:
        big = torch.zeros((x.shape[0], x.shape[1] + 2) + tuple(x.shape[2:]))
        big[:, 1:-1] = x
    alloc, view = sg.embed(big, None, {big.dim() - 2: pitch}, offset, gpu)
    return alloc, (view[:, 1] if sh.NCHAN[case.kind] is None else view[:, 1:-1])


@pytest.mark.parametrize("kind", ["ns_momentum", "wave", "mhd_energy"])
def test_screen_pitched_misaligned_views_in_poisoned_memory(gpu, kind):
    from cp_pre_amd import screen
    case = sh.Case(kind, sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    dense = run(case, gpu)
    for offset, pitch in ((1, 5), (3, 8), (0, 4)):
        alloc, xd = _embed(case, gpu, offset, pitch)
        malloc, md = sg.embed(case.mod, None, {1: pitch + 1}, offset, gpu)
        assert xd.stride(-2) > xd.shape[-1] and xd.stride(-1) == 1 and md.stride(1) > md.shape[2]
        masks = [sg.outside_mask(alloc, xd), sg.outside_mask(malloc, md)]
        for value in sg.POISONS:
            sg.poison(alloc, masks[0], value)
            sg.poison(malloc, masks[1], value)
            before = [alloc.clone(), malloc.clone()]
            got = run(case, gpu, xd, md)
            assert screen.last_route() == "fused:" + sh.FUSED_KIND[kind]
            assert torch.equal(sg.bits(got.score), sg.bits(dense.score)) and torch.equal(got.inside, dense.inside), (offset, pitch, value)
            assert torch.equal(sg.bits(alloc), sg.bits(before[0])) and torch.equal(sg.bits(malloc), sg.bits(before[1]))


def test_screen_non_finite_contract(gpu):
    from cp_pre_amd import screen
    case = sh.Case("ns_momentum", sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    base = run(case, gpu)
    B, T, X, Y = case.shape
    # a NaN in the modulation's rim changes nothing
    mod = case.mod.clone()
    mod[0], mod[-1], mod[:, 0], mod[:, -1], mod[:, :, 0], mod[:, :, -1] = [float("nan")] * 6
    got = run(case, gpu, mod=mod.to(gpu))
    assert torch.equal(sg.bits(got.score), sg.bits(base.score)) and torch.equal(got.inside, base.inside)
    # a NaN residual in a cropped rim cell changes nothing: NaN in p at the corner (0, 0, 0) reaches, through the star, only
    # residual cells with a zero index - all of them in the rim
    x = case.x.clone()
    x[1, 2, 0, 0, 0] = float("nan")
    got = run(case, gpu, x=x.to(gpu))
    assert torch.equal(sg.bits(got.score), sg.bits(base.score)) and torch.equal(got.inside, base.inside)
    # a NaN in a counted cell: that sample's score is NaN, the cells it reaches are outside at every level, no other sample differs
    x = case.x.clone()
    x[1, 0, 2, 5, 7] = float("nan")
    got = run(case, gpu, x=x.to(gpu))
    # (how many cells the NaN reaches: from the package's own residual pass - the same functor; the oracle's dense 3x3x3
    # convolution multiplies the NaN by its zero weights too)
    r = sh.method_of("ns_momentum", gpu)(x.to(gpu), boundary=True)
    nbad = int(torch.isnan(r[sh.region(case.shape, case.crop)][1]).sum())
    assert 1 <= nbad <= 27
    assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
    others = [0, 2]
    assert torch.equal(sg.bits(got.score[others]), sg.bits(base.score[others])) and torch.equal(got.inside[:, others], base.inside[:, others])
    top = case.q.argmax()                                    # the level above every score: everything finite is inside
    assert int(got.inside[top, 1]) == case.cells - nbad
    assert bool((got.inside[:, 1] <= base.inside[:, 1]).all())
    # m = 0 with r != 0: an inf score and the cell outside; r = 0 over m = 0: NaN, as numpy's 0/0
    mod = case.mod.clone()
    mod[2, 5, 7] = 0.0
    got = run(case, gpu, mod=mod.to(gpu))
    assert bool(torch.isinf(got.score).all()) and bool((got.inside[top] == case.cells - 1).all())
    zero = torch.zeros_like(case.x)
    got = run(case, gpu, x=zero.to(gpu), mod=mod.to(gpu))
    assert bool(torch.isnan(got.score).all())
    want = np.max(np.abs(np.zeros(3, np.float32)) / np.array([1.0, 0.0, 2.0], np.float32))
    assert np.isnan(want)


def test_screen_slabs_compose_bit_for_bit(gpu):
    from cp_pre_amd import screen
    kind, shape = "ns_momentum", (3, 12, 41, 64)
    case = sh.Case(kind, shape, False, True, 10)
    whole = run(case, gpu)
    method = sh.method_of(kind, gpu)
    xd, md, q = case.x.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    X = shape[2]
    # x-slabs of unequal length with halo rows, the rim rows left out by the cut itself
    s = screen.Screen(shape[0], case.nk, gpu)
    for x0, x1 in ((1, 10), (10, 33), (33, X - 1)):
        s.add_slab(method, xd[:, :, :, x0:x1], q, md[:, x0:x1], crop=(1, 0, 1), halo_x=True)
        assert screen.last_route() == "fused:ns_momentum"
    got = s.finish()
    assert got.cells == whole.cells
    assert torch.equal(sg.bits(got.score), sg.bits(whole.score)) and torch.equal(got.inside, whole.inside)
    # non-finite values where only PRE_FLAG_HALO_X makes the kernel load them - the halo row before the first slab and the
    # row at the end of the last one (which the x == X threads of the partial last tile load as their own and evaluate) -
    # at positions no counted cell's star reaches (column 0 / the last column, the first / last plane): nothing changes
    xp = case.x.clone()
    xp[:, :, :, 0, 0], xp[:, :, 0, 0, :] = float("nan"), float("inf")
    xp[:, :, :, X - 1, -1], xp[:, :, -1, X - 1, :] = float("inf"), float("nan")
    xpd = xp.to(gpu)
    s = screen.Screen(shape[0], case.nk, gpu)
    for x0, x1 in ((1, 10), (10, 33), (33, X - 1)):
        s.add_slab(method, xpd[:, :, :, x0:x1], q, md[:, x0:x1], crop=(1, 0, 1), halo_x=True)
        assert screen.last_route() == "fused:ns_momentum"
    got = s.finish()
    assert torch.equal(sg.bits(got.score), sg.bits(whole.score)) and torch.equal(got.inside, whole.inside)
    got = run(case, gpu, x=xpd)                              # (the same cells as rim cells of the whole grid)
    assert torch.equal(sg.bits(got.score), sg.bits(whole.score)) and torch.equal(got.inside, whole.inside)
    # t-slabs with their halo planes
    s = screen.Screen(shape[0], case.nk, gpu)
    for t0, t1 in ((0, 8), (6, 12)):
        s.add_slab(method, xd[:, :, t0:t1], q, md[t0:t1], crop=(1, 1, 1))
    got = s.finish()
    assert got.cells == whole.cells
    assert torch.equal(sg.bits(got.score), sg.bits(whole.score)) and torch.equal(got.inside, whole.inside)
    # two runs: identical bytes
    again = run(case, gpu)
    assert torch.equal(sg.bits(again.score), sg.bits(whole.score)) and torch.equal(again.inside, whole.inside)


@pytest.mark.parametrize("kind", ["lap", "ns_continuity", "mhd_gauss", "ns_momentum", "wave"])
def test_screen_halo_x_slab_that_cannot_fuse_equals_the_whole_grid_or_raises(gpu, kind):
    """an x-slab of an odd-width grid declines the fused launch; with halo_x it must then equal the whole grid or raise -
    never be evaluated against zero padding and counted"""
    from cp_pre_amd import screen
    shape = (3, 5, 20, 13)
    case = sh.Case(kind, shape, False, True, 4)
    whole = run(case, gpu)
    assert screen.last_route().startswith("fallback:")
    method = sh.method_of(kind, gpu)
    xd, md, q = case.x.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    s = screen.Screen(shape[0], case.nk, gpu)
    try:
        for x0, x1 in ((1, 8), (8, shape[2] - 1)):
            s.add_slab(method, xd[..., x0:x1, :], q, md[:, x0:x1], crop=(1, 0, 1), halo_x=True)
    except (RuntimeError, ValueError) as e:
        print(kind, "raises:", e)
        assert s.cells == 0
        return
    got = s.finish()
    assert torch.equal(sg.bits(got.score), sg.bits(whole.score)) and torch.equal(got.inside, whole.inside)


def test_screen_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screen_check.c on the device: scores and counts of the wave star against plain C loops, two t-slabs
    against the whole grid, PRE_FLAG_INTERIOR_T, and the argument errors of every pre_screen_* entry."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "screen_check"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(root, "tests", "c_abi", "screen_check.c"), "-I" + os.path.join(root, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(root, "cp_pre_amd"), "-l:libcp_pre_screen.so",
                           "-Wl,-rpath," + os.path.join(root, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") >= 20, out.stdout


def test_screen_refused_calls_launch_nothing_and_live_kernels_are_seen(gpu):
    from cp_pre_amd import screen
    case = sh.Case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    method = sh.method_of("ns_momentum", gpu)
    xd, md, q = case.x.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    s = screen.Screen(case.shape[0], case.nk, gpu)
    s.add_slab(method, xd, q, md)
    before = s.acc.clone()
    for bad in (lambda: s.add_slab(method, xd, q[:3], md), lambda: s.add_slab(method, xd, q, md[1:]),
                lambda: s.add_slab(method, xd[:2], q, md), lambda: s.add_slab(method, xd, q, md, crop=(9, 1, 1))):
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
    assert not torch.equal(sg.bits(a.score), sg.bits(b.score))
    assert torch.equal(sg.bits(a.score), sg.bits(c.score)) and torch.equal(a.inside, c.inside)


def test_screen_fallbacks_say_why_and_agree(gpu):
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    case = sh.Case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    fused = run(case, gpu)
    ns = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, device=gpu, fused=False)
    got = screen.screen(ns.residual_momentum, case.x.to(gpu), case.q.to(gpu), case.mod.to(gpu))
    assert screen.last_route() == "fallback:fused=False"
    check_against_ref(case, got, "fused=False")
    got = screen.screen(sh.method_of("ns_momentum", gpu), case.x.to(gpu), case.q.double().to(gpu), case.mod.to(gpu))
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, got, "float64 levels")
    got = screen.screen(sh.method_of("ns_momentum"), case.x, case.q, case.mod)
    assert screen.last_route() == "fallback:input on the CPU"
    check_against_ref(case, got, "CPU inputs")
    np.testing.assert_array_equal(fused.accept().cpu().numpy(), got.accept().cpu().numpy())
    # MHD continuity reads three channels; pre_screen_mhd_f32 takes six views: a three-channel input takes the three-pass route
    case = sh.Case("mhd_continuity", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    got = screen.screen(sh.method_of("mhd_continuity", gpu), case.x[:, :3].contiguous().to(gpu), case.q.to(gpu), case.mod.to(gpu))
    assert screen.last_route() == "fallback:fewer than six MHD channels"
    check_against_ref(case, got, "three-channel MHD continuity")
    with pytest.raises(ValueError, match="this Screen was made for"):
        screen.Screen(3, 10, "cpu").add_slab(sh.method_of("mhd_continuity", gpu), case.x.to(gpu), case.q.to(gpu), case.mod.to(gpu))


def test_screen_ns_momentum_memory(gpu):
    """one screen of NS momentum on [8,3,32,256,256] allocates less than one single-field tensor beyond its inputs"""
    from cp_pre_amd import screen
    method = sh.method_of("ns_momentum", gpu)
    x = torch.rand(8, 3, 32, 256, 256, device=gpu) + 0.5
    mod = torch.rand(32, 256, 256, device=gpu) + 0.5
    q = torch.linspace(0.1, 2.0, 10, device=gpu)
    screen.screen(method, x[:1], q, mod)                      # (library load, occupancy query)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    s = screen.screen(method, x, q, mod)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert screen.last_route() == "fused:ns_momentum"
    field = 8 * 32 * 256 * 256 * 4
    print(f"peak beyond the inputs: {extra} bytes (one field: {field})")
    assert extra < field
    assert s.cells == 30 * 254 * 254


# ------------------------------------------------------------------ the tap structures beside the reference's
@pytest.mark.parametrize("structure", sh.TAP_STRUCTURES)
@pytest.mark.parametrize("kind", sh.TAP_KINDS)
def test_screen_other_tap_structures_against_the_stored_residual(gpu, kind, structure):
    """The y-fixed (<1>) and general-star (<2>) instantiations of every functor compiled per tap structure, which the
    default operators never reach, against the residual stored with the same operators (``sh.check_against_stored`` has the
    bounds; the levels are the default operators' case's: what they split does not matter here) - and not the default
    operators' answer.  The general star of the MHD energy is not built: the library declines."""
    from cp_pre_amd import screen
    case = sh.Case(kind, sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    method = sh.method_with_taps(kind, structure, gpu)
    xd = case.x.to(gpu)
    s = run(case, gpu, x=xd, method=method)
    built = (kind, structure) != ("mhd_energy", "general")
    assert screen.last_route() == ("fused:" + sh.FUSED_KIND[kind] if built else "fallback:declined by the library")
    plain = run(case, gpu, x=xd)
    assert not (torch.equal(sg.bits(s.score), sg.bits(plain.score)) and torch.equal(s.inside, plain.inside))
    sh.check_against_stored(case, s, method(xd, boundary=True), case.q, f"{kind} {structure}")
