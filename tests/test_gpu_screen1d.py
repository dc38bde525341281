"""The fused screen of the 1-D family (cp_pre_amd.screen's rows route, csrc/screen_rows.hip) on the GPU, against float64
(pytest -m gpu).

Reference, tolerances and cases: tests/screen1d_helpers.py (the oracle in float64; tau = 1e-5 max |r_ref|; score within
tau / m_min + one ulp; counts within the undecided cells; accept exact).  tests/test_screen1d_cpu.py shows, with the oracle
alone, that every case used here keeps its undecided cells below 1 % and every level further than tau / m_min from every
per-sample score, and that the seam planes cross the seams of the kernel's split rule."""
import os
import subprocess

import numpy as np
import pytest
import torch

import screen1d_helpers as s1
import stencil_guards as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


_cases = {}


def case_of(kind, B, plane, layout, boundary=False, with_mod=True, nk=10):
    """(computed once per key and left unchanged)"""
    key = (kind, B, plane, layout, boundary, with_mod, nk)
    if key not in _cases:
        _cases[key] = s1.Case(kind, s1.logical_shape(B, plane, layout), boundary, with_mod, nk)
    return _cases[key]


def run(case, layout, gpu, x=None, mod=None, method=None):
    from cp_pre_amd import screen
    xd = s1.lay(case.x, layout, gpu) if x is None else x
    md = (s1.lay(case.mod, layout, gpu) if case.mod is not None else None) if mod is None else mod
    return screen.screen(method or s1.method_of(case.kind, gpu), xd, case.q.to(gpu), md, boundary=case.boundary)


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


def three_pass(case, layout, gpu):
    """The package's own three-pass route: ``Screen._fallback`` itself."""
    from cp_pre_amd import screen
    s = screen.Screen(case.shape[0], case.nk, gpu)
    md = s1.lay(case.mod, layout, gpu) if case.mod is not None else None
    s._fallback(screen._Spec(s1.method_of(case.kind, gpu)), s1.lay(case.x, layout, gpu), case.q.to(gpu), md, case.crop, False, None)
    s.cells = case.cells
    return s.finish()


def same(a, b):
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside)


# ------------------------------------------------------------------ 1. every operator against the reference
@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", s1.KINDS)
def test_screen1d_every_operator_against_fp64_and_three_pass(gpu, kind, boundary, with_mod):
    from cp_pre_amd import screen
    for nk, name in ((10, "chunks_and_idle_lanes"), (1, "wave_segments"), (16, "partial_last_strip")):
        B, plane = s1.SEAM_PLANES[name]
        for layout in s1.LAYOUTS:
            case = case_of(kind, B, plane, layout, boundary, with_mod, nk)
            s = run(case, layout, gpu)
            assert screen.last_route() == s1.ROUTE[kind]
            check_against_ref(case, s, f"{kind} {name} {layout} boundary={boundary} mod={with_mod} nk={nk}")
            s3 = three_pass(case, layout, gpu)
            check_against_ref(case, s3, "  three-pass")
            print(f"  fused and three-pass bit-identical: {same(s, s3)}")


# ------------------------------------------------------------------ 2. the seams of the split rule
@pytest.mark.parametrize("name", list(s1.SEAM_PLANES))
@pytest.mark.parametrize("kind", ["burgers", "advection"])
def test_screen1d_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES[name]
    for layout in s1.LAYOUTS:
        for boundary in (False, True):
            case = case_of(kind, B, plane, layout, boundary)
            s = run(case, layout, gpu)
            assert screen.last_route() == s1.ROUTE[kind]
            check_against_ref(case, s, f"{kind} {name} {layout} boundary={boundary}")


# ------------------------------------------------------------------ 3. pitched, misaligned views in poisoned allocations
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", ["burgers", "dxx"])
def test_screen1d_pitched_misaligned_views_in_poisoned_memory(gpu, kind, layout):
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES["partial_last_strip"]
    case = case_of(kind, B, plane, layout)
    dense = run(case, layout, gpu)
    order, morder, row = ((0, 1, 2), (0, 1), 1) if layout == "nx" else ((0, 2, 1), (1, 0), 2)
    for offset, pitch in ((1, 5), (3, 8), (0, 4)):
        alloc, xd = sg.embed(case.x, order, {row: pitch, 0: 7}, offset, gpu)
        malloc, md = sg.embed(case.mod, morder, {row - 1: pitch + 1}, offset, gpu)
        col = 3 - row
        assert xd.stride(col) == 1 and xd.stride(row) > xd.shape[col] and md.stride(col - 1) == 1 and md.stride(row - 1) > md.shape[col - 1]
        masks = [sg.outside_mask(alloc, xd), sg.outside_mask(malloc, md)]
        for value in sg.POISONS:
            sg.poison(alloc, masks[0], value)
            sg.poison(malloc, masks[1], value)
            before = [alloc.clone(), malloc.clone()]
            got = run(case, layout, gpu, xd, md)
            assert screen.last_route() == s1.ROUTE[kind]
            assert same(got, dense), (offset, pitch, value)
            assert torch.equal(sg.bits(alloc), sg.bits(before[0])) and torch.equal(sg.bits(malloc), sg.bits(before[1]))


# ------------------------------------------------------------------ 4. the non-finite contract
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_screen1d_non_finite_contract(gpu, layout):
    B, plane = s1.SEAM_PLANES["wave_segments"]
    case = case_of("burgers", B, plane, layout)
    base = run(case, layout, gpu)
    T, X = case.shape[1:]
    # NaN in the modulation's rim changes nothing
    mod = case.mod.clone()
    mod[0], mod[-1], mod[:, 0], mod[:, -1] = [float("nan")] * 4
    assert same(run(case, layout, gpu, mod=s1.lay(mod, layout, gpu)), base)
    # NaN / inf in cropped rim cells that no counted cell's star reaches (the corners) change nothing
    x = case.x.clone()
    x[:, 0, 0], x[:, -1, -1], x[:, 0, -1], x[:, -1, 0] = float("nan"), float("inf"), float("-inf"), float("nan")
    assert same(run(case, layout, gpu, x=s1.lay(x, layout, gpu)), base)
    # a NaN in a counted cell: that sample's score is NaN, the cells it reaches are outside at every level, no other
    # sample differs (how many cells it reaches: from the package's own residual pass - the same functor)
    x = case.x.clone()
    x[1, T // 2, X // 2] = float("nan")
    xd = s1.lay(x, layout, gpu)
    got = run(case, layout, gpu, x=xd)
    r = s1.method_of("burgers", gpu)(xd, boundary=True)
    nbad = int(torch.isnan(r[1, 1:-1, 1:-1]).sum())
    assert 1 <= nbad <= 9
    assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
    others = [0, 2]
    assert torch.equal(sg.bits(got.score[others]), sg.bits(base.score[others])) and torch.equal(got.inside[:, others], base.inside[:, others])
    top = case.q.argmax()                                    # the level above every score: everything finite is inside
    assert int(got.inside[top, 1]) == case.cells - nbad
    assert bool((got.inside[:, 1] <= base.inside[:, 1]).all())
    # m = 0 with r != 0: an inf score and the cell outside; r = 0 over m = 0: NaN, as numpy's 0/0
    mod = case.mod.clone()
    mod[T // 2, X // 2] = 0.0
    md = s1.lay(mod, layout, gpu)
    got = run(case, layout, gpu, mod=md)
    assert bool(torch.isinf(got.score).all()) and bool((got.inside[top] == case.cells - 1).all())
    got = run(case, layout, gpu, x=s1.lay(torch.zeros_like(case.x), layout, gpu), mod=md)
    assert bool(torch.isnan(got.score).all())


# ------------------------------------------------------------------ 5. composition
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", ["burgers", "advection"])
def test_screen1d_slabs_compose_bit_for_bit(gpu, kind, layout):
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES["wave_segments"]
    case = case_of(kind, B, plane, layout)
    whole = run(case, layout, gpu)
    method = s1.method_of(kind, gpu)
    xd, md, q = s1.lay(case.x, layout, gpu), s1.lay(case.mod, layout, gpu), case.q.to(gpu)
    # overlapping slabs of the rows with crop 1: [0:8] counts rows 1..6, [6:12] rows 7..10.  Nx-fastest the rows are Nt
    # (axis 1), Nt-fastest they are Nx (axis 2): in both layouts the plane has 12 rows
    s = screen.Screen(B, case.nk, gpu)
    for a, b in ((0, 8), (6, 12)):
        if layout == "nx":
            s.add_slab(method, xd[:, a:b], q, md[a:b], crop=(1, 1))
        else:
            s.add_slab(method, xd[:, :, a:b], q, md[:, a:b], crop=(1, 1))
        assert screen.last_route() == s1.ROUTE[kind]
    got = s.finish()
    assert got.cells == whole.cells and same(got, whole)
    # two runs: identical bytes
    assert same(run(case, layout, gpu), whole)


# ------------------------------------------------------------------ 6. refusals and live kernels
@pytest.mark.parametrize("plane", s1.ODD_PLANES)
@pytest.mark.parametrize("kind", ["burgers", "advection"])
def test_screen1d_odd_widths_take_the_three_pass_route(gpu, kind, plane):
    from cp_pre_amd import screen
    for layout in s1.LAYOUTS:
        case = case_of(kind, plane[0], plane[1], layout)
        s = run(case, layout, gpu)
        assert screen.last_route() == "fallback:contiguous-axis length not a multiple of 4"
        check_against_ref(case, s, f"{kind} {plane} {layout}")


def test_screen1d_fallbacks_say_why_and_agree(gpu):
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    from cp_pre_amd.convops_1d import ConvOperator as C1
    B, plane = s1.SEAM_PLANES["wave_segments"]
    case = case_of("burgers", B, plane, "nx")
    fused = run(case, "nx", gpu)
    xd, md, q = case.x.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    meth = s1.method_of("burgers", gpu)
    got = screen.screen(meth, xd[:, None], q, md)                      # [BS,1,Nt,Nx]: screened as vars[:, 0]
    assert screen.last_route() == "fallback:[BS,1,Nt,Nx] input"
    check_against_ref(case, got, "[BS,1,Nt,Nx]")
    got = screen.screen(R.Burgers(s1.DX, s1.DT, s1.NU, device=gpu, fused=False).residual, xd, q, md)
    assert screen.last_route() == "fallback:fused=False"
    check_against_ref(case, got, "fused=False")
    got = screen.screen(meth, xd, q.double(), md)
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, got, "float64 levels")
    got = screen.screen(s1.method_of("burgers"), case.x, case.q, case.mod)
    assert screen.last_route() == "fallback:input on the CPU"
    check_against_ref(case, got, "CPU inputs")
    np.testing.assert_array_equal(fused.accept().cpu().numpy(), got.accept().cpu().numpy())
    zero = torch.zeros_like(xd)
    got = screen.screen(meth, xd, q, md, minus=zero)                   # (r(0) == 0: the same residual by the paired pass)
    assert screen.last_route() == "fallback:minus="
    check_against_ref(case, got, "minus=")
    live = R.Burgers(s1.DX, s1.DT, s1.NU, device=gpu)
    live.D_x.kernel.requires_grad_(True)
    got = screen.screen(live.residual, xd, q, md)
    assert screen.last_route() == "fallback:operator kernel requires grad"
    check_against_ref(case, got, "requires grad")
    dcase = case_of("dxx", B, plane, "nx")
    got = screen.screen(C1("x", 2, conv="spectral", device=gpu), xd, dcase.q.to(gpu), dcase.mod.to(gpu))
    assert screen.last_route() == "fallback:spectral operator"
    assert bool(torch.isfinite(got.score).all()) and got.cells == dcase.cells
    # a dense 3x3 kernel with a corner tap falls back (and the three-pass route applies that kernel)
    op = C1("x", 2, device=gpu)
    op.kernel.data[0, 0] = 0.0
    dense = run(dcase, "nx", gpu, method=op)
    assert screen.last_route() == "fused:rows_stencil2d" and same(dense, run(dcase, "nx", gpu))
    op.kernel.data[0, 0] = 0.5
    corner = run(dcase, "nx", gpu, method=op)
    assert screen.last_route() == "fallback:operator kernel off the 5-point star"
    assert not torch.equal(sg.bits(corner.score), sg.bits(dense.score))
    bg = R.Burgers(s1.DX, s1.DT, s1.NU, device=gpu)
    bg.D_t.kernel.data[2, 2] = 0.5
    screen.screen(bg.residual, xd, q, md)
    assert screen.last_route() == "fallback:operator kernel off the 5-point star"
    # halo_x raises for this family, before any device work
    s = screen.Screen(B, case.nk, gpu)
    for m in (meth, s1.method_of("advection", gpu), C1("x", 2, device=gpu)):
        with pytest.raises(RuntimeError, match="halo_x"):
            s.add_slab(m, xd[:, 1:-1], q, md[1:-1], crop=(0, 1), halo_x=True)
    assert s.acc is None and s.cells == 0


def test_screen1d_refused_calls_launch_nothing_and_live_kernels_are_seen(gpu):
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES["wave_segments"]
    case = case_of("burgers", B, plane, "nx")
    method = s1.method_of("burgers", gpu)
    xd, md, q = case.x.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    s = screen.Screen(B, case.nk, gpu)
    s.add_slab(method, xd, q, md, crop=(1, 1))
    assert screen.last_route() == "fused:rows_burgers"
    before = s.acc.clone()
    for bad in (lambda: s.add_slab(method, xd, q[:3], md, crop=(1, 1)), lambda: s.add_slab(method, xd, q, md[1:], crop=(1, 1)),
                lambda: s.add_slab(method, xd[:2], q, md, crop=(1, 1)), lambda: s.add_slab(method, xd, q, md, crop=(9, 1)),
                lambda: s.add_slab(method, xd, q, md, crop=(1, 1, 1))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="halo_x"):
        s.add_slab(method, xd, q, md, crop=(1, 1), halo_x=True)
    torch.cuda.synchronize()
    assert torch.equal(s.acc, before) and s.cells == case.cells
    # a kernel mutated through .data between two calls is seen by the second
    a = screen.screen(method, xd, q, md)
    method.__self__.D_x.kernel.data.mul_(2.0)
    b = screen.screen(method, xd, q, md)
    method.__self__.D_x.kernel.data.mul_(0.5)
    c = screen.screen(method, xd, q, md)
    assert screen.last_route() == "fused:rows_burgers"
    assert not torch.equal(sg.bits(a.score), sg.bits(b.score)) and same(a, c)


# ------------------------------------------------------------------ 7. memory
def test_screen1d_burgers_memory(gpu):
    """one screen of Burgers on [64,200,512] allocates less than one field beyond its inputs, in both layouts"""
    from cp_pre_amd import screen
    method = s1.method_of("burgers", gpu)
    q = torch.linspace(0.1, 2.0, 10, device=gpu)
    for layout in s1.LAYOUTS:
        x = torch.rand(64, 200, 512, device=gpu) + 0.5
        mod = torch.rand(200, 512, device=gpu) + 0.5
        if layout == "nt":
            x, mod = x.transpose(1, 2).contiguous().transpose(1, 2), mod.t().contiguous().t()
        screen.screen(method, x[:1], q, mod)                      # (library load, occupancy query)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        s = screen.screen(method, x, q, mod)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base
        assert screen.last_route() == "fused:rows_burgers"
        field = 64 * 200 * 512 * 4
        print(f"{layout}: peak beyond the inputs: {extra} bytes (one field: {field})")
        assert extra < field
        assert s.cells == 198 * 510


# ------------------------------------------------------------------ 8. the C client
def test_screen1d_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screen1d_check.c on the device: both entries against plain C loops, both layouts, accumulation over two
    calls, and every argument error."""
    from test_screen1d_cpu import c_client_command
    exe = tmp_path / "screen1d_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") >= 50, out.stdout
