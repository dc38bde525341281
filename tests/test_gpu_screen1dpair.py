"""The opt-in paired screen of the 1-D family (cp_pre_amd.screen with ``minus=`` and ``pair="rows"``,
csrc/screen_rows_pair.hip) on the GPU, against float64 (pytest -m gpu).

Reference, tolerances and cases: tests/screen1dpair_helpers.py (the oracle in float64 on both sets, d_ref = r_ref(a) -
r_ref(b); tau = 1e-5 (max |r_ref(a)| + max |r_ref(b)|); score within tau / m_min + one ulp; counts within the undecided
cells; accept exact).  Planes and layouts are those of tests/screen1d_helpers.py, all but one with B = 3.
tests/test_screen1dpair_cpu.py shows, with the oracle alone, that every case compared with the reference here meets the caps
the tolerances rest on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import screen1d_helpers as s1
import screen1dpair_helpers as p1
import stencil_guards as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def put(t, layout, device):
    return None if t is None else s1.lay(t, layout, device)


def run(case, layout, gpu, x=None, y=None, mod="native", method=None, pair="rows", q=None):
    from cp_pre_amd import screen
    xd = put(case.x, layout, gpu) if x is None else x
    yd = put(case.y, layout, gpu) if y is None else y
    md = put(case.mod, layout, gpu) if isinstance(mod, str) else mod
    method = method or s1.method_of(case.kind, gpu)
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


def is_zero(s, cells):
    """score bits exactly +0 and every counted cell inside at every level"""
    return not bool(sg.bits(s.score).any()) and bool((s.inside == cells).all())


# ------------------------------------------------------------------ 1. every kind, both layouts, against fp64 and the three passes
@pytest.mark.parametrize("with_mod", [False, True], ids=["nomod", "mod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("layout", p1.LAYOUTS)
@pytest.mark.parametrize("kind", p1.KINDS)
def test_screen1dpair_every_kind_against_fp64_and_three_pass(gpu, kind, layout, boundary, with_mod):
    from cp_pre_amd import screen
    for nk in p1.NKS:
        case = p1.case(kind, *p1.BASE, layout, boundary, with_mod, nk)
        xd, yd, md = put(case.x, layout, gpu), put(case.y, layout, gpu), put(case.mod, layout, gpu)
        assert (xd.stride(1) == 1) == (layout == "nt") and (xd.stride(2) == 1) == (layout == "nx")
        s = run(case, layout, gpu, x=xd, y=yd, mod=md)
        assert screen.last_route() == p1.ROUTE[kind]
        check_against_ref(case, s, f"{kind} {layout} boundary={boundary} mod={with_mod} nk={nk}")
        s3 = run(case, layout, gpu, x=xd, y=yd, mod=md, pair=False)
        assert screen.last_route() == "fallback:minus="
        check_against_ref(case, s3, "  three-pass")
        check_against_route(case, s, s3, "  fused against three-pass")


# ------------------------------------------------------------------ 2. the seams of the split rule
@pytest.mark.parametrize("name", list(s1.SEAM_PLANES))
@pytest.mark.parametrize("kind", p1.SEAM_KINDS)
def test_screen1dpair_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES[name]
    for layout in p1.LAYOUTS:
        for boundary in (False, True):
            case = p1.case(kind, B, plane, layout, boundary)
            s = run(case, layout, gpu)
            assert screen.last_route() == p1.ROUTE[kind]
            check_against_ref(case, s, f"{kind} {name} {layout} boundary={boundary}")


# ------------------------------------------------------------------ 3. two pitches, misaligned views, poisoned allocations
@pytest.mark.parametrize("layout", p1.LAYOUTS)
@pytest.mark.parametrize("kind", ["burgers", "dxx"])
def test_screen1dpair_sets_of_different_pitch_in_poisoned_memory(gpu, kind, layout):
    """the truth and the prediction carry DIFFERENT row and sample pitches and base misalignments; whatever lies between
    their rows (NaN, 0, 1e30), the result has the bits of the dense run and nothing is written"""
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES["partial_last_strip"]
    case = p1.case(kind, B, plane, layout)
    dense = run(case, layout, gpu)
    order, morder, row = ((0, 1, 2), (0, 1), 1) if layout == "nx" else ((0, 2, 1), (1, 0), 2)
    col = 3 - row
    for (ox, px, bx), (oy, py, by) in (((1, 5, 7), (3, 8, 0)), ((0, 4, 0), (2, 12, 9)), ((0, 0, 0), (1, 3, 5))):
        ax, xd = sg.embed(case.x, order, {row: px, 0: bx}, ox, gpu)
        ay, yd = sg.embed(case.y, order, {row: py, 0: by}, oy, gpu)
        am, md = sg.embed(case.mod, morder, {row - 1: px + 1}, ox, gpu)
        assert xd.stride(col) == 1 and yd.stride(col) == 1 and md.stride(col - 1) == 1
        assert xd.stride(row) != yd.stride(row) and xd.stride(0) != yd.stride(0) and yd.stride(row) > yd.shape[col]
        allocs = [ax, ay, am]
        masks = [sg.outside_mask(a, v) for a, v in zip(allocs, (xd, yd, md))]
        for value in sg.POISONS:
            for a, m in zip(allocs, masks):
                sg.poison(a, m, value)
            before = [a.clone() for a in allocs]
            got = run(case, layout, gpu, x=xd, y=yd, mod=md)
            assert screen.last_route() == p1.ROUTE[kind]
            assert same(got, dense), (ox, px, oy, py, value)
            assert all(torch.equal(sg.bits(a), sg.bits(b)) for a, b in zip(allocs, before))


# ------------------------------------------------------------------ 4. minus = vars: exactly zero
@pytest.mark.parametrize("layout", p1.LAYOUTS)
@pytest.mark.parametrize("kind", p1.KINDS)
def test_screen1dpair_minus_equal_to_vars_gives_exactly_zero(gpu, kind, layout):
    """the same tensor and an equal copy: both halves of the paired functor round alike, so d is +-0 in every cell - score
    bits exactly 0 and every counted cell inside at every level (q_k * m >= 0)"""
    from cp_pre_amd import screen
    for boundary in (False, True):
        case = p1.case(kind, *p1.BASE, layout, boundary)
        xd = put(case.x, layout, gpu)
        for yd in (xd, xd.clone(memory_format=torch.preserve_format)):
            s = run(case, layout, gpu, x=xd, y=yd)
            assert screen.last_route() == p1.ROUTE[kind]
            assert is_zero(s, case.cells), (kind, layout, boundary, s.score, s.inside)


# ------------------------------------------------------------------ 5. the non-finite contract
@pytest.mark.parametrize("layout", p1.LAYOUTS)
def test_screen1dpair_non_finite_contract(gpu, layout):
    case = p1.case("burgers", *p1.BASE, layout)
    base = run(case, layout, gpu)
    T, X = case.shape[1:]
    # NaN / inf in cropped rim cells of EITHER set that no counted cell's star reaches (the corners) change nothing
    for which in ("x", "y"):
        t = getattr(case, which).clone()
        t[:, 0, 0], t[:, -1, -1], t[:, 0, -1], t[:, -1, 0] = float("nan"), float("inf"), float("-inf"), float("nan")
        assert same(run(case, layout, gpu, **{which: put(t, layout, gpu)}), base), which
    # NaN in the modulation's rim changes nothing
    mod = case.mod.clone()
    mod[0], mod[-1], mod[:, 0], mod[:, -1] = [float("nan")] * 4
    assert same(run(case, layout, gpu, mod=put(mod, layout, gpu)), base)
    # a NaN in one counted cell of the PREDICTION: that sample's score is NaN, the cells it reaches are outside at every
    # level, no other sample differs (how many cells it reaches: from the package's own residual pass - the same functor)
    y = case.y.clone()
    y[1, T // 2, X // 2] = float("nan")
    yd = put(y, layout, gpu)
    got = run(case, layout, gpu, y=yd)
    r = s1.method_of("burgers", gpu)(yd, boundary=True)
    nbad = int(torch.isnan(r[1, 1:-1, 1:-1]).sum())
    assert 1 <= nbad <= 9
    assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
    others = [0, 2]
    assert torch.equal(sg.bits(got.score[others]), sg.bits(base.score[others])) and torch.equal(got.inside[:, others], base.inside[:, others])
    top = case.q.argmax()                                    # the level above every score: everything finite is inside
    assert int(got.inside[top, 1]) == case.cells - nbad
    assert bool((got.inside[:, 1] <= base.inside[:, 1]).all())
    three = run(case, layout, gpu, y=yd, pair=False)
    assert bool(torch.isnan(three.score[1])) and torch.equal(three.inside[top], got.inside[top])


# ------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("layout", p1.LAYOUTS)
@pytest.mark.parametrize("kind", ["burgers", "advection"])
def test_screen1dpair_row_slabs_compose_bit_for_bit(gpu, kind, layout):
    from cp_pre_amd import screen
    B, plane = p1.BASE
    case = p1.case(kind, B, plane, layout)
    whole = run(case, layout, gpu)
    method = s1.method_of(kind, gpu)
    xd, yd, md, q = put(case.x, layout, gpu), put(case.y, layout, gpu), put(case.mod, layout, gpu), case.q.to(gpu)
    # overlapping slabs of the ROWS with crop 1: [0:8] counts rows 1..6, [6:12] rows 7..10.  Nx-fastest the rows are Nt
    # (axis 1), Nt-fastest they are Nx (axis 2): in both layouts the plane has 12 rows
    s = screen.Screen(B, case.nk, gpu)
    for a, b in ((0, 8), (6, 12)):
        if layout == "nx":
            s.add_slab(method, xd[:, a:b], q, md[a:b], crop=(1, 1), minus=yd[:, a:b], pair="rows")
        else:
            s.add_slab(method, xd[:, :, a:b], q, md[:, a:b], crop=(1, 1), minus=yd[:, :, a:b], pair="rows")
        assert screen.last_route() == p1.ROUTE[kind]
    got = s.finish()
    assert got.cells == whole.cells and same(got, whole)
    # two runs: identical bytes
    assert same(run(case, layout, gpu), whole)


# ------------------------------------------------------------------ 7. the general star of Burgers
@pytest.mark.parametrize("layout", p1.LAYOUTS)
def test_screen1dpair_general_star_burgers(gpu, layout):
    """Burgers with a D_t kernel that carries an x tap: neither Burgers<0> nor Burgers<3>, the general star
    Paired<Burgers<2>>.  Reference: the three-pass route of the same method, whose fp32 residuals give tau and the undecided
    cells as the helpers derive them from the oracle's; minus = vars is exactly 0 here too."""
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    case = p1.case("burgers", *p1.BASE, layout)
    bg = R.Burgers(s1.DX, s1.DT, s1.NU, device=gpu)
    bg.D_t.kernel.data[1, 0] = 0.25
    xd, yd, md, q = put(case.x, layout, gpu), put(case.y, layout, gpu), put(case.mod, layout, gpu), case.q.to(gpu)
    s = run(case, layout, gpu, x=xd, y=yd, mod=md, method=bg.residual)
    assert screen.last_route() == "fused:rows_pair_burgers"
    assert not same(s, run(case, layout, gpu))                   # (the x tap is applied)
    s3 = run(case, layout, gpu, x=xd, y=yd, mod=md, method=bg.residual, pair=False)
    assert screen.last_route() == "fallback:minus="
    ra, rb = bg.residual(xd, boundary=True).double().cpu(), bg.residual(yd, boundary=True).double().cpu()
    tau = 1e-5 * (float(ra.abs().max()) + float(rb.abs().max()))
    d = (ra - rb)[:, 1:-1, 1:-1].abs().reshape(ra.shape[0], -1)
    m = case.mod.double()[1:-1, 1:-1].reshape(-1)
    und = ((d[None] - (case.q.double()[:, None] * m[None])[:, None]).abs() <= tau).sum(dim=2)
    err = (s.score.cpu().double() - s3.score.cpu().double()).abs()
    ulp = torch.from_numpy(np.spacing(s3.score.cpu().numpy()).astype(np.float64))
    dcount = (s.inside.cpu() - s3.inside.cpu()).abs()
    print(f"general star {layout}: score diff {float(err.max()):.3e} (allowed {tau / float(m.min()):.3e} + ulp), count diff max "
          f"{int(dcount.max())} (undecided max {int(und.max())}), bit-identical: {same(s, s3)}")
    assert bool((err <= tau / float(m.min()) + ulp).all()) and bool((dcount <= und).all())
    for y0 in (xd, xd.clone(memory_format=torch.preserve_format)):
        assert is_zero(run(case, layout, gpu, x=xd, y=y0, mod=md, method=bg.residual), case.cells)
        assert screen.last_route() == "fused:rows_pair_burgers"


# ------------------------------------------------------------------ 8. the fallbacks
@pytest.mark.parametrize("plane", s1.ODD_PLANES)
@pytest.mark.parametrize("kind", p1.SEAM_KINDS)
def test_screen1dpair_odd_widths_take_the_three_pass_route(gpu, kind, plane):
    from cp_pre_amd import screen
    for layout in p1.LAYOUTS:
        case = p1.case(kind, plane[0], plane[1], layout)
        s = run(case, layout, gpu)
        assert screen.last_route() == "fallback:contiguous-axis length not a multiple of 4"
        check_against_ref(case, s, f"{kind} {plane} {layout}")


def test_screen1dpair_fallbacks_say_why_and_agree(gpu, monkeypatch):
    from cp_pre_amd import _lib, screen
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_1d import ConvOperator as C1
    B, plane = p1.BASE
    case = p1.case("burgers", B, plane, "nx")
    fused = run(case, "nx", gpu)
    assert screen.last_route() == "fused:rows_pair_burgers"
    three = run(case, "nx", gpu, pair=False)
    xd, yd, md, q = case.x.to(gpu), case.y.to(gpu), case.mod.to(gpu), case.q.to(gpu)
    meth = s1.method_of("burgers", gpu)

    def falls(why, s):
        assert screen.last_route() == "fallback:" + why, screen.last_route()
        check_against_ref(case, s, why)
        check_against_route(case, fused, s, "  fused against it")
        assert torch.equal(s.accept(), three.accept()), why

    falls("field sets in different layouts", run(case, "nx", gpu, y=put(case.y, "nt", gpu)))
    falls("field sets in different layouts", run(case, "nx", gpu, x=put(case.x, "nt", gpu)))
    wide = torch.zeros(B, 2 * plane[0], 2 * plane[1], device=gpu)
    wide[:, ::2, ::2] = yd
    falls("minus: no unit-stride axis", run(case, "nx", gpu, y=wide[:, ::2, ::2]))
    s = screen.screen(meth, xd[:, None], q, md, minus=yd[:, None], pair="rows")
    falls("[BS,1,Nt,Nx] input", s)
    s = screen.screen(s1.method_of("burgers"), case.x, case.q, case.mod, minus=case.y, pair="rows")
    assert screen.last_route() == "fallback:input on the CPU"
    check_against_ref(case, s, "CPU inputs")
    s = screen.screen(meth, xd, q, md, minus=case.y.to(gpu), pair="rows")
    assert screen.last_route() == "fused:rows_pair_burgers" and same(s, fused)
    s = screen.screen(meth, xd, q.double(), md, minus=yd, pair="rows")
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, s, "float64 levels")
    s = screen.screen(meth, xd, q, md.double(), minus=yd, pair="rows")
    assert screen.last_route() == "fallback:float64 levels or modulation"
    check_against_ref(case, s, "float64 modulation")
    falls("fused=False", run(case, "nx", gpu, method=R.Burgers(s1.DX, s1.DT, s1.NU, device=gpu, fused=False).residual))
    live = R.Burgers(s1.DX, s1.DT, s1.NU, device=gpu)
    live.D_x.kernel.requires_grad_(True)
    falls("operator kernel requires grad", run(case, "nx", gpu, method=live.residual))
    dcase = p1.case("dxx", B, plane, "nx")
    got = run(dcase, "nx", gpu, method=C1("x", 2, conv="spectral", device=gpu))
    assert screen.last_route() == "fallback:spectral operator"
    assert bool(torch.isfinite(got.score).all()) and got.cells == dcase.cells
    # a dense 3x3 kernel with a corner tap falls back (and the three-pass route applies that kernel)
    op = C1("x", 2, device=gpu)
    op.kernel.data[0, 0] = 0.0
    dense = run(dcase, "nx", gpu, method=op)
    assert screen.last_route() == "fused:rows_pair_stencil2d" and same(dense, run(dcase, "nx", gpu))
    op.kernel.data[0, 0] = 0.5
    corner = run(dcase, "nx", gpu, method=op)
    assert screen.last_route() == "fallback:operator kernel off the 5-point star"
    assert not torch.equal(sg.bits(corner.score), sg.bits(dense.score))
    bgc = R.Burgers(s1.DX, s1.DT, s1.NU, device=gpu)
    bgc.D_t.kernel.data[2, 2] = 0.5
    run(case, "nx", gpu, method=bgc.residual)
    assert screen.last_route() == "fallback:operator kernel off the 5-point star"
    # halo_x raises for this family, before any device work
    sc = screen.Screen(B, case.nk, gpu)
    for m in (meth, s1.method_of("advection", gpu), C1("x", 2, device=gpu)):
        with pytest.raises(RuntimeError, match="halo_x"):
            sc.add_slab(m, xd[:, 1:-1], q, md[1:-1], crop=(0, 1), halo_x=True, minus=yd[:, 1:-1], pair="rows")
    assert sc.acc is None and sc.cells == 0
    # the library declines (its code, returned in place of the launch): the three-pass route, named
    monkeypatch.setattr(screen._Spec, "launch", lambda self, *a, **k: _lib.PRE_E_UNSUPPORTED)
    falls("declined by the library", run(case, "nx", gpu))


# ------------------------------------------------------------------ 9. the defaults are unchanged
def test_screen1dpair_pair_true_is_unchanged(gpu):
    from cp_pre_amd import screen
    for kind in ("burgers", "advection"):
        case = p1.case(kind, *p1.BASE, "nx")
        a = run(case, "nx", gpu, pair=True)
        assert screen.last_route() == "fallback:no paired screen for the 1-D family"
        b = run(case, "nx", gpu, pair=False)
        assert screen.last_route() == "fallback:minus=" and same(a, b)
        c = run(case, "nx", gpu, pair="flat")                        # (any other value: its truthiness)
        assert screen.last_route() == "fallback:no paired screen for the 1-D family" and same(a, c)
        # pair="rows" without minus: the single-set rows screen
        m = s1.method_of(kind, gpu)
        d = screen.screen(m, case.x.to(gpu), case.q.to(gpu), case.mod.to(gpu), pair="rows")
        assert screen.last_route() == s1.ROUTE[kind]
        assert same(d, screen.screen(m, case.x.to(gpu), case.q.to(gpu), case.mod.to(gpu)))


def test_screen1dpair_library_stays_unloaded_without_the_keyword(gpu):
    """in a fresh interpreter: ``minus=`` without ``pair``, ``pair=True`` and ``pair="rows"`` without ``minus`` leave
    ``_lib._screen1dpair`` None; ``pair="rows"`` with ``minus`` loads it"""
    code = (
        "import sys, torch\n"
        "sys.path[:0] = [%r, %r]\n"
        "import screen1d_helpers as s1, screen1dpair_helpers as p1\n"
        "from cp_pre_amd import screen, _lib\n"
        "c = p1.case('burgers', *p1.BASE, 'nx')\n"
        "d = torch.device('cuda:0')\n"
        "m = s1.method_of('burgers', d)\n"
        "x, y, q, md = c.x.to(d), c.y.to(d), c.q.to(d), c.mod.to(d)\n"
        "a = screen.screen(m, x, q, md, minus=y)\n"
        "assert screen.last_route() == 'fallback:minus=', screen.last_route()\n"
        "b = screen.screen(m, x, q, md, minus=y, pair=True)\n"
        "assert screen.last_route() == 'fallback:no paired screen for the 1-D family', screen.last_route()\n"
        "e = screen.screen(m, x, q, md, pair='rows')\n"
        "assert screen.last_route() == 'fused:rows_burgers', screen.last_route()\n"
        "assert _lib._screen1dpair is None and _lib._screenpair is None\n"
        "f = screen.screen(m, x, q, md, minus=y, pair='rows')\n"
        "assert screen.last_route() == 'fused:rows_pair_burgers' and _lib._screen1dpair is not None and _lib._screenpair is None\n"
        "assert torch.equal(a.accept(), f.accept()) and torch.equal(a.inside, b.inside)\n"
        "print('default unchanged')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                           os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "default unchanged" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ 10. the C client
def test_screen1dpair_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screen1dpair_check.c on the device, as a child process under a time limit: both entries against plain C
    loops in both layouts with a pitched second set, two overlapping slabs of the plane's ROWS, b == a, and the argument
    errors of the header."""
    from test_screen1dpair_cpu import c_client_command
    exe = tmp_path / "screen1dpair_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") == 65, out.stdout
