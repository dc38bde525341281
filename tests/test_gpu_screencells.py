"""The per-cell screen (cp_pre_amd.screen.screen_cells / ScreenCells, csrc/screen_cells.hip) on Ny-fastest fields, on the GPU,
against float64 (pytest -m gpu).

Reference, level fields, tolerances and cases: tests/screencells_helpers.py (the oracle in float64; tau = 1e-5 max |r_ref|;
score within tau / m_min + one ulp; a count within the undecided cells of its (level, sample)).
tests/test_screencells_cpu.py shows, with the oracle alone, that every case used here keeps its undecided cells below 1 %
and has a level that splits the cells of a sample.  tests/SCREENCELLS_TESTS.md says which test reaches which branch."""
import os
import subprocess

import pytest
import torch

import screen_helpers as sh
import screencells_helpers as ch
import stencil_guards as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(c, gpu, x=None, q=None, mod=None, method=None):
    from cp_pre_amd import screen
    xd = c.x.to(gpu) if x is None else x
    qd = c.q.to(gpu) if q is None else q
    md = (c.mod.to(gpu) if c.mod is not None else None) if mod is None else mod
    return screen.screen_cells(method or sh.method_of(c.kind, gpu), xd, qd, md, boundary=c.boundary)


def same(a, b):
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside)


def three_pass(c, gpu):
    """The package's own three-pass route with per-cell levels: the functions the fallback calls."""
    from cp_pre_amd import inductive_cp as icp
    from cp_pre_amd import pipeline, screen
    method = sh.method_of(c.kind, gpu)
    xd = c.x.to(gpu)
    res = method(xd) if c.kind == "lap" else method(xd, boundary=True)
    mod = c.mod.to(gpu) if c.mod is not None else torch.ones(c.shape[1:], device=gpu)
    score = icp.ncf_metric_joint(res, None, mod) if c.boundary else icp.ncf_metric_joint(res, None, mod, crop=1)
    q = c.q.to(gpu)[(slice(None),) + c.reg[1:]]
    counts = torch.empty(c.nk, c.shape[0], dtype=torch.int64, device=gpu)
    cov = pipeline.CoverageLevels(1, c.nk, gpu)
    for i in range(c.shape[0]):
        cov.acc.zero_()
        cov.add_slab(res[c.reg][i:i + 1], q, modulation=mod[c.reg[1:]] if c.mod is not None else None)
        counts[:, i] = cov.acc
    return screen.Screened(score, counts, c.cells)


@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", sh.KINDS)
def test_screencells_every_kind_against_fp64_and_three_pass(gpu, kind, boundary, with_mod):
    from cp_pre_amd import screen
    for nk, name in ch.MAIN:
        c = ch.case(kind, sh.SEAM_SHAPES[name], boundary, with_mod, nk)
        s = run(c, gpu)
        assert screen.last_route() == ch.route(kind)
        ch.check(c, s, f"fused boundary={boundary} mod={with_mod}")
        s3 = three_pass(c, gpu)
        ch.check(c, s3, "  three-pass")
        print(f"  fused and three-pass bit-identical: {same(s, s3)}")


@pytest.mark.parametrize("name", list(sh.SEAM_SHAPES))
@pytest.mark.parametrize("kind", ch.SEAM_KINDS)
def test_screencells_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    c = ch.case(kind, sh.SEAM_SHAPES[name], False, True, 10)
    s = run(c, gpu)
    assert screen.last_route() == ch.route(kind)
    ch.check(c, s, name)


@pytest.mark.parametrize("kind", ch.GROUP_KINDS)
def test_screencells_across_the_sample_group(gpu, kind):
    """B = G + 1 and B = 2G - 1: a group with one sample and a group one short, next to whole ones"""
    from cp_pre_amd import screen
    G = screen.sample_group()
    assert G >= 1
    if G == 1:
        print("G == 1: the block order is the joint screens'; B = 3")
    for B in ch.group_batches(G):
        c = ch.case(kind, (B,) + ch.GROUP_TXY, True, True, 10)      # (every cell counted: screencells_helpers.GROUP_TXY)
        s = run(c, gpu)
        assert screen.last_route() == ch.route(kind)
        ch.check(c, s, f"G={G} B={B}")


def test_screencells_levels_are_per_level_and_per_cell(gpu):
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    base = run(c, gpu)
    perm = torch.tensor([3, 0, 9, 1, 7, 2, 8, 4, 6, 5])
    got = run(c, gpu, q=c.q[perm].to(gpu))
    assert torch.equal(got.inside, base.inside[perm.to(gpu)]) and torch.equal(sg.bits(got.score), sg.bits(base.score))
    # one counted cell's level at one k: below every |r| there, then above: only row k moves, by at most one per sample
    for value in (-1.0, float("inf")):
        q = c.q.clone()
        q[4, 9, 2, 6] = value
        got = run(c, gpu, q=q.to(gpu))
        others = [k for k in range(10) if k != 4]
        assert torch.equal(got.inside[others], base.inside[others])
        d = got.inside[4] - base.inside[4]
        assert bool((d.abs() <= 1).all()) and bool((d <= 0).all() if value < 0 else (d >= 0).all())
    lo, hi = c.q.clone(), c.q.clone()
    lo[4, 9, 2, 6], hi[4, 9, 2, 6] = -1.0, float("inf")
    d = run(c, gpu, q=hi.to(gpu)).inside[4] - run(c, gpu, q=lo.to(gpu)).inside[4]
    assert bool((d == 1).all())                                  # outside at a negative level, inside at +inf: every sample


def test_screencells_rim_and_non_finite_contract(gpu):
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    base = run(c, gpu)
    B, T, X, Y = c.shape
    # NaN / inf in the rim of the levels and of the modulation reach nothing
    q, mod = c.q.clone(), c.mod.clone()
    for v, t in ((float("nan"), q), (float("inf"), mod)):
        t[..., 0, :, :], t[..., -1, :, :], t[..., :, 0, :], t[..., :, -1, :], t[..., :, :, 0], t[..., :, :, -1] = [v] * 6
    got = run(c, gpu, q=q.to(gpu), mod=mod.to(gpu))
    assert same(got, base)
    # cropped levels: the bits of uncropped levels with any rim
    got = run(c, gpu, q=c.q_cropped().to(gpu))
    assert same(got, base)
    # a NaN residual in a rim cell reaches nothing (NaN in p at the corner reaches rim cells only)
    x = c.x.clone()
    x[1, 2, 0, 0, 0] = float("nan")
    assert same(run(c, gpu, x=x.to(gpu)), base)
    # a NaN residual in counted cells: outside at every level, +inf levels included; the other samples do not move
    x = c.x.clone()
    x[1, 0, 2, 5, 7] = float("nan")
    r = sh.method_of("ns_momentum", gpu)(x.to(gpu), boundary=True)
    nbad = int(torch.isnan(r[c.reg][1]).sum())
    assert 1 <= nbad <= 27
    qinf = torch.full_like(c.q, float("inf"))
    got = run(c, gpu, x=x.to(gpu), q=qinf.to(gpu))
    assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
    assert bool((got.inside[:, 1] == c.cells - nbad).all()) and bool((got.inside[:, [0, 2]] == c.cells).all())
    # a NaN level and a negative level in a counted cell: outside at that level; m == 0: hw = 0, outside where r != 0
    q = c.q.clone()
    q[:, 2, 5, 7] = float("inf")
    allin = run(c, gpu, q=q.to(gpu))
    for v in (float("nan"), -0.5):
        q[3, 2, 5, 7] = v
        got = run(c, gpu, q=q.to(gpu))
        assert bool((got.inside[3] == allin.inside[3] - 1).all())
        assert torch.equal(got.inside[[0, 1, 2, 4, 5, 6, 7, 8, 9]], allin.inside[[0, 1, 2, 4, 5, 6, 7, 8, 9]])
    mod = c.mod.clone()
    mod[2, 5, 7] = 0.0
    got = run(c, gpu, q=allin_q(c).to(gpu), mod=mod.to(gpu))
    # (inf * 0 is NaN: the cell is outside at every level, and r / 0 makes every score inf)
    assert bool(torch.isinf(got.score).all()) and bool((got.inside == allin.inside - 1).all())


def allin_q(c):
    q = c.q.clone()
    q[:, 2, 5, 7] = float("inf")
    return q


def _embed(c, gpu, offset, pitch):
    """``vars[:, i]`` views of a stacked tensor with two more channels, rows ``pitch`` floats further apart than they are
    long, the base ``offset`` floats off the allocation's 16-byte boundary, in a guarded allocation."""
    x = c.x
    if sh.NCHAN[c.kind] is None:
        big = torch.zeros((x.shape[0], 3) + tuple(x.shape[1:]))
        big[:, 1] = x
    else:
        big = torch.zeros((x.shape[0], x.shape[1] + 2) + tuple(x.shape[2:]))
        big[:, 1:-1] = x
    alloc, view = sg.embed(big, None, {big.dim() - 2: pitch}, offset, gpu)
    return alloc, (view[:, 1] if sh.NCHAN[c.kind] is None else view[:, 1:-1])


@pytest.mark.parametrize("kind", ["ns_momentum", "wave", "mhd_energy"])
def test_screencells_pitched_misaligned_views_in_poisoned_memory(gpu, kind):
    from cp_pre_amd import screen
    c = ch.case(kind, sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    dense = run(c, gpu)
    for offset, pitch in ((1, 5), (3, 8), (0, 4)):
        alloc, xd = _embed(c, gpu, offset, pitch)
        malloc, md = sg.embed(c.mod, None, {1: pitch + 1}, offset, gpu)
        qalloc, qd = sg.embed(c.q, None, {2: pitch + 2}, offset, gpu)
        assert qd.stride(2) > qd.shape[3] and qd.stride(3) == 1
        allocs = [alloc, malloc, qalloc]
        masks = [sg.outside_mask(alloc, xd), sg.outside_mask(malloc, md), sg.outside_mask(qalloc, qd)]
        for value in sg.POISONS:
            for a, m in zip(allocs, masks):
                sg.poison(a, m, value)
            before = [a.clone() for a in allocs]
            got = run(c, gpu, xd, qd, md)
            assert screen.last_route() == ch.route(kind)
            assert same(got, dense), (offset, pitch, value)
            assert all(torch.equal(sg.bits(a), sg.bits(b)) for a, b in zip(allocs, before))
    # the level tensor in the other layout (memory [nk,X,Y,T]): copied once, same bits
    qd = c.q.to(gpu).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert qd.stride(-1) != 1
    assert same(run(c, gpu, q=qd), dense) and screen.last_route() == ch.route(kind)


def test_screencells_slabs_compose_bit_for_bit(gpu):
    from cp_pre_amd import screen
    kind, shape = "ns_momentum", ch.SLAB_SHAPE
    c = ch.case(kind, shape, False, True, 10)
    whole = run(c, gpu)
    method = sh.method_of(kind, gpu)
    xd, md, q = c.x.to(gpu), c.mod.to(gpu), c.q.to(gpu)
    X = shape[2]
    for order in (((1, 10), (10, 33), (33, X - 1)), ((33, X - 1), (1, 10), (10, 33))):
        s = screen.ScreenCells(shape[0], c.nk, gpu)
        for x0, x1 in order:
            s.add_slab(method, xd[:, :, :, x0:x1], q[:, :, x0:x1], md[:, x0:x1], crop=(1, 0, 1), halo_x=True)
            assert screen.last_route() == ch.route(kind)
        got = s.finish()
        assert got.cells == whole.cells and same(got, whole)
    # non-finite values in the halo rows, at positions no counted cell's star reaches: nothing changes
    xp = c.x.clone()
    xp[:, :, :, 0, 0], xp[:, :, 0, 0, :] = float("nan"), float("inf")
    xp[:, :, :, X - 1, -1], xp[:, :, -1, X - 1, :] = float("inf"), float("nan")
    xpd = xp.to(gpu)
    s = screen.ScreenCells(shape[0], c.nk, gpu)
    for x0, x1 in ((1, 10), (10, 33), (33, X - 1)):
        s.add_slab(method, xpd[:, :, :, x0:x1], q[:, :, x0:x1], md[:, x0:x1], crop=(1, 0, 1), halo_x=True)
    assert same(s.finish(), whole)
    for order in (((0, 8), (6, 12)), ((6, 12), (0, 8))):
        s = screen.ScreenCells(shape[0], c.nk, gpu)
        for t0, t1 in order:
            s.add_slab(method, xd[:, :, t0:t1], q[:, t0:t1], md[t0:t1], crop=(1, 1, 1))
        got = s.finish()
        assert got.cells == whole.cells and same(got, whole)
    assert same(run(c, gpu), whole)                               # two runs: identical bytes


def test_screencells_fallbacks_say_why_and_agree(gpu):
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    fused = run(c, gpu)
    xd, qd, md = c.x.to(gpu), c.q.to(gpu), c.mod.to(gpu)
    ns = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, device=gpu, fused=False)
    got = screen.screen_cells(ns.residual_momentum, xd, qd, md)
    assert screen.last_route() == "fallback:fused=False"
    ch.check(c, got, "fused=False")
    got = screen.screen_cells(sh.method_of("ns_momentum", gpu), xd, qd.double(), md)
    assert screen.last_route() == "fallback:float64 levels or modulation"
    ch.check(c, got, "float64 levels")
    got = screen.screen_cells(sh.method_of("ns_momentum"), c.x, c.q_cropped(), c.mod)
    assert screen.last_route() == "fallback:input on the CPU"
    ch.check(c, got, "CPU inputs, cropped levels")
    assert not got.score.is_cuda
    got = screen.screen_cells(sh.method_of("ns_momentum", gpu), xd, qd, md, minus=xd * 0)
    assert screen.last_route() == "fallback:minus="
    for shape in sh.ODD_SHAPES[:1]:
        o = ch.case("ns_momentum", shape, False, True, 10)
        got = run(o, gpu)
        assert screen.last_route() == "fallback:row width not a multiple of 4"
        ch.check(o, got, "odd width")
    print("fused and fused=False bit-identical:", same(fused, screen.screen_cells(ns.residual_momentum, xd, qd, md)))


def test_screencells_refused_calls_launch_nothing(gpu):
    from cp_pre_amd import screen
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    method = sh.method_of("ns_momentum", gpu)
    xd, md, q = c.x.to(gpu), c.mod.to(gpu), c.q.to(gpu)
    s = screen.ScreenCells(c.shape[0], c.nk, gpu)
    for bad in (lambda: s.add_slab(method, xd, q[:3], md), lambda: s.add_slab(method, xd, q[:, 1:], md),
                lambda: s.add_slab(method, xd, q, md[1:]), lambda: s.add_slab(method, xd[:2], q, md),
                lambda: s.add_slab(method, xd, q, md, crop=(9, 1, 1)), lambda: s.add_slab(method, xd, c.q_cropped().to(gpu), md)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert s.acc is None or not bool(s.acc.any())
    assert s.cells == 0
    s.add_slab(method, xd, q, md)
    before = s.acc.clone()
    with pytest.raises(ValueError):
        s.add_slab(method, xd, q[:, :, 1:], md)
    torch.cuda.synchronize()
    assert torch.equal(s.acc, before) and s.cells == c.cells


def test_screencells_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screencells_check.c on the device: the wave star against plain C loops with per-cell levels, both forms,
    two t-slabs against the whole grid, B across the sample group, and the argument errors of the entries."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "screencells_check"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(root, "tests", "c_abi", "screencells_check.c"), "-I" + os.path.join(root, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(root, "cp_pre_amd"), "-l:libcp_pre_screencells.so",
                           "-Wl,-rpath," + os.path.join(root, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") >= 10, out.stdout


# ------------------------------------------------------------------ the tap structures beside the reference's
@pytest.mark.parametrize("structure", sh.TAP_STRUCTURES)
@pytest.mark.parametrize("kind", sh.TAP_KINDS)
def test_screencells_other_tap_structures_against_the_stored_residual(gpu, kind, structure):
    """The y-fixed (<1>) and general-star (<2>) instantiations of every functor compiled per tap structure, which the
    default operators never reach, against the residual stored with the same operators
    (``sh.check_against_stored`` has the bounds; the level fields are the default operators' case's) - and not the default
    operators' answer.  The general stars of the MHD momentum and energy are not built with per-cell sets: the library
    declines."""
    from cp_pre_amd import screen
    nk, name = ch.MAIN[0]
    c = ch.case(kind, sh.SEAM_SHAPES[name], False, True, nk)
    method = sh.method_with_taps(kind, structure, gpu)
    xd = c.x.to(gpu)
    s = run(c, gpu, x=xd, method=method)
    built = structure != "general" or kind not in ("mhd_momentum", "mhd_energy")
    assert screen.last_route() == (ch.route(kind) if built else "fallback:declined by the library")
    assert not same(s, run(c, gpu, x=xd))
    sh.check_against_stored(c, s, method(xd, boundary=True), c.q, f"{kind} {structure}")
