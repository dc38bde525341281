"""The per-cell screen of the data-driven scores (cp_pre_amd.screen.screen_cells / ScreenCells with ``minus=`` and
``pair=True``, csrc/screen_cells_pair.hip) on Ny-fastest field sets, on the GPU, against float64 (pytest -m gpu).

Reference, level fields, tolerances and cases: tests/screencellspair_helpers.py (the oracle in float64 on both sets, d_ref =
r_ref(a) - r_ref(b); tau = 1e-5 (max |r_ref(a)| + max |r_ref(b)|); score within tau / m_min + one ulp; a count within the
undecided cells of its (level, sample)).  tests/test_screencellspair_cpu.py shows, with the oracle alone, that every case
compared with the reference here meets the caps those bounds rest on.  tests/SCREENCELLSPAIR_TESTS.md says which test
reaches which branch."""
import os
import subprocess
import sys

import pytest
import torch

import screen_helpers as sh
import screencellspair_helpers as cp
import screenflat_helpers as fh
import screenpair_helpers as sp
import stencil_guards as sg

pytestmark = pytest.mark.gpu
FLAT = False


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(c, gpu, **kw):
    return cp.run(c, gpu, FLAT, **kw)


# ------------------------------------------------------------------ 1. every kind against fp64 and the three-pass route
@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", cp.KINDS)
def test_screencellspair_every_kind_against_fp64_and_three_pass(gpu, kind, boundary, with_mod):
    """nk = 10; nk = 1 (the first batch alone); nk = 16 (every later batch full); nk = 2, 5, 9 (a later batch with one live
    level, for each pair of batch sizes built)"""
    from cp_pre_amd import screen
    for nk, shape in cp.NY_MAIN:
        c = cp.case(kind, shape, boundary, with_mod, nk)
        s = run(c, gpu)
        assert screen.last_route() == cp.route(kind)
        cp.check(c, s, f"fused boundary={boundary} mod={with_mod}")
        s3 = run(c, gpu, pair=False)
        assert screen.last_route() == "fallback:minus="
        cp.check(c, s3, "  three-pass")
        cp.check_routes_agree(c, s, s3, "  fused against three-pass")


# ------------------------------------------------------------------ 2. identities, zero tolerance
@pytest.mark.parametrize("kind", cp.KINDS)
def test_screencellspair_constant_level_fields_give_the_bits_of_the_paired_joint_screen(gpu, kind):
    from cp_pre_amd import screen
    for boundary in (False, True):
        c = cp.case(kind, sp.NY_BASE, boundary, True, 10)
        q = sp.case(kind, sp.NY_BASE, boundary, True, nk=6).q                        # six scalar levels of the joint case
        xd, yd, md = c.x.to(gpu), c.y.to(gpu), c.mod.to(gpu)
        joint = screen.screen(sh.method_of(kind, gpu), xd, q.to(gpu), md, boundary=boundary, minus=yd, pair=True)
        assert screen.last_route() == sp.route(kind, "ny")
        qc = q[:, None, None, None].expand(6, *c.shape[1:]).contiguous().to(gpu)
        got = run(c, gpu, x=xd, y=yd, q=qc, mod=md)
        assert screen.last_route() == cp.route(kind)
        assert cp.same(got, joint) and got.cells == joint.cells


@pytest.mark.parametrize("kind", cp.KINDS)
def test_screencellspair_zero_minus_gives_the_bits_of_the_one_set_screen(gpu, kind):
    from cp_pre_amd import screen
    c = cp.case(kind, sp.NY_BASE, False, True, 10)
    xd, qd, md = c.x.to(gpu), c.q.to(gpu), c.mod.to(gpu)
    one = screen.screen_cells(sh.method_of(kind, gpu), xd, qd, md)
    assert screen.last_route() == "fused:cells_" + sp.PAIR_KIND[kind]
    got = run(c, gpu, x=xd, y=torch.zeros_like(xd), q=qd, mod=md)
    assert screen.last_route() == cp.route(kind)
    assert cp.same(got, one)


@pytest.mark.parametrize("kind", cp.KINDS)
def test_screencellspair_minus_equal_to_vars_gives_exactly_zero(gpu, kind):
    """the same tensor and an equal copy: score bits 0, every counted cell inside at every (non-negative, non-NaN) level"""
    from cp_pre_amd import screen
    for nk, shape in cp.NY_MAIN:
        c = cp.case(kind, shape, False, True, nk)
        assert bool((c.q >= 0).all())
        xd = c.x.to(gpu)
        for yd in (xd, xd.clone()):
            s = run(c, gpu, x=xd, y=yd)
            assert screen.last_route() == cp.route(kind)
            assert bool((sg.bits(s.score) == 0).all()) and bool((s.inside == c.cells).all()) and s.cells == c.cells


# ------------------------------------------------------------------ 3. the sample group
@pytest.mark.parametrize("kind", cp.GROUP_KINDS)
def test_screencellspair_across_the_sample_group(gpu, kind):
    """B = G + 1 and B = 2G - 1: a group with one sample and a group one short, next to whole ones; G from the library"""
    from cp_pre_amd import screen
    G = screen.sample_group_pair()
    assert G >= 1
    for B in cp.group_batches(G):
        c = cp.case(kind, (B,) + cp.GROUP_TXY, True, True, 10)
        s = run(c, gpu)
        assert screen.last_route() == cp.route(kind)
        cp.check(c, s, f"G={G} B={B}")


# ------------------------------------------------------------------ 4. levels are per level and per cell
@pytest.mark.parametrize("nk", [10, 16])
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_screencellspair_levels_are_per_level_and_per_cell(gpu, kind, nk):
    """(k = 0 is a level of the first batch for both kinds, k = 4 and nk - 1 levels of a later one: the batches are 1 + 15
    for the NS momentum and 4 + 12 for the wave star)"""
    c = cp.case(kind, sh.SEAM_SHAPES["two_tseg"], False, True, nk)
    base = run(c, gpu)
    perm = torch.tensor([3, 0, 9, 1, 7, 2, 8, 4, 6, 5] + [15, 10, 13, 11, 14, 12][:nk - 10])
    got = run(c, gpu, q=c.q[perm].to(gpu))
    assert torch.equal(got.inside, base.inside[perm.to(gpu)]) and torch.equal(sg.bits(got.score), sg.bits(base.score))
    # one counted cell's level at one k (k = 4 a later batch's level for the NS momentum, k = 0 its first batch's): below
    # every |d| there, then above: only row k moves, by exactly one per sample between the two
    for k in (0, 4, nk - 1):
        lo, hi = c.q.clone(), c.q.clone()
        lo[k, 9, 2, 6], hi[k, 9, 2, 6] = -1.0, float("inf")
        glo, ghi = run(c, gpu, q=lo.to(gpu)), run(c, gpu, q=hi.to(gpu))
        others = [j for j in range(nk) if j != k]
        assert torch.equal(glo.inside[others], base.inside[others]) and torch.equal(ghi.inside[others], base.inside[others])
        assert bool((ghi.inside[k] - glo.inside[k] == 1).all())
        assert bool(((glo.inside[k] - base.inside[k]).abs() <= 1).all()) and bool(((ghi.inside[k] - base.inside[k]).abs() <= 1).all())


# ------------------------------------------------------------------ 5. the rim and non-finite contract, on both sets
def test_screencellspair_rim_and_non_finite_contract(gpu):
    c = cp.case("ns_momentum", sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    base = run(c, gpu)
    method = sh.method_of("ns_momentum", gpu)
    # NaN / inf in the rim of the levels and of the modulation reach nothing
    q, mod = c.q.clone(), c.mod.clone()
    for v, t in ((float("nan"), q), (float("inf"), mod)):
        t[..., 0, :, :], t[..., -1, :, :], t[..., :, 0, :], t[..., :, -1, :], t[..., :, :, 0], t[..., :, :, -1] = [v] * 6
    assert cp.same(run(c, gpu, q=q.to(gpu), mod=mod.to(gpu)), base)
    # cropped levels: the bits of uncropped levels with any rim
    assert cp.same(run(c, gpu, q=c.q_cropped().to(gpu)), base)
    # a NaN / inf of either set where only rim cells' stars reach (p at a corner): nothing changes
    for which in ("x", "y"):
        for v in (float("nan"), float("inf")):
            t = getattr(c, which).clone()
            t[1, 2, 0, 0, 0] = v
            assert cp.same(run(c, gpu, **{which: t.to(gpu)}), base), (which, v)
    # a NaN of either set in counted cells: d is NaN there - outside at every level, +inf levels included, the sample's
    # score NaN; the other samples do not move
    qinf = torch.full_like(c.q, float("inf")).to(gpu)
    for which in ("x", "y"):
        t = getattr(c, which).clone()
        t[1, 0, 2, 5, 7] = float("nan")
        kw = {which: t.to(gpu)}
        xd, yd = kw.get("x", c.x.to(gpu)), kw.get("y", c.y.to(gpu))
        nbad = int(torch.isnan(method(xd, boundary=True, minus=yd)[c.reg][1]).sum())
        assert 1 <= nbad <= 27
        got = run(c, gpu, q=qinf, **kw)
        assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
        assert bool((got.inside[:, 1] == c.cells - nbad).all()) and bool((got.inside[:, [0, 2]] == c.cells).all())
    # a NaN level and a negative level in a counted cell: outside at that level; +inf: inside
    q = c.q.clone()
    q[:, 2, 5, 7] = float("inf")
    allin = run(c, gpu, q=q.to(gpu))
    rest = [0, 1, 2, 4, 5, 6, 7, 8, 9]
    for v in (float("nan"), -0.5):
        q[3, 2, 5, 7] = v
        got = run(c, gpu, q=q.to(gpu))
        assert bool((got.inside[3] == allin.inside[3] - 1).all()) and torch.equal(got.inside[rest], allin.inside[rest])
    # m == 0: inf * 0 is NaN - the cell is outside at every level - and d / 0 makes every score inf
    q[3, 2, 5, 7] = float("inf")
    mod = c.mod.clone()
    mod[2, 5, 7] = 0.0
    got = run(c, gpu, q=q.to(gpu), mod=mod.to(gpu))
    assert bool(torch.isinf(got.score).all()) and bool((got.inside == allin.inside - 1).all())


# ------------------------------------------------------------------ 6. pitched, 4-byte-aligned views in guarded allocations
def _embed(t, kind, gpu, offset, pitch, extra):
    """``vars[:, i]`` views of a stacked tensor with ``extra`` more channels, rows ``pitch`` floats further apart than they
    are long, the base ``offset`` floats off the allocation's 16-byte boundary, in a guarded allocation."""
    if sh.NCHAN[kind] is None:
        big = torch.zeros((t.shape[0], 1 + extra) + tuple(t.shape[1:]))
        big[:, 1] = t
    else:
        big = torch.zeros((t.shape[0], t.shape[1] + extra) + tuple(t.shape[2:]))
        big[:, 1:1 + t.shape[1]] = t
    alloc, view = sg.embed(big, None, {big.dim() - 2: pitch}, offset, gpu)
    return alloc, (view[:, 1] if sh.NCHAN[kind] is None else view[:, 1:1 + t.shape[1]])


@pytest.mark.parametrize("kind", cp.VIEW_KINDS)
def test_screencellspair_pitched_misaligned_views_in_poisoned_memory(gpu, kind):
    """nothing outside a view of either set, of the modulation or of the levels reaches a result, and nothing is written"""
    from cp_pre_amd import screen
    c = cp.case(kind, sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    dense = run(c, gpu)
    for offset, pitch in ((1, 5), (3, 8), (0, 4)):
        xa, xd = _embed(c.x, kind, gpu, offset, pitch, 2)
        ya, yd = _embed(c.y, kind, gpu, (offset + 2) % 4, pitch + 3, 3)
        ma, md = sg.embed(c.mod, None, {1: pitch + 1}, offset, gpu)
        qa, qd = sg.embed(c.q, None, {2: pitch + 2}, offset, gpu)
        assert qd.stride(2) > qd.shape[3] and qd.stride(3) == 1 and xd.stride(-2) != yd.stride(-2)
        allocs = [xa, ya, ma, qa]
        masks = [sg.outside_mask(a, v) for a, v in zip(allocs, (xd, yd, md, qd))]
        for value in sg.POISONS:
            for a, m in zip(allocs, masks):
                sg.poison(a, m, value)
            before = [a.clone() for a in allocs]
            got = run(c, gpu, x=xd, y=yd, q=qd, mod=md)
            assert screen.last_route() == cp.route(kind)
            assert cp.same(got, dense), (offset, pitch, value)
            assert all(torch.equal(sg.bits(a), sg.bits(b)) for a, b in zip(allocs, before))
    # the level tensor in the other layout (memory [nk,X,Y,T]): copied once, same bits
    qd = fh.to_layout(c.q, gpu)
    assert qd.stride(-1) != 1
    assert cp.same(run(c, gpu, q=qd), dense) and screen.last_route() == cp.route(kind)


# ------------------------------------------------------------------ 7. slabs compose bit for bit
def test_screencellspair_slabs_compose_bit_for_bit(gpu):
    from cp_pre_amd import screen
    kind, shape = "ns_momentum", cp.SLAB_SHAPE
    c = cp.case(kind, shape, False, True, 10)
    whole = run(c, gpu)
    method = sh.method_of(kind, gpu)
    xd, yd, md, q = c.x.to(gpu), c.y.to(gpu), c.mod.to(gpu), c.q.to(gpu)
    X = shape[2]
    for order in (((1, 10), (10, 33), (33, X - 1)), ((33, X - 1), (1, 10), (10, 33))):
        s = screen.ScreenCells(shape[0], c.nk, gpu)
        for x0, x1 in order:
            s.add_slab(method, xd[:, :, :, x0:x1], q[:, :, x0:x1], md[:, x0:x1], crop=(1, 0, 1), halo_x=True,
                       minus=yd[:, :, :, x0:x1], pair=True)
            assert screen.last_route() == cp.route(kind)
        got = s.finish()
        assert got.cells == whole.cells and cp.same(got, whole)
    for order in (((0, 8), (6, 12)), ((6, 12), (0, 8))):
        s = screen.ScreenCells(shape[0], c.nk, gpu)
        for t0, t1 in order:
            s.add_slab(method, xd[:, :, t0:t1], q[:, t0:t1], md[t0:t1], crop=(1, 1, 1), minus=yd[:, :, t0:t1], pair=True)
            assert screen.last_route() == cp.route(kind)
        got = s.finish()
        assert got.cells == whole.cells and cp.same(got, whole)
    assert cp.same(run(c, gpu), whole)                               # two runs: identical bytes


def test_screencellspair_halo_x_rules(gpu):
    """under halo_x both sets must be Ny-contiguous device views, as for ``pair=True`` on ``screen``; a fused launch that
    cannot run raises where no other pass of the method reads the halo rows"""
    from cp_pre_amd import screen
    c = cp.case("ns_continuity", sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    xd, yd, md, q = c.x.to(gpu), c.y.to(gpu), c.mod.to(gpu), c.q.to(gpu)
    method = sh.method_of("ns_continuity", gpu)
    kw = dict(crop=(1, 0, 1), halo_x=True, pair=True)
    whole = run(c, gpu)
    s = screen.ScreenCells(3, c.nk, gpu)
    for x0, x1 in ((1, 20), (20, 32)):
        s.add_slab(method, xd[..., x0:x1, :], q[:, :, x0:x1], md[:, x0:x1], minus=yd[..., x0:x1, :], **kw)
        assert screen.last_route() == "fused:cells_pair_linear2"
    assert cp.same(s.finish(), whole)
    s = screen.ScreenCells(3, c.nk, gpu)
    with pytest.raises(ValueError, match="Ny-contiguous device views"):
        s.add_slab(method, xd[..., 1:20, :], q[:, :, 1:20], md[:, 1:20], minus=fh.to_layout(c.y, gpu)[..., 1:20, :], **kw)
    with pytest.raises(RuntimeError, match="halo_x"):
        s.add_slab(method, xd[..., 1:20, :], q[:, :, 1:20].double(), md[:, 1:20], minus=yd[..., 1:20, :], **kw)
    with pytest.raises(RuntimeError, match="halo_x"):                # (without the keyword: minus= keeps the three passes)
        s.add_slab(method, xd[..., 1:20, :], q[:, :, 1:20], md[:, 1:20], minus=yd[..., 1:20, :], crop=(1, 0, 1), halo_x=True)
    assert s.cells == 0 and (s.acc is None or not bool(s.acc.any()))


# ------------------------------------------------------------------ 8. the tap structures beside the reference's
@pytest.mark.parametrize("structure", sh.TAP_STRUCTURES)
@pytest.mark.parametrize("kind", cp.TAP_KINDS)
def test_screencellspair_other_tap_structures(gpu, kind, structure):
    """The y-fixed paired MHD continuity (<1>) against the difference stored with the same operators; the y-fixed paired NS
    momentum and both general stars are not built: the library declines and the call is the three-pass route's answer."""
    from cp_pre_amd import screen
    c = cp.case(kind, sp.NY_BASE, False, True, 10)
    method = sh.method_with_taps(kind, structure, gpu)
    xd, yd = c.x.to(gpu), c.y.to(gpu)
    s = run(c, gpu, x=xd, y=yd, method=method)
    if cp.BUILT[kind, structure]:
        assert screen.last_route() == cp.route(kind)
        assert not cp.same(s, run(c, gpu, x=xd, y=yd))               # the other operators were applied
        cp.check_against_stored_difference(c, s, method, xd, yd, FLAT, f"{kind} {structure}")
    else:
        assert screen.last_route() == "fallback:declined by the library"
        s3 = run(c, gpu, x=xd, y=yd, method=method, pair=False)
        assert screen.last_route() == "fallback:minus=" and cp.same(s, s3)


# ------------------------------------------------------------------ 9. fallbacks, refused calls, the default
def test_screencellspair_fallbacks_say_why_and_agree(gpu):
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    kind = "ns_momentum"
    c = cp.case(kind, sp.NY_BASE, False, True, 10)
    fused = run(c, gpu)
    assert screen.last_route() == cp.route(kind)
    xd, yd, md, qd = c.x.to(gpu), c.y.to(gpu), c.mod.to(gpu), c.q.to(gpu)
    for other, why in sp.UNPAIRED.items():                           # no paired screen for the kind
        x6 = sh.fields(other, sp.NY_BASE)
        screen.screen_cells(sh.method_of(other, gpu), x6.to(gpu), qd, md, minus=x6.to(gpu) * 0.5, pair=True)
        assert screen.last_route() == "fallback:" + why
    s = screen.screen_cells(sh.method_of(kind), c.x, c.q_cropped(), c.mod, minus=c.y, pair=True)
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    cp.check(c, s, "CPU inputs, cropped levels")
    s = run(c, gpu, q=qd.double())
    assert screen.last_route() == "fallback:float64 levels or modulation"
    cp.check(c, s, "float64 levels")
    s = run(c, gpu, y=fh.to_layout(c.y, gpu))
    assert screen.last_route() == "fallback:field sets in different layouts"
    cp.check(c, s, "Ny-fastest vars, Nt-fastest minus")
    wide = torch.zeros(*c.y.shape[:-1], 2 * c.y.shape[-1], device=gpu)
    wide[..., ::2] = yd
    s = run(c, gpu, y=wide[..., ::2])
    assert screen.last_route() == "fallback:minus: no unit stride on the last axis"
    cp.check(c, s, "strided minus")
    oc = cp.case(kind, sp.ODD_NY, False, True, 10)
    s = run(oc, gpu)
    assert screen.last_route() == "fallback:row width not a multiple of 4"
    cp.check(oc, s, "Ny = 13")
    ns = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, device=gpu, fused=False)
    s = run(c, gpu, method=ns.residual_momentum)
    assert screen.last_route() == "fallback:fused=False"
    cp.check(c, s, "fused=False")
    # without the keyword: the three-pass route, with the bits it has whatever the keyword's spelling
    a = run(c, gpu, pair=False)
    assert screen.last_route() == "fallback:minus="
    b = screen.screen_cells(sh.method_of(kind, gpu), xd, qd, md, minus=yd)
    assert screen.last_route() == "fallback:minus=" and cp.same(a, b)
    cp.check_routes_agree(c, fused, a, "fused against fallback:minus=")
    # pair=True without minus: the one-set per-cell screen
    a = screen.screen_cells(sh.method_of(kind, gpu), xd, qd, md, pair=True)
    assert screen.last_route() == "fused:cells_ns_momentum"
    assert cp.same(a, screen.screen_cells(sh.method_of(kind, gpu), xd, qd, md))
    # rows=True with minus= on the 1-D family is as it was, with or without the keyword
    bu = R.Burgers(0.02, 0.01, 0.01, device=gpu)
    u, v, q1 = torch.rand(3, 12, 16, device=gpu) + 0.5, torch.rand(3, 12, 16, device=gpu) + 0.5, torch.rand(2, 12, 16, device=gpu)
    a = screen.screen_cells(bu.residual, u, q1, minus=v, rows=True)
    assert screen.last_route() == "fused:rows_cells_pair_burgers"
    b = screen.screen_cells(bu.residual, u, q1, minus=v, rows=True, pair=True)
    assert screen.last_route() == "fused:rows_cells_pair_burgers" and cp.same(a, b)
    screen.screen_cells(bu.residual, u, q1, minus=v, pair=True)
    assert screen.last_route() == "fallback:1-D family: the marched axis is the batch"


def test_screencellspair_refused_calls_launch_nothing(gpu):
    from cp_pre_amd import screen
    c = cp.case("ns_momentum", sp.NY_BASE, False, True, 10)
    method = sh.method_of("ns_momentum", gpu)
    xd, yd, md, q = c.x.to(gpu), c.y.to(gpu), c.mod.to(gpu), c.q.to(gpu)
    s = screen.ScreenCells(c.shape[0], c.nk, gpu)
    kw = dict(pair=True)
    for bad in (lambda: s.add_slab(method, xd, q[:3], md, minus=yd, **kw), lambda: s.add_slab(method, xd, q[:, 1:], md, minus=yd, **kw),
                lambda: s.add_slab(method, xd, q, md[1:], minus=yd, **kw), lambda: s.add_slab(method, xd[:2], q, md, minus=yd[:2], **kw),
                lambda: s.add_slab(method, xd, q, md, minus=yd[:2], **kw), lambda: s.add_slab(method, xd, q, md, minus=yd[:, :2], **kw),
                lambda: s.add_slab(method, xd, q, md, crop=(9, 1, 1), minus=yd, **kw),
                lambda: s.add_slab(method, xd, c.q_cropped().to(gpu), md, minus=yd, **kw)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        s.add_slab(method, xd, q, md, minus=yd.double(), **kw)
    torch.cuda.synchronize()
    assert (s.acc is None or not bool(s.acc.any())) and s.cells == 0
    s.add_slab(method, xd, q, md, minus=yd, **kw)
    before = s.acc.clone()
    with pytest.raises(ValueError):
        s.add_slab(method, xd, q[:, :, 1:], md, minus=yd, **kw)
    torch.cuda.synchronize()
    assert torch.equal(s.acc, before) and s.cells == c.cells


def test_screencellspair_default_route_is_unchanged_and_the_library_is_not_loaded(gpu):
    """``minus=`` without ``pair`` in a fresh interpreter: ``fallback:minus=`` and the library stays unloaded through every
    other screen; with the keyword it is loaded and the two routes agree"""
    code = (
        "import sys, torch\n"
        "sys.path[:0] = [%r, %r]\n"
        "import screen_helpers as sh, screencellspair_helpers as cp, screenpair_helpers as sp\n"
        "from cp_pre_amd import screen, _lib\n"
        "c = cp.case('ns_momentum', sp.NY_BASE)\n"
        "d = torch.device('cuda:0')\n"
        "m = sh.method_of('ns_momentum', d)\n"
        "x, y, q, mod = c.x.to(d), c.y.to(d), c.q.to(d), c.mod.to(d)\n"
        "a = screen.screen_cells(m, x, q, mod, minus=y)\n"
        "assert screen.last_route() == 'fallback:minus=', screen.last_route()\n"
        "screen.screen_cells(m, x, q, mod, pair=True)\n"
        "assert screen.last_route() == 'fused:cells_ns_momentum', screen.last_route()\n"
        "screen.screen(m, x, q[:, 0, 0, 0].contiguous(), mod, minus=y, pair=True)\n"
        "assert screen.last_route() == 'fused:pair_ns_momentum', screen.last_route()\n"
        "assert _lib._screencellspair is None\n"
        "f = screen.screen_cells(m, x, q, mod, minus=y, pair=True)\n"
        "assert screen.last_route() == 'fused:cells_pair_ns_momentum' and _lib._screencellspair is not None\n"
        "cp.check(c, a, 'three-pass'); cp.check(c, f, 'fused'); cp.check_routes_agree(c, f, a, 'both')\n"
        "print('default unchanged')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                           os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "default unchanged" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ 10. the C client
def test_screencellspair_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screencellspair_check.c on the device, as a child process under a time limit: the paired star in both
    layouts against plain C loops with B = G + 1, two t-slabs, b == a, and the argument errors of the entries."""
    from test_screencellspair_cpu import c_client_command
    exe = tmp_path / "screencellspair_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") >= 20, out.stdout
