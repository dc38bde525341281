"""The per-cell screen of the data-driven scores (cp_pre_amd.screen.screen_cells with ``minus=`` and ``pair=True``,
csrc/screen_cells_pair.hip) on Nt-fastest field sets - ``pred.permute(0,1,4,2,3)``, what the Marginal/ NS and MHD scripts pass -
on the GPU, against float64 (pytest -m gpu).

Reference, level fields, tolerances and cases: tests/screencellspair_helpers.py; layout and seams: tests/screenflat_helpers.py.
tests/test_screencellspair_cpu.py asserts the reference's own caps for every case compared with the reference here."""
import pytest
import torch

import screen_helpers as sh
import screencellspair_helpers as cp
import screenflat_helpers as fh
import screenpair_helpers as sp
import stencil_guards as sg

pytestmark = pytest.mark.gpu
FLAT = True


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(c, gpu, **kw):
    return cp.run(c, gpu, FLAT, **kw)


def lay(t, gpu):
    return fh.to_layout(t, gpu)


@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", cp.KINDS)
def test_screencellspair_flat_every_kind_against_fp64_and_three_pass(gpu, kind, boundary, with_mod):
    """(3, 10, 5, 12) at nk = 10, 1 (the first batch alone), 16 (every later batch full) and 2, 5, 9 (a later batch with one
    live level, for each pair of batch sizes built)"""
    from cp_pre_amd import screen
    for nk, shape in cp.FLAT_MAIN:
        c = cp.case(kind, shape, boundary, with_mod, nk)
        xd = lay(c.x, gpu)
        assert xd.stride(-3) == 1 and xd.stride(-1) == shape[1]
        s = run(c, gpu, x=xd)
        assert screen.last_route() == cp.route(kind, flat=True)
        cp.check(c, s, f"flat fused boundary={boundary} mod={with_mod}")
        s3 = run(c, gpu, x=xd, pair=False)
        assert screen.last_route() == "fallback:minus="
        cp.check(c, s3, "  three-pass")
        cp.check_routes_agree(c, s, s3, "  fused against three-pass")


@pytest.mark.parametrize("name", cp.FLAT_SEAMS)
@pytest.mark.parametrize("kind", cp.FLAT_SEAM_KINDS)
def test_screencellspair_flat_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    c = cp.case(kind, fh.SEAM_SHAPES[name], False, True, 10)
    s = run(c, gpu)
    assert screen.last_route() == cp.route(kind, flat=True)
    cp.check(c, s, name)


@pytest.mark.parametrize("kind", cp.KINDS)
def test_screencellspair_flat_identities(gpu, kind):
    """zero tolerance: constant level fields give the bits of the paired joint screen at those levels; a zero ``minus`` the
    bits of the one-set per-cell screen; ``minus is vars`` score bits 0 and every counted cell inside"""
    from cp_pre_amd import screen
    method = sh.method_of(kind, gpu)
    for boundary in (False, True):
        c = cp.case(kind, sp.FLAT_BASE, boundary, True, 10)
        q = sp.case(kind, sp.FLAT_BASE, boundary, True, nk=10, form="flat").q
        xd, yd, md = lay(c.x, gpu), lay(c.y, gpu), lay(c.mod, gpu)
        joint = screen.screen(method, xd, q.to(gpu), md, boundary=boundary, minus=yd, pair=True)
        assert screen.last_route() == sp.route(kind, "flat")
        qc = lay(q[:, None, None, None].expand(10, *c.shape[1:]).contiguous(), gpu)
        got = run(c, gpu, x=xd, y=yd, q=qc, mod=md)
        assert screen.last_route() == cp.route(kind, flat=True)
        assert cp.same(got, joint) and got.cells == joint.cells
    c = cp.case(kind, sp.FLAT_BASE, False, True, 10)
    xd, qd, md = lay(c.x, gpu), lay(c.q, gpu), lay(c.mod, gpu)
    one = screen.screen_cells(method, xd, qd, md)
    assert screen.last_route() == "fused:flat_cells_" + sp.PAIR_KIND[kind]
    got = run(c, gpu, x=xd, y=torch.zeros_like(xd), q=qd, mod=md)
    assert screen.last_route() == cp.route(kind, flat=True) and cp.same(got, one)
    assert bool((c.q >= 0).all())
    for nk, shape in cp.FLAT_MAIN:
        c = cp.case(kind, shape, False, True, nk)
        xd = lay(c.x, gpu)
        for yd in (xd, xd.clone(memory_format=torch.preserve_format)):
            s = run(c, gpu, x=xd, y=yd)
            assert screen.last_route() == cp.route(kind, flat=True)
            assert bool((sg.bits(s.score) == 0).all()) and bool((s.inside == c.cells).all()) and s.cells == c.cells


@pytest.mark.parametrize("kind", cp.GROUP_KINDS)
def test_screencellspair_flat_across_the_sample_group(gpu, kind):
    from cp_pre_amd import screen
    G = screen.sample_group_pair()
    for B in cp.group_batches(G):
        c = cp.case(kind, (B,) + cp.GROUP_TXY, True, True, 10)
        s = run(c, gpu)
        assert screen.last_route() == cp.route(kind, flat=True)
        cp.check(c, s, f"flat G={G} B={B}")


@pytest.mark.parametrize("nk", [10, 16])
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_screencellspair_flat_levels_are_per_level_and_per_cell(gpu, kind, nk):
    """(k = 0 is a level of the first batch for both kinds, k = 4 and nk - 1 levels of a later one: the batches are 1 + 15
    for the NS momentum and 4 + 12 for the wave star)"""
    c = cp.case(kind, sp.FLAT_BASE, False, True, nk)
    base = run(c, gpu)
    perm = torch.tensor([3, 0, 9, 1, 7, 2, 8, 4, 6, 5] + [15, 10, 13, 11, 14, 12][:nk - 10])
    got = run(c, gpu, q=lay(c.q[perm], gpu))
    assert torch.equal(got.inside, base.inside[perm.to(gpu)]) and torch.equal(sg.bits(got.score), sg.bits(base.score))
    for k in (0, 4, nk - 1):                                         # (k = 0: the NS momentum's first batch, else a later one)
        lo, hi = c.q.clone(), c.q.clone()
        lo[k, 5, 2, 6], hi[k, 5, 2, 6] = -1.0, float("inf")
        glo, ghi = run(c, gpu, q=lay(lo, gpu)), run(c, gpu, q=lay(hi, gpu))
        others = [j for j in range(nk) if j != k]
        assert torch.equal(glo.inside[others], base.inside[others]) and torch.equal(ghi.inside[others], base.inside[others])
        assert bool((ghi.inside[k] - glo.inside[k] == 1).all())
        assert bool(((glo.inside[k] - base.inside[k]).abs() <= 1).all()) and bool(((ghi.inside[k] - base.inside[k]).abs() <= 1).all())


def test_screencellspair_flat_rim_and_non_finite_contract(gpu):
    from cp_pre_amd import screen
    c = cp.case("ns_momentum", sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    base = run(c, gpu)
    method = sh.method_of("ns_momentum", gpu)
    q, mod = c.q.clone(), c.mod.clone()
    for v, t in ((float("nan"), q), (float("inf"), mod)):
        t[..., 0, :, :], t[..., -1, :, :], t[..., :, 0, :], t[..., :, -1, :], t[..., :, :, 0], t[..., :, :, -1] = [v] * 6
    assert cp.same(run(c, gpu, q=lay(q, gpu), mod=lay(mod, gpu)), base)
    # cropped levels (dense [nk, T-2, X-2, Y-2]): padded in the fields' layout; levels in the other layout: copied once
    assert cp.same(run(c, gpu, q=c.q_cropped().to(gpu)), base)
    assert cp.same(run(c, gpu, q=c.q.to(gpu)), base) and screen.last_route() == cp.route(c.kind, flat=True)
    for which in ("x", "y"):
        for v in (float("nan"), float("inf")):
            t = getattr(c, which).clone()
            t[1, 2, 0, 0, 0] = v
            assert cp.same(run(c, gpu, **{which: lay(t, gpu)}), base), (which, v)
    qinf = lay(torch.full_like(c.q, float("inf")), gpu)
    for which in ("x", "y"):
        t = getattr(c, which).clone()
        t[1, 0, 2, 5, 7] = float("nan")
        kw = {which: lay(t, gpu)}
        xd, yd = kw.get("x", lay(c.x, gpu)), kw.get("y", lay(c.y, gpu))
        nbad = int(torch.isnan(method(xd, boundary=True, minus=yd)[c.reg][1]).sum())
        assert 1 <= nbad <= 27
        got = run(c, gpu, q=qinf, **kw)
        assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
        assert bool((got.inside[:, 1] == c.cells - nbad).all()) and bool((got.inside[:, [0, 2]] == c.cells).all())
    q = c.q.clone()
    q[:, 2, 5, 7] = float("inf")
    allin = run(c, gpu, q=lay(q, gpu))
    rest = [0, 1, 2, 4, 5, 6, 7, 8, 9]
    for v in (float("nan"), -0.5):
        q[3, 2, 5, 7] = v
        got = run(c, gpu, q=lay(q, gpu))
        assert bool((got.inside[3] == allin.inside[3] - 1).all()) and torch.equal(got.inside[rest], allin.inside[rest])
    q[3, 2, 5, 7] = float("inf")
    mod = c.mod.clone()
    mod[2, 5, 7] = 0.0
    got = run(c, gpu, q=lay(q, gpu), mod=lay(mod, gpu))
    assert bool(torch.isinf(got.score).all()) and bool((got.inside == allin.inside - 1).all())


def _embedded(t, gpu, extra):
    """(allocation, view holding ``t``): channels [1:1+F] of a larger stacked tensor, or the field / the levels / the
    modulation itself, Nt-fastest in a guarded allocation"""
    n = t.dim()
    order = tuple(range(n - 3)) + (n - 2, n - 1, n - 3)
    if n == 5:
        big = torch.zeros(t.shape[0], t.shape[1] + extra, *t.shape[2:])
        big[:, 1:1 + t.shape[1]] = t
        alloc, view = sg.embed(big, order, None, 0, gpu)
        return alloc, view[:, 1:1 + t.shape[1]]
    return sg.embed(t, order, None, 0, gpu)


@pytest.mark.parametrize("kind", cp.VIEW_KINDS)
def test_screencellspair_flat_views_in_poisoned_memory(gpu, kind):
    """``vars[:, i]`` / ``minus[:, i]`` of larger storages, the modulation and the levels in guarded allocations filled with
    NaN, 0 and 1e30 around the views: the bits of the dense run, and nothing written"""
    from cp_pre_amd import screen
    c = cp.case(kind, sp.FLAT_BASE, False, True, 10)
    dense = run(c, gpu)
    xa, xd = _embedded(c.x, gpu, 2)
    ya, yd = _embedded(c.y, gpu, 3)
    ma, md = _embedded(c.mod, gpu, 0)
    qa, qd = _embedded(c.q, gpu, 0)
    allocs = [xa, ya, ma, qa]
    masks = [sg.outside_mask(a, v) for a, v in zip(allocs, (xd, yd, md, qd))]
    for value in sg.POISONS:
        for a, m in zip(allocs, masks):
            sg.poison(a, m, value)
        before = [a.clone() for a in allocs]
        got = run(c, gpu, x=xd, y=yd, q=qd, mod=md)
        assert screen.last_route() == cp.route(kind, flat=True), screen.last_route()
        assert cp.same(got, dense), (kind, value)
        assert all(torch.equal(sg.bits(a), sg.bits(b)) for a, b in zip(allocs, before))


@pytest.mark.parametrize("kind", ["ns_momentum", "mhd_continuity"])
def test_screencellspair_flat_slabs_along_x_equal_the_whole_grid(gpu, kind):
    """the merged-row march composes along its marched axis (logical x: slabs with their halo rows and crop 1), in two
    orders, and over batch halves"""
    from cp_pre_amd import screen
    c = cp.case(kind, fh.SEAM_SHAPES["two_marches"], False, True, 10)
    whole = run(c, gpu)
    assert screen.last_route() == cp.route(kind, flat=True)
    method = sh.method_of(kind, gpu)
    xd, yd, md, q = lay(c.x, gpu), lay(c.y, gpu), lay(c.mod, gpu), lay(c.q, gpu)
    for order in (((0, 9), (7, 17)), ((7, 17), (0, 9))):
        s = screen.ScreenCells(3, c.nk, gpu)
        for x0, x1 in order:
            s.add_slab(method, xd[..., x0:x1, :], q[:, :, x0:x1], md[:, x0:x1], minus=yd[..., x0:x1, :], pair=True)
            assert screen.last_route() == cp.route(kind, flat=True)
        got = s.finish()
        assert got.cells == whole.cells and cp.same(got, whole)
    parts = []
    for a, b in ((0, 2), (2, 3)):
        s = screen.ScreenCells(b - a, c.nk, gpu)
        s.add_slab(method, xd[a:b], q, md, minus=yd[a:b], pair=True)
        parts.append(s.finish())
    assert torch.equal(sg.bits(torch.cat([p.score for p in parts])), sg.bits(whole.score))
    assert torch.equal(torch.cat([p.inside for p in parts], dim=1), whole.inside)


def test_screencellspair_flat_fallbacks_say_why_and_agree(gpu):
    from cp_pre_amd import screen
    kind = "ns_momentum"
    c = cp.case(kind, sp.FLAT_BASE, False, True, 10)
    s = run(c, gpu, y=c.y.to(gpu))
    assert screen.last_route() == "fallback:field sets in different layouts"
    cp.check(c, s, "Nt-fastest vars, Ny-fastest minus")
    big = torch.full((3, 3, 16, 5, 12), 7.0)
    big[:, :, 2:12] = c.y
    s = run(c, gpu, y=lay(big, gpu)[:, :, 2:12])
    assert screen.last_route() == "fallback:minus: rows not dense"
    cp.check(c, s, "t-slab of an Nt-fastest minus")
    oc = cp.case(kind, sp.ODD_FLAT, False, True, 10)
    s = run(oc, gpu)
    assert screen.last_route() == "fallback:merged row Ny*Nt not a multiple of 4"
    cp.check(oc, s, "flat Ny = 13")
    a = run(c, gpu, pair=False)
    assert screen.last_route() == "fallback:minus="
    cp.check_routes_agree(c, run(c, gpu), a, "fused against fallback:minus=")


@pytest.mark.parametrize("structure", sh.TAP_STRUCTURES)
@pytest.mark.parametrize("kind", cp.TAP_KINDS)
def test_screencellspair_flat_other_tap_structures(gpu, kind, structure):
    """The y-fixed paired MHD continuity (<4>) against the difference stored with the same operators on the same Nt-fastest
    views; the y-fixed paired NS momentum and both general stars are not built: the library declines and the call is the
    three-pass route's answer."""
    from cp_pre_amd import screen
    c = cp.case(kind, sp.FLAT_BASE, False, True, 10)
    method = sh.method_with_taps(kind, structure, gpu)
    xd, yd = lay(c.x, gpu), lay(c.y, gpu)
    s = run(c, gpu, x=xd, y=yd, method=method)
    if cp.BUILT[kind, structure]:
        assert screen.last_route() == cp.route(kind, flat=True)
        assert not cp.same(s, run(c, gpu, x=xd, y=yd))
        cp.check_against_stored_difference(c, s, method, xd, yd, FLAT, f"{kind} {structure} flat")
    else:
        assert screen.last_route() == "fallback:declined by the library"
        s3 = run(c, gpu, x=xd, y=yd, method=method, pair=False)
        assert screen.last_route() == "fallback:minus=" and cp.same(s, s3)
