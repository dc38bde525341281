"""The per-cell screen of the 1-D family (cp_pre_amd.screen.screen_cells / ScreenCells with ``rows=True``,
csrc/screen_rows_cells.hip) on the GPU, against float64 (pytest -m gpu).

Reference, level fields, tolerances and cases: tests/screen1dcells_helpers.py (the oracle in float64; tau = 1e-5 max |r_ref|;
score within tau / m_min + one ulp; a count within the undecided cells of its (level, sample)).
tests/test_screen1dcells_cpu.py shows, with the oracle alone, that every case used here keeps its undecided cells below 1 %
and has a level that splits the cells of a sample.  tests/SCREEN1DCELLS_TESTS.md says which test reaches which branch.
No test here provokes a fault: every guard is checked through results in valid memory."""
import ctypes
import os
import subprocess

import pytest
import torch

import screen1d_helpers as s1
import screen1dcells_helpers as h
import stencil_guards as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def same(a, b):
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside)


def agree(c, a, b):
    """two routes that each meet the reference of ``c``: scores within twice its slack, counts within the undecided cells"""
    ds = (a.score.double().cpu() - b.score.double().cpu()).abs()
    assert bool((ds <= 2 * c.tol_s + 2.4e-7 * c.s_ref).all()), ds
    assert bool(((a.inside.cpu() - b.inside.cpu()).abs() <= c.undecided).all())


# ------------------------------------------------------------------ every kind, layout, crop, modulation; three nk
@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", s1.KINDS)
def test_screen1dcells_every_kind_against_fp64_and_the_three_pass_route(gpu, kind, layout, boundary, with_mod):
    from cp_pre_amd import screen
    for nk, name in h.MAIN:
        c = h.case(kind, *s1.SEAM_PLANES[name], layout, boundary, with_mod, nk)
        s = h.run(c, layout, gpu)
        assert screen.last_route() == h.ROUTE[kind]
        h.check(c, s, f"fused {layout} boundary={boundary} mod={with_mod}")
        s3 = h.run(c, layout, gpu, rows=False)
        assert screen.last_route() == h.FALLBACK
        h.check(c, s3, "  three-pass")
        agree(c, s, s3)
        print(f"  fused and three-pass bit-identical: {same(s, s3)}")


@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("name", list(s1.SEAM_PLANES))
@pytest.mark.parametrize("kind", h.SEAM_KINDS)
def test_screen1dcells_at_the_seams(gpu, kind, name, layout):
    from cp_pre_amd import screen
    c = h.case(kind, *s1.SEAM_PLANES[name], layout, False, True, 10)
    s = h.run(c, layout, gpu)
    assert screen.last_route() == h.ROUTE[kind]
    h.check(c, s, f"{name} {layout}")


@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_screen1dcells_across_the_sample_group(gpu, layout):
    """B = G + 1 and B = 2G - 1: a group with one sample and a group one short, next to whole ones"""
    from cp_pre_amd import screen
    G = screen.sample_group_rows()
    assert G >= 1
    for B in h.group_batches(G):
        c = h.case("burgers", B, h.GROUP_PLANE, layout, True, True, 10)
        s = h.run(c, layout, gpu)
        assert screen.last_route() == h.ROUTE["burgers"]
        h.check(c, s, f"G={G} B={B} {layout}")
        # a sample's verdict does not depend on its place in a group: the first three alone give the same bits
        x3, m = s1.lay(c.x[:3], layout, gpu), s1.method_of("burgers", gpu)
        s3 = screen.screen_cells(m, x3, s1.lay(c.q, layout, gpu), s1.lay(c.mod, layout, gpu), boundary=True, rows=True)
        assert torch.equal(sg.bits(s3.score), sg.bits(s.score[:3])) and torch.equal(s3.inside, s.inside[:, :3])
        s3 = screen.screen_cells(m, s1.lay(c.x[-3:], layout, gpu), s1.lay(c.q, layout, gpu), s1.lay(c.mod, layout, gpu),
                                 boundary=True, rows=True)
        assert torch.equal(sg.bits(s3.score), sg.bits(s.score[-3:])) and torch.equal(s3.inside, s.inside[:, -3:])


# ------------------------------------------------------------------ constant level fields: the joint screens' bits
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", ["burgers", "advection"])
@pytest.mark.parametrize("pair", [False, True], ids=["one_set", "pair"])
def test_screen1dcells_constant_level_fields_give_the_joint_screens_bits(gpu, kind, layout, pair):
    from cp_pre_amd import screen
    for nk, name in ((10, "wave_segments"), (16, "partial_last_strip")):
        c = h.case(kind, *s1.SEAM_PLANES[name], layout, False, True, nk, pair)
        m, xd, md = s1.method_of(kind, gpu), s1.lay(c.x, layout, gpu), s1.lay(c.mod, layout, gpu)
        kw = dict(minus=s1.lay(c.y, layout, gpu), pair="rows") if pair else {}
        for mod in (md, None):
            # [nk] levels that split the cells: the medians of the level fields of the case with / without the modulation
            cq = h.case(kind, *s1.SEAM_PLANES[name], layout, False, mod is not None, nk, pair).q
            q = cq.reshape(nk, -1).median(dim=1).values.contiguous()
            joint = screen.screen(m, xd, q.to(gpu), mod, **kw)
            assert screen.last_route() == (s1.ROUTE[kind].replace("rows_", "rows_pair_") if pair else s1.ROUTE[kind])
            print(f"{kind} {layout} pair={pair} nk={nk} mod={mod is not None}: levels {q.tolist()}, joint score {joint.score.tolist()}, "
                  f"inside of sample 0 {joint.inside[:, 0].tolist()} of {joint.cells}")
            assert bool(((joint.inside > 0) & (joint.inside < joint.cells)).any())
            qc = q[:, None, None].expand(nk, *c.shape[1:])
            for qd in (qc.to(gpu), s1.lay(qc.contiguous(), layout, gpu)):   # (strides 0: copied once; then the fields' layout)
                got = h.run(c, layout, gpu, qcells=qd, modulation=mod)
                assert screen.last_route() == (h.ROUTE_PAIR if pair else h.ROUTE)[kind]
                assert got.cells == joint.cells and same(got, joint), (kind, layout, pair, nk)


# ------------------------------------------------------------------ levels are per level and per cell
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_screen1dcells_levels_are_per_level_and_per_cell(gpu, layout):
    c = h.case("burgers", *s1.SEAM_PLANES["wave_segments"], layout, False, True, 10)
    base = h.run(c, layout, gpu)
    perm = torch.tensor([3, 0, 9, 1, 7, 2, 8, 4, 6, 5])
    got = h.run(c, layout, gpu, qcells=s1.lay(c.q[perm], layout, gpu))
    assert torch.equal(got.inside, base.inside[perm.to(gpu)]) and torch.equal(sg.bits(got.score), sg.bits(base.score))
    # one counted cell's level at one k past every sample's |r| there: row k only, by one
    t, x = (5, 37) if layout == "nx" else (37, 5)
    lo, hi = c.q.clone(), c.q.clone()
    lo[4, t, x], hi[4, t, x] = 0.5 * float(c.r_ref[:, t, x].abs().min()) * float(1.0 / c.mod[t, x]), float("inf")
    glo, ghi = h.run(c, layout, gpu, qcells=s1.lay(lo, layout, gpu)), h.run(c, layout, gpu, qcells=s1.lay(hi, layout, gpu))
    others = [k for k in range(10) if k != 4]
    for g in (glo, ghi):
        assert torch.equal(g.inside[others], base.inside[others]) and torch.equal(sg.bits(g.score), sg.bits(base.score))
    assert bool((ghi.inside[4] - glo.inside[4] == 1).all())          # below every |r| / m there, then above: every sample
    assert bool(((ghi.inside[4] - base.inside[4]) >= 0).all()) and bool(((base.inside[4] - glo.inside[4]) >= 0).all())


# ------------------------------------------------------------------ pairs
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", h.PAIR_KINDS)
def test_screen1dcells_pairs_against_fp64_and_minus_equal_vars(gpu, kind, layout):
    from cp_pre_amd import screen
    c = h.case(kind, *s1.SEAM_PLANES["wave_segments"], layout, False, True, 10, True)
    s = h.run(c, layout, gpu)
    assert screen.last_route() == h.ROUTE_PAIR[kind]
    h.check(c, s, f"pair {layout}")
    s3 = h.run(c, layout, gpu, rows=False)
    assert screen.last_route() == h.FALLBACK                        # (the family's reason comes before ``minus=``)
    h.check(c, s3, "  three-pass")
    agree(c, s, s3)
    # minus == vars: score exactly 0, every counted cell inside at every non-negative, non-NaN level (the order statistics
    # are); for every star mode of the Burgers entry: the reference taps in either layout, and a general star
    methods = [s1.method_of(kind, gpu)]
    if kind == "burgers":
        g = s1.method_of(kind, gpu)
        g.__self__.D_t.kernel.data[1, 0] = 0.25                      # D_t with a tap along Nx too: the general star
        methods.append(g)
    xd = s1.lay(c.x, layout, gpu)
    for m in methods:
        for x2 in (xd, xd.clone()):
            got = screen.screen_cells(m, xd, s1.lay(c.q, layout, gpu), s1.lay(c.mod, layout, gpu), minus=x2, rows=True)
            assert screen.last_route() == h.ROUTE_PAIR[kind]
            assert bool((sg.bits(got.score) == 0).all()) and bool((got.inside == c.cells).all())
    # sets in different layouts keep the three-pass route and say so
    other = "nt" if layout == "nx" else "nx"
    got = h.run(c, layout, gpu, minus=s1.lay(c.y, other, gpu))
    assert screen.last_route() == "fallback:field sets in different layouts"
    h.check(c, got, "  sets in different layouts")
    # each set with its own pitches, in poisoned memory
    order, row = ((0, 1, 2), 1) if layout == "nx" else ((0, 2, 1), 2)
    aa, av = sg.embed(c.x, order, {row: 4, 0: 8}, 0, gpu)
    ba, bv = sg.embed(c.y, order, {row: 12}, 3, gpu)
    assert av.stride() != bv.stride()
    for value in sg.POISONS:
        sg.poison(aa, sg.outside_mask(aa, av), value)
        sg.poison(ba, sg.outside_mask(ba, bv), value)
        got = screen.screen_cells(s1.method_of(kind, gpu), av, s1.lay(c.q, layout, gpu), s1.lay(c.mod, layout, gpu), minus=bv, rows=True)
        assert screen.last_route() == h.ROUTE_PAIR[kind] and same(got, s), value


# ------------------------------------------------------------------ the rim and the non-finite contract
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_screen1dcells_rim_and_non_finite_contract(gpu, layout):
    from cp_pre_amd import screen
    c = h.case("burgers", *s1.SEAM_PLANES["wave_segments"], layout, False, True, 10)
    base = h.run(c, layout, gpu)
    m = s1.method_of("burgers", gpu)
    L = lambda t: s1.lay(t, layout, gpu)
    ij = (5, 37) if layout == "nx" else (37, 5)                      # a counted cell, away from the rim
    # NaN / inf in the rim of the levels, of the modulation and of the fields' neighbours reach nothing
    q, mod = c.q.clone(), c.mod.clone()
    for v, t in ((float("nan"), q), (float("inf"), mod)):
        t[..., 0, :], t[..., -1, :], t[..., :, 0], t[..., :, -1] = [v] * 4
    assert same(h.run(c, layout, gpu, qcells=L(q), modulation=L(mod)), base)
    # cropped levels: the bits of uncropped levels with any rim
    assert same(h.run(c, layout, gpu, qcells=c.q_cropped().to(gpu)), base)
    # a NaN field value in a corner reaches rim cells only (the star has no corner taps)
    x = c.x.clone()
    x[1, 0, 0] = x[1, -1, -1] = float("nan")
    assert same(screen.screen_cells(m, L(x), L(c.q), L(c.mod), rows=True), base)
    # a NaN residual in counted cells: outside at every level, +inf levels included; the other samples do not move
    x = c.x.clone()
    x[(1,) + ij] = float("nan")
    r = m(L(x), boundary=True)
    nbad = int(torch.isnan(r[c.reg][1]).sum())
    assert 1 <= nbad <= 5
    qinf = torch.full_like(c.q, float("inf"))
    got = screen.screen_cells(m, L(x), L(qinf), L(c.mod), rows=True)
    assert bool(torch.isnan(got.score[1])) and not bool(torch.isnan(got.score[[0, 2]]).any())
    assert bool((got.inside[:, 1] == c.cells - nbad).all()) and bool((got.inside[:, [0, 2]] == c.cells).all())
    # a NaN level and a negative level in a counted cell: outside at that level only
    q = c.q.clone()
    q[(slice(None),) + ij] = float("inf")
    allin = h.run(c, layout, gpu, qcells=L(q))
    rest = [0, 1, 2, 4, 5, 6, 7, 8, 9]
    for v in (float("nan"), -0.5):
        q[(3,) + ij] = v
        got = h.run(c, layout, gpu, qcells=L(q))
        assert bool((got.inside[3] == allin.inside[3] - 1).all()) and torch.equal(got.inside[rest], allin.inside[rest])
    # m == 0 in a counted cell: inf * 0 is NaN, the cell is outside at every level, and r / 0 makes every score inf
    q[(3,) + ij] = float("inf")
    mod = c.mod.clone()
    mod[ij] = 0.0
    got = h.run(c, layout, gpu, qcells=L(q), modulation=L(mod))
    assert bool(torch.isinf(got.score).all()) and bool((got.inside == allin.inside - 1).all())


# ------------------------------------------------------------------ pitched views in poisoned memory
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", ["burgers", "dxx"])
def test_screen1dcells_pitched_views_in_poisoned_memory(gpu, kind, layout):
    from cp_pre_amd import _lib, screen
    from cp_pre_amd.screen import _Spec
    c = h.case(kind, *s1.SEAM_PLANES["wave_segments"], layout, False, True, 10)
    dense = h.run(c, layout, gpu)
    f_order, q_order, m_order, row = ((0, 1, 2), (0, 1, 2), (0, 1), 1) if layout == "nx" else ((0, 2, 1), (0, 2, 1), (1, 0), 2)
    method = s1.method_of(kind, gpu)
    for offset, pitch in ((1, 5), (3, 8), (0, 4)):
        alloc, xd = sg.embed(c.x, f_order, {row: pitch, 0: 3}, offset, gpu)
        malloc, md = sg.embed(c.mod, m_order, {row - 1: pitch + 1}, offset, gpu)
        qalloc, qd = sg.embed(c.q, q_order, {row: pitch + 2, 0: 7}, offset, gpu)
        assert xd.stride(3 - row) == 1 and qd.stride(3 - row) == 1 and md.stride(2 - row) == 1
        assert qd.stride(row) > qd.shape[3 - row] and qd.stride(0) > qd.stride(row) * qd.shape[row]
        allocs = [alloc, malloc, qalloc]
        masks = [sg.outside_mask(alloc, xd), sg.outside_mask(malloc, md), sg.outside_mask(qalloc, qd)]
        for value in sg.POISONS:
            for a, m in zip(allocs, masks):
                sg.poison(a, m, value)
            before = [a.clone() for a in allocs]
            got = screen.screen_cells(method, xd, qd, md, rows=True)
            assert screen.last_route() == h.ROUTE[kind]
            assert same(got, dense), (offset, pitch, value)
            assert all(torch.equal(sg.bits(a), sg.bits(b)) for a, b in zip(allocs, before))
    # levels and modulation in the other layout: copied once, same bits
    other = "nt" if layout == "nx" else "nx"
    got = h.run(c, layout, gpu, qcells=s1.lay(c.q, other, gpu), modulation=s1.lay(c.mod, other, gpu))
    assert same(got, dense) and screen.last_route() == h.ROUTE[kind]
    # score / count beyond [B] stay as they are: the launch itself, on accumulators wider than the batch
    B, nk, ld = c.shape[0], c.nk, c.shape[0] + 5
    acc = torch.full((nk + 1, ld), 0x5a5a5a5a, dtype=torch.int32, device=gpu)
    acc[:, :B] = 0
    spec = _Spec(method)
    xd, qd, md = s1.lay(c.x, layout, gpu), s1.lay(c.q, layout, gpu), s1.lay(c.mod, layout, gpu)
    why, kernels = spec.prepare_rows(xd, None, qd, md)
    assert why is None
    st = _lib.PreScreen1dCells(_lib.ptr(qd), nk, *qd.stride(), _lib.ptr(md), *md.stride(), 1, 1,
                               ctypes.c_void_p(acc[0].data_ptr()), ctypes.c_void_p(acc[1].data_ptr()), ld)
    assert spec.launch(kernels, xd, st, 0, "rows", cells=True) == _lib.PRE_OK
    torch.cuda.synchronize()
    assert bool((acc[:, B:] == 0x5a5a5a5a).all())
    assert torch.equal(acc[0, :B], sg.bits(dense.score)) and torch.equal(acc[1:, :B].to(torch.int64), dense.inside)


# ------------------------------------------------------------------ row slabs
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("pair", [False, True], ids=["one_set", "pair"])
def test_screen1dcells_row_slabs_compose_bit_for_bit(gpu, layout, pair):
    """slabs of the plane's rows (Nt for Nx-fastest fields, Nx for Nt-fastest ones) with crops that count every cell once"""
    from cp_pre_amd import screen
    c = h.case("burgers", *s1.SEAM_PLANES["wave_segments"], layout, False, True, 10, pair)
    whole = h.run(c, layout, gpu)
    assert same(h.run(c, layout, gpu), whole)                         # two runs: identical bytes
    method = s1.method_of("burgers", gpu)
    xd, qd, md = s1.lay(c.x, layout, gpu), s1.lay(c.q, layout, gpu), s1.lay(c.mod, layout, gpu)
    yd = s1.lay(c.y, layout, gpu) if pair else None
    ax = 1 if layout == "nx" else 2                                   # the rows of the plane, as an axis of [B,Nt,Nx]
    n = c.shape[ax]
    cuts = ((0, n // 2 + 1), (n // 2 - 1, n))                         # overlap 2: crop 1 of each counts every row once
    for order in (cuts, cuts[::-1]):
        s = screen.ScreenCells(c.shape[0], c.nk, gpu)
        for a, b in order:
            sl = lambda t, d=0: t.narrow(ax - d, a, b - a)
            s.add_slab(method, sl(xd), qd.narrow(ax, a, b - a), sl(md, 1), crop=(1, 1), minus=sl(yd) if pair else None, rows=True)
            assert screen.last_route() == (h.ROUTE_PAIR if pair else h.ROUTE)["burgers"]
        got = s.finish()
        assert got.cells == whole.cells and same(got, whole), order
    # three slabs, the middle one cropped on the rows only by its neighbours' overlap
    s = screen.ScreenCells(c.shape[0], c.nk, gpu)
    thirds = ((0, n // 3 + 1), (n // 3 - 1, 2 * n // 3 + 1), (2 * n // 3 - 1, n))
    for a, b in thirds[::-1]:
        s.add_slab(method, xd.narrow(ax, a, b - a), qd.narrow(ax, a, b - a), md.narrow(ax - 1, a, b - a), crop=(1, 1),
                   minus=yd.narrow(ax, a, b - a) if pair else None, rows=True)
    assert same(s.finish(), whole)


# ------------------------------------------------------------------ what keeps the three-pass route, and refused calls
def test_screen1dcells_fallbacks_say_why_launch_nothing_and_agree(gpu, monkeypatch):
    from cp_pre_amd import _lib, screen
    c = h.case("burgers", *s1.SEAM_PLANES["wave_segments"], "nx", False, True, 10)
    fused = h.run(c, "nx", gpu)
    xd, qd, md = c.x.to(gpu), c.q.to(gpu), c.mod.to(gpu)
    m = s1.method_of("burgers", gpu)

    def never():
        raise AssertionError("libcp_pre_screen1dcells.so was asked for on a three-pass route")
    monkeypatch.setattr(_lib, "load_screen1dcells", never)
    for label, call, why in (
            ("rows=False", lambda: screen.screen_cells(m, xd, qd, md), "1-D family: the marched axis is the batch"),
            ("CPU inputs", lambda: screen.screen_cells(s1.method_of("burgers"), c.x, c.q_cropped(), c.mod, rows=True), "input on the CPU"),
            ("float64 levels", lambda: screen.screen_cells(m, xd, qd.double(), md, rows=True), "float64 levels or modulation"),
            ("[BS,1,Nt,Nx]", lambda: screen.screen_cells(m, xd[:, None], qd, md, rows=True), "[BS,1,Nt,Nx] input")):
        got = call()
        assert screen.last_route() == "fallback:" + why, label
        h.check(c, got, label)
        agree(c, got, fused)
    live = s1.method_of("burgers", gpu)
    live.__self__.D_x.kernel.requires_grad_(True)
    got = screen.screen_cells(live, xd, qd, md, rows=True)
    assert screen.last_route() == "fallback:operator kernel requires grad"
    h.check(c, got, "kernels that require grad")
    # no unit-stride axis; an odd contiguous length (in both layouts)
    wide = torch.zeros(c.shape[0], c.shape[1], 2 * c.shape[2], device=gpu)
    wide[:, :, ::2] = xd
    got = screen.screen_cells(m, wide[:, :, ::2], qd, md, rows=True)
    assert screen.last_route() == "fallback:no unit-stride axis"
    h.check(c, got, "no unit-stride axis")
    for layout in s1.LAYOUTS:
        o = h.case("burgers", *s1.ODD_PLANES[1], layout, False, True, 10)
        got = h.run(o, layout, gpu)
        assert screen.last_route() == "fallback:contiguous-axis length not a multiple of 4"
        h.check(o, got, "odd contiguous length " + layout)
    # a method outside the family: rows=True has no effect
    import screen_helpers as sh
    import screencells_helpers as ch
    w = ch.case("wave", sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    got = screen.screen_cells(sh.method_of("wave", gpu), w.x.to(gpu), w.q.to(gpu), w.mod.to(gpu), rows=True)
    assert screen.last_route() == ch.route("wave")
    ch.check(w, got, "rows=True on a 2-D method")
    # refused calls: every argument error is raised before any device work
    s = screen.ScreenCells(c.shape[0], c.nk, gpu)
    for bad in (lambda: s.add_slab(m, xd, qd[:3], md, crop=(1, 1), rows=True), lambda: s.add_slab(m, xd, qd[:, 1:], md, crop=(1, 1), rows=True),
                lambda: s.add_slab(m, xd, qd, md[1:], crop=(1, 1), rows=True), lambda: s.add_slab(m, xd[:2], qd, md, crop=(1, 1), rows=True),
                lambda: s.add_slab(m, xd, qd, md, crop=(6, 1), rows=True), lambda: s.add_slab(m, xd, qd, md, rows=True),
                lambda: s.add_slab(m, xd, c.q_cropped().to(gpu), md, crop=(1, 1), rows=True),
                lambda: s.add_slab(m, xd, qd, md, crop=(1, 1), minus=xd[:2], rows=True)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="halo_x"):
        s.add_slab(m, xd, qd, md, crop=(1, 1), halo_x=True, rows=True)
    torch.cuda.synchronize()
    assert s.acc is None and s.cells == 0


def test_screen1dcells_refused_calls_leave_the_accumulators(gpu):
    from cp_pre_amd import screen
    c = h.case("burgers", *s1.SEAM_PLANES["wave_segments"], "nt", False, True, 10)
    m = s1.method_of("burgers", gpu)
    xd, qd, md = s1.lay(c.x, "nt", gpu), s1.lay(c.q, "nt", gpu), s1.lay(c.mod, "nt", gpu)
    s = screen.ScreenCells(c.shape[0], c.nk, gpu)
    s.add_slab(m, xd, qd, md, crop=(1, 1), rows=True)
    assert screen.last_route() == h.ROUTE["burgers"]
    before = s.acc.clone()
    for bad in (lambda: s.add_slab(m, xd, qd[:, :, 1:], md, crop=(1, 1), rows=True),
                lambda: s.add_slab(m, xd, qd, md, crop=(1, 1, 1), rows=True)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(s.acc, before) and s.cells == c.cells


def test_screen1dcells_c_client_runs(gpu, tmp_path):
    """tests/c_abi/screen1dcells_check.c on the device: all four entries in both layouts against plain C loops with per-cell
    levels, B one past the sample group, a run without a modulation, two row slabs against the whole plane, b == a, and the
    argument errors of the entries.

    Its row-slab check of the one-set Burgers entry on Nt-fastest fields (17 samples of a [12,24] plane) is the one that
    shows a row step of the march rounding unlike the others: before ``RowsFn<Burgers<3>>`` (csrc/screen_rows.h) stated the
    order of the functor's last operations, 2 of the 17 scores differed by 1 and 2 ulp between the whole plane and its two
    slabs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "screen1dcells_check"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(root, "tests", "c_abi", "screen1dcells_check.c"), "-I" + os.path.join(root, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(root, "cp_pre_amd"), "-l:libcp_pre_screen1dcells.so",
                           "-Wl,-rpath," + os.path.join(root, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") >= 60, out.stdout
