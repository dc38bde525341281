"""Per-sample statistics of the 1-D residuals on [B,Nt,Nx] in both layouts (cp_pre_amd.screen.screen_stats,
csrc/screen_rows_stats.hip) on the GPU, against float64 (pytest -m gpu).  Reference, tolerances and cases:
tests/screenstats_helpers.py; layouts and seams: tests/screen1d_helpers.py."""
import pytest
import torch

import screen1d_helpers as s1
import screenstats_helpers as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(c, layout, gpu, x=None, method=None):
    from cp_pre_amd import screen
    xd = s1.lay(c.x, layout, gpu) if x is None else x
    return screen.screen_stats(method or s1.method_of(c.kind, gpu), xd, boundary=c.boundary)


# ------------------------------------------------------------------ 1. every kind, both layouts, both boundary values
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", s1.KINDS)
def test_rows_stats_every_kind_against_fp64_and_the_fallback(gpu, kind, layout, boundary):
    from cp_pre_amd import screen
    for name in ("wave_segments", "chunks_and_idle_lanes", "partial_last_strip"):
        B, plane = s1.SEAM_PLANES[name]
        c = st.rows_case(kind, B, plane, layout, boundary)
        xd = s1.lay(c.x, layout, gpu)
        assert xd.stride(2 if layout == "nx" else 1) == 1
        got = run(c, layout, gpu, xd)
        assert screen.last_route() == st.route(kind, "rows")          # (the rows route by default: nothing to opt into)
        st.check(got, c.ref, f"{kind} {name} {layout} boundary={boundary}")
        fb = screen.screen_stats(s1.method_of(kind), s1.lay(c.x, layout, "cpu"), boundary=boundary)
        assert screen.last_route() == "fallback:input on the CPU" and not fb.sum.is_cuda
        st.check(fb, c.ref, "  fallback")


# ------------------------------------------------------------------ 2. the seams, B = 1 and B = 5
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("name", list(s1.SEAM_PLANES))
@pytest.mark.parametrize("kind", st.ROWS_SEAM_KINDS)
def test_rows_stats_at_the_seams(gpu, kind, name, layout):
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES[name]
    for boundary in (False, True):
        c = st.rows_case(kind, B, plane, layout, boundary)
        got = run(c, layout, gpu)
        assert screen.last_route() == st.route(kind, "rows")
        st.check(got, c.ref, f"{kind} {name} {layout} boundary={boundary}")


@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind", st.ROWS_SEAM_KINDS)
def test_rows_stats_one_and_five_samples(gpu, kind, B, layout):
    from cp_pre_amd import screen
    c = st.rows_case(kind, B, (12, 64), layout)
    got = run(c, layout, gpu)
    assert screen.last_route() == st.route(kind, "rows")
    st.check(got, c.ref, f"{kind} B={B} {layout}")


# ------------------------------------------------------------------ 3. against the parent's own kernel
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_rows_stats_max_abs_has_the_bits_of_the_joint_screens_score(gpu, layout):
    from cp_pre_amd import screen
    for name in ("wave_segments", "chunks_odd_rows", "two_strips_and_a_quad"):
        B, plane = s1.SEAM_PLANES[name]
        c = st.rows_case("burgers", B, plane, layout)
        xd = s1.lay(c.x, layout, gpu)
        s = screen.screen(s1.method_of("burgers", gpu), xd, torch.ones(1, device=gpu), None)
        assert screen.last_route() == "fused:rows_burgers"
        got = run(c, layout, gpu, xd)
        assert torch.equal(got.max_abs.view(torch.int32), s.score.view(torch.int32)), (name, layout)


# ------------------------------------------------------------------ 4. bytes
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_rows_stats_same_bytes_on_every_run_whatever_the_workspace_held(gpu, layout):
    from cp_pre_amd import screen
    B, plane = s1.SEAM_PLANES["fewer_rows_than_segments"]          # (waves with no counted row: their slots still count)
    for kind, (B, plane) in (("burgers", (B, plane)), ("advection", s1.SEAM_PLANES["two_strips_and_a_quad"])):
        c = st.rows_case(kind, B, plane, layout)
        xd = s1.lay(c.x, layout, gpu)
        first = run(c, layout, gpu, xd)
        assert screen.last_route() == st.route(kind, "rows") and screen._stats_ws
        for ws in screen._stats_ws.values():
            ws.fill_(float("nan"))
        second = run(c, layout, gpu, xd)
        assert st.same_bits(first, second) and not bool(torch.isnan(second.sum).any())


# ------------------------------------------------------------------ 5. row slabs
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_rows_stats_row_slabs_compose(gpu, layout):
    """slabs of the plane's ROWS (Nt for Nx-fastest fields, Nx for Nt-fastest ones), overlapping by the two rows a slab
    reads for nothing, in two orders"""
    from cp_pre_amd import screen
    kind, (B, plane) = "burgers", s1.SEAM_PLANES["chunks_and_idle_lanes"]       # 130 rows x 12 columns
    c = st.rows_case(kind, B, plane, layout)
    method, xd = s1.method_of(kind, gpu), s1.lay(c.x, layout, gpu)
    whole = run(c, layout, gpu, xd)
    st.check(whole, c.ref, "whole plane")
    cuts = ((0, 41), (39, 100), (98, 130))
    for order in (cuts, cuts[::-1]):
        s = screen.ScreenStats(B, gpu)
        for r0, r1 in order:
            slab = xd[:, r0:r1] if layout == "nx" else xd[:, :, r0:r1]
            s.add_slab(method, slab, crop=(1, 1))
            assert screen.last_route() == "fused:rows_stats_burgers"
        got = s.finish()
        assert got.cells == whole.cells
        assert torch.equal(got.max_abs.view(torch.int32), whole.max_abs.view(torch.int32))
        assert st.sums_close(got, whole)
    with pytest.raises(RuntimeError, match="halo_x"):
        screen.ScreenStats(B, gpu).add_slab(method, xd, crop=(1, 1), halo_x=True)


# ------------------------------------------------------------------ 6. non-finite values
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_rows_stats_non_finite_contract(gpu, layout):
    c = st.rows_case("burgers", 3, (12, 64), layout)
    base = run(c, layout, gpu)
    for value in (float("nan"), float("inf")):
        x = c.x.clone()
        x[1, 0, 0], x[2, -1, -1] = value, value                  # (corners: the star reaches rim cells only)
        assert st.same_bits(run(c, layout, gpu, s1.lay(x, layout, gpu)), base), value
    x = c.x.clone()
    x[1, 5, 7] = float("nan")
    got = run(c, layout, gpu, s1.lay(x, layout, gpu))
    for t, b in ((got.sum, base.sum), (got.sum_abs, base.sum_abs), (got.sum_sq, base.sum_sq), (got.max_abs, base.max_abs)):
        assert bool(torch.isnan(t[1])) and torch.equal(t[[0, 2]], b[[0, 2]])


# ------------------------------------------------------------------ 7. pitched views
@pytest.mark.parametrize("layout", s1.LAYOUTS)
def test_rows_stats_rows_padded_beyond_their_length(gpu, layout):
    from cp_pre_amd import screen
    c = st.rows_case("advection", 3, (12, 64), layout)
    dense = run(c, layout, gpu)
    x = s1.lay(c.x, layout, gpu)
    mem = x if layout == "nx" else x.transpose(1, 2)             # the contiguous [B,R,C] memory
    for pad, value in ((4, float("nan")), (12, float("inf"))):
        big = torch.full((mem.shape[0] + 1, mem.shape[1] + 2, mem.shape[2] + pad), value, device=gpu)
        big[:-1, 1:-1, :mem.shape[2]] = mem
        view = big[:-1, 1:-1, :mem.shape[2]]
        view = view if layout == "nx" else view.transpose(1, 2)
        assert tuple(view.shape) == tuple(x.shape) and view.stride(0) > x.stride(0)
        got = run(c, layout, gpu, view)
        assert screen.last_route() == st.route("advection", "rows")
        assert st.same_bits(got, dense), (layout, pad)


# ------------------------------------------------------------------ 8. odd widths, and the 4-D input
@pytest.mark.parametrize("layout", s1.LAYOUTS)
@pytest.mark.parametrize("kind", st.ROWS_SEAM_KINDS)
def test_rows_stats_odd_planes_take_the_fallback(gpu, kind, layout):
    from cp_pre_amd import screen
    for B, plane in s1.ODD_PLANES:
        for boundary in (False, True):
            c = st.rows_case(kind, B, plane, layout, boundary)
            got = run(c, layout, gpu)
            assert screen.last_route() == "fallback:contiguous-axis length not a multiple of 4"
            st.check(got, c.ref, f"{kind} {plane} {layout} boundary={boundary}")
    c = st.rows_case(kind, 3, (12, 64), "nx")
    got = screen.screen_stats(s1.method_of(kind, gpu), c.x.to(gpu)[:, None])
    assert screen.last_route() == "fallback:[BS,1,Nt,Nx] input"
    st.check(got, c.ref, f"{kind} [BS,1,Nt,Nx]")


# ------------------------------------------------------------------ 9. live kernels
def test_rows_stats_see_the_kernels_the_operators_hold_now(gpu):
    from cp_pre_amd import screen
    c = st.rows_case("dxx", 3, (12, 64), "nx")
    op = s1.method_of("dxx", gpu)
    xd = c.x.to(gpu)
    base = screen.screen_stats(op, xd)
    op.kernel = 2 * op.kernel
    got = screen.screen_stats(op, xd)
    assert screen.last_route() == "fused:rows_stats_stencil2d"
    assert torch.equal(got.sum, 2 * base.sum) and torch.equal(got.sum_abs, 2 * base.sum_abs)
    assert torch.equal(got.sum_sq, 4 * base.sum_sq) and torch.equal(got.max_abs, 2 * base.max_abs)
