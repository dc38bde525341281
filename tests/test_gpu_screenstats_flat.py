"""Per-sample statistics of the 2-D residuals on Nt-fastest views - ``pred.permute(0,1,4,2,3)`` of the surrogate's native
output, the view ``Active_Learning/Wave_AL_Joint.py`` passes - (cp_pre_amd.screen.screen_stats, csrc/screen_stats.hip with
the merged-row march) on the GPU, against float64 (pytest -m gpu).  Reference, tolerances and cases:
tests/screenstats_helpers.py; layouts and seams: tests/screenflat_helpers.py."""
import pytest
import torch

import screen_helpers as sh
import screenflat_helpers as sf
import screenstats_helpers as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(c, gpu, x=None, method=None):
    from cp_pre_amd import screen
    xd = sf.to_layout(c.x, gpu) if x is None else x
    return screen.screen_stats(method or sh.method_of(c.kind, gpu), xd, boundary=c.boundary)


# ------------------------------------------------------------------ 1. every kind, both boundary values, and the fallback
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", sf.KINDS)
def test_flat_stats_every_kind_against_fp64_and_the_fallback(gpu, kind, boundary):
    from cp_pre_amd import screen
    for name in st.FLAT_MAIN:
        c = st.flat_case(kind, sf.SEAM_SHAPES[name], boundary)
        xd = sf.to_layout(c.x, gpu)
        assert xd.stride(-3) == 1 and xd.stride(-1) == c.shape[1]
        got = run(c, gpu, xd)
        assert screen.last_route() == st.route(kind, "flat")
        st.check(got, c.ref, f"{kind} {name} boundary={boundary}")
        fb = screen.screen_stats(sh.method_of(kind), sf.to_layout(c.x, "cpu"), boundary=boundary)
        assert screen.last_route() == "fallback:input on the CPU" and not fb.sum.is_cuda
        st.check(fb, c.ref, "  fallback")


# ------------------------------------------------------------------ 2. the seams, B = 1 and B = 5
@pytest.mark.parametrize("name", list(sf.SEAM_SHAPES))
@pytest.mark.parametrize("kind", st.FLAT_SEAM_KINDS)
def test_flat_stats_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        c = st.flat_case(kind, sf.SEAM_SHAPES[name], boundary)
        got = run(c, gpu)
        assert screen.last_route() == st.route(kind, "flat")
        st.check(got, c.ref, f"{kind} {name} boundary={boundary}")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind", st.FLAT_SEAM_KINDS)
def test_flat_stats_one_and_five_samples(gpu, kind, B):
    from cp_pre_amd import screen
    c = st.flat_case(kind, (B,) + sf.BASE[1:])
    got = run(c, gpu)
    assert screen.last_route() == st.route(kind, "flat")
    st.check(got, c.ref, f"{kind} B={B}")


# ------------------------------------------------------------------ 3. against the parent's own kernel
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_flat_stats_max_abs_has_the_bits_of_the_joint_screens_score(gpu, kind):
    from cp_pre_amd import screen
    for name in st.FLAT_MAIN:
        c = st.flat_case(kind, sf.SEAM_SHAPES[name])
        xd = sf.to_layout(c.x, gpu)
        s = screen.screen(sh.method_of(kind, gpu), xd, torch.ones(1, device=gpu), None)
        assert screen.last_route() == sf.ROUTE[kind]
        got = run(c, gpu, xd)
        assert torch.equal(got.max_abs.view(torch.int32), s.score.view(torch.int32)), (kind, name)


# ------------------------------------------------------------------ 4. bytes
@pytest.mark.parametrize("kind", ["ns_momentum", "mhd_momentum"])
def test_flat_stats_same_bytes_on_every_run_whatever_the_workspace_held(gpu, kind):
    from cp_pre_amd import screen
    c = st.flat_case(kind, sf.SEAM_SHAPES["many_marches_last_one"])      # (cropped: the last march counts one plane)
    xd = sf.to_layout(c.x, gpu)
    first = run(c, gpu, xd)
    assert screen.last_route() == st.route(kind, "flat") and screen._stats_ws
    for ws in screen._stats_ws.values():
        ws.fill_(float("nan"))
    second = run(c, gpu, xd)
    assert st.same_bits(first, second) and not bool(torch.isnan(second.sum).any())


# ------------------------------------------------------------------ 6. non-finite values
def test_flat_stats_non_finite_contract(gpu):
    c = st.flat_case("ns_momentum", sf.SEAM_SHAPES["two_chunks"])
    base = run(c, gpu)
    for value in (float("nan"), float("inf")):
        x = c.x.clone()
        x[1, 2, 0, 0, 0] = value                                 # (p at a corner: reaches rim cells only)
        x[2, 0, -1, -1, -1] = value
        assert st.same_bits(run(c, gpu, sf.to_layout(x, gpu)), base), value
    x = c.x.clone()
    x[1, 0, 3, 2, 70] = float("nan")
    got = run(c, gpu, sf.to_layout(x, gpu))
    for t, b in ((got.sum, base.sum), (got.sum_abs, base.sum_abs), (got.sum_sq, base.sum_sq), (got.max_abs, base.max_abs)):
        assert bool(torch.isnan(t[1])) and torch.equal(t[[0, 2]], b[[0, 2]])


# ------------------------------------------------------------------ 7. pitched views
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_flat_stats_pitched_views(gpu, kind):
    """``vars[:, i]`` of a stacked tensor with more channels, and an x-range of a longer grid (a pitched sample stride and
    a base offset), the rest poisoned"""
    from cp_pre_amd import screen
    c = st.flat_case(kind, sf.BASE)
    dense = run(c, gpu)
    x = c.x if c.x.dim() == 5 else c.x[:, None]
    B, F, T, X, Y = x.shape
    for value in (float("nan"), float("inf")):
        big = torch.full((B, F + 2, X + 4, Y, T), value, device=gpu)      # memory [B,F,X,Y,T]
        big[:, 1:-1, 2:-2] = x.permute(0, 1, 3, 4, 2).to(gpu)
        view = big[:, 1:-1, 2:-2].permute(0, 1, 4, 2, 3)                  # logical [B,F,T,X,Y], Nt-fastest
        view = view if c.x.dim() == 5 else view[:, 0]
        assert view.stride(-3) == 1 and view.stride(-1) == T and view.stride(0) > view[0].numel()
        got = run(c, gpu, view)
        assert screen.last_route() == st.route(kind, "flat")
        assert st.same_bits(got, dense), (kind, value)


# ------------------------------------------------------------------ 8. what the flat form does not take
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_flat_stats_shapes_outside_the_layout_take_the_fallback(gpu, kind):
    from cp_pre_amd import screen
    for shape, why in sf.FALLBACK_SHAPES.items():
        c = st.flat_case(kind, shape)
        got = run(c, gpu)
        assert screen.last_route() == why
        st.check(got, c.ref, f"{kind} {shape}")
    shape, sl = sf.SLAB                                          # a t-slab of an Nt-fastest tensor: rows not dense
    c = st.flat_case(kind, shape)
    xd = sf.to_layout(c.x, gpu)[..., sl, :, :]
    got = screen.screen_stats(sh.method_of(kind, gpu), xd, boundary=True)
    assert screen.last_route() == "fallback:rows not dense"
    full = st.Ref(sh.oracle_residual(kind, c.x[..., sl, :, :].contiguous().double()), (0, 0, 0))
    st.check(got, full, f"{kind} t-slab")


# ------------------------------------------------------------------ 9. live kernels
def test_flat_stats_see_the_kernels_the_operators_hold_now(gpu):
    from cp_pre_amd import screen
    c = st.flat_case("lap", sf.BASE)
    op = sh.method_of("lap", gpu)
    xd = sf.to_layout(c.x, gpu)
    base = screen.screen_stats(op, xd)
    op.kernel = 2 * op.kernel
    got = screen.screen_stats(op, xd)
    assert screen.last_route() == "fused:flat_stats_stencil3d"
    assert torch.equal(got.sum, 2 * base.sum) and torch.equal(got.sum_abs, 2 * base.sum_abs)
    assert torch.equal(got.sum_sq, 4 * base.sum_sq) and torch.equal(got.max_abs, 2 * base.max_abs)
