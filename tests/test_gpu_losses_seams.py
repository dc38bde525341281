"""The fused VJP and loss kernels (csrc/residual_vjp.hip) at their seams, against float64 (pytest -m gpu).

``vjp_march_kernel`` cuts a grid into t-segments (``pick_tseg`` halves Nt until <= 16; marches of 8 planes where no star
has a tap along the marched axis), row tiles and column tiles (32 rows x 64 columns for Ny < 192, else 8 x 256).  The
shapes of ``losses_helpers.SEAM_SHAPES`` put every one of these seams into grids of a few workgroups, so ``pick_tseg`` takes
its shortest candidate: segment lengths 9+8, 12+11, 14+13, 9+9+9+6, 4x10, 4x16 (all four exits of the register rotation,
both LDS parities at a cut), last marches of 1, 2, 3, 5 and 8 planes, 2 and 3 row seams in either tile, column seams with
a partial last quad of 1, 2 and 3 cells.  The linear routes run asymmetric stars (tm != tp, xm != xp, ym != yp).

Every case is compared with the float64 autograd gradient of ``losses_helpers.ref64`` under TOL - per channel for stacked
inputs - and run again on ``vars[:, i]`` views of a larger, pitched, misaligned tensor whose surroundings are NaN, 0.0 and
1e30 in turn: the bits must equal the dense run's.  tests/test_losses_ref_cpu.py shows the same formulas in fp32 on the
CPU within TOL / 4 of float64 at every one of these shapes (tests/LOSSES_TESTS.md)."""
import ctypes

import pytest
import torch

import stencil_guards as sg
from losses_helpers import LOSS_SHAPES, ROUTES, SEAM_SHAPES, Route, channel_errs, ref_loss, ref_vjp, seam_groups, seam_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-5
VIEWS = ((1, 5), (3, 8))            # (base offset in floats, extra floats per row): sX > Y, rows 4 and 12 bytes off 16


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def place(route, x, gpu, offset, pitch):
    """(allocation, view): the CPU input ``x`` as ``vars[:, i]`` views of a larger tensor in a guarded allocation, rows
    ``pitch`` floats further apart than they are long, the base ``offset`` floats off the guard's 16-byte boundary."""
    if route.nchan is None:
        big = torch.zeros((x.shape[0], 3) + tuple(x.shape[1:]))
        big[:, 1] = x
    else:
        big = torch.zeros((x.shape[0], x.shape[1] + 2) + tuple(x.shape[2:]))
        big[:, 1:-1] = x
    alloc, view = sg.embed(big, None, {big.dim() - 2: pitch}, offset, gpu)
    return alloc, (view[:, 1] if route.nchan is None else view[:, 1:-1])


def poisoned_runs(owned, run):
    """``sg.three_ways`` for several allocations: ``owned`` = [(allocation, view), ...]"""
    masks = [sg.outside_mask(a, v) for a, v in owned]
    seen, last = [], None
    for value in sg.POISONS:
        for (a, _), m in zip(owned, masks):
            sg.poison(a, m, value)
        last = run()
        seen.append(sg.bits(last))
    assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]), \
        "the result depends on memory outside the views (NaN / 0.0 / 1e30 around them give different bits)"
    return last


def check_seam(route, shape, boundary, gpu):
    from cp_pre_amd import losses
    x, g = seam_inputs(route, shape, boundary)
    want = ref_vjp(route, x.double(), g.double(), boundary)
    gd = g.to(gpu)
    dense = losses.residual_vjp(route.method, x.to(gpu), gd, boundary=boundary)
    assert losses.last_route() == "fused:" + route.kind
    assert dense.shape == x.shape
    errs = channel_errs(dense, want)
    print(f"{route.name} {shape} boundary={boundary}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (route.name, shape, boundary, k, v)
    for offset, pitch in VIEWS:
        alloc, xd = place(route, x, gpu, offset, pitch)
        assert xd.stride(-2) > xd.shape[-1] and xd.stride(-1) == 1
        owned = [(alloc, xd)]
        gv = gd
        if boundary:                                             # g is read where it lies: a pitched view of its own
            galloc, gv = sg.embed(g, None, {g.dim() - 2: pitch + 1}, offset, gpu)
            owned.append((galloc, gv))
        got = poisoned_runs(owned, lambda: losses.residual_vjp(route.method, xd, gv, boundary=boundary))
        assert losses.last_route() == "fused:" + route.kind
        assert torch.equal(sg.bits(got), sg.bits(dense)), (route.name, shape, boundary, offset, pitch)


_routes = {}


def route_of(name):
    if name not in _routes:
        _routes[name] = Route(name, asym=True)
    return _routes[name]


CASES = [(n, grp) for n in ROUTES for grp in seam_groups(n)]


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("name,group", CASES, ids=[f"{n}-{g}" for n, g in CASES])
def test_residual_vjp_at_the_seams_against_fp64(gpu, name, group, boundary):
    route = route_of(name)
    if group == "tseg":
        assert route.has_t_taps()
    if group.startswith("tfree"):
        assert not route.has_t_taps()
    for shape in SEAM_SHAPES[group]:
        check_seam(route, shape, boundary, gpu)


# ------------------------------------------------------------------ the losses: many rows, long rows, an upstream factor
def _loss_case(route, x, yy, boundary, gpu, upstream):
    from cp_pre_amd import losses
    v64, g64 = ref_loss(route, x.double(), boundary, None if yy is None else yy.double(), upstream)
    xd = x.to(gpu).requires_grad_(True)
    loss = losses.pi_loss(route.method, xd, boundary=boundary) if yy is None else \
        losses.pisl_loss(route.method, xd, yy.to(gpu), boundary=boundary)
    assert losses.last_route() == "fused:" + route.kind and loss.dim() == 0 and loss.dtype == torch.float32
    (upstream * loss).backward()
    ev = abs(float(loss.detach()) - v64) / abs(v64)
    errs = channel_errs(xd.grad, g64)
    print(f"{'pi' if yy is None else 'pisl'} {route.name} {tuple(x.shape)} boundary={boundary}: loss {float(loss.detach()):.6e} "
          f"(fp64 {v64:.6e}, rel {ev:.2e}), gradient " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert ev <= TOL
    for k, v in errs.items():
        assert v <= TOL, (route.name, tuple(x.shape), boundary, k, v)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["8960rows-300cols", "8400rows-13cols"])
@pytest.mark.parametrize("name", ["ns_momentum", "ns_continuity", "burgers", "wave", "advection"])
def test_pi_and_pisl_loss_past_the_sumsq_grid_against_fp64(gpu, name, shape):
    """rows = BS*Nt*Nx > 4 * PRE_VJP_SUMSQ_WORKSPACE (the grid-stride loop of ``sumsq_partial_kernel``), Ny > 256 (its inner
    loop); 2-D routes see (BS*Nt, Nx, Ny): fewer, longer rows - the same two kernels"""
    from cp_pre_amd import _lib
    route = route_of(name)
    assert shape[0] * shape[1] * shape[2] > 4 * _lib.PRE_VJP_SUMSQ_WORKSPACE
    x, _ = seam_inputs(route, shape, True, seed=2)
    yy = x + 0.1 * torch.rand(x.shape, generator=torch.Generator().manual_seed(3))
    for boundary in (False, True):
        _loss_case(route, x, None, boundary, gpu, 1000.0)
        _loss_case(route, x, yy, boundary, gpu, 1000.0)


@pytest.mark.parametrize("name", ["ns_momentum", "wave", "burgers"])
def test_loss_upstream_factor_at_a_seam_shape(gpu, name):
    """``lp + 1000 * PISL`` at a shape with a t seam and an x seam: the device-resident upstream factor reaches every segment"""
    from cp_pre_amd import losses
    route = route_of(name)
    x, _ = seam_inputs(route, (2, 17, 33, 16), True, seed=4)
    yy = x + 0.1 * torch.rand(x.shape, generator=torch.Generator().manual_seed(5))
    for boundary in (False, True):
        _loss_case(route, x, yy, boundary, gpu, 1000.0)
        _loss_case(route, x, None, boundary, gpu, 1.0)
        # and in the sum the reference's scripts form
        _, g64 = ref_loss(route, x.double(), boundary, yy.double(), 1000.0)
        xd = x.to(gpu).requires_grad_(True)
        (xd.pow(2).mean() + 1000 * losses.pisl_loss(route.method, xd, yy.to(gpu), boundary=boundary)).backward()
        want = g64 + 2 * x.double() / x.numel()
        for k, v in channel_errs(xd.grad, want).items():
            assert v <= TOL, (name, boundary, k, v)


def sumsq(r4, flags, gpu):
    """``pre_vjp_sumsq_f32`` on the view ``r4`` [B,T,X,Y] where it lies -> the float64 sum as a 1-element device tensor"""
    from cp_pre_amd import _lib
    ws = torch.zeros(_lib.PRE_VJP_SUMSQ_WORKSPACE + 1, dtype=torch.float64, device=gpu)
    _lib.check(_lib.load_vjp().pre_vjp_sumsq_f32(ctypes.byref(_lib.field(r4)), *r4.shape, flags, _lib.ptr(ws),
                                                 ctypes.c_void_p(ws.data_ptr() + 8 * _lib.PRE_VJP_SUMSQ_WORKSPACE), _lib.stream()),
               "pre_vjp_sumsq_f32")
    torch.cuda.synchronize()
    return ws[-1:].clone()


@pytest.mark.parametrize("shape,view3d", [((4, 16, 140, 300), False), ((3, 7, 400, 13), False), ((1, 21, 400, 13), True),
                                          ((2, 3, 1400, 257), False)])
def test_sumsq_of_a_pitched_view_past_the_grid(gpu, shape, view3d):
    """the loss allocates r itself, dense: a pitched r (sX != Y, planes and samples apart, base 4 bytes off) goes through the
    entry directly.  fp64 accumulation of fp32 squares: N * 2^-53 relative at the very worst (N = 2.7e6: 3e-10)"""
    from cp_pre_amd import _lib
    gen = torch.Generator().manual_seed(sum(shape))
    r = torch.randn(shape, generator=gen)
    dense = r.to(gpu)
    alloc, view = sg.embed(r, None, {2: 12, 1: 40, 0: 100}, 1, gpu)
    assert view.stride(2) != view.shape[3]
    for crop in (False, True):
        flags = (_lib.PRE_VJP_CROP if crop else 0) | (_lib.PRE_VJP_VIEW3D if view3d else 0)
        m = r.double()
        if crop:
            m = m[:, :, 1:-1, 1:-1] if view3d else m[:, 1:-1, 1:-1, 1:-1]
        want = float(m.pow(2).sum())
        got = sg.three_ways(alloc, [view], lambda: sumsq(view, flags, gpu))
        d = sumsq(dense, flags, gpu)
        print(f"sumsq {shape} crop={crop}: {float(got):.15e} (fp64 {want:.15e})")
        assert torch.equal(sg.bits(got), sg.bits(d)), "a pitched view sums to other bits than the dense tensor"
        assert abs(float(got) - want) <= 1e-9 * want
