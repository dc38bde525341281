"""GPU guard-band tests (pytest -m gpu): an output depends on the cells of the view, the zero / boundary padding and the
operator's current kernel - and on nothing else.

Every input view lies inside a larger allocation the test owns (tests/stencil_guards.py); each case runs three times on
the same allocation and views with NaN, 0.0 and 1e30 around the view.  (a) the three results are bit-identical, (b) they
match the float64 oracle of the dense copy of the view within RES_TOL, (c) every bit of the output allocation outside
the output view is untouched.  The cases reuse the shape and tap-set families of the route tests in test_gpu_parity.py /
test_gpu_fuzz.py so that each lands on a named kernel (star march, row march, accumulator march, tiled / flat tap list,
generic strided, paired, ODE, spatial)."""
import ctypes

import numpy as np
import pytest
import torch

import stencil_guards as sg
from conftest import rel_err

pytestmark = pytest.mark.gpu

RES_TOL = 1e-5


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ tap sets
def _kernels():
    from cp_pre_amd.convops_1d import ConvOperator as C1
    from cp_pre_amd.convops_2d import ConvOperator as C2
    g = torch.Generator().manual_seed(41)
    star = torch.zeros(3, 3, 3)
    for i, idx in enumerate([(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]):
        star[idx] = 0.3 * (i + 1) * (-1) ** i
    lap4 = C2(("x", "y"), 2, taylor_order=4).kernel
    k5 = torch.zeros(5, 5, 5)
    k5[1:4, 1:4, 1:4] = C2("t", 2).kernel
    two = torch.zeros(5, 5, 5)
    two[0, 1:4, 1:4] = torch.randn(3, 3, generator=g)
    two[3, 0:5, 0:5] = torch.randn(5, 5, generator=g)
    corners = torch.zeros(3, 3, 3)
    corners[0, 2, 0], corners[2, 0, 2] = 2.0, -3.0
    return {"star": star, "lap": C2(("x", "y"), 2).kernel, "dt": C2("t", 2).kernel, "dx": C2("x", 1).kernel,
            "lap4": lap4, "lap6": C2(("x", "y"), 2, taylor_order=6).kernel,                  # one plane: row march
            "wave4": k5 - 0.25 * lap4, "dense3": torch.randn(3, 3, 3, generator=g), "corners": corners,      # three planes
            "two_planes": two, "dense5": torch.randn(5, 5, 5, generator=g),
            "dense7": torch.randn(7, 7, 7, generator=g) * (torch.rand(7, 7, 7, generator=g) < 0.2),
            "d1_x": C1("x", 2).kernel, "d1_dense3": torch.randn(3, 3, generator=g), "d1_dense5": torch.randn(5, 5, generator=g)}


KERNELS = None


def _k(name):
    global KERNELS
    if KERNELS is None:
        KERNELS = _kernels()
    return KERNELS[name]


def _stencil_out(view, k, nd=3, flags=0, gaps=None):
    """``pre_stencil{3,2}d_f32`` as ``ConvOperator.__call__`` reaches it, into an output view the test owns (laid out like the
    input); (c) is asserted here."""
    from cp_pre_amd import _dispatch
    o_alloc, o_view, o_mask = sg.guarded_out(tuple(view.shape), sg.memory_order(view), gaps, device=view.device)
    got = _dispatch._xcorr_impl(view, k, nd, flags, out=o_view)
    assert got.data_ptr() == o_view.data_ptr()
    assert sg.untouched(o_alloc, o_mask), "the kernel wrote outside its output view"
    return got


def _check_stencil(gpu, x, kname, order=None, gaps=None, offset=0, nd=3, flags=0, tag=None):
    from oracle.cstencil import xcorr_c
    k = _k(kname)
    alloc, view = sg.embed(x, order, gaps, offset, gpu)
    got = sg.three_ways(alloc, [view], lambda: _stencil_out(view, k, nd, flags, gaps))
    want = xcorr_c(x.numpy(), k.numpy())
    assert rel_err(got.cpu().numpy(), np.abs(want) if flags & 1 else want) <= RES_TOL, (tag, kname, tuple(x.shape))


ROUTES = [
    # the streaming star march: whole quads, and widths that leave <= 3 tail columns to the generic kernel
    ("star", (2, 5, 16, 64)), ("star", (1, 1, 8, 256)), ("star", (1, 9, 11, 260)), ("star", (1, 3, 7, 1028)),
    ("star", (2, 4, 9, 101)), ("lap", (2, 2, 33, 510)), ("dt", (1, 3, 20, 1030)), ("lap", (3, 5, 6, 5)), ("dx", (1, 17, 9, 66)),
    # one input plane per output plane: the register-window row march
    ("lap4", (2, 3, 20, 64)), ("lap6", (1, 4, 3, 128)), ("lap4", (2, 2, 70, 260)), ("lap6", (1, 3, 150, 72)),
    # two and three planes: the accumulator march (and its tiled fall-back where the width is not a multiple of 4)
    ("wave4", (2, 7, 19, 64)), ("dense3", (1, 40, 9, 320)), ("corners", (2, 1, 12, 128)), ("dense3", (1, 2, 1, 68)),
    ("two_planes", (2, 3, 20, 64)), ("two_planes", (1, 4, 7, 128)), ("wave4", (1, 2, 30, 516)),
    # the LDS-tiled tap-list kernel: dense 5^3 / 7^3, widths off the quad and off the tile
    ("dense5", (2, 3, 20, 64)), ("dense5", (1, 5, 37, 130)), ("dense7", (2, 2, 16, 259)), ("dense7", (1, 9, 5, 515)),
    # the generic strided kernel: small views
    ("dense3", (1, 1, 1, 4)), ("lap", (2, 1, 1, 1)), ("dt", (1, 3, 1, 8)), ("lap", (1, 2, 5, 1)), ("dense5", (2, 3, 4, 7)),
]


@pytest.mark.parametrize("kname,shape", ROUTES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in ROUTES])
def test_stencil3d_routes_in_a_poisoned_allocation(gpu, kname, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    _check_stencil(gpu, x, kname)
    _check_stencil(gpu, x, kname, flags=1, tag="abs")


@pytest.mark.parametrize("kname", ["star", "lap4", "dense3", "dense5"])
def test_stencil3d_layouts_in_a_poisoned_allocation(gpu, kname):
    """Pitched rows / planes / samples (gaps that hold poison), a base 4 bytes off a 16-byte boundary, the surrogate's
    Nt-fastest layout (long and short Nt: tiled and flat tap-list forms), an Nx-fastest view, a view with no unit stride."""
    g = torch.Generator().manual_seed(len(kname))
    x = torch.randn(2, 4, 18, 64, generator=g)
    _check_stencil(gpu, x, kname, gaps={2: 8}, tag="row pitch")
    _check_stencil(gpu, x, kname, gaps={1: 64 * 3 + 4, 0: 12}, tag="plane and sample pitch")
    _check_stencil(gpu, x, kname, gaps={2: 5}, offset=1, tag="odd pitch, base 4 bytes off")
    _check_stencil(gpu, x, kname, offset=1, tag="base 4 bytes off")
    _check_stencil(gpu, x, kname, gaps={3: 1}, tag="no unit stride")
    for nt in (10, 12, 30, 72):                                           # [BS,Nx,Ny,Nt] memory, [BS,Nt,Nx,Ny] view
        xs = torch.randn(2, nt, 9, 14, generator=g)
        _check_stencil(gpu, xs, kname, order=(0, 2, 3, 1), tag=f"Nt fastest, Nt = {nt}")
    xs = torch.randn(2, 5, 64, 12, generator=g)
    _check_stencil(gpu, xs, kname, order=(0, 1, 3, 2), tag="Nx fastest")
    _check_stencil(gpu, xs, kname, order=(0, 1, 3, 2), gaps={3: 4}, tag="Nx fastest, pitched")


@pytest.mark.parametrize("kname", ["star", "lap4", "dense3"])
def test_stencil3d_field_slices_slabs_and_crops(gpu, kname):
    """``vars[:, i]`` (the neighbouring fields hold the poison), an x-slab without ``halo_x`` (the rows next to it hold the
    poison and must read as zero padding), and a cropped ``[..., 1:-1]`` view (poison in the cropped cells, base 4 bytes off)."""
    from oracle.cstencil import xcorr_c
    k = _k(kname)
    g = torch.Generator().manual_seed(7)
    for Y in (64, 66):
        v = torch.randn(2, 3, 4, 12, Y, generator=g)
        alloc, vars_ = sg.embed(v, device=gpu)
        for view, dense in ((vars_[:, 1], v[:, 1]), (vars_[:, 1, :, 3:9], v[:, 1, :, 3:9]), (vars_[:, 2, ..., 1:-1], v[:, 2, ..., 1:-1]),
                            (vars_[:, 0, 1:-1, 1:-1, 1:-1], v[:, 0, 1:-1, 1:-1, 1:-1])):
            vars_.copy_(v)                                                # (the poison of the last view lies in this one's cells)
            got = sg.three_ways(alloc, [view], lambda: _stencil_out(view, k))
            assert rel_err(got.cpu().numpy(), xcorr_c(dense.contiguous().numpy(), k.numpy())) <= RES_TOL, (kname, Y, tuple(view.shape))


@pytest.mark.parametrize("Y", [64, 128])
def test_stencil3d_x_slab_with_halo_rows(gpu, Y):
    """PRE_FLAG_HALO_X: rows -1 and X of the slab belong to the input, the guard starts beyond them; the result is the
    whole-rows oracle of the slab with its two halo rows, on the slab's rows."""
    from cp_pre_amd import _lib
    from oracle.cstencil import xcorr_c
    k = _k("star")
    g = torch.Generator().manual_seed(Y)
    v = torch.randn(2, 5, 14, Y, generator=g)
    alloc, whole = sg.embed(v, device=gpu)
    for x0, x1 in ((1, 9), (4, 13), (6, 7)):
        slab = whole[:, :, x0:x1]
        whole.copy_(v)                                                    # (the poison of the last slab lies in this one's rows)
        got = sg.three_ways(alloc, [whole[:, :, x0 - 1:x1 + 1]], lambda: _stencil_out(slab, k, flags=_lib.PRE_FLAG_HALO_X))
        want = xcorr_c(v[:, :, x0 - 1:x1 + 1].contiguous().numpy(), k.numpy())[:, :, 1:-1]
        assert rel_err(got.cpu().numpy(), want) <= RES_TOL, (x0, x1)


@pytest.mark.parametrize("T", [1, 2, 3, 8, 9])
@pytest.mark.parametrize("Y", [1, 3, 4, 5, 64, 260])
def test_stencil3d_tensor_edges(gpu, T, Y):
    """B = 1; T around the 8-plane segment of the tap-free star; X = 1, a row count that ends on a tile edge (8, 16) and one
    past it; Y from one cell to several quads with and without tail columns."""
    g = torch.Generator().manual_seed(100 * T + Y)
    for X in (1, 8, 9, 16):
        x = torch.randn(1, T, X, Y, generator=g)
        for kname in ("star", "dense3", "lap4"):
            _check_stencil(gpu, x, kname, tag="edges")


def test_stencil2d_routes_in_a_poisoned_allocation(gpu):
    """``pre_stencil2d_f32`` ([BS,Nt,Nx] fields, the 1-D operators): reference order, the surrogate's [BS,Nx,Nt] memory,
    pitched rows, a misaligned base, tiny extents."""
    g = torch.Generator().manual_seed(2)
    for shape in [(3, 9, 64), (2, 100, 200), (1, 1, 5), (4, 1, 1), (2, 7, 1), (3, 20, 130), (2, 33, 66)]:
        x = torch.randn(*shape, generator=g)
        for kname in ("d1_x", "d1_dense3", "d1_dense5"):
            _check_stencil(gpu, x, kname, nd=2)
            _check_stencil(gpu, x, kname, nd=2, gaps={1: 4}, tag="row pitch")
            _check_stencil(gpu, x, kname, nd=2, offset=1, flags=1, tag="base 4 bytes off, abs")
            _check_stencil(gpu, x, kname, nd=2, order=(0, 2, 1), tag="Nt fastest")


# ------------------------------------------------------------------------------------------------ fused residuals
def _vars(g, B, F, T, X, Y):
    return torch.rand(B, F, T, X, Y, generator=g) + 0.5


def _out_like(view4, interior_t=False):
    shape = list(view4.shape)
    if interior_t:
        shape[1] -= 2
    return sg.guarded_out(tuple(shape), None, None, device=view4.device)


@pytest.mark.parametrize("shape", [(2, 5, 10, 64), (1, 9, 16, 128), (2, 3, 7, 66), (1, 4, 9, 36)])
def test_ns_residuals_in_a_poisoned_allocation(gpu, shape):
    """NS momentum through its class into an owned output (full planes, ``skip_t_rim`` with a full-size and with an
    interior-planes output, ``halo_x``), and NS continuity (library-allocated output: (a) and (b) through the class, (c)
    through the C entry ``pre_residual_linear2_f32``).  Widths 66 / 36 are not streamable in whole quads."""
    from cp_pre_amd import _dispatch, _lib
    from cp_pre_amd.residuals import NavierStokes
    from oracle import residuals as orr
    B, T, X, Y = shape
    g = torch.Generator().manual_seed(sum(shape))
    v = _vars(g, B, 3, T, X, Y)
    ns = NavierStokes(0.01, 1.0 / X, 1.0 / Y)
    want = orr.ns_momentum(v, 0.01, 1.0 / X, 1.0 / Y, boundary=True).numpy()
    for gaps in (None, {3: 8}):
        alloc, vars_ = sg.embed(v, gaps=gaps, device=gpu)

        def run(absolute=False, **kw):
            o_alloc, o_view, o_mask = _out_like(vars_[:, 0])
            got = ns.residual_momentum(vars_, boundary=True, absolute=absolute, out=o_view, **kw)
            assert sg.untouched(o_alloc, o_mask)
            return got
        got = sg.three_ways(alloc, [vars_], run)
        assert rel_err(got.cpu().numpy(), want) <= RES_TOL
        got = sg.three_ways(alloc, [vars_], lambda: run(absolute=True))
        assert rel_err(got.cpu().numpy(), np.abs(want)) <= RES_TOL
        # continuity
        wc = orr.ns_continuity(v[:, :2], 1.0 / X, 1.0 / Y, boundary=True).numpy()
        got = sg.three_ways(alloc, [vars_], lambda: ns.residual_continuity(vars_[:, :2], boundary=True))
        assert rel_err(got.cpu().numpy(), wc) <= RES_TOL

        def run_c():
            o_alloc, o_view, o_mask = _out_like(vars_[:, 0])
            fa, fb, fo = _lib.field(vars_[:, 0]), _lib.field(vars_[:, 1]), _lib.field(o_view)
            rc = _lib.load().pre_residual_linear2_f32(ctypes.byref(fa), ctypes.byref(fb), ctypes.byref(fo), _dispatch.dense27(ns.D_x.kernel),
                                                      _dispatch.dense27(ns.D_y.kernel), float(ns.dx / ns.dy), B, T, X, Y, 0, _lib.stream())
            if rc == _lib.PRE_E_UNSUPPORTED:
                return None
            _lib.check(rc, "pre_residual_linear2_f32")
            assert sg.untouched(o_alloc, o_mask)
            return o_view
        if run_c() is not None:
            got = sg.three_ways(alloc, [vars_], run_c)
            assert rel_err(got.cpu().numpy(), wc) <= RES_TOL
    if Y % 4 == 0 and T >= 3:
        # the skipped t rim: rim planes of a full-size output are inside the view and exempt; an interior-planes output
        alloc, vars_ = sg.embed(v, device=gpu)

        def run_rim(interior):
            o_alloc, o_view, o_mask = _out_like(vars_[:, 0], interior_t=interior)
            got = ns.residual_momentum(vars_, boundary=True, out=o_view, skip_t_rim=True)
            assert sg.untouched(o_alloc, o_mask)
            return got if interior else got[:, 1:-1]
        for interior in (False, True):
            got = sg.three_ways(alloc, [vars_], lambda: run_rim(interior))
            assert rel_err(got.cpu().numpy(), want[:, 1:-1]) <= RES_TOL, interior
        # an x-slab with its halo rows: the guard starts beyond rows x0 - 1 and x1
        x0, x1 = 2, X - 1

        def run_halo():
            o_alloc, o_view, o_mask = _out_like(vars_[:, 0, :, x0:x1])
            got = ns.residual_momentum(vars_[:, :, :, x0:x1], boundary=True, out=o_view, halo_x=True)
            assert sg.untouched(o_alloc, o_mask)
            return got
        got = sg.three_ways(alloc, [vars_[:, :, :, x0 - 1:x1 + 1]], run_halo)
        wh = orr.ns_momentum(v[:, :, :, x0 - 1:x1 + 1], 0.01, 1.0 / X, 1.0 / Y, boundary=True).numpy()[:, :, 1:-1]
        assert rel_err(got.cpu().numpy(), wh) <= RES_TOL


@pytest.mark.parametrize("eq", ["continuity", "momentum", "energy", "induction", "gauss"])
def test_mhd_residuals_in_a_poisoned_allocation(gpu, eq):
    """The five MHD equations through their class: an owned output where the method takes ``out=`` (all but gauss), in the
    reference layout (whole quads, a width with tail columns, pitched rows) and the surrogate's Nt-fastest layout."""
    from cp_pre_amd.residuals import MHD
    from oracle import residuals as orr
    mhd = MHD()
    fn, ref = getattr(mhd, "residual_" + eq), getattr(orr, "mhd_" + eq)
    g = torch.Generator().manual_seed(len(eq))
    for shape, order, gaps in (((2, 6, 5, 10, 64), None, None), ((1, 6, 3, 9, 66), None, None), ((2, 6, 4, 7, 128), None, {4: 4}),
                               ((2, 6, 10, 9, 16), (0, 1, 3, 4, 2), None), ((1, 6, 1, 1, 4), None, None)):
        v = _vars(g, *shape)
        want = ref(v, boundary=True).numpy()
        alloc, vars_ = sg.embed(v, order, gaps, device=gpu)
        for absolute in (False, True):
            def run():
                if eq == "gauss":
                    return fn(vars_, True, absolute=absolute)
                o_alloc, o_view, o_mask = sg.guarded_out(tuple(vars_[:, 0].shape), sg.memory_order(vars_[:, 0]), device=gpu)
                try:
                    got = fn(vars_, True, absolute=absolute, out=o_view)
                except RuntimeError as e:                                 # no streaming form for this view: out= is refused,
                    assert "out need views" in str(e), e                  # never written partly; the class allocates instead
                    assert sg.untouched(o_alloc, sg.outside_mask(o_alloc))
                    return fn(vars_, True, absolute=absolute)
                assert got.data_ptr() == o_view.data_ptr() and sg.untouched(o_alloc, o_mask)
                return got
            got = sg.three_ways(alloc, [vars_], run)
            assert rel_err(got.cpu().numpy(), np.abs(want) if absolute else want) <= RES_TOL, (eq, shape, absolute)
    # an x-slab with its halo rows (every equation that takes halo_x)
    if eq != "gauss":
        v = _vars(g, 2, 6, 4, 12, 64)
        alloc, vars_ = sg.embed(v, device=gpu)
        got = sg.three_ways(alloc, [vars_[:, :, :, 2:10]], lambda: fn(vars_[:, :, :, 3:9], True, halo_x=True))
        assert rel_err(got.cpu().numpy(), ref(v[:, :, :, 2:10], boundary=True).numpy()[:, :, 1:-1]) <= RES_TOL, eq


def test_wave_burgers_jorek_in_a_poisoned_allocation(gpu, monkeypatch):
    """``linear2`` / the wave's additive kernel (owned output), Burgers 1-D ((a), (b) through the class, (c) through
    ``pre_residual_burgers_f32``) and the two JOREK equations on the script's layout ((a), (b) through the class; (c) with the
    class's output allocation replaced by a view the test owns)."""
    from cp_pre_amd import _dispatch, _lib
    from cp_pre_amd import residuals as R
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(19)
    wv = R.PRE_Wave(0.01, 0.02)
    for shape, order, gaps in (((2, 5, 12, 64), None, None), ((1, 9, 7, 66), None, {2: 2}), ((2, 10, 9, 16), (0, 2, 3, 1), None)):
        u = torch.randn(*shape, generator=g)
        want = orr.wave_residual(u, 1.0, 0.01, 0.02, boundary=True).numpy()
        alloc, view = sg.embed(u, order, gaps, device=gpu)

        def run():
            o_alloc, o_view, o_mask = sg.guarded_out(tuple(shape), sg.memory_order(view), device=gpu)
            got = wv.residual(view, boundary=True, out=o_view)
            assert got.data_ptr() == o_view.data_ptr() and sg.untouched(o_alloc, o_mask)
            return got
        got = sg.three_ways(alloc, [view], run)
        assert rel_err(got.cpu().numpy(), want) <= RES_TOL, shape
    bu = R.Burgers(0.05, 0.01, 0.002)
    for shape, order, gaps in (((3, 9, 64), None, None), ((2, 40, 130), None, {1: 2}), ((4, 10, 36), (0, 2, 1), None), ((1, 1, 1), None, None)):
        u = torch.rand(*shape, generator=g) + 0.5
        want = orr.burgers_residual(u, 0.05, 0.01, 0.002, boundary=True).numpy()
        alloc, view = sg.embed(u, order, gaps, device=gpu)
        got = sg.three_ways(alloc, [view], lambda: bu.residual(view, boundary=True))
        assert rel_err(got.cpu().numpy(), want) <= RES_TOL, shape
        ks = [_dispatch.dense9(o.kernel) for o in (bu.D_t, bu.D_x, bu.D_xx)]

        def run_c():
            o_alloc, o_view, o_mask = sg.guarded_out(tuple(shape), sg.memory_order(view), device=gpu)
            rc = _lib.load().pre_residual_burgers_f32(_lib.ptr(view), _lib.iarr64(view.stride()), _lib.ptr(o_view), _lib.iarr64(o_view.stride()),
                                                      *ks, float(bu.dx), float(bu.dt), float(bu.nu), float(2 * bu.dt / bu.dx), *shape, 0,
                                                      _lib.stream())
            if rc == _lib.PRE_E_UNSUPPORTED:                              # (the class then composes single-operator passes)
                assert sg.untouched(o_alloc, sg.outside_mask(o_alloc))
                return None
            _lib.check(rc, "pre_residual_burgers_f32")
            assert sg.untouched(o_alloc, o_mask)
            return o_view
        if run_c() is not None:
            got = sg.three_ways(alloc, [view], run_c)
            assert rel_err(got.cpu().numpy(), want) <= RES_TOL, shape
    for (B, N, Nt) in ((2, 16, 10), (1, 40, 24)):
        v3 = torch.rand(B, 3, N, N, Nt, generator=g) + 0.5                 # the script's [BS,F,Nx,Ny,Nt]
        Rg = torch.linspace(1.0, 2.0, N)
        jo = R.JOREK(Rg, dx=0.1, dy=0.1, dt=0.02)
        alloc, d3 = sg.embed(v3, device=gpu)
        # (c): the class takes no out=; its output comes from _lib.empty_like_layout, which hands out a view the test owns
        owned = []

        def owned_like(t, score_rows=False):
            o_alloc, o_view, o_mask = sg.guarded_out(tuple(t.shape), sg.memory_order(t), device=gpu)
            owned.append((o_alloc, o_mask))
            return o_view
        monkeypatch.setattr(_lib, "empty_like_layout", owned_like)
        for fn in (jo.residual_continuity, jo.residual_temperature):
            fn(d3, True)
        assert len(owned) == 2 and all(sg.untouched(a, m) for a, m in owned), "pre_residual_jorek_f32 wrote outside its output view"
        monkeypatch.undo()
        got = sg.three_ways(alloc, [d3], lambda: jo.residual_continuity(d3, True))
        assert rel_err(got.cpu().numpy(), orr.jorek_continuity(v3, Rg, 3.4, boundary=True).numpy()) <= RES_TOL
        got = sg.three_ways(alloc, [d3], lambda: jo.residual_temperature(d3, True))
        assert rel_err(got.cpu().numpy(), orr.jorek_temperature(v3, Rg, boundary=True).numpy()) <= RES_TOL


def test_paired_entries_in_a_poisoned_allocation(gpu):
    """``minus=`` (libcp_pre_pair.so): both field sets in poisoned allocations of their own; r(a) - r(b) against the two
    float64 oracles, the error scaled by the larger of the two residuals (what the paired pass can resolve)."""
    from cp_pre_amd import _dispatch
    from cp_pre_amd import residuals as R
    from oracle import residuals as orr
    from oracle.cstencil import xcorr_c
    g = torch.Generator().manual_seed(53)

    def both(a, b, run, ra, rb, tag):
        al_a, va = sg.embed(a, device=gpu)
        al_b, vb = sg.embed(b, device=gpu)
        seen = []
        ma, mb = sg.outside_mask(al_a, va), sg.outside_mask(al_b, vb)
        for pa, pb in ((float("nan"), 1e30), (0.0, float("nan")), (1e30, 0.0)):
            sg.poison(al_a, ma, pa)
            sg.poison(al_b, mb, pb)
            got = run(va, vb)
            seen.append(sg.bits(got))
        assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]), tag
        scale = max(np.abs(ra).max(), np.abs(rb).max())
        assert np.abs(got.cpu().numpy().astype(np.float64) - (ra.astype(np.float64) - rb)).max() <= RES_TOL * scale, tag

    for shape in ((2, 5, 10, 64), (1, 3, 9, 66)):
        B, T, X, Y = shape
        a, b = _vars(g, B, 6, T, X, Y), _vars(g, B, 6, T, X, Y)
        ns, mhd, wv = R.NavierStokes(0.01, 0.1, 0.1), R.MHD(), R.PRE_Wave(0.01, 0.02)

        def ns_out(x, m):
            o_alloc, o_view, o_mask = sg.guarded_out(shape, device=gpu)
            got = ns.residual_momentum(x[:, :3], True, minus=m[:, :3], out=o_view)
            assert sg.untouched(o_alloc, o_mask)
            return got
        both(a, b, ns_out, orr.ns_momentum(a[:, :3], 0.01, 0.1, 0.1, boundary=True).numpy(),
             orr.ns_momentum(b[:, :3], 0.01, 0.1, 0.1, boundary=True).numpy(), ("ns momentum", shape))
        both(a, b, lambda x, m: ns.residual_continuity(x[:, :2], True, minus=m[:, :2]),
             orr.ns_continuity(a[:, :2], 0.1, 0.1, boundary=True).numpy(), orr.ns_continuity(b[:, :2], 0.1, 0.1, boundary=True).numpy(),
             ("ns continuity", shape))
        for eq in ("continuity", "momentum", "energy", "induction", "gauss"):
            ref = getattr(orr, "mhd_" + eq)
            both(a, b, lambda x, m: getattr(mhd, "residual_" + eq)(x, True, minus=m), ref(a, boundary=True).numpy(),
                 ref(b, boundary=True).numpy(), (eq, shape))
        both(a, b, lambda x, m: wv.residual(x[:, :1], True, minus=m[:, :1]), orr.wave_residual(a[:, 0], 1.0, 0.01, 0.02, boundary=True).numpy(),
             orr.wave_residual(b[:, 0], 1.0, 0.01, 0.02, boundary=True).numpy(), ("wave", shape))
        k = _k("star")
        both(a[:, 0], b[:, 0], lambda x, m: _dispatch.xcorr_pair(x, m, k, 3), xcorr_c(a[:, 0].contiguous().numpy(), k.numpy()),
             xcorr_c(b[:, 0].contiguous().numpy(), k.numpy()), ("pair stencil3d", shape))
    bu = R.Burgers(0.05, 0.01, 0.002)
    a, b = torch.rand(3, 9, 64, generator=g) + 0.5, torch.rand(3, 9, 64, generator=g) + 0.5
    both(a, b, lambda x, m: bu.residual(x, True, minus=m), orr.burgers_residual(a, 0.05, 0.01, 0.002, boundary=True).numpy(),
         orr.burgers_residual(b, 0.05, 0.01, 0.002, boundary=True).numpy(), "burgers")
    k2 = _k("d1_x")
    both(a, b, lambda x, m: _dispatch.xcorr_pair(x, m, k2, 2), xcorr_c(a.numpy(), k2.numpy()), xcorr_c(b.numpy(), k2.numpy()), "pair stencil2d")


def test_spatial_family_in_a_poisoned_allocation(gpu):
    """The spatial / boundary-condition family (``pre_spatial2d_bc_f32``, ``pre_spatial2d_linear2_bc_f32``): every operator
    class with every boundary kind on every side in turn and mixed, fields embedded in poisoned allocations; the cells a
    boundary kind supplies come from the view (periodic wrap, mirrored, repeated) or from its value, never from beyond."""
    from cp_pre_amd import _dispatch, _lib
    from cp_pre_amd import vector_convops_spatial as VS
    from oracle import spatial as osp
    g = torch.Generator().manual_seed(61)
    types = ["dirichlet", "neumann", "outflow", "periodic", "symmetric"]
    kinds = {"gradient": VS.Gradient, "laplace": VS.Laplace, "divergence": VS.Divergence, "curl": VS.Curl,
             "vector_gradient": VS.Vector_Gradient}
    sides_all = ("left", "right", "top", "bottom")
    cases = [{s: t for s in sides_all} for t in types] + [dict(zip(sides_all, types[i:] + types[:i])) for i in range(5)]
    for n, sides in enumerate(cases):
        for kind, cls in kinds.items():
            B, X, Y = [(2, 9, 64), (1, 2, 3), (3, 17, 65), (1, 33, 260), (2, 5, 4)][(n + len(kind)) % 5]
            a, b = torch.randn(B, 1, X, Y, generator=g), torch.randn(B, 1, X, Y, generator=g)
            vals = {s: 0.25 * (i + 1) for i, s in enumerate(sides_all)}
            ref = osp.VectorOp(kind, scale=1.5, boundary_cond="periodic")
            ref.types, ref.values = dict(sides), dict(vals)
            op = cls(scale=1.5, boundary_cond="periodic", device=gpu)
            for s in sides:
                op.bc.set_boundary_type(s, sides[s], vals[s])
            al_a, va = sg.embed(a, gaps={2: 4} if n % 2 else None, device=gpu)
            al_b, vb = sg.embed(b, offset=n % 2, device=gpu)
            ma, mb = sg.outside_mask(al_a, va), sg.outside_mask(al_b, vb)
            seen = []
            for p in sg.POISONS:
                sg.poison(al_a, ma, p)
                sg.poison(al_b, mb, p)
                with torch.no_grad():
                    got = op(va, vb) if kind != "laplace" else op(va)
                seen.append(sg.bits(got))
            assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]), (kind, sides)
            want = ref(a, b) if kind != "laplace" else ref(a)
            assert tuple(got.shape) == tuple(want.shape) and rel_err(got.cpu().numpy(), want.numpy()) <= RES_TOL, (kind, sides, (B, X, Y))
            # (c) through the C entries, into output views the test owns: pre_spatial2d_bc_f32 (one operator; VS._fused1 takes
            # the destination) and pre_spatial2d_linear2_bc_f32 (two operators, called as VS._fused2 calls it)
            ops = [op.laplace] if kind == "laplace" else [op.grad_x, op.grad_y]
            st = VS._bc_struct(op.bc)
            o_alloc, o_view, o_mask = sg.guarded_out((B, 1, X, Y), None, {2: 3} if n % 2 else None, n % 2, gpu)
            one = VS._fused1(va, ops[0], op.bc, dst=o_view)
            assert sg.untouched(o_alloc, o_mask), (kind, sides)
            if one is not None:
                w1 = osp.conv_valid(ref.pad(a), ref.lap if kind == "laplace" else ref.gx)
                assert rel_err(one.cpu().numpy(), w1.numpy()) <= RES_TOL, (kind, sides)
            if st is not None and len(ops) == 2:
                o_alloc, o_view, o_mask = sg.guarded_out((B, 1, X, Y), None, {2: 3} if n % 2 else None, n % 2, gpu)
                k0, k1 = _dispatch.dense9(ops[0].kernel), _dispatch.dense9(ops[1].kernel)
                v0, v1 = va[:, 0], vb[:, 0]
                rc = _lib.load().pre_spatial2d_linear2_bc_f32(_lib.ptr(v0), _lib.iarr64(v0.stride()), _lib.ptr(v1), _lib.iarr64(v1.stride()),
                                                              _lib.ptr(o_view), _lib.iarr64(o_view[:, 0].stride()), k0, k1, -0.5,
                                                              ctypes.byref(st), B, X, Y, 0, _lib.stream())
                assert sg.untouched(o_alloc, o_mask), (kind, sides)
                if rc != _lib.PRE_E_UNSUPPORTED:
                    _lib.check(rc, "pre_spatial2d_linear2_bc_f32")
                    w2 = osp.conv_valid(ref.pad(a), ref.gx) - 0.5 * osp.conv_valid(ref.pad(b), ref.gy)
                    assert rel_err(o_view.cpu().numpy(), w2.numpy()) <= RES_TOL, (kind, sides)


def test_ode_entries_in_a_poisoned_allocation(gpu):
    """``pre_ode_stencil_f32`` / ``pre_ode_residual_f32``: [BS,Nt] rows with a pitch, [Nt,BS] memory, owned outputs."""
    import torch.nn.functional as F
    from cp_pre_amd import convops_0d as C0
    from cp_pre_amd import ode
    g = torch.Generator().manual_seed(67)
    taps = [np.array([1.0, -2.0, 1.0], np.float32), np.array([1 / 12, -2 / 3, 0, 2 / 3, -1 / 12], np.float32),
            np.array([1 / 90, -3 / 20, 3 / 2, -49 / 18, 3 / 2, -3 / 20, 1 / 90], np.float32), np.array([2.0], np.float32)]
    for shape, order, gaps in (((6, 40), None, None), ((3, 1), None, None), ((1, 7), None, {0: 5}), ((5, 150), (1, 0), None),
                               ((4, 100), None, {0: 3})):
        x = torch.randn(*shape, generator=g)
        alloc, view = sg.embed(x, order, gaps, device=gpu)
        for t in taps:
            def run():
                o_alloc, o_view, o_mask = sg.guarded_out(shape, order, gaps, device=gpu)
                got = C0.stencil(view, t, out=o_view)
                assert sg.untouched(o_alloc, o_mask)
                return got
            got = sg.three_ways(alloc, [view], run)
            want = F.conv1d(x.double()[:, None], torch.from_numpy(t).double()[None, None], padding=len(t) // 2)[:, 0].numpy()
            assert rel_err(got.cpu().numpy(), want) <= RES_TOL, (shape, len(t))
        sho = ode.SHO(2.0, 0.05)
        k = sho.terms[0][2]

        def run_res():
            o_alloc, o_view, o_mask = sg.guarded_out(shape, order, gaps, device=gpu)
            got = sho.residual([view], out=o_view)
            assert sg.untouched(o_alloc, o_mask)
            return got
        got = sg.three_ways(alloc, [view], run_res)
        want = F.conv1d(x.double()[:, None], torch.from_numpy(np.asarray(k)).double()[None, None], padding=len(k) // 2)[:, 0].numpy()
        assert rel_err(got.cpu().numpy(), want) <= RES_TOL, shape


def test_edge_residual_in_a_poisoned_allocation(gpu):
    """``pre_edge_residual_f32`` through ``NavierStokes.periodic_bc_residual``: the two walls of a field embedded in a
    poisoned allocation."""
    from cp_pre_amd import _lib
    from cp_pre_amd.residuals import NavierStokes
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(71)
    ns = NavierStokes(0.01, 0.1, 0.1)
    for shape, gaps in (((2, 5, 12, 64), None), ((1, 3, 9, 7), {2: 3})):
        u = torch.randn(*shape, generator=g)
        alloc, view = sg.embed(u, gaps=gaps, device=gpu)
        for wall in ("right", "left", "top", "bottom"):
            got = sg.three_ways(alloc, [view], lambda: ns.periodic_bc_residual(view, wall=wall))
            want = orr.periodic_bc_residual(u, 0.1, wall=wall)
            assert rel_err(got.cpu().numpy(), np.asarray(want)) <= RES_TOL, (shape, wall)

            def run_c():                                                  # (c): the C entry into an output the test owns
                o_alloc, o_view, o_mask = sg.guarded_out(tuple(want.shape), device=gpu)
                f = _lib.field(view)
                _lib.check(_lib.load().pre_edge_residual_f32(ctypes.byref(f), ns._WALLS[wall], float(ns.dx), *shape, _lib.ptr(o_view),
                                                             _lib.stream()), "pre_edge_residual_f32")
                assert sg.untouched(o_alloc, o_mask), (shape, wall)
                return o_view
            got = sg.three_ways(alloc, [view], run_c)
            assert rel_err(got.cpu().numpy(), np.asarray(want)) <= RES_TOL, (shape, wall)


def test_row_padded_score_output_pads_stay_clean(gpu):
    """A row-padded |residual| output (rows PAD floats further apart than they are long, as the library allocates score
    matrices): carved from an allocation the test owns, every bit of the pads between its rows and of the band around it is
    untouched after the call; the library-allocated output has the same pitch and values; and the per-cell select over the
    padded rows equals the select over the dense copy."""
    from cp_pre_amd import _lib
    from cp_pre_amd import inductive_cp as icp
    from cp_pre_amd import pipeline
    from cp_pre_amd import residuals as R
    B, T, X, Y = 256, 8, 64, 64
    M = T * X * Y
    g = torch.Generator(device=gpu).manual_seed(5)
    alphas = [0.1, 0.5, 0.9]
    v = torch.rand(B, 6, T, X, Y, device=gpu, generator=g) + 0.5
    ns, mhd, wv = R.NavierStokes(0.01, 1 / X, 1 / Y), R.MHD(), R.PRE_Wave(0.01, 0.02)
    for name, fn in (("ns", lambda **kw: ns.residual_momentum(v[:, :3], True, absolute=True, **kw)),
                     ("induction", lambda **kw: mhd.residual_induction(v, True, absolute=True, **kw)),
                     ("wave", lambda **kw: wv.residual(v[:, 0], True, absolute=True, **kw))):
        o_alloc, o_view, o_mask = sg.guarded_out((B, T, X, Y), None, {0: _lib.PAD}, device=gpu)
        assert o_view.stride(0) == M + _lib.PAD and int(o_mask.sum()) >= (B - 1) * _lib.PAD
        a = fn(out=o_view)
        assert a.data_ptr() == o_view.data_ptr() and sg.untouched(o_alloc, o_mask), name
        lib = fn()                                                        # the library's own allocation: same pitch, same bits
        assert lib.stride(0) == M + _lib.PAD and torch.equal(sg.bits(lib), sg.bits(a)), name
        dense = a.contiguous()
        assert dense.stride(0) == M and not torch.isnan(dense).any()
        want = torch.sort(dense, dim=0).values[[icp.kth_index(B, B, al) for al in alphas]]
        for padded in (a, lib):
            assert torch.equal(pipeline.marginal_qhat(padded, alphas), pipeline.marginal_qhat(dense, alphas)), name
            assert torch.equal(pipeline.marginal_qhat(padded, alphas), want), name
