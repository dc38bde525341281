"""GPU tests (pytest -m gpu) of where the marched residual kernels write their result and of the planes they request
ahead.  The store is a plain 16-byte store through a 64-bit pointer; the experiment build MARCH_ST_SC1 (star_march.h)
replaces it by a write-through buffer store through a descriptor of the output plane and a 32-bit offset wherever the
host finds that the offset fits (tests/test_march_store_checks_cpu.py has that check at both sides of 2^32).  These tests
hold for either build.  NS momentum in the reference's tap structure requests a plane's halo rows and edge scalars two
planes ahead into one of three halo sets (MARCH_HALO_AHEAD): marches of 1, 2, 3, 5 and 13 planes pass every phase of the
three sets against the four-plane window, and marches shorter than the lead.

Every output view lies in a larger NaN-filled allocation the test owns: the result matches the float64 CPU oracle within
the suite's tensor-scale 1e-5, and every float of the allocation outside the view is still NaN.  The shapes are the smallest
at which the store path can go wrong: 520 columns = two column tiles, the second partial; 19 rows = two whole row tiles of
8 and a partial third; 515 columns = the marched kernel and the generic kernel for the last three columns meet in every
row; [2,F,16,24,10] Nt-fastest = the merged-row (flat) form.  The last test hands the same `out` to two launches with a
moments pass after each: what the second pass reads is what the second launch wrote."""
import numpy as np
import pytest
import torch

import stencil_guards as sg
from conftest import rel_err

pytestmark = pytest.mark.gpu

RES_TOL = 1e-5
DT, NU = 0.01, 1e-3
B, T, X, Y = 2, 6, 19, 520


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ns_case(gpu):
    """NS momentum on [2,3,6,21,520]: the fields on the GPU, and the oracle's residual of the whole grid (computed once,
    never written to) and of rows 1..19 as an x-slab with real halo rows."""
    from cp_pre_amd.residuals import NavierStokes
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(520)
    v = torch.rand(B, 3, T, X + 2, Y, generator=g) + 0.5
    dx, dy = 1.0 / X, 1.0 / Y
    whole = orr.ns_momentum(v[:, :, :, 1:-1].contiguous(), DT, dx, dy, nu=NU, boundary=True).numpy()
    slab = orr.ns_momentum(v, DT, dx, dy, nu=NU, boundary=True).numpy()[:, :, 1:-1]
    whole.setflags(write=False)
    slab.setflags(write=False)
    return NavierStokes(DT, dx, dy, nu=NU), v.to(gpu), whole, slab


def _nan_out(shape, order=None, gaps=None, offset=0, device=None):
    """(allocation, view, mask of the allocation outside the view): everything NaN"""
    alloc, view = sg.guarded(tuple(shape), order, gaps, offset, device)
    alloc.fill_(float("nan"))
    return alloc, view, sg.outside_mask(alloc, view)


def _still_nan(alloc, mask):
    return bool(torch.isnan(alloc[mask]).all())


# name -> (order, gaps, offset) of the output view [B,T,X,Y] inside its allocation
LAYOUTS = {
    "contiguous": (None, None, 0),
    "samples 64 floats apart": (None, {0: 64}, 0),             # pipeline.row_padded: the marginal score buffer
    "rows 64 floats apart": (None, {2: 64}, 0),                # a pitched row: the x stride is not the width
    "time-major": ((1, 0, 2, 3), {0: 64}, 0),                  # pipeline.time_major(pad=64): memory [T][B][plane + 64]
    "base 4 bytes off": (None, None, 1),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ns_momentum_into_an_owned_output(gpu, ns_case, layout):
    ns, v, whole, _ = ns_case
    order, gaps, offset = LAYOUTS[layout]
    alloc, out, mask = _nan_out((B, T, X, Y), order, gaps, offset, gpu)
    if layout == "base 4 bytes off":
        assert out.data_ptr() % 16 == 4
    got = ns.residual_momentum(v[:, :, :, 1:-1], boundary=True, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert rel_err(got.cpu().numpy(), whole) <= RES_TOL
    assert _still_nan(alloc, mask), "the kernel wrote outside its output view"


def test_the_pipeline_buffers_are_the_layouts_tested(gpu):
    """pipeline.row_padded / time_major hand out the strides two of the layouts above spell out"""
    from cp_pre_amd import pipeline
    rp = pipeline.row_padded(B, (T, X, Y), device=gpu)
    assert rp.stride() == sg.guarded((B, T, X, Y), *LAYOUTS["samples 64 floats apart"][:2])[1].stride()
    tm = pipeline.time_major(B, (T, X, Y), pad=64, device=gpu)
    assert tm.stride() == sg.guarded((B, T, X, Y), *LAYOUTS["time-major"][:2])[1].stride()


@pytest.mark.parametrize("variant", ["absolute", "halo_x", "skip_t_rim", "skip_t_rim interior planes"])
def test_ns_momentum_flags_into_an_owned_output(gpu, ns_case, variant):
    ns, v, whole, slab = ns_case
    inner = v[:, :, :, 1:-1]
    shape = (B, T - 2, X, Y) if variant.endswith("interior planes") else (B, T, X, Y)
    alloc, out, mask = _nan_out(shape, device=gpu)
    if variant == "absolute":
        got, want = ns.residual_momentum(inner, boundary=True, absolute=True, out=out), np.abs(whole)
    elif variant == "halo_x":               # rows 1:-1 of the 21-row tensor: rows 0 and 20 are read, not written
        got, want = ns.residual_momentum(inner, boundary=True, out=out, halo_x=True), slab
    else:                                   # planes 0 and T-1 are neither computed nor stored
        got = ns.residual_momentum(inner, boundary=True, out=out, skip_t_rim=True)
        want = whole[:, 1:-1]
        if shape[1] == T:                   # (the rim planes of a full-size output may or may not be written)
            got = got[:, 1:-1]
    assert rel_err(got.cpu().numpy(), want) <= RES_TOL
    assert _still_nan(alloc, mask), "the kernel wrote outside its output view"


@pytest.mark.parametrize("halo_x", [False, True], ids=["zero padding", "halo_x"])
@pytest.mark.parametrize("planes", [1, 2, 3, 5, 13])
def test_ns_momentum_marches_of_every_halo_phase(gpu, planes, halo_x):
    """[2,3,T,19(+2),260]: three row tiles (the last partial) by two column tiles (the second of one quad), so that halo
    rows come from memory above and below a tile and edge scalars from either side of a wave"""
    from cp_pre_amd.residuals import NavierStokes
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(1000 + planes)
    x, y = 19, 260
    v = torch.rand(2, 3, planes, x + 2, y, generator=g) + 0.5
    ns = NavierStokes(DT, 1.0 / x, 1.0 / y, nu=NU)
    if halo_x:
        want = orr.ns_momentum(v, DT, 1.0 / x, 1.0 / y, nu=NU, boundary=True).numpy()[:, :, 1:-1]
    else:
        want = orr.ns_momentum(v[:, :, :, 1:-1].contiguous(), DT, 1.0 / x, 1.0 / y, nu=NU, boundary=True).numpy()
    alloc, out, mask = _nan_out((2, planes, x, y), device=gpu)
    got = ns.residual_momentum(v.to(gpu)[:, :, :, 1:-1], boundary=True, out=out, halo_x=halo_x)
    assert rel_err(got.cpu().numpy(), want) <= RES_TOL
    assert _still_nan(alloc, mask), "the kernel wrote outside its output view"


def test_a_width_with_tail_columns(gpu):
    """515 columns: the marched kernel writes columns 0..511 of a row, the generic kernel 512..514"""
    from cp_pre_amd import _dispatch
    from oracle.cstencil import xcorr_c
    g = torch.Generator().manual_seed(515)
    x = torch.randn(2, 6, 19, 515, generator=g)
    star = torch.zeros(3, 3, 3)
    for i, idx in enumerate([(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]):
        star[idx] = 0.3 * (i + 1) * (-1) ** i
    want = xcorr_c(x.numpy(), star.numpy())
    xd = x.to(gpu)
    for flags in (0, 1):
        alloc, out, mask = _nan_out(tuple(x.shape), device=gpu)
        got = _dispatch._xcorr_impl(xd, star, 3, flags, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert rel_err(got.cpu().numpy(), np.abs(want) if flags else want) <= RES_TOL, flags
        assert _still_nan(alloc, mask), "a kernel wrote outside the output view"


@pytest.mark.parametrize("eq", ["ns_momentum", "mhd_induction"])
def test_flat_form_into_an_owned_output(gpu, eq):
    """[2,F,16,24,10].permute(0,1,4,2,3): Nt = 10 fastest, the merged-row march"""
    from cp_pre_amd import residuals as R
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(10)
    F = 3 if eq == "ns_momentum" else 6
    mem = torch.rand(2, F, 16, 24, 10, generator=g) + 0.5
    v = mem.permute(0, 1, 4, 2, 3)                                          # logical [B,F,Nt,Nx,Ny]
    if eq == "ns_momentum":
        fn = R.NavierStokes(DT, 1 / 16, 1 / 24, nu=NU).residual_momentum
        want = orr.ns_momentum(v.contiguous(), DT, 1 / 16, 1 / 24, nu=NU, boundary=True).numpy()
    else:
        fn = R.MHD().residual_induction
        want = orr.mhd_induction(v.contiguous(), boundary=True).numpy()
    vd = mem.to(gpu).permute(0, 1, 4, 2, 3)
    for absolute in (False, True):
        alloc, out, mask = _nan_out((2, 10, 16, 24), order=(0, 2, 3, 1), device=gpu)      # laid out like the fields
        got = fn(vd, boundary=True, absolute=absolute, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert rel_err(got.cpu().numpy(), np.abs(want) if absolute else want) <= RES_TOL, absolute
        assert _still_nan(alloc, mask), "the kernel wrote outside its output view"


def test_the_moments_pass_reads_what_the_last_launch_wrote(gpu):
    """inputs A -> out -> moments, inputs B -> the SAME out -> moments: the second modulation is bit for bit the one from a
    fresh buffer.  [300,6,16,256] takes the pruned route where the slab allows it, and the plain one is run as well."""
    from cp_pre_amd import pipeline
    from cp_pre_amd.residuals import NavierStokes
    n, t, x, y = 300, 6, 16, 256
    g = torch.Generator(device=gpu).manual_seed(300)
    va = torch.rand(n, 3, t, x, y, device=gpu, generator=g) + 0.5
    vb = torch.rand(n, 3, t, x, y, device=gpu, generator=g) * 3.0 + 0.25
    ns = NavierStokes(DT, 1.0 / x, 1.0 / y, nu=NU)
    for prune in ("always", False):
        out = torch.empty(n, t, x, y, device=gpu)
        mods = []
        for v in (va, vb):
            ns.residual_momentum(v, boundary=True, out=out)
            jc = pipeline.JointCalibration(n, gpu, prune=prune)
            mods.append((jc.add_slab(out).clone(), jc.scores.clone()))
        fresh = torch.empty(n, t, x, y, device=gpu)
        ns.residual_momentum(vb, boundary=True, out=fresh)
        jc = pipeline.JointCalibration(n, gpu, prune=prune)
        mod, scores = jc.add_slab(fresh), jc.scores
        assert torch.equal(sg.bits(mods[1][0]), sg.bits(mod)) and torch.equal(sg.bits(mods[1][1]), sg.bits(scores)), prune
        assert not torch.equal(sg.bits(mods[0][0]), sg.bits(mod)), "the two inputs must differ for the test to say anything"
