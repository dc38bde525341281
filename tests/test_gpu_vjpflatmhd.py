"""The fused backward of the ideal-MHD residual losses on Nt-fastest views (``mhd="flat"``, csrc/vjp_flat_mhd.hip) on the
device (pytest -m gpu).

The reference everywhere is fp64 autograd of the composed expressions as ``mhdvjp_helpers.MHDRoute`` restates them (for the
entries called directly: the header's closed forms in fp64, which tests/test_mhdvjp_cpu.py holds against that autograd to
1e-13); the measure is the tensor-scale relative error overall and per gradient channel, the bound TOL = 1e-5
(tests/LOSSES_TESTS.md).  Inputs are ``rand + 0.5``: rho stays away from 0.  The shapes are the seams of
``vjpflat_helpers.SEAM_SHAPES`` - the smallest that cross each seam of the merged-row march - and three degenerate extents;
tests/test_vjpflatmhd_cpu.py shows the same formulas in fp32 on the CPU within TOL / 4 of fp64 at every one.

On the parent commit ``mhd="flat"`` is ``mhd=True``: an Nt-fastest view answers ``fallback:no unit stride on the last axis``,
so every test that asserts a ``fused:flat_*`` route fails there, and the direct-entry tests fail with a missing library."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import stencil_guards as sg
import vjpflatmhd_helpers as fh
from losses_helpers import D, channel_errs, ref_loss, ref_vjp, seam_inputs
from mhdvjp_helpers import pad_g, unread
from test_vjpflatmhd_cpu import built_constants, c_client_command

pytestmark = pytest.mark.gpu
TOL = fh.TOL
_routes, _refs = {}, {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def route_of(eq, opset="default"):
    if (eq, opset) not in _routes:
        _routes[eq, opset] = fh.MHDRoute(eq, opset)
    return _routes[eq, opset]


def case(route, shape, boundary, seed=0):
    """(x, g, the fp64 gradient) of one case: computed once, shared, never written to"""
    key = (route.name, shape, boundary, seed)
    if key not in _refs:
        x, g = seam_inputs(route, shape, boundary, seed)
        _refs[key] = (x, g, ref_vjp(route, x.double(), g.double(), boundary))
    return _refs[key]


def check_grad(route, got, want, what):
    errs = channel_errs(got, want)
    print(f"{route.name} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (route.name, what, k, v)
    for c in unread(route, got.shape[1]):
        assert not bool(got[:, c].any()), (route.name, what, "channel %d is not read: its gradient is exactly zero" % c)


def dense_in_memory_order(got):
    """dense in memory order [BS,F,Nx,Ny,Nt]"""
    return got.permute(0, 1, 3, 4, 2).is_contiguous()


def bands_hold(alloc, mask, value):
    band = alloc[mask]
    return bool(torch.isnan(band).all()) if value != value else bool((band == value).all())


def three_ways(alloc, xv, run):
    """``stencil_guards.three_ways`` that also looks at the bands after each run: nothing was written there"""
    mask = sg.outside_mask(alloc, xv)
    seen, last = [], None
    for value in sg.POISONS:
        sg.poison(alloc, mask, value)
        last = run()
        torch.cuda.synchronize()
        assert bands_hold(alloc, mask, value), "the guard bands around the input were written to"
        seen.append(sg.bits(last))
    assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]), \
        "the result depends on memory outside the view (NaN / 0.0 / 1e30 around it give different bits)"
    return last


# ------------------------------------------------------------------ (1) residual_vjp at the seams
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("opset", fh.OPSETS)
@pytest.mark.parametrize("eq", fh.EQS)
def test_residual_vjp_at_the_seams_against_fp64(gpu, eq, opset, boundary):
    from cp_pre_amd import losses
    route = route_of(eq, opset)
    for shape in fh.GPU_SHAPES:
        x, g, want = case(route, shape, boundary)
        gd = g.to(gpu)
        xd = fh.nt_fastest_exact(x, gpu)
        assert xd.stride(2) == 1 and fh.is_flat_view(xd) == (shape[1] > 1)
        got = losses.residual_vjp(route.method, xd, gd, boundary=boundary, mhd="flat")
        assert losses.last_route() == fh.expected_route(route, xd), (shape, losses.last_route())
        assert got.shape == x.shape and dense_in_memory_order(got)
        if min(shape) > 1:                                         # (an axis of extent 1 may carry any stride)
            assert got.stride() == xd.stride()
        check_grad(route, got, want, f"{shape} boundary={boundary}")
        # the same view inside an allocation of the test's, base 4 bytes off a 16-byte boundary, samples further apart than
        # they are long, NaN / 0 / 1e30 around it: the same bits, the bands as they were
        alloc, xv = fh.nt_fastest_embedded(x, gpu)
        again = three_ways(alloc, xv, lambda: losses.residual_vjp(route.method, xv, gd, boundary=boundary, mhd="flat"))
        assert losses.last_route() == fh.expected_route(route, xv)
        assert torch.equal(sg.bits(again), sg.bits(got)), (route.name, shape, boundary, "embedded")
        # channels 1..6 of a stacked F = 8 tensor whose channels and samples are pitched
        big = torch.zeros((x.shape[0], 8) + tuple(x.shape[2:]))
        big[:, 1:7] = x
        alloc, bv = sg.embed(big, [0, 1, 3, 4, 2], {0: 20, 1: 8}, 3, gpu)
        xs = bv[:, 1:7]
        assert xs.stride(1) > x.shape[2] * x.shape[3] * x.shape[4] and xs.stride(2) == 1
        again = three_ways(alloc, xs, lambda: losses.residual_vjp(route.method, xs, gd, boundary=boundary, mhd="flat"))
        assert losses.last_route() == fh.expected_route(route, xs)
        assert again.shape == x.shape and dense_in_memory_order(again)
        assert torch.equal(sg.bits(again), sg.bits(got)), (route.name, shape, boundary, "F = 8 slice")


def test_pre_mhd_residual_is_the_induction_route(gpu):
    from cp_pre_amd import losses
    route = fh.MHDRoute("induction", pre=True)
    shape = fh.SEAM_SHAPES["chunk_seam"]
    x, g = seam_inputs(route, shape, False)
    got = losses.residual_vjp(route.method, fh.nt_fastest(x, gpu), g.to(gpu), mhd="flat")
    assert losses.last_route() == "fused:flat_mhd_induction"
    check_grad(route, got, ref_vjp(route, x.double(), g.double(), False), "PRE_MHD.residual")


# ------------------------------------------------------------------ (2) the losses, through the script's permute
@pytest.mark.parametrize("opset", fh.OPSETS)
@pytest.mark.parametrize("eq", fh.EQS)
def test_pi_and_pisl_loss_through_the_scripts_permute_against_fp64(gpu, eq, opset):
    """``pred`` is the surrogate's [BS,6,Nx,Ny,Nt]; the loss sees ``pred.permute(0,1,4,2,3)`` and ``(3 * loss).backward()``
    fills ``pred.grad``: the device-resident upstream factor reaches every march of every launch"""
    from cp_pre_amd import losses
    route = route_of(eq, opset)
    for shape in (fh.SEAM_SHAPES["straddle_10"], fh.SEAM_SHAPES["two_marches"]):
        x, _ = seam_inputs(route, shape, True, seed=4)
        yy = x + 0.1 * torch.rand(x.shape, generator=torch.Generator().manual_seed(5))
        for boundary in (False, True):
            for y in (None, yy):
                v64, g64 = ref_loss(route, x.double(), boundary, None if y is None else y.double(), 3.0)
                pred = x.permute(0, 1, 3, 4, 2).contiguous().to(gpu).requires_grad_(True)
                view = pred.permute(0, 1, 4, 2, 3)
                loss = losses.pi_loss(route.method, view, boundary=boundary, mhd="flat") if y is None else \
                    losses.pisl_loss(route.method, view, fh.nt_fastest(y, gpu), boundary=boundary, mhd="flat")
                assert losses.last_route() == "fused:flat_" + route.kind, losses.last_route()
                assert loss.dim() == 0 and loss.dtype == torch.float32
                (3 * loss).backward()
                value = float(loss.detach())
                print(f"{'pi' if y is None else 'pisl'} {route.name} {shape} boundary={boundary}: loss {value:.6e} (fp64 {v64:.6e})")
                assert abs(value - v64) <= TOL * abs(v64)
                assert pred.grad.shape == pred.shape and pred.grad.is_contiguous()
                check_grad(route, pred.grad.permute(0, 1, 4, 2, 3), g64, f"loss {shape} boundary={boundary}")


# ------------------------------------------------------------------ (3) general stars: what the library says, correct either way
@pytest.mark.parametrize("eq", fh.EQS)
def test_general_stars_follow_supported_and_are_correct_either_way(gpu, eq):
    from cp_pre_amd import _dispatch, _lib, losses
    from cp_pre_amd._method import MHD_EQ
    route = route_of(eq, "stars")
    if eq == "gauss":
        want_route = "fused:flat_linear2"
    else:
        ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in route.ops]
        rc = _lib.load_vjpflatmhd().pre_vjpflatmhd_supported(MHD_EQ.index(eq), *ks)
        assert rc in (0, _lib.PRE_E_UNSUPPORTED) and (rc == 0) == bool(built_constants()[eq])
        want_route = "fused:flat_mhd_" + eq if rc == 0 else "fallback:declined by the library"
    for name in ("straddle_10", "chunk_seam", "two_marches"):
        for boundary in (False, True):
            x, g, want = case(route, fh.SEAM_SHAPES[name], boundary)
            got = losses.residual_vjp(route.method, fh.nt_fastest(x, gpu), g.to(gpu), boundary=boundary, mhd="flat")
            assert losses.last_route() == want_route
            check_grad(route, got, want, f"stars {name} boundary={boundary}")
    x, _ = seam_inputs(route, fh.SEAM_SHAPES["straddle_10"], True, seed=8)
    v64, g64 = ref_loss(route, x.double(), False)
    xd = fh.nt_fastest(x, gpu).requires_grad_(True)
    loss = losses.pi_loss(route.method, xd, mhd="flat")
    assert losses.last_route() == want_route
    loss.backward()
    assert abs(float(loss.detach()) - v64) <= TOL * abs(v64)
    check_grad(route, xd.grad, g64, "stars, pi_loss")


# ------------------------------------------------------------------ (4) declines, each with the correct gradient
@pytest.mark.parametrize("eq", fh.EQS)
def test_declines_have_their_reasons_and_the_correct_gradient(gpu, eq):
    from cp_pre_amd import losses
    route = fh.MHDRoute(eq)
    for shape, why in fh.DECLINED.items():                         # Nt = 96; Ny*Nt % 4 != 0
        x, g, want = case(route, shape, False)
        got = losses.residual_vjp(route.method, fh.nt_fastest(x, gpu), g.to(gpu), mhd="flat")
        assert losses.last_route() == why
        check_grad(route, got, want, why)
    # a t-slab of a longer tensor: Nt-fastest, rows not dense
    shape = fh.SEAM_SHAPES["one_chunk_one_march"]
    x, g, want = case(route, shape, False)
    long = torch.zeros(x.shape[:2] + (shape[1] + 2,) + x.shape[3:])
    long[:, :, :shape[1]] = x
    slab = fh.nt_fastest(long, gpu)[:, :, :shape[1]]
    assert slab.stride(2) == 1 and slab.stride(-1) == shape[1] + 2
    got = losses.residual_vjp(route.method, slab, g.to(gpu), mhd="flat")
    if eq == "gauss":                                              # linear: its launch reads no field
        assert losses.last_route() in ("fused:flat_linear2", "fallback:declined by the library")
    else:
        assert losses.last_route() == "fallback:rows of the fields not dense"
    check_grad(route, got, want, "a t-slab")
    # the parent's answers on the same view are still there
    xt = fh.nt_fastest(x, gpu)
    got = losses.residual_vjp(route.method, xt, g.to(gpu), flat=True, mhd=True)
    assert losses.last_route() == "fallback:no flat VJP for MHD"
    got = losses.residual_vjp(route.method, xt, g.to(gpu), mhd=True)
    assert losses.last_route() == "fallback:no unit stride on the last axis"
    check_grad(route, got, want, "mhd=True")
    # a unit-stride input under mhd="flat" is mhd=True's
    got = losses.residual_vjp(route.method, x.to(gpu), g.to(gpu), mhd="flat")
    assert losses.last_route() == "fused:" + route.kind
    check_grad(route, got, want, "unit stride")
    flat_too = losses.residual_vjp(route.method, xt, g.to(gpu), flat=True, mhd="flat")
    assert losses.last_route() == "fused:flat_" + route.kind
    assert torch.equal(sg.bits(flat_too), sg.bits(losses.residual_vjp(route.method, xt, g.to(gpu), mhd="flat")))
    # a kernel that requires grad (last: the route object is spent)
    route.obj.D_x.kernel.requires_grad_(True)
    got = losses.residual_vjp(route.method, xt, g.to(gpu), mhd="flat")
    assert losses.last_route() == "fallback:operator kernel requires grad"
    check_grad(route, got, want, "a kernel that requires grad")


# ------------------------------------------------------------------ (5) the entries themselves
def launch(route, g, fields, outs, flags=0, host_scale=1.0, dev_scale=None):
    """``pre_vjpflatmhd_<eq>_f32`` on device views where they lie -> return code.  ``fields`` / ``outs``: the [B,T,X,Y] views
    of the channels ``route.chan``, in that order."""
    from cp_pre_amd import _dispatch, _lib
    lib = _lib.load_vjpflatmhd()
    ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in route.ops]
    fa = (_lib.PreField * len(fields))(*[_lib.field(v) for v in fields])
    oa = (_lib.PreField * len(outs))(*[_lib.field(v) for v in outs])
    extra = (float(route.obj.gamma),) if route.eq == "energy" else ()
    return getattr(lib, "pre_vjpflatmhd_%s_f32" % route.eq)(ctypes.byref(_lib.field(g)), fa, oa, *ks, *extra, float(host_scale),
                                                             _lib.ptr(dev_scale), *g.shape, flags, _lib.stream())


def dense_run(route, g, x, gpu, flags=0, host_scale=1.0):
    """the entry of ``route`` on the Nt-fastest copies of ``g`` [B,T,X,Y] and ``x`` [B,6,T,X,Y] -> [B,6,T,X,Y] on the CPU
    (the channels the equation does not read stay zero)"""
    gd, xd = fh.nt_fastest_exact(g, gpu), fh.nt_fastest_exact(x, gpu)
    out = fh.nt_fastest_exact(torch.zeros(x.shape), gpu)
    assert launch(route, gd, [xd[:, c] for c in route.chan], [out[:, c] for c in route.chan], flags, host_scale) == 0
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("opset", ["default", "yfix"])
@pytest.mark.parametrize("eq", fh.EQ4)
def test_entries_at_the_degenerate_extents_against_the_closed_forms(gpu, eq, opset):
    """Nt = 1 among them, which the losses hand to the tiled library (the view is Ny-fastest too): one halo quad per side,
    the x-neighbour the adjacent cell, no y-neighbour anywhere"""
    route = route_of(eq, opset)
    for shape in fh.DEGENERATE + [fh.SEAM_SHAPES["straddle_6"]]:
        for boundary in (False, True):
            x, g = seam_inputs(route, shape, boundary, seed=1)
            gfull = pad_g(g, boundary, shape)
            want = fh.closed_form(route, x.double(), gfull.double())
            got = dense_run(route, gfull, x, gpu)
            check_grad(route, got, want, f"entry {shape} boundary={boundary}")
            if not boundary:                                       # the crop flag on the uncropped g of the same case
                spread = torch.randn(gfull.shape, generator=torch.Generator().manual_seed(2))
                inner = torch.zeros_like(spread)
                inner[:, 1:-1, 1:-1, 1:-1] = spread[:, 1:-1, 1:-1, 1:-1]
                from cp_pre_amd import _lib
                a = dense_run(route, spread, x, gpu, _lib.PRE_VJP_CROP)
                b = dense_run(route, inner, x, gpu)
                assert torch.equal(sg.bits(a), sg.bits(b)), (eq, shape, "the crop is per logical cell")


def rim_mask(shape):
    m = np.ones(shape, bool)
    m[(slice(None),) + (slice(1, -1),) * (len(shape) - 1)] = False
    return torch.from_numpy(m)


@pytest.mark.parametrize("eq", fh.EQ4)
def test_nonfinite_g_on_the_rim_changes_no_bit_under_the_crop(gpu, eq):
    from cp_pre_amd import _lib
    route = route_of(eq)
    for name in ("straddle_10", "chunk_seam", "two_marches"):
        shape = fh.SEAM_SHAPES[name]
        x, _ = seam_inputs(route, shape, True, seed=2)
        g = torch.randn(shape, generator=torch.Generator().manual_seed(3))
        rim = rim_mask(shape)
        zeros = g.clone()
        zeros[rim] = 0.0
        want = dense_run(route, zeros, x, gpu, _lib.PRE_VJP_CROP, 0.25)
        assert torch.isfinite(want).all()
        for bad in (float("nan"), float("inf"), float("-inf")):
            spoiled = g.clone()
            spoiled[rim] = bad
            got = dense_run(route, spoiled, x, gpu, _lib.PRE_VJP_CROP, 0.25)
            assert torch.equal(sg.bits(got), sg.bits(want)), (eq, shape, bad)
        # without the crop the same g does reach the result (the test would notice a kernel that ignores the rim)
        assert not torch.isfinite(dense_run(route, spoiled, x, gpu, 0, 0.25)).all()


@pytest.mark.parametrize("eq", fh.EQ4)
def test_two_runs_give_the_same_bytes(gpu, eq):
    route = route_of(eq, "rescaled")
    for name in ("chunk_seam", "one_plane_last_march"):
        shape = fh.SEAM_SHAPES[name]
        x, _ = seam_inputs(route, shape, True, seed=3)
        g = torch.randn(shape, generator=torch.Generator().manual_seed(4))
        a = dense_run(route, g, x, gpu, 0, 0.5)
        b = dense_run(route, g, x, gpu, 0, 0.5)
        assert torch.equal(sg.bits(a), sg.bits(b)), (eq, shape)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("eq,opset", [(e, "default") for e in fh.EQ4] + [("induction", "stars")])
def test_a_nan_in_a_field_reaches_the_cells_the_fp64_reference_says(gpu, eq, opset, boundary):
    """The sandwich of tests/test_gpu_mhdvjp.py on the merged-row march: non-finite wherever the fp64 autograd over the
    NON-ZERO taps is, finite and within TOL wherever the dense reference (every tap of the 3^3 box, 0 * NaN included) is
    finite; with general stars whose taps are all non-zero exactly the reference's set.  One sample per bad cell: both sides
    of the cut of the marched axis (Nx = 18: marches of 9 planes), both ends of a row of Nt = 10 cells (quads straddle them),
    corners, a face; the bad field goes round the channels the equation reads."""
    from cp_pre_amd import losses
    if opset == "stars" and not built_constants()[eq]:
        pytest.fail("the general-star instantiation this case was written for is not built: choose another equation")
    route = route_of(eq, opset)
    cells = [(0, 8, 2), (9, 9, 3), (0, 0, 0), (9, 17, 5), (5, 8, 0), (4, 9, 5), (3, 0, 3), (6, 17, 2)]      # (t, x, y)
    shape = (len(cells), 10, 18, 6)
    assert fh.split(shape)["tSeg"] == 9 and fh.split(shape)["nTSeg"] == 2
    x, g = seam_inputs(route, shape, boundary, seed=6)
    clean = x.clone()
    for p, c in enumerate(cells):
        x[(p, route.chan[p % len(route.chan)]) + c] = float("nan")
    got = losses.residual_vjp(route.method, fh.nt_fastest(x, gpu), g.to(gpu), boundary=boundary, mhd="flat").cpu().numpy()
    assert losses.last_route() == "fused:flat_" + route.kind
    sparse = ref_vjp(route, x.double(), g.double(), boundary).numpy()                     # non-zero taps only
    xr = x.double().requires_grad_(True)
    route.residual(xr, boundary, D).backward(g.double())                                  # every tap of the box
    dense = xr.grad.numpy()
    must, may = ~np.isfinite(sparse), ~np.isfinite(dense)
    assert must.any() and not (must & ~may).any()
    bad = ~np.isfinite(got)
    assert not (must & ~bad).any(), f"a NaN the reference propagates was hidden, e.g. at {np.argwhere(must & ~bad)[:4].tolist()}"
    assert not (bad & ~may).any(), f"a NaN outside the reference's set, e.g. at {np.argwhere(bad & ~may)[:4].tolist()}"
    if opset == "stars":
        assert np.array_equal(bad, must), "the non-finite set differs from the fp64 autograd reference's"
    ref = ref_vjp(route, clean.double(), g.double(), boundary).numpy()
    fin = ~may
    err = np.max(np.abs(got[fin] - ref[fin])) / np.max(np.abs(ref))
    print(f"{route.name} boundary={boundary}: {int(must.sum())} <= {int(bad.sum())} <= {int(may.sum())} non-finite, rel err elsewhere {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("eq", fh.EQS)
def test_loss_applies_the_kernels_its_operators_hold_now(gpu, eq):
    """a tap changed in place between two calls (no new tensor identity) is the one the next forward AND backward apply"""
    from cp_pre_amd import losses
    route = fh.MHDRoute(eq, "rescaled", device=gpu)
    x, _ = seam_inputs(route, fh.SEAM_SHAPES["two_marches"], True, seed=7)

    def step():
        xd = fh.nt_fastest(x, gpu).requires_grad_(True)
        loss = losses.pi_loss(route.method, xd, mhd="flat")
        loss.backward()
        assert losses.last_route() == "fused:flat_" + route.kind
        v64, g64 = ref_loss(route, x.double(), False)              # (from the taps the operators hold now)
        assert abs(float(loss.detach()) - v64) <= TOL * abs(v64), "the loss applied other taps"
        check_grad(route, xd.grad, g64, "after a tap update")
        return float(loss.detach())
    l0 = step()
    for op, idx in ((route.obj.D_x, (1, 2, 1)), (route.obj.D_y, (2, 1, 1))):      # one tap of D_x, one of D_y
        assert op.kernel.is_cuda and float(op.kernel[idx]) != 0.0
        op.kernel.data[idx] *= 1.75
        l1 = step()
        assert l1 != l0
        l0 = l1


# ------------------------------------------------------------------ (6) the C client
def test_c_client_on_the_device(gpu, tmp_path):
    exe = tmp_path / "vjpflatmhd_check"
    subprocess.check_call(c_client_command(exe), stderr=subprocess.DEVNULL)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "no device" not in r.stdout, r.stdout + r.stderr
