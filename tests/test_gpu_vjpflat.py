"""The fused loss backward for Nt-fastest views (``flat=True`` of cp_pre_amd.losses, csrc/vjp_flat.hip) on the device
(pytest -m gpu): every built route at the seams tests/vjpflat_helpers.py names from the split rule, against the float64
autograd gradient of ``losses_helpers`` under TOL (per channel for stacked inputs); the reference script's cropped view;
the default keyword; the declines; guard bands, non-finite footprints, refusals, determinism, current taps; the C client.
tests/test_vjpflat_cpu.py shows the same formulas in fp32 on the CPU within TOL / 4 of float64 at every one of these
shapes."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import stencil_guards as sg
import vjpflat_helpers as vf
from losses_helpers import Route, asym_star, channel_errs, ref_loss, ref_vjp, seam_inputs
from test_vjpflat_cpu import c_client_command, routes

pytestmark = pytest.mark.gpu
TOL = vf.TOL
ROUTES = dict(routes())


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def flat_route(route):
    return "fused:flat_" + route.kind


def check(got, want, what):
    errs = channel_errs(got, want)
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (what, k, v)


# ------------------------------------------------------------------ every route at every seam
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("seam", list(vf.SEAM_SHAPES))
@pytest.mark.parametrize("label", list(ROUTES))
def test_flat_vjp_at_the_seams_against_fp64(gpu, label, seam, boundary):
    from cp_pre_amd import losses
    route, shape = ROUTES[label], vf.SEAM_SHAPES[seam]
    x, g = seam_inputs(route, shape, boundary)
    want = ref_vjp(route, x.double(), g.double(), boundary)
    xd = vf.nt_fastest(x, gpu)
    assert xd.stride(-1) != 1 and xd.stride(-3) == 1
    got = losses.residual_vjp(route.method, xd, g.to(gpu), boundary=boundary, flat=True)
    assert losses.last_route() == flat_route(route)
    assert got.shape == x.shape and got.stride() == xd.stride()                   # dense, in the input's memory order
    check(got, want, f"{label} {seam} {shape} boundary={boundary}")
    # the same view inside a poisoned allocation, base 4 bytes off a 16-byte boundary: the same bits
    alloc, xv = vf.nt_fastest_embedded(x, gpu)
    assert vf.is_nt_fastest_dense(xv)
    again = sg.three_ways(alloc, [xv], lambda: losses.residual_vjp(route.method, xv, g.to(gpu), boundary=boundary, flat=True))
    assert losses.last_route() == flat_route(route)
    assert torch.equal(sg.bits(again), sg.bits(got)), (label, seam, boundary)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("label", ["wave", "ns_continuity", "ns_momentum_stars"])
def test_flat_losses_against_fp64(gpu, label, boundary):
    """pi_loss and pisl_loss with an upstream factor at a chunk seam and at a marched-axis cut, twice: the same bytes"""
    from cp_pre_amd import losses
    route = ROUTES[label]
    for shape in (vf.SEAM_SHAPES["straddle_10"], vf.SEAM_SHAPES["two_marches"]):
        x, _ = seam_inputs(route, shape, True, seed=2)
        yy = x + 0.1 * torch.rand(x.shape, generator=torch.Generator().manual_seed(3))
        for y in (None, yy):
            v64, g64 = ref_loss(route, x.double(), boundary, None if y is None else y.double(), 1000.0)
            seen = []
            for rep in range(2):
                xd = vf.nt_fastest(x, gpu).requires_grad_(True)
                loss = losses.pi_loss(route.method, xd, boundary=boundary, flat=True) if y is None else \
                    losses.pisl_loss(route.method, xd, vf.nt_fastest(y, gpu), boundary=boundary, flat=True)
                assert losses.last_route() == flat_route(route), losses.last_route()
                assert loss.dim() == 0 and loss.dtype == torch.float32
                (1000.0 * loss).backward()
                seen.append((sg.bits(loss.detach().reshape(1)), sg.bits(xd.grad)))
            assert abs(float(loss.detach()) - v64) <= TOL * abs(v64)
            check(xd.grad, g64, f"{'pi' if y is None else 'pisl'} {label} {shape} boundary={boundary}")
            assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1]), "two runs, other bytes"


# ------------------------------------------------------------------ the script's view: the new ground
SCRIPT_PREDS = [(2, 1, 12, 18, 10), (2, 1, 19, 8, 12)]        # [BS,1,Nx,Ny,Nt]: interiors (8,10,16) and (10,17,6) as (Nt,Nx,Ny)


@pytest.mark.parametrize("shape", SCRIPT_PREDS)
def test_the_script_view_takes_the_flat_route(gpu, shape):
    """Physics_Informed/Wave_FNO_PISL.py:209-217: PI_loss / PISL on field[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2) and
    backward() into ``pred``.  Without the flat route ``last_route()`` is ``fallback:no unit stride on the last axis``."""
    from cp_pre_amd import losses
    route = ROUTES["wave"]
    gen = torch.Generator().manual_seed(sum(shape))
    pred, yy = torch.rand(shape, generator=gen) + 0.5, torch.rand(shape, generator=gen) + 0.5
    inner = vf.script_view(pred).contiguous()
    reach = torch.zeros(shape, dtype=torch.bool)
    reach[:, 0, 1:-1, 1:-1, 1:-1] = True
    for y in (None, yy):
        for boundary in (False, True):
            v64, g64 = ref_loss(route, inner.double(), boundary, None if y is None else vf.script_view(y).contiguous().double())
            want = torch.zeros(shape, dtype=torch.float64)
            want[:, 0, 1:-1, 1:-1, 1:-1] = g64.permute(0, 2, 3, 1)
            pd = pred.to(gpu).requires_grad_(True)
            view = vf.script_view(pd)
            assert view.stride(-1) != 1 and view.stride(1) == 1 and not vf.is_nt_fastest_dense(view)
            loss = losses.pi_loss(route.method, view, boundary=boundary, flat=True) if y is None else \
                losses.pisl_loss(route.method, view, vf.script_view(y.to(gpu)), boundary=boundary, flat=True)
            assert losses.last_route() == "fused:flat_stencil3d", losses.last_route()
            loss.backward()
            assert abs(float(loss.detach()) - v64) <= TOL * abs(v64)
            check(pd.grad, want, f"script view {shape} {'pi' if y is None else 'pisl'} boundary={boundary}")
            assert not pd.grad.cpu()[~reach].any(), "a gradient where the view does not reach"
            # the default keyword: the fallback it was, the same gradient
            pf = pred.to(gpu).requires_grad_(True)
            vw = vf.script_view(pf)
            lf = losses.pi_loss(route.method, vw, boundary=boundary) if y is None else \
                losses.pisl_loss(route.method, vw, vf.script_view(y.to(gpu)), boundary=boundary)
            assert losses.last_route() == "fallback:no unit stride on the last axis"
            lf.backward()
            assert abs(float(lf.detach()) - v64) <= TOL * abs(v64)
            check(pf.grad, want, f"script view {shape} default keyword boundary={boundary}")


def test_a_unit_stride_input_takes_the_tiled_route_under_flat(gpu):
    from cp_pre_amd import losses
    route = ROUTES["ns_momentum"]
    x, g = seam_inputs(route, (2, 8, 10, 16), False)
    a = losses.residual_vjp(route.method, x.to(gpu), g.to(gpu), flat=True)
    assert losses.last_route() == "fused:ns_momentum"
    b = losses.residual_vjp(route.method, x.to(gpu), g.to(gpu))
    assert losses.last_route() == "fused:ns_momentum" and torch.equal(sg.bits(a), sg.bits(b))


# ------------------------------------------------------------------ declines
@pytest.mark.parametrize("shape", list(vf.DECLINED))
@pytest.mark.parametrize("label", ["wave", "ns_momentum"])
def test_flat_declines_fall_back_with_a_reason(gpu, label, shape):
    from cp_pre_amd import losses
    route = ROUTES[label]
    x, g = seam_inputs(route, shape, False)
    got = losses.residual_vjp(route.method, vf.nt_fastest(x, gpu), g.to(gpu), flat=True)
    assert losses.last_route() == vf.DECLINED[shape]
    check(got, ref_vjp(route, x.double(), g.double(), False), f"declined {label} {shape}")


def test_ns_momentum_on_rows_that_are_not_dense_falls_back(gpu):
    from cp_pre_amd import losses
    route = ROUTES["ns_momentum"]
    x, g = seam_inputs(route, (2, 8, 10, 16), False)
    big = torch.zeros(2, 3, 12, 10, 16)
    big[:, :, 2:10] = x
    slab = vf.nt_fastest(big, gpu)[:, :, 2:10]                     # a t-slab: Nt-fastest, rows 12 floats apart
    assert slab.stride(2) == 1 and slab.stride(4) == 12
    got = losses.residual_vjp(route.method, slab, g.to(gpu), flat=True)
    assert losses.last_route() == "fallback:rows of u, v not dense"
    check(got, ref_vjp(route, x.double(), g.double(), False), "ns_momentum t-slab")
    xd = slab.detach().requires_grad_(True)
    losses.pi_loss(route.method, xd, flat=True).backward()
    assert losses.last_route() == "fallback:rows of u, v not dense"
    check(xd.grad, ref_loss(route, x.double(), False)[1], "ns_momentum t-slab loss")


# ------------------------------------------------------------------ guards: the entries where the views lie
def launch(route, g, ins, outs, flags=0, host_scale=1.0, dev_scale=None, dims=None, g_field=None, out_fields=None):
    """The ``pre_vjpflat_<kind>_f32`` entry of ``route`` on device views where they lie -> return code"""
    from cp_pre_amd import _dispatch, _lib
    from cp_pre_amd import residuals as R
    lib, o = _lib.load_vjpflat(), route.obj
    ks = [_dispatch.host_kernel(op.kernel) for op in route.ops]
    k27 = [_lib.farr(k.reshape(-1)) for k in ks]
    scale = (float(host_scale), _lib.ptr(dev_scale))
    dims = tuple(g.shape) if dims is None else tuple(dims)
    st = _lib.stream()
    gf = g_field if g_field is not None else _lib.field(g)
    of = out_fields if out_fields is not None else [_lib.field(v) for v in outs]
    oa = (_lib.PreField * len(of))(*of)
    if route.kind == "ns_momentum":
        return lib.pre_vjpflat_ns_momentum_f32(ctypes.byref(gf), R._arr(ins), oa, *k27, float(o.dt), float(o.dx), float(o.dy),
                                               float(o.nu), *scale, *dims, flags, st)
    if route.kind == "linear2":
        return lib.pre_vjpflat_linear2_f32(ctypes.byref(gf), oa, *k27, float(o.dx / o.dy), *scale, *dims, flags, st)
    w, off = _dispatch.taps_of(ks[0])
    return lib.pre_vjpflat_stencil3d_f32(ctypes.byref(gf), ctypes.byref(oa[0]), _lib.farr(w), _lib.iarr32(off.reshape(-1)), len(w),
                                         *scale, *dims, flags, st)


N_IN = {"ns_momentum": 2}
N_OUT = {"ns_momentum": 3, "linear2": 2}
ENTRY_ROUTES = ["op3d", "ns_continuity_stars", "ns_momentum_stars"]             # one per entry, full asymmetric stars


def fields(route, shape, seed=0):
    gen = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(shape, generator=gen), [torch.rand(shape, generator=gen) + 0.5 for _ in range(N_IN.get(route.kind, 0))]


def dense_run(route, g, ins, gpu, flags=0, host_scale=1.0):
    """[BS,nout,Nt,Nx,Ny] (logical order) of a launch on dense Nt-fastest tensors"""
    outs = [vf.nt_fastest(torch.zeros(g.shape), gpu) for _ in range(N_OUT.get(route.kind, 1))]
    rc = launch(route, vf.nt_fastest(g, gpu), [vf.nt_fastest(f, gpu) for f in ins], outs, flags, host_scale)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return torch.stack(outs, 1)


def rim_mask(shape):
    m = np.ones(shape, bool)
    m[(slice(None),) + (slice(1, -1),) * (len(shape) - 1)] = False
    return torch.from_numpy(m)


@pytest.mark.parametrize("label", ENTRY_ROUTES)
def test_flat_entries_stay_inside_their_views(gpu, label):
    """inputs and outputs in allocations of their own, 4 bytes off, samples apart, NaN / 0 / 1e30 around the inputs: the
    outputs hold the dense run's bits and nothing outside an output view is written"""
    from cp_pre_amd import _lib
    route = ROUTES[label]
    for shape in (vf.SEAM_SHAPES["straddle_10"], vf.SEAM_SHAPES["chunk_seam"], vf.SEAM_SHAPES["two_marches"]):
        g, ins = fields(route, shape, seed=1)
        want = dense_run(route, g, ins, gpu, _lib.PRE_VJP_CROP, 0.5)
        owned = [vf.nt_fastest_embedded(t, gpu, 1 + i, 12 + 4 * i) for i, t in enumerate([g] + ins)]
        masks = [sg.outside_mask(a, v) for a, v in owned]
        for value in sg.POISONS:
            for (a, _), m in zip(owned, masks):
                sg.poison(a, m, value)
            triples = [sg.guarded_out(shape, [0, 2, 3, 1], {0: 20}, 1, gpu) for _ in range(N_OUT.get(route.kind, 1))]
            assert launch(route, owned[0][1], [v for _, v in owned[1:]], [t[1] for t in triples], _lib.PRE_VJP_CROP, 0.5) == 0
            torch.cuda.synchronize()
            for i, (alloc, view, mask) in enumerate(triples):
                assert sg.untouched(alloc, mask), (label, shape, value, "output %d wrote outside its view" % i)
                assert torch.equal(sg.bits(view), sg.bits(want[:, i])), (label, shape, value, i)


@pytest.mark.parametrize("label", ENTRY_ROUTES)
def test_nonfinite_g_on_the_rim_reaches_nothing_under_the_crop(gpu, label):
    from cp_pre_amd import _lib
    route = ROUTES[label]
    for shape in (vf.SEAM_SHAPES["straddle_6"], vf.SEAM_SHAPES["chunk_seam"], vf.SEAM_SHAPES["two_marches"]):
        g, ins = fields(route, shape, seed=2)
        rim = rim_mask(shape)
        zeros = g.clone()
        zeros[rim] = 0.0
        want = dense_run(route, zeros, ins, gpu, _lib.PRE_VJP_CROP, 0.25)
        assert torch.isfinite(want).all()
        for bad in (float("nan"), float("inf")):
            spoiled = g.clone()
            spoiled[rim] = bad
            got = dense_run(route, spoiled, ins, gpu, _lib.PRE_VJP_CROP, 0.25)
            assert torch.equal(sg.bits(got), sg.bits(want)), (label, shape, bad)
        assert not torch.isfinite(dense_run(route, spoiled, ins, gpu, 0, 0.25)).all()       # (without the crop it does)


def test_a_nan_of_g_reaches_exactly_the_mirrored_star(gpu):
    """one sample per bad cell (logical (t, x, y) of (Nt, Nx, Ny) = (30, 20, 70): chunks of 320 + 205 quads, marches of
    10 + 10 planes of Nx): on both sides of the march cut, of the chunk seam (merged position 1280 = y 42, t 20), at row ends
    inside quads, in corners"""
    from cp_pre_amd import losses
    route = ROUTES["op3d"]
    shape = (30, 20, 70)
    sp = vf.split((8,) + shape)
    assert (sp["nt"], sp["nCh"], sp["last"], sp["tSeg"], sp["nTSeg"]) == (320, 2, 205, 10, 2) and 42 * 30 + 20 == 4 * 320
    cells = [(5, 9, 20), (5, 10, 20), (19, 4, 42), (20, 4, 42), (29, 7, 41), (0, 7, 42), (0, 0, 0), (29, 19, 69)]
    gen = torch.Generator().manual_seed(21)
    x = torch.rand((len(cells),) + shape, generator=gen)
    g = torch.randn((len(cells),) + shape, generator=gen)
    bad = np.zeros(tuple(g.shape), bool)
    spoiled = g.clone()
    for p, c in enumerate(cells):
        bad[(p,) + c] = True
        spoiled[(p,) + c] = float("nan")
    xd = vf.nt_fastest(x, gpu)
    clean = losses.residual_vjp(route.method, xd, g.to(gpu), boundary=True, flat=True)
    got = losses.residual_vjp(route.method, xd, spoiled.to(gpu), boundary=True, flat=True)
    assert losses.last_route() == "fused:flat_stencil3d"
    must, may = sg.footprint(torch.flip(asym_star(3), (0, 1, 2)).numpy(), bad)         # the adjoint: the mirrored star
    want = ref_vjp(route, x.double(), g.double(), True).numpy()
    sg.check_sandwich(got.cpu().numpy(), want, must, may, TOL, lone_nan=True)
    assert np.array_equal(~np.isfinite(got.cpu().numpy()), must), "the non-finite cells are not exactly the mirrored star"
    keep = torch.from_numpy(~must)
    assert torch.equal(sg.bits(got.cpu())[keep], sg.bits(clean.cpu())[keep]), "a cell outside the star changed"


@pytest.mark.parametrize("label", ENTRY_ROUTES)
def test_refused_flat_calls_leave_their_outputs_untouched(gpu, label):
    from cp_pre_amd import _lib
    route = ROUTES[label]
    shape = (2, 10, 5, 6)
    g, ins = fields(route, shape, seed=3)
    gd, ind = vf.nt_fastest(g, gpu), [vf.nt_fastest(f, gpu) for f in ins]
    no = N_OUT.get(route.kind, 1)

    def fresh(s=shape):
        outs = [vf.nt_fastest(torch.zeros(s), gpu) for _ in range(no)]
        for o in outs:
            o.permute(0, 2, 3, 1).view(torch.int32).fill_(sg.PATTERN)
        return outs

    def untouched(ts):
        torch.cuda.synchronize()
        return all(bool((t.permute(0, 2, 3, 1).contiguous().view(torch.int32) == sg.PATTERN).all()) for t in ts)
    U, S = _lib.PRE_E_UNSUPPORTED, _lib.PRE_E_SHAPE
    outs = fresh()
    assert launch(route, gd, ind, outs, dims=(0,) + shape[1:]) == _lib.PRE_E_NULL and untouched(outs)
    # the layout: a unit-stride last axis (the tiled library's), rows that are not dense, Nt = 96, a merged row of 63 cells
    assert launch(route, g.to(gpu), [f.to(gpu) for f in ins], [torch.zeros(shape, device=gpu) for _ in range(no)]) == U
    for which in ("sY", "sX", "sT"):
        gf = _lib.field(gd)
        setattr(gf, which, getattr(gf, which) + 2)
        assert launch(route, gd, ind, outs, g_field=gf) == U and untouched(outs)
        of = [_lib.field(o) for o in outs]
        setattr(of[-1], which, getattr(of[-1], which) + 2)
        assert launch(route, gd, ind, outs, out_fields=of) == U and untouched(outs)
    assert launch(route, gd, ind, outs, dims=(2, 96, 5, 6)) == U and untouched(outs)
    assert launch(route, gd, ind, outs, dims=(2, 9, 5, 7)) == U and untouched(outs)
    assert launch(route, gd, ind, outs, flags=4) == U and untouched(outs)
    if ins:                                                        # u with rows that are not dense
        big = vf.nt_fastest(torch.zeros(2, 12, 5, 6), gpu)
        assert launch(route, gd, [big[:, 1:11], ind[1]], outs) == U and untouched(outs)
    # aliasing: an output overlapping g, and every field the route reads; two outputs at one address
    for which in range(1 + len(ins)):
        args = [gd] + ind
        before = sg.bits(args[which])
        assert launch(route, gd, ind, [args[which]] + outs[1:]) == S
        assert untouched(outs[1:]) and torch.equal(sg.bits(args[which]), before)
    if no > 1:
        assert launch(route, gd, ind, [outs[0]] * no) == S and untouched(outs)


@pytest.mark.parametrize("update", ["data.mul_(2)", "data = other"])
@pytest.mark.parametrize("name", ["op3d", "ns_momentum"])
def test_flat_loss_applies_the_kernel_its_operator_holds_now(gpu, name, update):
    from cp_pre_amd import losses
    route = Route(name, device=gpu)
    target = route.ops[1] if len(route.ops) > 1 else route.ops[0]
    x, _ = seam_inputs(route, (2, 10, 17, 6), True, seed=7)

    def step():
        xd = vf.nt_fastest(x, gpu).requires_grad_(True)
        loss = losses.pi_loss(route.method, xd, flat=True)
        loss.backward()
        assert losses.last_route() == flat_route(route)
        v64, g64 = ref_loss(route, x.double(), False)                       # (from the taps the operators hold now)
        assert abs(float(loss.detach()) - v64) <= TOL * abs(v64), "the loss applied other taps"
        assert max(channel_errs(xd.grad, g64).values()) <= TOL, "the backward pass applied other taps"
        return float(loss.detach())
    l0 = step()
    for rep in range(2):
        if update == "data.mul_(2)":
            target.kernel.data.mul_(2)
        else:
            k = target.kernel
            target.kernel.data = ((torch.rand(k.shape, generator=torch.Generator().manual_seed(31 + rep)) + 0.5) * (k.cpu() != 0)).to(gpu)
        l1 = step()
        assert l1 != l0
        l0 = l1


# ------------------------------------------------------------------ the C client on the device
def test_vjpflat_c_client_runs_on_the_device(gpu, tmp_path):
    exe = tmp_path / "vjpflat_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "FAIL" not in out.stdout and "no device" not in out.stdout, out.stdout + out.stderr
