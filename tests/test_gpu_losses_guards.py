"""Guard bands, non-finite footprints, refusals and kernel updates of the fused VJP and loss kernels (pytest -m gpu).

What the header comment of csrc/residual_vjp.hip promises and tests/test_gpu_losses.py does not check: the entries write
only inside their output views and read only inside their input views; the crop is a select (a NaN / inf of g outside the
averaged interior changes no bit); a NaN of g inside reaches exactly the mirrored star; a NaN in a field of a non-linear
route reaches the cells the float64 autograd reference says; refused calls launch nothing; and a loss applies the taps its
operators hold NOW (``.data.mul_(2)`` / ``.data = other`` after a first call)."""
import ctypes

import numpy as np
import pytest
import torch

import stencil_guards as sg
from losses_helpers import D, Route, asym_star, channel_errs, ref_loss, ref_vjp, seam_inputs
from test_gpu_losses_seams import gpu, route_of, sumsq  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-5
KINDS = ["op3d", "op2d", "ns_continuity_yfix", "ns_momentum", "burgers"]          # one route per pre_vjp_*_f32 entry


def launch(route, g, ins, outs, flags=0, host_scale=1.0, dev_scale=None, dims=None, g_field=None, out_fields=None):
    """The ``pre_vjp_<kind>_f32`` entry of ``route`` on device views where they lie -> return code.  ``g``, ``ins`` (the
    fields the route is non-linear in), ``outs``: [B,T,X,Y] views, [B,T,X] for the 2-D routes.  ``dims`` / ``g_field`` /
    ``out_fields`` override the extents and the descriptors (refusal tests)."""
    from cp_pre_amd import _dispatch, _lib
    from cp_pre_amd import residuals as R
    lib, o = _lib.load_vjp(), route.obj
    ks = [_dispatch.host_kernel(op.kernel) for op in route.ops]
    k27 = [_lib.farr(k.reshape(-1)) for k in ks]
    scale = (float(host_scale), _lib.ptr(dev_scale))
    dims = tuple(g.shape) if dims is None else tuple(dims)
    st = _lib.stream()
    if route.nd == 3:
        gf = g_field if g_field is not None else _lib.field(g)
        of = out_fields if out_fields is not None else [_lib.field(v) for v in outs]
        oa = (_lib.PreField * len(of))(*of)
    if route.kind == "ns_momentum":
        return lib.pre_vjp_ns_momentum_f32(ctypes.byref(gf), R._arr(ins), oa, *k27, float(o.dt), float(o.dx), float(o.dy), float(o.nu),
                                           *scale, *dims, flags, st)
    if route.kind == "linear2":
        return lib.pre_vjp_linear2_f32(ctypes.byref(gf), oa, *k27, float(o.dx / o.dy), *scale, *dims, flags, st)
    if route.kind == "burgers":
        return lib.pre_vjp_burgers_f32(*[a for t in (g, ins[0], outs[0]) for a in (_lib.ptr(t), _lib.iarr64(t.stride()))], *k27,
                                       float(o.dx), float(o.dt), float(o.nu), float(2 * o.dt / o.dx), *scale, *dims, flags, st)
    w, off = _dispatch.taps_of(ks[0])
    wv, ov = _lib.farr(w), _lib.iarr32(off.reshape(-1))
    if route.kind == "stencil3d":
        return lib.pre_vjp_stencil3d_f32(ctypes.byref(gf), ctypes.byref(oa[0]), wv, ov, len(w), *scale, *dims, flags, st)
    return lib.pre_vjp_stencil2d_f32(_lib.ptr(g), _lib.iarr64(g.stride()), _lib.ptr(outs[0]), _lib.iarr64(outs[0].stride()), wv, ov,
                                     len(w), *scale, *dims, flags, st)


def n_in(route):
    return {"ns_momentum": 2, "burgers": 1}.get(route.kind, 0)


def n_out(route):
    return {"ns_momentum": 3, "linear2": 2}.get(route.kind, 1)


def fields(route, shape, seed=0):
    """(g, [inputs]) CPU tensors of the residual's uncropped shape"""
    gen = torch.Generator().manual_seed(seed + sum(shape))
    rs = tuple(shape) if route.nd == 3 else (shape[0] * shape[1],) + tuple(shape[2:])
    return torch.randn(rs, generator=gen), [torch.rand(rs, generator=gen) + 0.5 for _ in range(n_in(route))]


def dense_run(route, g, ins, gpu, flags=0, host_scale=1.0):
    outs = [torch.zeros(g.shape, device=gpu) for _ in range(n_out(route))]
    rc = launch(route, g.to(gpu), [f.to(gpu) for f in ins], outs, flags, host_scale)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return torch.stack(outs, 1)


GUARD_SHAPES = [(2, 17, 33, 61), (1, 9, 10, 257), (2, 5, 9, 130), (1, 3, 5, 64)]       # Y % 4 = 1, 1, 2, 0; t, x and y seams


# ------------------------------------------------------------------ writes stay in the view
@pytest.mark.parametrize("name", KINDS)
def test_vjp_entries_write_only_inside_their_output_views(gpu, name):
    route = route_of(name)
    for shape in GUARD_SHAPES + [(1, 4, 9, 67)]:                                     # (Y % 4 = 3)
        g, ins = fields(route, shape)
        want = dense_run(route, g, ins, gpu)
        gd, ind = g.to(gpu), [f.to(gpu) for f in ins]
        nd1, no = g.dim(), n_out(route)
        # (a) every output a view of its own: pitched rows, planes and samples, base 4 bytes off
        triples = [sg.guarded_out(tuple(g.shape), None, {nd1 - 2: 5, nd1 - 3: 9, 0: 13}, 1, gpu) for _ in range(no)]
        assert launch(route, gd, ind, [t[1] for t in triples]) == 0
        torch.cuda.synchronize()
        for i, (alloc, view, mask) in enumerate(triples):
            assert sg.untouched(alloc, mask), (name, shape, "output %d wrote outside its view" % i)
            assert torch.equal(sg.bits(view), sg.bits(want[:, i])), (name, shape, i)
        # (b) the real layout: the slots of ONE stacked gradient tensor (two foreign channels around them), pitched
        alloc, big, mask = sg.guarded_out((g.shape[0], no + 2) + tuple(g.shape[1:]), None, {nd1 - 1: 3, nd1 - 2: 8, 1: 20}, 3, gpu)
        slots = [big[:, 1 + i] for i in range(no)]
        mask = sg.outside_mask(alloc, *slots)
        assert launch(route, gd, ind, slots) == 0
        torch.cuda.synchronize()
        assert sg.untouched(alloc, mask), (name, shape, "a gradient slot wrote outside itself")
        assert torch.equal(sg.bits(big[:, 1:-1]), sg.bits(want))


# ------------------------------------------------------------------ reads stay in the view
@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("name", KINDS)
def test_vjp_entries_read_only_inside_their_input_views(gpu, name, crop):
    from cp_pre_amd import _lib
    route = route_of(name)
    flags = _lib.PRE_VJP_CROP if crop else 0
    for shape in GUARD_SHAPES + [(1, 4, 9, 67), (1, 4, 9, 191)]:
        g, ins = fields(route, shape, seed=1)
        want = dense_run(route, g, ins, gpu, flags, 0.5)
        nd1 = g.dim()
        owned = [sg.embed(t, None, {nd1 - 2: 3 + i, nd1 - 3: 8}, 1 + i, gpu) for i, t in enumerate([g] + ins)]
        masks = [sg.outside_mask(a, v) for a, v in owned]
        outs = [torch.zeros(g.shape, device=gpu) for _ in range(n_out(route))]
        for value in sg.POISONS:
            for (a, _), m in zip(owned, masks):
                sg.poison(a, m, value)
            assert launch(route, owned[0][1], [v for _, v in owned[1:]], outs, flags, 0.5) == 0
            torch.cuda.synchronize()
            assert torch.equal(sg.bits(torch.stack(outs, 1)), sg.bits(want)), (name, shape, crop, value)


# ------------------------------------------------------------------ the crop is a select
def rim_mask(shape):
    m = np.ones(shape, bool)
    m[(slice(None),) + (slice(1, -1),) * (len(shape) - 1)] = False
    return torch.from_numpy(m)


@pytest.mark.parametrize("name", KINDS)
def test_nonfinite_g_on_the_rim_changes_no_bit_under_the_crop(gpu, name):
    from cp_pre_amd import _lib
    route = route_of(name)
    for shape in [(2, 17, 33, 61), (1, 9, 10, 257)]:
        g, ins = fields(route, shape, seed=2)
        rim = rim_mask(tuple(g.shape))               # first and last cell of every residual axis, corners included
        zeros = g.clone()
        zeros[rim] = 0.0
        want = dense_run(route, zeros, ins, gpu, _lib.PRE_VJP_CROP, 0.25)
        assert torch.isfinite(want).all()
        for bad in (float("nan"), float("inf"), float("-inf")):
            spoiled = g.clone()
            spoiled[rim] = bad
            got = dense_run(route, spoiled, ins, gpu, _lib.PRE_VJP_CROP, 0.25)
            assert torch.equal(sg.bits(got), sg.bits(want)), (name, shape, bad)
            if route.nd == 3:
                a = sumsq(spoiled.to(gpu), _lib.PRE_VJP_CROP, gpu)
                b = sumsq(zeros.to(gpu), _lib.PRE_VJP_CROP, gpu)
            else:
                a = sumsq(spoiled.to(gpu)[None], _lib.PRE_VJP_CROP | _lib.PRE_VJP_VIEW3D, gpu)
                b = sumsq(zeros.to(gpu)[None], _lib.PRE_VJP_CROP | _lib.PRE_VJP_VIEW3D, gpu)
            assert torch.equal(sg.bits(a), sg.bits(b)) and bool(torch.isfinite(a).all()), (name, shape, bad)
        # without the crop the same g does reach the result (the test would notice a kernel that ignores the rim)
        assert not torch.isfinite(dense_run(route, spoiled, ins, gpu, 0, 0.25)).all()


@pytest.mark.parametrize("name", ["op3d", "op2d", "wave", "ns_continuity_yfix"])
def test_pi_loss_ignores_a_nonfinite_rim_of_the_residual(gpu, name, monkeypatch):
    """The residual the loss keeps gets NaN / inf on its rim (first and last cell of every residual axis) between the forward
    pass and the sum: ``_Spec.full`` is wrapped, everything after it is the real ``pi_loss``.  Loss and gradient must equal,
    bit for bit, those of the untouched residual: the rim of r is neither summed nor propagated."""
    from cp_pre_amd import losses
    route = route_of(name)
    x, _ = seam_inputs(route, (2, 17, 33, 61), True, seed=11)
    v64, g64 = ref_loss(route, x.double(), False)
    real = losses._Spec.full
    state = {"bad": None}

    def full(self, pred, minus):
        r = real(self, pred, minus)
        if state["bad"] is not None:
            r = r.clone()
            r[rim_mask(tuple(r.shape)).to(r.device)] = state["bad"]
        return r
    monkeypatch.setattr(losses._Spec, "full", full)

    def run():
        xd = x.to(gpu).requires_grad_(True)
        loss = losses.pi_loss(route.method, xd)
        loss.backward()
        assert losses.last_route() == "fused:" + route.kind
        return loss.detach().reshape(1), xd.grad
    l0, g0 = run()
    assert abs(float(l0) - v64) <= TOL * abs(v64) and max(channel_errs(g0, g64).values()) <= TOL
    for bad in (float("nan"), float("inf"), float("-inf")):
        state["bad"] = bad
        l1, g1 = run()
        assert torch.equal(sg.bits(l1), sg.bits(l0)) and torch.equal(sg.bits(g1), sg.bits(g0)), bad


# ------------------------------------------------------------------ a NaN of g inside: exactly the mirrored star
@pytest.mark.parametrize("shape,cells", [((17, 40, 70), [(8, 20, 30), (9, 20, 30), (4, 31, 30), (4, 32, 30), (4, 20, 63), (4, 20, 64), (8, 31, 63), (9, 32, 64)]),
                                         ((17, 10, 260), [(8, 4, 100), (9, 4, 100), (4, 7, 100), (4, 8, 100), (4, 4, 255), (4, 4, 256), (8, 7, 255), (9, 8, 256)])],
                         ids=["narrow", "wide"])
def test_a_nan_of_g_reaches_exactly_the_mirrored_star(gpu, shape, cells):
    """one sample per bad cell, on both sides of a t-segment cut (8 | 9), a row-tile seam and a column-tile seam"""
    from cp_pre_amd import losses
    route = route_of("op3d")
    k = asym_star(3)
    gen = torch.Generator().manual_seed(21)
    x = torch.rand((len(cells),) + shape, generator=gen)
    g = torch.randn((len(cells),) + shape, generator=gen)
    bad = np.zeros(tuple(g.shape), bool)
    spoiled = g.clone()
    for p, c in enumerate(cells):
        bad[(p,) + c] = True
        spoiled[(p,) + c] = float("nan")
    clean = losses.residual_vjp(route.method, x.to(gpu), g.to(gpu), boundary=True)
    got = losses.residual_vjp(route.method, x.to(gpu), spoiled.to(gpu), boundary=True)
    assert losses.last_route() == "fused:stencil3d"
    must, may = sg.footprint(torch.flip(k, (0, 1, 2)).numpy(), bad)              # the adjoint: the star with mirrored taps
    assert must.sum() == 7 * len(cells)
    want = ref_vjp(route, x.double(), g.double(), True).numpy()
    sg.check_sandwich(got.cpu().numpy(), want, must, may, TOL, lone_nan=True)
    gn = got.cpu().numpy()
    assert np.array_equal(~np.isfinite(gn), must), "the non-finite cells are not exactly the mirrored star of the bad cell"
    keep = torch.from_numpy(~must)
    assert torch.equal(sg.bits(got.cpu())[keep], sg.bits(clean.cpu())[keep]), "a cell outside the star changed"


# ------------------------------------------------------------------ a NaN in a field of a non-linear route
def _full_stars(route):
    """every operator a star with all its taps non-zero and unequal (distinct per operator)"""
    for i, op in enumerate(route.ops):
        op.kernel = asym_star(route.nd) * (1.0 + 0.25 * i)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("full_stars", [False, True])
@pytest.mark.parametrize("name", ["ns_momentum", "ns_momentum_yfix", "burgers"])
def test_a_nan_in_u_reaches_the_cells_the_fp64_reference_says(gpu, name, full_stars, boundary):
    """The expected sets are not restated: they are where the float64 autograd gradient is non-finite.  ``ref64`` adds the
    NON-ZERO taps only; with ``D`` (the oracle's dense convolution) every tap of the 3^nd box is multiplied, 0 * NaN
    included.  The kernels multiply the zero x / y weights of a star and skip zero weights along the marched axis
    (star_march.hip, ``apply<K_STAR7>``), which the non-finite contract of include/cp_pre_hip.h allows: between the two
    references the value is unspecified.  So: non-finite wherever the non-zero-tap reference is, finite and within TOL
    wherever the dense reference is finite - and where every tap of every operator is non-zero (``full_stars``), where the
    kernel has no zero weight to multiply, EXACTLY the set of the reference."""
    from cp_pre_amd import losses
    route = Route(name)
    if full_stars:
        _full_stars(route)
    # one sample per bad cell: on both sides of a t-segment cut / a row seam / a column seam, corners, faces
    if route.nd == 3:
        cells = [(8, 31, 63), (9, 32, 64), (0, 0, 0), (16, 39, 69), (0, 20, 69), (5, 0, 30)]
        x, g = seam_inputs(route, (len(cells), 17, 40, 70), boundary, seed=6)
    else:                                                          # [P*17, Nx, Ny]: the bad samples 17 apart
        cells = [(31, 63), (32, 64), (0, 0), (39, 69), (0, 30), (20, 69)]
        x, g = seam_inputs(route, (len(cells), 17, 40, 70), boundary, seed=6)
    clean = x.clone()
    for p, c in enumerate(cells):
        x[((p, 0) if route.nd == 3 else (17 * p + 8,)) + c] = float("nan")
    got = losses.residual_vjp(route.method, x.to(gpu), g.to(gpu), boundary=boundary).cpu().numpy()
    assert losses.last_route() == "fused:" + route.kind
    sparse = ref_vjp(route, x.double(), g.double(), boundary).numpy()                     # non-zero taps only
    xr = x.double().requires_grad_(True)
    y = route.residual(xr, boundary, D)                                                  # every tap of the box
    y.backward(g.double())
    dense = xr.grad.numpy()
    must, may = ~np.isfinite(sparse), ~np.isfinite(dense)
    assert must.any() and not (must & ~may).any()
    bad = ~np.isfinite(got)
    assert not (must & ~bad).any(), "a NaN the reference propagates was hidden"
    assert not (bad & ~may).any(), f"a NaN outside the reference's set, e.g. at {np.argwhere(bad & ~may)[:4].tolist()}"
    if full_stars:
        assert np.array_equal(bad, must), "the non-finite set differs from the fp64 autograd reference's"
    ref = ref_vjp(route, clean.double(), g.double(), boundary).numpy()
    fin = ~may
    err = np.max(np.abs(got[fin] - ref[fin])) / np.max(np.abs(ref))
    print(f"{name} full_stars={full_stars} boundary={boundary}: {int(must.sum())} <= {int(bad.sum())} <= {int(may.sum())} non-finite, rel err elsewhere {err:.2e}")
    assert err <= TOL


# ------------------------------------------------------------------ refusals: a return code and no launch
@pytest.mark.parametrize("name", KINDS)
def test_refused_calls_launch_nothing(gpu, name):
    from cp_pre_amd import _lib
    route = route_of(name)
    shape = (2, 5, 9, 20)
    g, ins = fields(route, shape, seed=3)
    gd, ind = g.to(gpu), [f.to(gpu) for f in ins]
    no = n_out(route)

    def fresh():
        outs = [torch.empty(g.shape, device=gpu) for _ in range(no)]
        for o in outs:
            o.view(torch.int32).fill_(sg.PATTERN)
        return outs

    def untouched(ts):
        torch.cuda.synchronize()
        return all(bool((t.view(torch.int32) == sg.PATTERN).all()) for t in ts)
    outs = fresh()
    # an empty batch
    assert launch(route, gd, ind, outs, dims=(0,) + tuple(g.shape[1:])) == _lib.PRE_E_NULL and untouched(outs)
    # an output overlapping an input (shifted by one row inside one buffer): g, and every field the route reads
    N, Y = g.numel(), g.shape[-1]
    for which, src in enumerate([g] + ins):
        buf = torch.full((N + Y,), 7.0, device=gpu)
        buf[:N] = src.reshape(-1).to(gpu)
        before = sg.bits(buf)
        args = [gd] + ind
        args[which] = buf[:N].view(g.shape)
        outs = fresh()
        assert launch(route, args[0], args[1:], [buf[Y:].view(g.shape)] + outs[1:]) == _lib.PRE_E_SHAPE
        assert untouched(outs[1:]) and torch.equal(sg.bits(buf), before)
    # two outputs at one address
    if no > 1:
        outs = fresh()
        assert launch(route, gd, ind, [outs[0]] * no) == _lib.PRE_E_SHAPE and untouched(outs)
    # no unit stride on the last axis: of an output, of g
    outs = fresh()
    if route.nd == 3:
        of = [_lib.field(o) for o in outs]
        of[-1].sY = 2
        assert launch(route, gd, ind, outs, out_fields=of) == _lib.PRE_E_UNSUPPORTED and untouched(outs)
        gf = _lib.field(gd)
        gf.sY = 2
        assert launch(route, gd, ind, outs, g_field=gf) == _lib.PRE_E_UNSUPPORTED and untouched(outs)
    else:
        wide = torch.empty(tuple(g.shape[:-1]) + (2 * g.shape[-1],), device=gpu)
        wide.view(torch.int32).fill_(sg.PATTERN)
        assert launch(route, gd, ind, [wide[..., ::2]]) == _lib.PRE_E_UNSUPPORTED and untouched([wide])
        assert launch(route, torch.zeros_like(wide)[..., ::2], ind, outs) == _lib.PRE_E_UNSUPPORTED and untouched(outs)
    # the sum of squares: an empty extent, a strided last axis
    ws = torch.zeros(_lib.PRE_VJP_SUMSQ_WORKSPACE + 1, dtype=torch.float64, device=gpu)
    r4 = gd if gd.dim() == 4 else gd[None]
    out = ctypes.c_void_p(ws.data_ptr() + 8 * _lib.PRE_VJP_SUMSQ_WORKSPACE)
    lib = _lib.load_vjp()
    assert lib.pre_vjp_sumsq_f32(ctypes.byref(_lib.field(r4)), 0, *r4.shape[1:], 0, _lib.ptr(ws), out, _lib.stream()) == _lib.PRE_E_NULL
    f = _lib.field(r4)
    f.sY = 2
    assert lib.pre_vjp_sumsq_f32(ctypes.byref(f), *r4.shape, 0, _lib.ptr(ws), out, _lib.stream()) == _lib.PRE_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not ws.any()


# ------------------------------------------------------------------ the current kernel is the one applied
def _other(k, seed, gpu):
    return ((torch.rand(k.shape, generator=torch.Generator().manual_seed(seed)) + 0.5) * (k.cpu() != 0)).to(gpu)


@pytest.mark.parametrize("update", ["data.mul_(2)", "data = other"])
@pytest.mark.parametrize("name", ["op3d", "op2d", "ns_momentum", "burgers"])
def test_loss_applies_the_kernel_its_operator_holds_now(gpu, name, update):
    """``Spec.prepare`` takes its taps through ``_dispatch.host_kernel``: a device kernel rewritten in place (no new tensor
    identity, no version bump) must be the one the next forward AND backward apply"""
    from cp_pre_amd import losses
    route = Route(name, device=gpu)
    target = route.ops[1] if len(route.ops) > 1 else route.ops[0]           # D_x of NS momentum / Burgers, the operator itself
    assert target.kernel.is_cuda
    x, _ = seam_inputs(route, (2, 17, 33, 16), True, seed=7)

    def step():
        xd = x.to(gpu).requires_grad_(True)
        loss = losses.pi_loss(route.method, xd)
        loss.backward()
        assert losses.last_route() == "fused:" + route.kind
        v64, g64 = ref_loss(route, x.double(), False)                       # (from the taps the operators hold now)
        assert abs(float(loss.detach()) - v64) <= TOL * abs(v64), "the loss applied other taps"
        assert max(channel_errs(xd.grad, g64).values()) <= TOL, "the backward pass applied other taps"
        return float(loss.detach())
    l0 = step()
    for rep in range(2):                                                     # the second update is seen too
        if update == "data.mul_(2)":
            target.kernel.data.mul_(2)
        else:
            target.kernel.data = _other(target.kernel, 31 + rep, gpu)
        l1 = step()
        assert l1 != l0
        l0 = l1
