"""The fused backward of the reduced-MHD (JOREK) residual losses on the layout the scripts hold (``jorek=True``,
csrc/vjp_flat_jorek.hip) on the device (pytest -m gpu).

The reference everywhere is fp64 autograd of the composed expressions as ``jorekvjp_helpers.JorekRoute`` restates them
(tests/test_jorekvjp_cpu.py pins the restatement to the oracle); the measure is the tensor-scale relative error overall and
per gradient channel, the bound TOL = 1e-5.  Inputs are ``rand + 0.5``, ``R = linspace(1, 2, Ny)``.  The shapes are the
seams of ``vjpflat_helpers.SEAM_SHAPES`` and three degenerate extents; every JOREK object is built with K = 0.75 as well as
the default (at the default the whole a3 term of d T is below the tolerance).  tests/test_jorekvjp_cpu.py shows the same
formulas in fp32 on the CPU within TOL / 4 of fp64 at every shape.

On the parent commit ``jorek=True`` is a ``TypeError`` and the library does not exist: every test here fails there."""
import subprocess

import numpy as np
import pytest
import torch

import jorekvjp_helpers as jh
import stencil_guards as sg
from losses_helpers import channel_errs, ref_loss, ref_vjp, seam_inputs
from test_gpu_vjpflatmhd import rim_mask, three_ways
from test_jorekvjp_cpu import c_client_command

pytestmark = pytest.mark.gpu
TOL = jh.TOL
_routes, _refs = {}, {}
KS = [None, jh.K_BIG]
# (eq, norms): norms=True is the continuity equation's alone
EQ_NORMS = [("continuity", False), ("continuity", True), ("temperature", False)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def route_of(eq, ny, opset="default", K=None, norms=False):
    key = (eq, ny, opset, K, norms)
    if key not in _routes:
        _routes[key] = jh.JorekRoute(eq, ny, opset, K=K, norms=norms)
    return _routes[key]


def case(route, shape, boundary, seed=0):
    """(x, g, the fp64 gradient) of one case on the logical axes: computed once, shared, never written to"""
    key = (route.name, shape, boundary, seed)
    if key not in _refs:
        x, g = seam_inputs(route, shape, boundary, seed)
        _refs[key] = (x, g, ref_vjp(route, x.double(), g.double(), boundary))
    return _refs[key]


def check_grad(route, got_vars, want, what):
    """``got_vars``: a gradient in the layout of ``vars`` [BS,F,Nx,Ny,Nt]; ``want`` logical"""
    got = jh.to_logical(got_vars)
    errs = channel_errs(got, want)
    print(f"{route.name} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (route.name, what, k, v)
    for c in jh.unread(route, got.shape[1]):
        assert not bool(got[:, c].any()), (route.name, what, "channel %d is not read: its gradient is exactly zero" % c)


def fused_route(route):
    return "fused:flat_" + route.kind


# ------------------------------------------------------------------ (1) residual_vjp at the seams
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("opset", jh.OPSETS)
@pytest.mark.parametrize("eq,norms", EQ_NORMS)
def test_residual_vjp_at_the_seams_against_fp64(gpu, eq, norms, opset, boundary, K):
    from cp_pre_amd import losses
    for shape in jh.GPU_SHAPES:
        route = route_of(eq, shape[3], opset, K, norms)
        x, g, want = case(route, shape, boundary)
        gd, xd = g.to(gpu), jh.vars_on(x, gpu)
        got = losses.residual_vjp(route.method, xd, gd, boundary=boundary, jorek=True)
        assert losses.last_route() == fused_route(route), (shape, losses.last_route())
        assert got.shape == xd.shape and got.is_contiguous()       # dense in the input's memory order
        check_grad(route, got, want, f"{shape} boundary={boundary}")
        # the same vars inside an allocation of the test's, base 4 bytes off a 16-byte boundary, samples further apart than
        # they are long, NaN / 0 / 1e30 around it: the same bits, the bands as they were
        alloc, xv = sg.embed(jh.to_vars(x).contiguous(), None, {0: 12}, 1, gpu)
        assert xv.data_ptr() % 16 == 4 and xv.stride(0) > xv[0].numel()
        assert all(n == 1 or a == b for n, a, b in zip(xv.shape[1:], xv.stride()[1:], xd.stride()[1:]))      # (the rows stay dense)
        again = three_ways(alloc, xv, lambda: losses.residual_vjp(route.method, xv, gd, boundary=boundary, jorek=True))
        assert losses.last_route() == fused_route(route)
        assert again.is_contiguous() and torch.equal(sg.bits(again), sg.bits(got)), (route.name, shape, boundary, "embedded")
    # more channels than the equations read: the rest is exactly zero, the three as before
    shape = jh.SEAM_SHAPES["straddle_10"]
    route = route_of(eq, shape[3], opset, K, norms)
    x, g, want = case(route, shape, boundary)
    big = torch.cat([jh.to_vars(x), torch.rand(x.shape[0], 2, shape[2], shape[3], shape[1])], 1).contiguous().to(gpu)
    first = losses.residual_vjp(route.method, jh.vars_on(x, gpu), g.to(gpu), boundary=boundary, jorek=True)
    spec = losses._Spec(route.method, False, True)                 # (the methods unstack exactly three: the VJP alone takes more)
    why, ks = spec.prepare_jorek(big)
    assert why is None
    gfull = jh.pad_g(g, boundary, shape).to(gpu).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wide = spec.vjp_jorek(ks, gfull, big, False, 1.0, None)
    assert wide.shape == big.shape and not bool(wide[:, route.nread:].any())
    assert torch.equal(sg.bits(wide[:, :3]), sg.bits(first))


# ------------------------------------------------------------------ (2) the losses on the surrogate's leaf
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("opset", jh.OPSETS)
@pytest.mark.parametrize("eq,norms", EQ_NORMS)
def test_pi_and_pisl_loss_on_a_leaf_against_fp64(gpu, eq, norms, opset, K):
    """``pred`` is the surrogate's [BS,3,Nx,Ny,Nt] leaf; ``(3 * loss).backward()`` fills ``pred.grad``: the device-resident
    upstream factor reaches every march of every launch"""
    from cp_pre_amd import losses
    for shape in (jh.SEAM_SHAPES["straddle_10"], jh.SEAM_SHAPES["two_marches"]):
        route = route_of(eq, shape[3], opset, K, norms)
        x, _ = seam_inputs(route, shape, True, seed=4)
        yy = x + 0.1 * torch.rand(x.shape, generator=torch.Generator().manual_seed(5))
        for boundary in (False, True):
            for y in (None, yy):
                v64, g64 = ref_loss(route, x.double(), boundary, None if y is None else y.double(), 3.0)
                pred = jh.vars_on(x, gpu).requires_grad_(True)
                loss = losses.pi_loss(route.method, pred, boundary=boundary, jorek=True) if y is None else \
                    losses.pisl_loss(route.method, pred, jh.vars_on(y, gpu), boundary=boundary, jorek=True)
                assert losses.last_route() == fused_route(route), losses.last_route()
                assert loss.dim() == 0 and loss.dtype == torch.float32
                (3 * loss).backward()
                value = float(loss.detach())
                print(f"{'pi' if y is None else 'pisl'} {route.name} {shape} boundary={boundary}: loss {value:.6e} (fp64 {v64:.6e})")
                assert abs(value - v64) <= TOL * abs(v64)
                assert pred.grad.shape == pred.shape and pred.grad.is_contiguous()
                check_grad(route, pred.grad, g64, f"loss {shape} boundary={boundary}")


# ------------------------------------------------------------------ (3) the box footprint
# one NaN in a phi cell per sample, (t, x, y) on the logical axes
CUT_CELLS = [(0, 0, 0), (9, 17, 5), (0, 17, 5), (9, 0, 0),         # corners of the view
             (0, 8, 2), (9, 8, 3), (0, 9, 3), (9, 9, 2),           # both ends of a row of Nt = 10 cells, on each side of the cut
             (5, 8, 0), (4, 9, 5)]                                 # inside a row, on each side of the cut
SEAM_CELLS = [(19, 2, 21), (20, 2, 21), (19, 0, 21), (20, 4, 21)]  # merged positions 1279 | 1280: the chunk seam


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("where", ["cut", "chunk_seam"])
@pytest.mark.parametrize("eq", jh.EQS)
def test_a_nan_in_phi_reaches_exactly_the_cells_fp64_autograd_says(gpu, eq, where, boundary):
    """The gradient at a cell reads phi at the four corners of the (R, Z) plane.  Non-finite exactly where fp64 autograd over
    the non-zero taps is - the diagonal cells among them - finite and within TOL elsewhere."""
    from cp_pre_amd import losses
    cells = CUT_CELLS if where == "cut" else SEAM_CELLS
    shape = (len(cells), 10, 18, 6) if where == "cut" else (len(cells),) + jh.SEAM_SHAPES["chunk_seam"][1:]
    sp = jh.split(shape)
    if where == "cut":
        assert sp["tSeg"] == 9 and sp["nTSeg"] == 2
    else:
        assert sp["nCh"] == 2 and sp["nt"] == 320 and 21 * shape[1] + 20 == 4 * 320
    route = route_of(eq, shape[3], "rescaled", jh.K_BIG)
    x, g = seam_inputs(route, shape, boundary, seed=6)
    clean = x.clone()
    for p, c in enumerate(cells):
        x[(p, 1) + c] = float("nan")
    got = jh.to_logical(losses.residual_vjp(route.method, jh.vars_on(x, gpu), g.to(gpu), boundary=boundary, jorek=True)).cpu().numpy()
    assert losses.last_route() == fused_route(route)
    must = ~np.isfinite(ref_vjp(route, x.double(), g.double(), boundary).numpy())             # non-zero taps only
    assert must.any() and not must[:, 1].any()                     # (no equation's d phi reads phi)
    diagonal = [(p, ch) + (c[0] + dt, c[1] + dx, c[2]) for p, c in enumerate(cells) for ch in (0, 2) for dt in (-1, 1) for dx in (-1, 1)
                if 0 <= c[0] + dt < shape[1] and 0 <= c[1] + dx < shape[2]]
    assert sum(bool(must[d]) for d in diagonal) >= len(cells), "the reference's set has no diagonal cell: restate the case"
    bad = ~np.isfinite(got)
    assert not (must & ~bad).any(), f"a NaN the reference propagates was hidden, e.g. at {np.argwhere(must & ~bad)[:4].tolist()}"
    assert not (bad & ~must).any(), f"a NaN outside the reference's set, e.g. at {np.argwhere(bad & ~must)[:4].tolist()}"
    ref = ref_vjp(route, clean.double(), g.double(), boundary).numpy()
    err = np.max(np.abs(got[~must] - ref[~must])) / np.max(np.abs(ref))
    print(f"{route.name} {where} boundary={boundary}: {int(must.sum())} non-finite cells, rel err elsewhere {err:.2e}")
    assert err <= TOL


# ------------------------------------------------------------------ (4), (5) the crop on load; the same bytes twice
def entry_run(route, gfull, x, gpu, crop, host_scale=1.0):
    """``vjp_jorek`` on the uncropped ``gfull`` [B,Nt,Nx,Ny] and the logical ``x`` -> the gradient in ``vars``' layout (CPU)"""
    from cp_pre_amd import losses
    spec = losses._Spec(route.method, False, True)
    xd = jh.vars_on(x, gpu)
    why, ks = spec.prepare_jorek(xd)
    assert why is None
    gd = gfull.permute(0, 2, 3, 1).contiguous().to(gpu).permute(0, 3, 1, 2)
    out = spec.vjp_jorek(ks, gd, xd, crop, host_scale, None)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("eq", jh.EQS)
def test_nonfinite_g_on_the_rim_changes_no_bit_under_the_crop(gpu, eq):
    for name in ("straddle_10", "chunk_seam", "two_marches"):
        shape = jh.SEAM_SHAPES[name]
        route = route_of(eq, shape[3], "default", jh.K_BIG)
        x, _ = seam_inputs(route, shape, True, seed=2)
        g = torch.randn(shape, generator=torch.Generator().manual_seed(3))
        rim = rim_mask(shape)
        zeros = g.clone()
        zeros[rim] = 0.0
        want = entry_run(route, zeros, x, gpu, True, 0.25)
        assert torch.isfinite(want).all()
        assert torch.equal(sg.bits(want), sg.bits(entry_run(route, zeros, x, gpu, False, 0.25)))
        for bad in (float("nan"), float("inf"), float("-inf")):
            spoiled = g.clone()
            spoiled[rim] = bad
            got = entry_run(route, spoiled, x, gpu, True, 0.25)
            assert torch.equal(sg.bits(got), sg.bits(want)), (eq, shape, bad)
        # without the crop the same g does reach the result (the test would notice a kernel that ignores the rim)
        assert not torch.isfinite(entry_run(route, spoiled, x, gpu, False, 0.25)).all()


@pytest.mark.parametrize("eq", jh.EQS)
def test_two_runs_give_the_same_bytes(gpu, eq):
    for name in ("chunk_seam", "one_plane_last_march"):
        shape = jh.SEAM_SHAPES[name]
        route = route_of(eq, shape[3], "rescaled", jh.K_BIG)
        x, _ = seam_inputs(route, shape, True, seed=3)
        g = torch.randn(shape, generator=torch.Generator().manual_seed(4))
        a = entry_run(route, g, x, gpu, False, 0.5)
        b = entry_run(route, g, x, gpu, False, 0.5)
        assert torch.equal(sg.bits(a), sg.bits(b)), (eq, shape)


# ------------------------------------------------------------------ (6) the kernels the operators hold now
@pytest.mark.parametrize("eq", jh.EQS)
def test_loss_applies_the_kernels_its_operators_hold_now(gpu, eq):
    """a tap changed in place between two calls (no new tensor identity) is the one the next forward AND backward apply"""
    from cp_pre_amd import losses
    shape = jh.SEAM_SHAPES["two_marches"]
    route = jh.JorekRoute(eq, shape[3], "rescaled", K=jh.K_BIG, device=gpu)
    x, _ = seam_inputs(route, shape, True, seed=7)

    def step():
        pred = jh.vars_on(x, gpu).requires_grad_(True)
        loss = losses.pi_loss(route.method, pred, jorek=True)
        loss.backward()
        assert losses.last_route() == fused_route(route)
        v64, g64 = ref_loss(route, x.double(), False)              # (from the taps the operators hold now)
        assert abs(float(loss.detach()) - v64) <= TOL * abs(v64), "the loss applied other taps"
        check_grad(route, pred.grad, g64, "after a tap update")
        return float(loss.detach())
    l0 = step()
    for op, idx in ((route.obj.D_R, (1, 2, 1)), (route.obj.D_Z, (2, 1, 1)), (route.obj.D_t, (0, 1, 1))):
        assert op.kernel.is_cuda and float(op.kernel[idx]) != 0.0
        op.kernel.data[idx] *= 1.75
        l1 = step()
        assert l1 != l0
        l0 = l1


# ------------------------------------------------------------------ (7) declines, each with the correct gradient
@pytest.mark.parametrize("eq", jh.EQS)
def test_declines_have_their_reasons_and_the_correct_gradient(gpu, eq):
    from cp_pre_amd import losses

    def run(route, xd, g, **kw):
        return losses.residual_vjp(route.method, xd, g.to(gpu), jorek=True, **kw)
    for shape, why in jh.DECLINED_SHAPES.items():                  # Nt = 96; Ny*Nt % 4 != 0
        route = route_of(eq, shape[3], "default", jh.K_BIG)
        x, g, want = case(route, shape, False)
        got = run(route, jh.vars_on(x, gpu), g)
        assert losses.last_route() == why
        check_grad(route, got, want, why)
    shape = jh.SEAM_SHAPES["one_chunk_one_march"]
    route = jh.JorekRoute(eq, shape[3], K=jh.K_BIG)
    x, g, want = case(route, shape, False)
    # a t-slab of a longer tensor: Nt-fastest, rows not dense
    long = torch.zeros(x.shape[0], 3, shape[2], shape[3], shape[1] + 2)
    long[..., :shape[1]] = jh.to_vars(x)
    slab = long.to(gpu)[..., :shape[1]]
    assert slab.stride(-1) == 1 and slab.stride(-2) == shape[1] + 2
    got = run(route, slab, g)
    assert losses.last_route() == "fallback:rows of the fields not dense"
    check_grad(route, got, want, "a t-slab")
    # the permuted view of memory [BS,F,Nt,Nx,Ny]: the field views are Ny-fastest
    nyf = jh.to_vars(x.to(gpu))
    assert nyf.stride(3) == 1 and nyf.stride(4) != 1
    got = run(route, nyf, g)
    assert losses.last_route() == "fallback:fields not Nt-fastest"
    check_grad(route, got, want, "Ny-fastest")
    # operators the library is not built for
    for opset in jh.DECLINED_SETS:
        other = jh.JorekRoute(eq, shape[3], opset, K=jh.K_BIG)
        xo, go, wo = case(other, shape, False)
        got = run(other, jh.vars_on(xo, gpu), go)
        assert losses.last_route() == "fallback:declined by the library", opset
        check_grad(other, got, wo, opset)
    # without the keyword: the parent's answer
    xd = jh.vars_on(x, gpu)
    got = losses.residual_vjp(route.method, xd, g.to(gpu))
    assert losses.last_route() == "fallback:no fused VJP for JOREK"
    check_grad(route, got, want, "no keyword")
    got = losses.residual_vjp(route.method, xd, g.to(gpu), flat=True, mhd="flat")
    assert losses.last_route() == "fallback:no fused VJP for JOREK"
    loss = losses.pi_loss(route.method, xd.clone().requires_grad_(True))
    assert losses.last_route() == "fallback:no fused VJP for JOREK" and loss.requires_grad
    # whatever ``flat`` says
    a, b = run(route, xd, g, flat=True), run(route, xd, g)
    assert losses.last_route() == fused_route(route) and torch.equal(sg.bits(a), sg.bits(b))
    # a kernel that requires grad (last: the route object is spent)
    route.obj.D_Z.kernel.requires_grad_(True)
    got = run(route, xd, g)
    assert losses.last_route() == "fallback:operator kernel requires grad"
    check_grad(route, got, want, "a kernel that requires grad")


# ------------------------------------------------------------------ (8) the C client
def test_c_client_on_the_device(gpu, tmp_path):
    exe = tmp_path / "vjpjorek_check"
    subprocess.check_call(c_client_command(exe), stderr=subprocess.DEVNULL)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "no device" not in r.stdout, r.stdout + r.stderr
