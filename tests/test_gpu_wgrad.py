"""GPU tests of the fused kernel gradient of the residual losses (``wgrad=True`` / ``kernel_vjp`` of cp_pre_amd.losses,
libcp_pre_wgrad.so) on the MI355X (pytest -m gpu): ``kernel_vjp`` at the seams tests/wgrad_helpers.py names from the
kernel's own rule, against the float64 reference under the derived bound (L + 4) 2^-24 S per tap; the mask by select;
determinism; the losses with ``wgrad=True``; the fallbacks; the refusals through ctypes; the C client.
tests/WGRAD_TESTS.md records what they showed."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import wgrad_helpers as wh
from losses_helpers import Route
from test_wgrad_cpu import c_client_command

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_wgrad()
    return torch.device("cuda:0")


def operator(ext, device):
    """a ConvOperator of the family ``ext`` belongs to, holding a dense kernel of that extent (dk does not depend on it)"""
    from cp_pre_amd.convops_1d import ConvOperator as C1
    from cp_pre_amd.convops_2d import ConvOperator as C2
    op = C2() if len(ext) == 3 else C1()
    op.kernel = torch.ones(ext, device=device)
    return op


def logical(shape, ext):
    """the kernel-axes shape (B,T,X,Y) as the input of an operator with ``ext``: the VIEW3D form marches the batch"""
    return shape if len(ext) == 3 else (shape[0] * shape[1],) + tuple(shape[2:])


def check(losses, op, g, x, y, ext, boundary, dev, put=lambda t, d: t.to(d), label=""):
    """kernel_vjp on the device against ref_dk; returns the worst ratio to the bound"""
    crop = (slice(None),) + (slice(None) if boundary else slice(1, -1),) * len(ext)
    gc = g[crop].contiguous()
    dk = losses.kernel_vjp(op, put(x, dev), gc.to(dev), boundary=boundary, minus=None if y is None else put(y, dev))
    assert losses.last_route().startswith("fused:") and losses.last_route().endswith("+wgrad"), (label, losses.last_route())
    gfull = torch.zeros_like(g)
    gfull[crop] = gc
    dk64, S = wh.ref_dk(gfull, x, y, ext, False)
    ratio = wh.worst_ratio(dk, dk64, S)
    assert ratio <= 1.0, (label, ratio, dk.cpu(), dk64)
    return ratio


# ------------------------------------------------------------------ kernel_vjp at the seams
@pytest.mark.parametrize("ext", [(3, 3, 3), (3, 1, 1), (1, 3, 3), (3, 3)], ids=str)
def test_kernel_vjp_matches_fp64_at_the_seams(gpu, ext):
    from cp_pre_amd import losses
    op = operator(ext, gpu)
    worst = 0.0
    for name, shape in wh.SEAM_SHAPES.items():
        shp = logical(shape, ext)
        g, x, y = wh.inputs(shp, seed=1)
        for boundary in (False, True):
            for yy in ((None, y) if name in ("base", "Y=33", "T=9", "X=33") else (None,)):
                r = check(losses, op, g, x, yy, ext, boundary, gpu, label=(name, boundary, yy is not None))
                worst = max(worst, r)
    print(f"kernel_vjp {ext}: worst |dk - dk64| / ((L + 4) 2^-24 S) = {worst:.3f}")


def test_kernel_vjp_with_an_empty_interior_is_exactly_zero(gpu):
    """T == 2 under the crop leaves no cell: every tap has S == 0 and is exactly 0 - by the launch, not by a host shortcut"""
    from cp_pre_amd import _lib
    g, x, _ = wh.inputs((2, 2, 10, 16))
    dk = raw(_lib, g.to(gpu), x.to(gpu), None, (3, 3, 3), _lib.PRE_VJP_CROP)
    assert torch.equal(dk.cpu(), torch.zeros(3, 3, 3))


@pytest.mark.parametrize("ext", [(3, 3, 3), (1, 3, 3), (3, 3)], ids=str)
def test_kernel_vjp_reads_views_where_they_lie(gpu, ext):
    from cp_pre_amd import losses
    op = operator(ext, gpu)
    shp = logical(wh.BASE, ext)
    g, x, y = wh.inputs(shp, seed=2)

    def pitched(t, d):                                    # vars[:, 0] of a stacked [B,2,...] tensor
        big = torch.full((t.shape[0], 2) + tuple(t.shape[1:]), float("nan"), device=d)
        big[:, 0] = t.to(d)
        return big[:, 0]
    worst = max(check(losses, op, g, x, yy, ext, b, gpu, pitched, "pitched") for b in (False, True) for yy in (None, y))
    if len(ext) == 3:
        def ntfast(t, d):                                 # permute(0,3,1,2) of a dense [B,X,Y,T]
            return t.to(d).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

        def script(t, d):                                 # the cropped view of the reference's scripts: rows not dense
            big = torch.full((t.shape[0], 1, t.shape[2] + 2, t.shape[3] + 2, t.shape[1] + 2), float("nan"), device=d)
            big[:, 0, 1:-1, 1:-1, 1:-1] = t.to(d).permute(0, 2, 3, 1)
            return big[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2)
        assert (wh.BASE[3] * wh.BASE[1]) % 4 == 0
        for put, label in ((ntfast, "ntfast"), (script, "script view")):
            assert put(x, gpu).stride(1) == 1
            for b in (False, True):
                for yy in (None, y):
                    worst = max(worst, check(losses, op, g, x, yy, ext, b, gpu, put, label))
                    assert losses.last_route() == "fused:flat_stencil3d+wgrad"
    print(f"kernel_vjp {ext} on views: worst ratio {worst:.3f}")


# ------------------------------------------------------------------ the entry through ctypes
def raw(_lib, g, x, y, ext, flags, dk=None, ws=None, scale=1.0, dev_scale=None, shape=None, fields=None):
    """one pre_wgrad_stencil3d_f32 call on 4-D device views; returns dk (or the return code when ``fields`` / a refusal)"""
    lib = _lib.load_wgrad()
    ws = torch.empty(_lib.PRE_WGRAD_WORKSPACE, dtype=torch.float64, device=x.device) if ws is None else ws
    out = torch.full(ext, 7.0, device=x.device) if dk is None else dk
    fs = [ctypes.byref(_lib.field(v)) if v is not None else None for v in (g, x, y)]
    rc = lib.pre_wgrad_stencil3d_f32(*fs, *ext, float(scale), _lib.ptr(dev_scale), *(shape or x.shape), flags, _lib.ptr(ws),
                                     _lib.ptr(out), _lib.stream())
    if dk is not None:
        return rc
    assert rc == 0, rc
    return out


def test_mask_is_a_select_on_g(gpu):
    from cp_pre_amd import _lib
    g, x, y = wh.inputs(wh.BASE, seed=4)
    rim = wh.mask(wh.BASE, (1, 2, 3)) == 0
    g0, gn = g.clone(), g.clone()
    g0[rim] = 0.0
    gn[rim] = float("nan")
    gn[:, 0] = float("inf")
    for lay in (lambda t: t.to(gpu), lambda t: t.to(gpu).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):
        a = raw(_lib, lay(g0), lay(x), lay(y), (3, 3, 3), _lib.PRE_VJP_CROP)
        b = raw(_lib, lay(gn), lay(x), lay(y), (3, 3, 3), _lib.PRE_VJP_CROP)
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    # [B,T,X] as [1,B,T,X]: the crop runs on T and X only, samples 0 and B-1 count
    g3, x3, _ = wh.inputs((4, 10, 16), seed=5)
    dk = raw(_lib, g3.to(gpu)[None], x3.to(gpu)[None], None, (1, 3, 3), _lib.PRE_VJP_CROP | _lib.PRE_VJP_VIEW3D)
    dk64, S = wh.ref_dk(g3, x3, None, (3, 3), True)
    assert wh.worst_ratio(dk[0], dk64, S) <= 1.0


def test_same_bytes_every_run_and_on_a_second_stream(gpu):
    from cp_pre_amd import _lib
    g, x, y = (t.to(gpu) for t in wh.inputs((3, 20, 70, 130), seed=6))
    up = torch.tensor([1000.0], device=gpu)
    runs = [raw(_lib, g, x, y, (3, 3, 3), _lib.PRE_VJP_CROP, scale=0.25, dev_scale=up) for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(raw(_lib, g, x, y, (3, 3, 3), _lib.PRE_VJP_CROP, scale=0.25, dev_scale=up))
    side.synchronize()
    torch.cuda.synchronize()
    assert all(r.cpu().numpy().tobytes() == runs[0].cpu().numpy().tobytes() for r in runs[1:])
    dk64, S = wh.ref_dk(g.cpu(), x.cpu(), y.cpu(), (3, 3, 3), True, 250.0)
    assert wh.worst_ratio(runs[0], dk64, S) <= 1.0


def test_refusals_launch_nothing(gpu):
    from cp_pre_amd import _lib
    g, x, _ = (None if t is None else t.to(gpu) for t in wh.inputs(wh.BASE))
    dk = torch.full((27,), 7.0, device=gpu)
    ws = torch.zeros(_lib.PRE_WGRAD_WORKSPACE, dtype=torch.float64, device=gpu)
    E = _lib
    null_field = _lib.PreField(0, 1, 1, 1, 1)
    lib = _lib.load_wgrad()
    call = lambda *a: lib.pre_wgrad_stencil3d_f32(*a, _lib.stream())                   # noqa: E731
    fg, fx = ctypes.byref(_lib.field(g)), ctypes.byref(_lib.field(x))
    tail = (1.0, None, *wh.BASE, 0, _lib.ptr(ws), _lib.ptr(dk))
    assert call(None, fx, None, 3, 3, 3, *tail) == E.PRE_E_NULL
    assert call(fg, ctypes.byref(null_field), None, 3, 3, 3, *tail) == E.PRE_E_NULL
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, *wh.BASE, 0, None, _lib.ptr(dk)) == E.PRE_E_NULL
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, *wh.BASE, 0, _lib.ptr(ws), None) == E.PRE_E_NULL
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, 2, 0, 10, 16, 0, _lib.ptr(ws), _lib.ptr(dk)) == E.PRE_E_NULL
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, 2, 1 << 31, 10, 16, 0, _lib.ptr(ws), _lib.ptr(dk)) == E.PRE_E_SHAPE
    assert call(fg, fx, None, 5, 3, 3, *tail) == E.PRE_E_UNSUPPORTED
    assert call(fg, fx, None, 3, 3, 2, *tail) == E.PRE_E_UNSUPPORTED
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, *wh.BASE, 8, _lib.ptr(ws), _lib.ptr(dk)) == E.PRE_E_UNSUPPORTED
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, *wh.BASE, _lib.PRE_VJP_VIEW3D, _lib.ptr(ws), _lib.ptr(dk)) == E.PRE_E_UNSUPPORTED
    odd = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)                        # unit stride on X: neither layout
    assert odd.stride(3) != 1 and odd.stride(1) != 1
    assert call(fg, ctypes.byref(_lib.field(odd)), None, 3, 3, 3, *tail) == E.PRE_E_UNSUPPORTED
    mixed = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                      # g Y-fastest, x Nt-fastest
    assert call(fg, ctypes.byref(_lib.field(mixed)), None, 3, 3, 3, *tail) == E.PRE_E_UNSUPPORTED
    inside = ctypes.c_void_p(x.data_ptr() + 4 * 100)
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, *wh.BASE, 0, _lib.ptr(ws), inside) == E.PRE_E_SHAPE
    assert call(fg, fx, None, 3, 3, 3, 1.0, None, *wh.BASE, 0, ctypes.c_void_p(g.data_ptr()), _lib.ptr(dk)) == E.PRE_E_SHAPE
    torch.cuda.synchronize()
    assert bool((dk == 7.0).all()) and bool((ws == 0).all())
    assert torch.equal(x.cpu(), wh.inputs(wh.BASE)[1])


# ------------------------------------------------------------------ the losses
LOSS_CASES = [("op3d", "dense"), ("op3d", "flat"), ("wave", "dense"), ("wave", "flat"), ("advection", "dense"), ("op2d", "dense")]


def loss_inputs(route, layout, dev, seed):
    shape = (2, 6, 10, 16) if route.nd == 3 else (4, 10, 16)
    _, x, y = wh.inputs(shape, seed=seed)
    put = (lambda t: t.to(dev)) if layout == "dense" else (lambda t: t.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    return x, y, put


@pytest.mark.parametrize("pisl", [False, True], ids=["pi", "pisl"])
@pytest.mark.parametrize("name,layout", LOSS_CASES)
def test_losses_with_wgrad(gpu, name, layout, pisl):
    from cp_pre_amd import losses
    route = Route(name, device=gpu)
    if name == "op3d":                                    # a ConvOperator holding the wave kernel
        route.ops[0].kernel = Route("wave", device=gpu).ops[0].kernel.clone()
    flat = layout == "flat"
    x, y, put = loss_inputs(route, layout, gpu, 7)
    yy = put(y) if pisl else None
    loss_fn = (lambda p, **kw: losses.pisl_loss(route.method, p, yy, flat=flat, **kw)) if pisl else \
        (lambda p, **kw: losses.pi_loss(route.method, p, flat=flat, **kw))
    kind = ("flat_" if flat else "") + route.kind
    # the same call with the kernel not requiring grad
    p0 = put(x).requires_grad_(True)
    l0 = loss_fn(p0)
    assert losses.last_route() == "fused:" + kind
    l0.backward()
    with torch.no_grad():
        r = route.method(put(x), boundary=True, minus=yy) if not route.method is route.obj else \
            (route.method(put(x)) if yy is None else route.method(put(x)) - route.method(yy))
    # the reference: g = the fp32 residual the launch reads, scale = fp32(2 / N) * upstream
    n = int(np.prod([s - 2 for s in x.shape[1:]])) * x.shape[0]
    ext = tuple(route.ops[0].kernel.shape)
    ref = lambda up: wh.ref_dk(r.cpu(), x, y if pisl else None, ext, True, float(np.float32(2.0 / n)) * up)   # noqa: E731
    route.ops[0].kernel.requires_grad_(True)
    k = route.ops[0].kernel
    # both require grad
    p1 = put(x).requires_grad_(True)
    l1 = loss_fn(p1, wgrad=True)
    assert losses.last_route() == "fused:" + kind + "+wgrad"
    l1.backward()
    assert torch.equal(l1.detach(), l0.detach()) and torch.equal(p1.grad, p0.grad)
    dk64, S = ref(1.0)
    r1 = wh.worst_ratio(k.grad, dk64, S)
    assert k.grad.shape == k.shape and r1 <= 1.0, (r1, k.grad, dk64)
    first = k.grad.clone()
    # a second backward on a fresh loss accumulates
    loss_fn(put(x).requires_grad_(True), wgrad=True).backward()
    assert torch.equal(k.grad, first + first)
    # only the kernel requires grad: the field VJP is skipped
    k.grad = None
    p2 = put(x)
    loss_fn(p2, wgrad=True).backward()
    assert losses.last_route() == "fused:" + kind + "+wgrad" and p2.grad is None and torch.equal(k.grad, first)
    # only pred requires grad: the route it took before
    k.requires_grad_(False)
    k.grad = None
    p3 = put(x).requires_grad_(True)
    loss_fn(p3, wgrad=True).backward()
    assert losses.last_route() == "fused:" + kind and torch.equal(p3.grad, p0.grad)
    # the upstream gradient reaches dk from the device
    k.requires_grad_(True)
    p4 = put(x).requires_grad_(True)
    lp = (p4 * p4).mean()
    (lp + 1000 * loss_fn(p4, wgrad=True)).backward()
    dk64, S = ref(1000.0)
    r2 = wh.worst_ratio(k.grad, dk64, S)
    assert r2 <= 1.0, r2
    print(f"{name} {layout} {'pisl' if pisl else 'pi'}: kernel.grad worst ratio to the bound {max(r1, r2):.3f}")


def test_fallbacks_say_why_and_still_give_the_autograd_gradient(gpu):
    from cp_pre_amd import losses
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_2d import ConvOperator as C2

    def both(method, kernel, x, why, without="operator kernel requires grad", **kw):
        grads = []
        for wg in (True, False):
            kernel.grad = None
            losses.pi_loss(method, x, wgrad=wg, **kw).backward()
            assert losses.last_route() == "fallback:" + (why if wg else without), losses.last_route()
            grads.append(kernel.grad.clone())
        kernel.grad = None
        (method(x)[:, 1:-1, 1:-1, 1:-1] if isinstance(method, C2) else method(x, boundary=False)).pow(2).mean().backward()
        for got in grads:
            assert torch.allclose(got, kernel.grad, rtol=1e-4, atol=1e-4 * float(kernel.grad.abs().max()))
    ns = R.NavierStokes(0.01, 1 / 64, 1 / 32, device=gpu)
    ns.D_x.kernel.requires_grad_(True)
    both(ns.residual_momentum, ns.D_x.kernel, torch.rand(2, 3, 6, 10, 16, device=gpu) + 0.5, "operator kernel requires grad")
    box = C2(("x", "y"), 2, device=gpu)
    box.kernel = torch.rand(3, 3, 3, device=gpu).requires_grad_(True)
    both(box, box.kernel, torch.rand(2, 6, 10, 16, device=gpu), "operator kernel off the 7-point star")
    adv = R.Advection(1.0, 0.005, 0.01, device=gpu)
    adv.D.kernel.requires_grad_(True)
    xt = torch.rand(4, 16, 10, device=gpu).permute(0, 2, 1)
    both(adv.residual, adv.D.kernel, xt, "no flat VJP for the 1-D family", without="no flat VJP for the 1-D family", flat=True)


# ------------------------------------------------------------------ the C client on the device
def test_wgrad_c_client_runs_on_the_device(gpu, tmp_path):
    exe = tmp_path / "wgrad_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "FAIL" not in out.stdout and "no device" not in out.stdout, out.stdout + out.stderr
