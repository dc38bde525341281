"""Physics-informed residual losses on the MI355X (cp_pre_amd.losses, libcp_pre_vjp.so): ``residual_vjp``, ``pi_loss`` and
``pisl_loss`` - values and gradients - against torch autograd on the CPU through oracle/residuals.py (the reference's own
F.conv3d / F.conv2d arithmetic), under the tolerance every residual and gradient test of this suite uses."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import residuals as orr
from losses_helpers import D, ns_kernels

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, DX, DY, NU = 0.01, 1 / 64, 1 / 32, 0.001
BDX, BDT, BNU = 0.05, 0.01, 0.002


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def _R():
    from cp_pre_amd import residuals as R
    return R


# name -> (method factory, oracle fn(x, boundary), input shape maker (BS, Nt, Nx, Ny) -> shape)
def _cases():
    R = _R()
    from cp_pre_amd.convops_1d import ConvOperator as ConvOperator1D
    from oracle.convops import ConvOperator1D as OracleOp1D
    ns = R.NavierStokes(DT, DX, DY, nu=NU)
    op1, oop1 = ConvOperator1D("x", 2), OracleOp1D("x", 2)

    def op1_oracle(x, b):
        r = oop1(x)
        return r if b else r[..., 1:-1, 1:-1]
    return {
        "pre_ns": (R.PRE_NS(DT, DX, DY).residual, lambda x, b: orr.ns_momentum(x, DT, DX, DY, 0.001, boundary=b), lambda s: (s[0], 3) + s[1:]),
        "op1d": (op1, op1_oracle, lambda s: (s[0] * s[1],) + s[2:]),
        "ns_momentum": (ns.residual_momentum, lambda x, b: orr.ns_momentum(x, DT, DX, DY, NU, boundary=b), lambda s: (s[0], 3) + s[1:]),
        "ns_continuity": (ns.residual_continuity, lambda x, b: orr.ns_continuity(x, DX, DY, boundary=b), lambda s: (s[0], 2) + s[1:]),
        "burgers": (R.Burgers(BDX, BDT, BNU).residual, lambda x, b: orr.burgers_residual(x, BDX, BDT, BNU, boundary=b), lambda s: (s[0] * s[1],) + s[2:]),
        "wave": (R.PRE_Wave(0.01, 0.02).residual, lambda x, b: orr.wave_residual(x, 1.0, 0.01, 0.02, boundary=b), lambda s: s),
        "advection": (R.Advection(1.0, 0.005, 0.01).residual, lambda x, b: orr.advection_residual(x, 1.0, 2, 0.005, 0.01, boundary=b),
                      lambda s: (s[0] * s[1],) + s[2:]),
    }


def _oracle_vjp(fn, x, boundary, g):
    x = x.clone().requires_grad_(True)
    fn(x, boundary).backward(g)
    return x.grad


def _check_vjp(name, shape, boundary, gpu, stacked=False, seed=0):
    from cp_pre_amd import losses
    method, oracle, mk = _cases()[name]
    torch.manual_seed(seed)
    x = torch.rand(mk(shape)) + 0.5
    with torch.no_grad():
        y = oracle(x, boundary)
    g = torch.randn(y.shape)
    want = _oracle_vjp(oracle, x, boundary, g) if g.numel() else torch.zeros_like(x)
    if stacked and x.dim() == 5:                 # the vars[:, i] views of a larger stacked tensor
        big = torch.zeros((x.shape[0], x.shape[1] + 2) + tuple(x.shape[2:]), device=gpu)
        big[:, 1:-1] = x.to(gpu)
        xd = big[:, 1:-1]
    else:
        xd = x.to(gpu)
    got = losses.residual_vjp(method, xd, g.to(gpu), boundary=boundary)
    assert got.shape == x.shape and got.is_cuda
    err = rel_err(got.cpu().numpy(), want.numpy())
    print(f"{name} {shape} boundary={boundary} stacked={stacked}: route {losses.last_route()}, rel err {err:.2e}")
    assert losses.last_route() == "fused:" + {"ns_momentum": "ns_momentum", "ns_continuity": "linear2", "burgers": "burgers",
                                              "wave": "stencil3d", "advection": "stencil2d", "pre_ns": "ns_momentum",
                                              "op1d": "stencil2d"}[name]
    assert err <= TOL, (name, shape, boundary, err)


@pytest.mark.parametrize("name", ["ns_momentum", "ns_continuity", "burgers", "wave", "advection", "pre_ns", "op1d"])
@pytest.mark.parametrize("boundary", [False, True])
def test_residual_vjp_matches_oracle_autograd(gpu, name, boundary):
    for shape in ((2, 6, 10, 16), (2, 5, 9, 13), (1, 4, 12, 510), (2, 3, 8, 256)):       # tail widths 13 / 510, minimum Nt = 3
        _check_vjp(name, shape, boundary, gpu)
    _check_vjp(name, (2, 6, 10, 16), boundary, gpu, stacked=True)


@pytest.mark.parametrize("name", ["ns_momentum", "ns_continuity", "wave"])
@pytest.mark.parametrize("nt", [1, 2])
def test_residual_vjp_degenerate_extents(gpu, name, nt):
    """Nt = 1, 2: with the crop nothing is left to average over (an empty g, a zero gradient); uncropped they are grids
    like any other"""
    for boundary in (False, True):
        _check_vjp(name, (2, nt, 9, 16), boundary, gpu)


@pytest.mark.parametrize("name", ["burgers", "advection", "op1d"])
@pytest.mark.parametrize("nt", [1, 2])
def test_residual_vjp_degenerate_extents_2d(gpu, name, nt):
    """the same for the [BS,Nt,Nx] views: Nt = 1, 2"""
    for boundary in (False, True):
        _check_vjp(name, (3, 1, nt, 16), boundary, gpu)


def test_residual_vjp_rescaled_and_general_star_kernels(gpu):
    from cp_pre_amd import losses
    R = _R()
    ns = R.NavierStokes(DT, DX, DY, nu=NU)
    ns.D_x.kernel = 2 * ns.D_x.kernel
    star = torch.zeros(3, 3, 3)
    for i, idx in enumerate(((1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2))):
        star[idx] = 0.3 * (i + 1) * (-1) ** i
    ns.D_y.kernel = star                                             # a general 7-point star: every tap, all unequal
    # (the base kernels are the ORACLE's: that cp_pre_amd's NS operators are built equal to them is pinned by the kernel
    # goldens of tests/test_oracle_golden.py / test_host_cpu.py, and by every unscaled case above)
    Kt, Kx, Ky, KL = (k.float() for k in ns_kernels())
    Kx, Ky = 2 * Kx, star.clone()

    def ref(x):                                                       # the oracle's expression with these kernels
        u, v, p = x[:, 0], x[:, 1], x[:, 2]
        rx = D(u, Kt)*DX*DY + u*D(u, Kx)*DT*DY + v*D(u, Ky)*DT*DX - NU*D(u, KL)*DT + D(p, Kx)*DT*DY
        ry = D(v, Kt)*DX*DY + u*D(v, Kx)*DT*DX + v*D(v, Ky)*DT*DY - NU*D(v, KL)*DT + D(p, Ky)*DT*DX
        return rx + ry
    torch.manual_seed(3)
    x = torch.rand(2, 3, 6, 10, 20) + 0.5
    g = torch.randn(2, 6, 10, 20)
    xr = x.clone().requires_grad_(True)
    ref(xr).backward(g)
    got = losses.residual_vjp(ns.residual_momentum, x.to(gpu), g.to(gpu), boundary=True)
    assert losses.last_route() == "fused:ns_momentum"
    assert rel_err(got.cpu().numpy(), xr.grad.numpy()) <= TOL
    # a general star as a single operator
    from cp_pre_amd.convops_2d import ConvOperator
    op = ConvOperator()
    op.kernel = star.clone()
    f = torch.rand(2, 6, 10, 20)
    fr = f.clone().requires_grad_(True)
    D(fr, star).backward(g)
    got = losses.residual_vjp(op, f.to(gpu), g.to(gpu), boundary=True)
    assert losses.last_route() == "fused:stencil3d"
    assert rel_err(got.cpu().numpy(), fr.grad.numpy()) <= TOL


def test_residual_vjp_fallbacks_still_match(gpu):
    from cp_pre_amd import losses
    from cp_pre_amd.convops_2d import ConvOperator
    torch.manual_seed(4)
    # a kernel with a tap off the star
    box = torch.zeros(3, 3, 3)
    box[1, 1, 1], box[0, 0, 1], box[2, 1, 2] = 1.0, -0.5, 0.25
    op = ConvOperator()
    op.kernel = box.clone()
    f, g = torch.rand(2, 6, 10, 20), torch.randn(2, 6, 10, 20)
    fr = f.clone().requires_grad_(True)
    D(fr, box).backward(g)
    got = losses.residual_vjp(op, f.to(gpu), g.to(gpu), boundary=True)
    assert losses.last_route().startswith("fallback:")
    assert rel_err(got.cpu().numpy(), fr.grad.numpy()) <= TOL
    # the surrogate's Nt-fastest layout
    method, oracle, _ = _cases()["ns_momentum"]
    x = torch.rand(2, 3, 8, 10, 16) + 0.5
    with torch.no_grad():
        y = oracle(x, False)
    g = torch.randn(y.shape)
    want = _oracle_vjp(oracle, x, False, g)
    xt = x.to(gpu).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    got = losses.residual_vjp(method, xt, g.to(gpu), boundary=False)
    assert losses.last_route().startswith("fallback:")
    assert rel_err(got.cpu().numpy(), want.numpy()) <= TOL


def _loss64(r):
    return float(np.mean(np.asarray(r, np.float64) ** 2)) if r.numel() else float("nan")


@pytest.mark.parametrize("name", ["ns_momentum", "ns_continuity", "burgers", "wave", "advection"])
@pytest.mark.parametrize("boundary", [False, True])
def test_pi_and_pisl_loss_value_and_gradient(gpu, name, boundary):
    from cp_pre_amd import losses
    method, oracle, mk = _cases()[name]
    torch.manual_seed(5)
    for shape in ((2, 6, 10, 16), (2, 5, 9, 13)):
        x = torch.rand(mk(shape)) + 0.5
        yy = x + 0.1 * torch.rand(mk(shape))
        # PI
        xr = x.clone().requires_grad_(True)
        lref = oracle(xr, boundary).pow(2).mean()
        lref.backward()
        xd = x.to(gpu).requires_grad_(True)
        loss = losses.pi_loss(method, xd, boundary=boundary)
        assert losses.last_route().startswith("fused:") and loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
        loss.backward()
        want = _loss64(oracle(x, boundary))
        print(f"pi {name} {shape} b={boundary}: loss {float(loss.detach()):.6e} (fp64 {want:.6e}), grad err {rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()):.2e}")
        assert abs(float(loss.detach()) - want) <= TOL * abs(want)
        assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) <= TOL
        # lp + 1000 * PISL: an upstream gradient other than 1, on the device
        xr = x.clone().requires_grad_(True)
        (xr.pow(2).mean() + 1000 * (oracle(xr, boundary) - oracle(yy, boundary)).pow(2).mean()).backward()
        xd = x.to(gpu).requires_grad_(True)
        pisl = losses.pisl_loss(method, xd, yy.to(gpu), boundary=boundary)
        assert losses.last_route().startswith("fused:")
        (xd.pow(2).mean() + 1000 * pisl).backward()
        want = _loss64(oracle(x, boundary) - oracle(yy, boundary))
        print(f"pisl {name} {shape} b={boundary}: loss {float(pisl.detach()):.6e} (fp64 {want:.6e}), grad err {rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()):.2e}")
        assert abs(float(pisl.detach()) - want) <= TOL * abs(want)
        assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) <= TOL


def test_loss_through_a_non_leaf_reaches_the_model_weights(gpu):
    from cp_pre_amd import losses
    method, oracle, _ = _cases()["ns_momentum"]
    torch.manual_seed(6)
    conv = torch.nn.Conv3d(3, 3, 3, padding=1)
    x = torch.rand(2, 3, 6, 10, 16) + 0.5
    yy = torch.rand(2, 3, 6, 10, 16) + 0.5
    pred = conv(x) + 1.0
    (1000 * (oracle(pred, False) - oracle(yy, False)).pow(2).mean()).backward()
    wref, bref = conv.weight.grad.clone(), conv.bias.grad.clone()
    conv.zero_grad()
    convd = torch.nn.Conv3d(3, 3, 3, padding=1).to(gpu)
    convd.load_state_dict(conv.state_dict())
    predd = convd(x.to(gpu)) + 1.0
    (1000 * losses.pisl_loss(method, predd, yy.to(gpu))).backward()
    assert losses.last_route() == "fused:ns_momentum"
    # (the device convolution's own backward is in the chain: MIOpen against the CPU's, same tolerance)
    assert rel_err(convd.weight.grad.cpu().numpy(), wref.numpy()) <= TOL
    assert rel_err(convd.bias.grad.cpu().numpy(), bref.numpy()) <= TOL


@pytest.mark.parametrize("name", ["ns_momentum", "burgers", "wave"])
def test_pisl_of_a_field_with_itself_is_exactly_zero(gpu, name):
    from cp_pre_amd import losses
    method, _, mk = _cases()[name]
    torch.manual_seed(7)
    x = (torch.rand(mk((2, 6, 10, 16))) + 0.5).to(gpu).requires_grad_(True)
    loss = losses.pisl_loss(method, x, x.detach().clone())
    loss.backward()
    assert losses.last_route().startswith("fused:")
    assert float(loss.detach()) == 0.0 and not x.grad.any()


@pytest.mark.parametrize("name", ["ns_momentum", "burgers"])
def test_loss_and_gradient_are_bit_identical_run_to_run(gpu, name):
    from cp_pre_amd import losses
    method, _, mk = _cases()[name]
    torch.manual_seed(8)
    x = torch.rand(mk((4, 12, 40, 264))) + 0.5
    out = []
    for _ in range(2):
        xd = x.to(gpu).requires_grad_(True)
        loss = losses.pi_loss(method, xd)
        loss.backward()
        out.append((loss.detach().cpu().numpy().tobytes(), xd.grad.cpu().numpy().tobytes()))
    assert out[0] == out[1]


def test_fused_backward_runs_without_the_recompute_route(gpu, monkeypatch):
    from cp_pre_amd import _dispatch, losses

    def boom(ctx, gout):
        raise AssertionError("the composed backward ran")
    monkeypatch.setattr(_dispatch._Recompute, "backward", staticmethod(boom))
    for name in ("ns_momentum", "burgers"):
        method, oracle, mk = _cases()[name]
        x = torch.rand(mk((2, 6, 10, 16))) + 0.5
        xr = x.clone().requires_grad_(True)
        oracle(xr, False).pow(2).mean().backward()
        xd = x.to(gpu).requires_grad_(True)
        losses.pi_loss(method, xd).backward()
        assert losses.last_route() == "fused:" + name
        assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) <= TOL


def test_mhd_energy_loss_takes_the_fallback_and_matches(gpu):
    from cp_pre_amd import losses
    mhd = _R().MHD()
    torch.manual_seed(9)
    x = torch.rand(2, 6, 6, 10, 16) + 0.5
    xr = x.clone().requires_grad_(True)
    lref = orr.mhd_energy(xr, boundary=False).pow(2).mean()
    lref.backward()
    xd = x.to(gpu).requires_grad_(True)
    loss = losses.pi_loss(mhd.residual_energy, xd)
    loss.backward()
    assert losses.last_route().startswith("fallback:")
    assert abs(float(loss.detach()) - float(lref.detach())) <= TOL * abs(float(lref.detach()))
    assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) <= TOL


def test_ns_momentum_loss_step_memory(gpu):
    """A bound that follows from the design: over forward + backward the loss allocates one saved residual and three
    gradients = 4 single-field tensors; the fifth is room for the sum's workspace and the allocator's rounding.  (The
    route this replaces - residual_momentum(v).pow(2).mean().backward() through the composed expression - keeps a saved
    tensor for most of its ~30 elementwise and stencil results alive at once; it is not run at this size here.)"""
    from cp_pre_amd import losses
    ns = _R().NavierStokes(DT, DX, DY, nu=NU)
    BS, Nt, Nx, Ny = 8, 32, 256, 256
    field = BS * Nt * Nx * Ny * 4
    x = (torch.rand(BS, 3, Nt, Nx, Ny, device=gpu) + 0.5).requires_grad_(True)
    losses.pi_loss(ns.residual_momentum, x[:1].detach())             # (libraries loaded, kernels' code objects resident)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = losses.pi_loss(ns.residual_momentum, x)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak over forward + backward: {peak / field:.3f} single-field tensors")
    assert losses.last_route() == "fused:ns_momentum"
    assert x.grad is not None and peak <= 5 * field


def test_c_client_on_the_device(gpu, tmp_path):
    exe = tmp_path / "vjp_check"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "c_abi", "vjp_check.c"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_vjp.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
