"""GPU tests of the fused compressible-NS right-hand side (``cp_pre_amd.cns.Euler_FV_OS_rhs``, libcp_pre_cns.so) against
the fp64 restatement of tests/cns_helpers.py and the golden fixture the reference's own ``forward`` produced.

``TOL`` = 1e-5 tensor-scale relative error per output channel (cns_helpers); tests/test_cns_cpu.py shows that the fp32
restatement alone stays within ``TOL / 4`` at every shape used here.  The shapes sit below, at and beyond every seam of
the kernel's tile (``cns.TILE``): all six row counts against all six column counts, for both batch sizes and every
boundary condition."""
import subprocess

import pytest
import torch

import cns_helpers as H
from conftest import load_golden
from test_cns_cpu import CONFIG, c_client_command

pytestmark = pytest.mark.gpu

CONDITIONS = {k: H.sides(k, 0.75 if k == "dirichlet" else 0.0) for k in H.BC_KINDS}
CONDITIONS.update(mixed=H.MIXED, mixed_fusable=H.MIXED_FUSABLE, true_wrap=H.TRUE_WRAP)
# (cns_helpers.MIXED: the last row's neighbour is row 1, a mapping pre_bc_t cannot express; served by the composed route)
ROUTE = {k: "fused:cns_rhs" for k in CONDITIONS}
ROUTE["mixed"] = "fallback:boundary condition without a fused mapping"


def module(bc="periodic", kernels=None, **kw):
    from cp_pre_amd.cns import Euler_FV_OS_rhs
    m = Euler_FV_OS_rhs(CONFIG, "cuda", **kw)
    for op in (m.gradient, m.divergence, m.laplace):
        for side, (kind, value) in H.sides(bc).items():
            op.bc.set_boundary_type(side, kind, value)
    if kernels is not None:
        set_kernels(m, kernels)
    return m


def set_kernels(m, kernels):
    ops = dict(zip(H.KERNEL_NAMES, m._operators()))
    for name, k in kernels.items():
        ops[name].kernel = k.detach().clone().cuda()


def tile():
    from cp_pre_amd.cns import TILE
    return TILE


def check(got, v, bc, kernels=None, what=""):
    err = H.channel_err(got, H.rhs64(v.cpu(), bc, kernels), H.zero_scale(v, kernels))
    print(f"{what}: channel error {err:.3e}")
    assert err <= H.TOL, what
    return err


# ------------------------------------------------------------------ shapes and boundary conditions
@pytest.mark.parametrize("bs", (1, 3))
@pytest.mark.parametrize("bc", list(CONDITIONS))
def test_fused_rhs_at_every_seam(bc, bs):
    from cp_pre_amd.cns import last_route
    m = module(CONDITIONS[bc])
    nxs, nys = H.gpu_extents(*tile())
    worst = 0.0
    for nx in nxs:
        for ny in nys:
            v = H.make_vars((bs, 4, nx, ny), seed=nx * 1000 + ny)
            got = m(v.cuda())
            assert last_route() == ROUTE[bc] and got.shape == v.shape and got.is_cuda
            err = H.channel_err(got, H.rhs64(v, CONDITIONS[bc]), H.zero_scale(v))
            assert err <= H.TOL, (nx, ny, err)
            worst = max(worst, err)
    print(f"{bc}, BS {bs}: worst channel error {worst:.3e}")


def test_fused_rhs_agrees_with_the_golden_fixture():
    from cp_pre_amd.cns import last_route
    g = load_golden("cns.npz")
    for bc, value in zip(g["bcs"], g["bc_values"]):
        m = module(H.sides(str(bc), float(value)))
        for i in range(2):
            got = m(torch.from_numpy(g[f"vars_{i}"]).cuda())
            assert last_route() == "fused:cns_rhs"
            err = H.channel_err(got, torch.from_numpy(g[f"rhs_{bc}_{i}"]))
            print(f"{bc} {i}: against the reference's forward {err:.3e}")
            assert err <= H.TOL, (bc, i)


def test_cpu_input_is_staged_through_the_gpu():
    from cp_pre_amd.cns import last_route
    v = H.make_vars((2, 4, 9, 12), seed=5)
    got = module()(v)
    assert last_route() == "fused:cns_rhs" and not got.is_cuda
    check(got, v, "periodic", what="cpu input")


# ------------------------------------------------------------------ the taps are the ones handed over
@pytest.mark.parametrize("bc", ("periodic", "mixed_fusable"))
def test_callers_kernels_are_the_taps(bc):
    from cp_pre_amd.cns import last_route
    nr, nc = tile()
    k = H.asymmetric_kernels()
    m = module(CONDITIONS[bc], k)
    v = H.make_vars((2, 4, nr + 1, nc + 4), seed=7)
    got = m(v.cuda())
    assert last_route() == "fused:cns_rhs"
    check(got, v, CONDITIONS[bc], k, "asymmetric crosses")
    assert H.channel_err(got, H.rhs64(v, CONDITIONS[bc])) > 100 * H.TOL          # (not the constructor's kernels)


def test_kernel_changed_between_two_calls_is_honoured():
    from cp_pre_amd.cns import last_route
    k = H.asymmetric_kernels()
    m = module("neumann", k)
    v = H.make_vars((1, 4, 9, 12), seed=8)
    check(m(v.cuda()), v, "neumann", k, "first call")
    m.gradient.grad_y.kernel.data.mul_(-3.0)                                     # in place: same tensor, same version counter
    m.laplace.laplace.kernel = (0.5 * k["lap"]).cuda()                           # replaced
    k2 = dict(k, gy=-3.0 * k["gy"], lap=0.5 * k["lap"])
    check(m(v.cuda()), v, "neumann", k2, "second call")
    assert last_route() == "fused:cns_rhs"


# ------------------------------------------------------------------ views
@pytest.mark.parametrize("bs", (1, 3))
def test_views_are_read_and_written_where_they_lie(bs):
    from cp_pre_amd.cns import last_route
    nr, nc = tile()
    nx, ny = nr + 1, nc + 4
    m = module(H.MIXED_FUSABLE)
    v = H.make_vars((bs, 4, nx, ny), seed=9).cuda()
    dense = m(v)
    big = torch.full((bs, 6, nx + 8, ny + 16), float("nan"), device="cuda")
    big[:, 1:5, 4:4 + nx, 8:8 + ny] = v
    sentinel = -12345.5
    buf = torch.full((bs, 6, nx + 8, ny + 16), sentinel, device="cuda")
    out = buf[:, 1:5, 4:4 + nx, 8:8 + ny]
    res = m(big[:, 1:5, 4:4 + nx, 8:8 + ny], out=out)
    assert last_route() == "fused:cns_rhs" and res.data_ptr() == out.data_ptr()
    assert torch.equal(out, dense) and not torch.isnan(out).any()
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, 1:5, 4:4 + nx, 8:8 + ny] = False
    assert bool((buf[mask] == sentinel).all())
    # without out: the same bits in a new dense tensor
    assert torch.equal(m(big[:, 1:5, 4:4 + nx, 8:8 + ny]), dense)


# ------------------------------------------------------------------ non-finite footprint
@pytest.mark.parametrize("bc", ("periodic", "mixed_fusable", "true_wrap"))
def test_nan_reaches_exactly_the_cells_of_the_restatement(bc):
    from cp_pre_amd.cns import last_route
    nr, nc = tile()
    nx, ny = nr + 2, nc + 4
    m = module(CONDITIONS[bc])
    clean = H.make_vars((1, 4, nx, ny), seed=10)
    cells = {"interior": (5, 9), "tile seam": (nr, nc), "corner 00": (0, 0), "corner 11": (nx - 1, ny - 1), "corner 01": (0, ny - 1),
             "top edge": (0, 9), "bottom edge": (nx - 1, 9), "left edge": (5, 0), "right edge": (5, ny - 1)}
    for name, (i, j) in cells.items():
        v = clean.clone()
        v[0, 1, i, j] = float("nan")
        got = m(v.cuda()).cpu()
        assert last_route() == "fused:cns_rhs"
        want = H.rhs64(v, CONDITIONS[bc])
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, torch.isnan(got).sum(), torch.isnan(want).sum())
        assert torch.isnan(want).any() and not torch.isinf(got).any()
        ok = ~torch.isnan(want)
        assert float((got[ok].double() - want[ok]).abs().max()) <= H.TOL * float(want[ok].abs().max()), name


# ------------------------------------------------------------------ the integrator epilogue
def step_err(got, v, base, h, bc):
    want = base.double().cpu() + h * H.rhs64(v.cpu(), bc)
    return H.channel_err(got, want)


def test_step_is_base_plus_h_rhs():
    from cp_pre_amd.cns import last_route
    nr, nc = tile()
    m = module(H.TRUE_WRAP)
    v = H.make_vars((3, 4, nr + 1, nc + 4), seed=11).cuda()
    h = 1e-4
    got = m.step(v, h)
    assert last_route() == "fused:cns_rhs+axpy" and got.data_ptr() != v.data_ptr()
    e0 = step_err(got, v, v, h, H.TRUE_WRAP)
    # a separate out
    out = torch.full_like(v, float("nan"))
    assert m.step(v, h, out=out) is out and torch.equal(out, got)
    # in place on a clone of vars: out is base
    y = v.clone()
    assert m.step(v, h, out=y, base=y) is y and torch.equal(y, got) and last_route() == "fused:cns_rhs+axpy"
    # another base
    base = H.make_vars(tuple(v.shape), seed=12).cuda()
    e1 = step_err(m.step(v, h, base=base), v, base, h, H.TRUE_WRAP)
    print(f"step: {e0:.3e}, with a base of its own {e1:.3e}")
    assert e0 <= H.TOL and e1 <= H.TOL


def test_step_refuses_out_on_vars():
    from cp_pre_amd import cns
    m = module()
    v = H.make_vars((2, 4, 9, 12), seed=13).cuda()
    keep = v.clone()
    with pytest.raises(ValueError, match="must not overlap vars"):
        m.step(v, 1e-3, out=v)
    big = torch.cat((v, v), dim=2)
    keep_big = big.clone()
    with pytest.raises(ValueError, match="must not overlap vars"):
        m.step(big[:, :, 0:9], 1e-3, out=big[:, :, 8:17])                       # shares one row
    torch.cuda.synchronize()
    assert torch.equal(v, keep) and torch.equal(big, keep_big)
    with pytest.raises(RuntimeError, match=r"vars \+ h\*forward\(vars\)"):
        m.step(v.clone().requires_grad_(), 1e-3)


# ------------------------------------------------------------------ refusals
def test_refusals_fall_back_with_their_reason(monkeypatch):
    from cp_pre_amd import cns, vector_convops_spatial as V

    def no_library():
        raise AssertionError("the library must not be reached")

    monkeypatch.setattr(cns._lib, "load_cns", no_library)
    # Ny = 6
    m = module("neumann")
    v = H.make_vars((2, 4, 9, 6), seed=14)
    got = m(v.cuda())
    assert cns.last_route() == "fallback:Ny % 4 != 0"
    check(got, v, "neumann", what="Ny = 6")
    # a view off by one float
    v = H.make_vars((2, 4, 9, 12), seed=15)
    flat = torch.zeros(v.numel() + 4, device="cuda")
    flat[1:1 + v.numel()] = v.cuda().reshape(-1)
    shifted = flat[1:1 + v.numel()].view(v.shape)
    assert shifted.data_ptr() % 16 == 4
    got = m(shifted)
    assert cns.last_route() == "fallback:misaligned view"
    check(got, v, "neumann", what="offset by one float")
    # a 5x5 Laplacian
    m = module("neumann")
    m.laplace = V.Laplace(scale=1 / (m.dx ** 2), taylor_order=4, boundary_cond="neumann", device="cuda", requires_grad=True)
    assert tuple(m.laplace.laplace.kernel.shape) == (5, 5)
    got = m(v.cuda())
    assert cns.last_route() == "fallback:5x5 / 7x7 Taylor stencil"
    k5 = dict(H.default_kernels(), lap=m.laplace.laplace.kernel.detach().cpu())
    g, d, _ = H.make_ops(H.default_kernels(), "neumann", torch.float64)
    from oracle.spatial import VectorOp
    lap5 = VectorOp("laplace", taylor_order=4, boundary_cond="neumann")
    lap5.lap = k5["lap"].double()
    want = H.expression(v.double(), g, d, lap5, H.gamma32().double())
    err = H.channel_err(got, want)
    print(f"5x5 Laplacian: {err:.3e}")
    assert err <= H.TOL
    # free_slip has no padding rule: the reference's expression cannot be formed (the operators' outputs shrink), here neither
    m = module("neumann")
    for op in (m.gradient, m.divergence, m.laplace):
        op.bc.set_boundary_type("left", "free_slip")
    with pytest.raises(RuntimeError):
        H.rhs(v, dict(CONDITIONS["neumann"], left=("free_slip", 0.0)))
    with pytest.raises(RuntimeError):
        m(v.cuda())
    assert cns.last_route() == "fallback:boundary condition without a fused mapping"
    # fused=False
    got = module("neumann", fused=False)(v.cuda())
    assert cns.last_route() == "fallback:fused=False"
    check(got, v, "neumann", what="fused=False")


# ------------------------------------------------------------------ autograd
def grad_err(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().cpu().abs().max())


def test_backward_recomputes_the_composed_expression():
    from cp_pre_amd.cns import last_route
    nr, nc = tile()
    m = module(H.MIXED_FUSABLE)
    v = H.make_vars((2, 4, nr + 1, nc + 4), seed=16).cuda().requires_grad_()
    out = m(v)
    assert last_route() == "fused:cns_rhs" and out.requires_grad
    out.sum().backward()
    w = v.detach().clone().requires_grad_()
    H.rhs(w, H.MIXED_FUSABLE).sum().backward()
    err = grad_err(v.grad, w.grad)
    print(f"d sum(rhs) / d vars: {err:.3e}")
    assert err <= H.TOL
    for op in m._operators():
        assert op.kernel.grad is None
    assert m.gamma.grad is None


def test_param_grads_reach_the_operator_kernels():
    from cp_pre_amd.cns import last_route
    m = module(H.MIXED_FUSABLE, param_grads=True)
    m.gamma = m.gamma.detach().clone().requires_grad_()                          # (a leaf: .to(device) of the constructor's is not)
    leaf = m.gradient.grad_x.kernel.detach().clone().requires_grad_()
    m.gradient.grad_x.kernel = leaf
    v = H.make_vars((2, 4, 9, 12), seed=17).cuda().requires_grad_()
    weight = H.make_vars((2, 4, 9, 12), seed=18).cuda()
    out = m(v)
    assert last_route() == "fused:cns_rhs"
    (out * weight).sum().backward()
    kernels = {n: op.kernel.detach() for n, op in zip(H.KERNEL_NAMES, m._operators())}
    kref = kernels["gx"].clone().requires_grad_()
    kernels["gx"] = kref
    w = v.detach().clone().requires_grad_()
    g32 = H.gamma32().cuda().requires_grad_()
    ops = H.make_ops(kernels, H.MIXED_FUSABLE, torch.float32, "cuda", detach=False)
    (H.expression(w, *ops, g32) * weight).sum().backward()
    assert leaf.grad is not None and m.gamma.grad is not None
    e_k, e_v, e_g = grad_err(leaf.grad, kref.grad), grad_err(v.grad, w.grad), grad_err(m.gamma.grad, g32.grad)
    print(f"d/d kernel {e_k:.3e}, d/d vars {e_v:.3e}, d/d gamma {e_g:.3e}")
    # (the corners of the dense kernel see the padded field too: the whole 3x3 gradient is compared)
    assert e_k <= H.TOL and e_v <= H.TOL and e_g <= H.TOL


# ------------------------------------------------------------------ determinism, graphs, the C client
def test_two_runs_give_the_same_bits():
    nr, nc = tile()
    m = module()
    v = H.make_vars((3, 4, 2 * nr + 1, 2 * nc + 4), seed=19).cuda()
    a, b = m(v), m(v)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    assert torch.equal(m.step(v, 1e-4), m.step(v, 1e-4))


def test_graph_replay_equals_eager():
    from cp_pre_amd.cns import last_route
    nr, nc = tile()
    m = module(H.TRUE_WRAP)
    static = H.make_vars((2, 4, nr + 1, nc + 4), seed=20).cuda()
    eager = m(static)                                                            # (also: the taps a capture is recorded with)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = m(static)
    assert last_route() == "fused:cns_rhs"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    fresh = H.make_vars(tuple(static.shape), seed=21).cuda()
    want = m(fresh)
    static.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, want)


def test_c_client(tmp_path):
    exe = tmp_path / "cns_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "FAIL" not in out.stdout and "no device" not in out.stdout, out.stdout + out.stderr
