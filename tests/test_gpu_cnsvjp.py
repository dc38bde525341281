"""GPU tests of the fused backward of the compressible-NS right-hand side (``cp_pre_amd.cns.Euler_FV_OS_rhs`` built with
``backward="fused"``, its ``vjp`` and its differentiable ``step``; libcp_pre_cnsvjp.so) against fp64 autograd through the
pinned restatement of the reference's expression (``cnsvjp_helpers.vjp64``).

``TOL`` = 1e-5 tensor-scale relative error per gradient channel (cns_helpers); tests/test_cnsvjp_cpu.py shows that fp32
autograd alone stays within ``TOL / 4`` at every shape used here, and that the mathematics the kernel implements is the
gradient to 1e-12.  The shapes sit below, at and beyond every seam of the kernel's tile (PRE_CNSVJP_TILE_ROWS / _COLS).
Inputs are ``cns_helpers.make_vars`` (rho, p in U(0.5, 1.5)) and a seeded ``randn`` cotangent."""
import subprocess

import pytest
import torch

import cns_helpers as H
import cnsvjp_helpers as V
from test_cnsvjp_cpu import FUSED_CONDITIONS, c_client_command, tile
from test_gpu_cns import module

pytestmark = pytest.mark.gpu


def fused(bc="periodic", kernels=None, **kw):
    return module(bc, kernels, backward="fused", **kw)


def pair(shape, seed):
    return H.make_vars(shape, seed=seed), V.make_cot(shape, seed=seed)


def check(got, v, g, bc, kernels=None, what=""):
    err = V.channel_err(got, V.vjp64(v, g, bc, kernels), V.zero(v, g, kernels))
    print(f"{what}: channel error {err:.3e}")
    assert err <= H.TOL, what
    return err


# ------------------------------------------------------------------ shapes and boundary conditions
@pytest.mark.parametrize("bs", (1, 3))
@pytest.mark.parametrize("bc", list(FUSED_CONDITIONS))
def test_fused_vjp_at_every_seam(bc, bs):
    from cp_pre_amd.cns import last_backward_route
    cond = FUSED_CONDITIONS[bc]
    m = fused(cond)
    nxs, nys = H.gpu_extents(*tile())
    worst = 0.0
    for nx in nxs:
        for ny in nys:
            v, g = pair((bs, 4, nx, ny), nx * 1000 + ny)
            got = m.vjp(v.cuda(), g.cuda())
            assert last_backward_route() == "fused:cns_vjp" and got.shape == v.shape and got.is_cuda
            assert bool(torch.isfinite(got).all()), (nx, ny)
            err = V.channel_err(got, V.vjp64(v, g, cond), V.zero(v, g))
            assert err <= H.TOL, (nx, ny, err)
            worst = max(worst, err)
    print(f"{bc}, BS {bs}: worst channel error {worst:.3e}")


# ------------------------------------------------------------------ the taps are the ones handed over
@pytest.mark.parametrize("bc", ("periodic", "mixed_fusable", "symmetric", "dirichlet0"))
def test_callers_kernels_are_the_taps(bc):
    nr, nc = tile()
    k = H.asymmetric_kernels()
    cond = FUSED_CONDITIONS[bc]
    m = fused(cond, k)
    for shape in ((2, 4, nr + 1, nc + 4), (1, 4, 2, 8)):
        v, g = pair(shape, 7)
        got = m.vjp(v.cuda(), g.cuda())
        check(got, v, g, cond, k, f"asymmetric crosses, {bc}, {shape}")
        assert V.channel_err(got, V.vjp64(v, g, cond)) > 100 * H.TOL              # (not the constructor's kernels)


def test_kernel_changed_between_forward_and_backward_uses_the_forwards():
    from cp_pre_amd.cns import last_backward_route, last_route
    k = H.asymmetric_kernels()
    m = fused("neumann", k)
    v, g = pair((2, 4, 9, 12), 8)
    x = v.cuda().requires_grad_()
    out = m(x)
    assert last_route() == "fused:cns_rhs" and out.requires_grad
    m.gradient.grad_y.kernel.data.mul_(-3.0)                                     # in place
    m.laplace.laplace.kernel = (0.5 * k["lap"]).cuda()                           # replaced
    m.gamma = (2 * m.gamma).detach()
    out.backward(g.cuda())
    assert last_backward_route() == "fused:cns_vjp"
    check(x.grad, v, g, "neumann", k, "the forward's kernels")
    k2 = dict(k, gy=-3.0 * k["gy"], lap=0.5 * k["lap"])
    assert V.channel_err(x.grad, V.vjp64(v, g, "neumann", k2)) > 100 * H.TOL


# ------------------------------------------------------------------ views
@pytest.mark.parametrize("bs", (1, 3))
def test_views_are_read_and_written_where_they_lie(bs):
    from cp_pre_amd.cns import last_backward_route
    nr, nc = tile()
    nx, ny = nr + 1, nc + 4
    m = fused(H.MIXED_FUSABLE)
    v, g = pair((bs, 4, nx, ny), 9)
    v, g = v.cuda(), g.cuda()
    dense = m.vjp(v, g)
    big_v = torch.full((bs, 6, nx + 8, ny + 16), float("nan"), device="cuda")
    big_g = torch.full((bs, 5, nx + 4, ny + 8), float("nan"), device="cuda")
    big_v[:, 1:5, 4:4 + nx, 8:8 + ny] = v
    big_g[:, 0:4, 2:2 + nx, 4:4 + ny] = g
    sentinel = -12345.5
    buf = torch.full((bs, 6, nx + 8, ny + 16), sentinel, device="cuda")
    out = buf[:, 1:5, 4:4 + nx, 8:8 + ny]
    res = m.vjp(big_v[:, 1:5, 4:4 + nx, 8:8 + ny], big_g[:, 0:4, 2:2 + nx, 4:4 + ny], out=out)
    assert last_backward_route() == "fused:cns_vjp" and res.data_ptr() == out.data_ptr()
    assert torch.equal(out, dense) and not torch.isnan(out).any()
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, 1:5, 4:4 + nx, 8:8 + ny] = False
    assert bool((buf[mask] == sentinel).all())
    # without out: the same bits in a new dense tensor
    assert torch.equal(m.vjp(big_v[:, 1:5, 4:4 + nx, 8:8 + ny], big_g[:, 0:4, 2:2 + nx, 4:4 + ny]), dense)


# ------------------------------------------------------------------ cotangent layouts
def test_expanded_and_misaligned_cotangents_are_made_contiguous():
    from cp_pre_amd.cns import last_backward_route
    nr, nc = tile()
    m = fused(H.TRUE_WRAP)
    v = H.make_vars((2, 4, nr + 1, nc + 4), seed=10)
    ones = torch.ones(v.shape)
    x = v.cuda().requires_grad_()
    m(x).sum().backward()                                                        # autograd hands over an expanded scalar
    assert last_backward_route() == "fused:cns_vjp"
    check(x.grad, v, ones, H.TRUE_WRAP, what="sum().backward()")
    got = m.vjp(v.cuda(), torch.ones((), device="cuda").expand(v.shape))
    assert torch.equal(got, x.grad)
    # a cotangent off by one float
    g = V.make_cot(tuple(v.shape), seed=10)
    flat = torch.zeros(g.numel() + 4, device="cuda")
    flat[1:1 + g.numel()] = g.cuda().reshape(-1)
    shifted = flat[1:1 + g.numel()].view(g.shape)
    assert shifted.data_ptr() % 16 == 4
    check(m.vjp(v.cuda(), shifted), v, g, H.TRUE_WRAP, what="offset by one float")


def test_cpu_inputs_are_staged_through_the_gpu():
    from cp_pre_amd.cns import last_backward_route, last_route
    m = fused()
    v, g = pair((2, 4, 9, 12), 11)
    got = m.vjp(v, g)
    assert last_backward_route() == "fused:cns_vjp" and not got.is_cuda
    check(got, v, g, "periodic", what="cpu vjp")
    x = v.clone().requires_grad_()
    out = m(x)
    assert last_route() == "fused:cns_rhs" and not out.is_cuda
    out.backward(g)
    assert not x.grad.is_cuda and torch.equal(x.grad, got)


# ------------------------------------------------------------------ the epilogue
def test_epilogue_accumulates_in_place_and_onto_the_cotangent():
    from cp_pre_amd.cns import last_backward_route
    nr, nc = tile()
    m = fused(H.MIXED_FUSABLE)
    v, g = pair((3, 4, nr + 1, nc + 4), 12)
    want = V.vjp64(v, g, H.MIXED_FUSABLE)
    init = V.make_cot(tuple(v.shape), seed=13)
    acc = init.cuda()
    assert m.vjp(v.cuda(), g.cuda(), out=acc, add_to=acc, scale=0.5) is acc
    assert last_backward_route() == "fused:cns_vjp+axpy"
    e0 = V.channel_err(acc, init.double() + 0.5 * want)
    other = m.vjp(v.cuda(), g.cuda(), add_to=init.cuda(), scale=0.5)             # a separate add_to: the same bits
    assert torch.equal(other, acc)
    h = 1e-4
    gd = g.cuda()
    got = m.vjp(v.cuda(), gd, add_to=gd, scale=h)
    assert last_backward_route() == "fused:cns_vjp+axpy" and torch.equal(gd.cpu(), g)
    e1 = V.channel_err(got, g.double() + h * want)
    print(f"in place {e0:.3e}, onto the cotangent {e1:.3e}")
    assert e0 <= H.TOL and e1 <= H.TOL


# ------------------------------------------------------------------ through autograd
def test_loss_backward_through_forward():
    from cp_pre_amd.cns import last_backward_route, last_route
    nr, nc = tile()
    m = fused(H.MIXED_FUSABLE)
    v, weight = pair((2, 4, nr + 1, nc + 4), 14)
    x = v.cuda().requires_grad_()
    out = m(x)
    assert last_route() == "fused:cns_rhs" and out.requires_grad
    loss = (out * weight.cuda()).sum()
    loss.backward()
    assert last_backward_route() == "fused:cns_vjp"
    check(x.grad, v, weight, H.MIXED_FUSABLE, what="d sum(w * rhs) / d vars")
    for op in m._operators():
        assert op.kernel.grad is None
    # once differentiable
    y = v.cuda().requires_grad_()
    (gy,) = torch.autograd.grad(m(y).sum(), y, create_graph=True)
    with pytest.raises(RuntimeError):
        gy.sum().backward()


def rollout64(v, scheme, steps, h, bc, weight):
    """d loss / d v0 of the same rollout in fp64 autograd."""
    ops = H.make_ops(H.default_kernels(), bc, torch.float64)
    gamma = H.gamma32().double()
    y = v.double().requires_grad_()
    state = y
    for _ in range(steps):
        state = scheme(state, lambda s, hh, base=None: (s if base is None else base) + hh * H.expression(s, *ops, gamma), h)
    (state * weight.double()).sum().backward()
    return y.grad


def euler(state, step, h):
    return step(state, h)


def midpoint(state, step, h):
    return step(step(state, h / 2), h, base=state)                               # a base of its own


@pytest.mark.parametrize("scheme", (euler, midpoint))
def test_three_step_rollout(scheme):
    from cp_pre_amd.cns import last_backward_route, last_route
    nr, nc = tile()
    h = 1e-5
    m = fused(H.TRUE_WRAP)
    v, weight = pair((2, 4, nr + 1, nc + 4), 15)
    x = v.cuda().requires_grad_()
    state = x
    for _ in range(3):
        state = scheme(state, m.step, h)
        assert last_route() == "fused:cns_rhs+axpy" and state.requires_grad
    (state * weight.cuda()).sum().backward()
    # (euler: every step folds g + h * J^T g into its launch; midpoint mixes both forms, in autograd's order)
    assert last_backward_route() == "fused:cns_vjp+axpy" if scheme is euler else last_backward_route().startswith("fused:cns_vjp")
    want = rollout64(v, scheme, 3, h, H.TRUE_WRAP, weight)
    err = V.channel_err(x.grad, want)
    print(f"{scheme.__name__}: d loss / d vars through three steps {err:.3e}")
    assert err <= H.TOL


def test_step_delivers_the_gradient_of_a_separate_base():
    m = fused("neumann")
    v, g = pair((2, 4, 9, 12), 16)
    base = H.make_vars(tuple(v.shape), seed=17)
    h = 1e-3
    x, b = v.cuda().requires_grad_(), base.cuda().requires_grad_()
    m.step(x, h, base=b).backward(g.cuda())
    assert torch.equal(b.grad.cpu(), g)
    assert V.channel_err(x.grad, h * V.vjp64(v, g, "neumann")) <= H.TOL
    # only the base asks for a gradient: no launch in the backward is needed, d_base = g
    b2 = base.cuda().requires_grad_()
    m.step(v.cuda(), h, base=b2).backward(g.cuda())
    assert torch.equal(b2.grad.cpu(), g)
    with pytest.raises(RuntimeError, match="out="):
        m.step(x, h, out=torch.empty_like(x))


# ------------------------------------------------------------------ routes
def test_param_grads_keep_the_recompute_route():
    from cp_pre_amd.cns import last_backward_route, last_route
    m = fused(H.MIXED_FUSABLE, param_grads=True)
    leaf = m.gradient.grad_x.kernel.detach().clone().requires_grad_()
    m.gradient.grad_x.kernel = leaf
    v, g = pair((2, 4, 9, 12), 18)
    x = v.cuda().requires_grad_()
    out = m(x)
    assert last_route() == "fused:cns_rhs" and m.plan_backward(x) == "fallback:param_grads=True"
    out.backward(g.cuda())
    assert last_backward_route() == "fallback:param_grads=True" and leaf.grad is not None
    check(x.grad, v, g, H.MIXED_FUSABLE, what="recompute route")
    with pytest.raises(RuntimeError, match=r"vars \+ h\*forward\(vars\)"):
        m.step(x, 1e-3)


def test_default_module_is_untouched():
    from cp_pre_amd import cns
    m = module("neumann")
    assert m.backward == "recompute"
    v, g = pair((2, 4, 9, 12), 19)
    x = v.cuda().requires_grad_()
    before = cns.last_backward_route()
    m(x).backward(g.cuda())
    assert cns.last_backward_route() == before                                  # (the recompute route of the default says nothing)
    check(x.grad, v, g, "neumann", what="default backward")
    with pytest.raises(RuntimeError, match=r"vars \+ h\*forward\(vars\)"):
        m.step(x, 1e-3)
    # the bare product needs no opt-in
    check(m.vjp(v.cuda(), g.cuda()), v, g, "neumann", what="vjp of a default module")


def test_forward_that_fell_back_is_differentiated_by_autograd():
    from cp_pre_amd import cns
    m = fused("neumann")
    v, g = pair((2, 4, 9, 6), 20)                                                # Ny = 6
    x = v.cuda().requires_grad_()
    out = m(x)
    assert cns.last_route() == "fallback:Ny % 4 != 0" and m.plan_backward(x) == "fallback:Ny % 4 != 0"
    out.backward(g.cuda())
    check(x.grad, v, g, "neumann", what="Ny = 6")
    y = m.step(x, 1e-3)
    assert cns.last_route() == "fallback:Ny % 4 != 0" and y.requires_grad


# ------------------------------------------------------------------ refusals
def test_vjp_refuses_out_on_vars_or_on_the_cotangent():
    m = fused()
    v, g = pair((2, 4, 9, 12), 21)
    v, g = v.cuda(), g.cuda()
    keep_v, keep_g = v.clone(), g.clone()
    with pytest.raises(ValueError, match="must not overlap vars"):
        m.vjp(v, g, out=v)
    with pytest.raises(ValueError, match="must not overlap vars"):
        m.vjp(v, g, out=g)
    big = torch.cat((v, v), dim=2)
    keep_big = big.clone()
    with pytest.raises(ValueError, match="must not overlap vars"):
        m.vjp(big[:, :, 0:9], g, out=big[:, :, 8:17])                            # shares one row
    with pytest.raises(ValueError, match="cotangent"):
        m.vjp(v, g[:, :, :8])
    torch.cuda.synchronize()
    assert torch.equal(v, keep_v) and torch.equal(g, keep_g) and torch.equal(big, keep_big)


# ------------------------------------------------------------------ determinism, graphs, the C client
def test_two_runs_give_the_same_bits():
    nr, nc = tile()
    m = fused(H.MIXED_FUSABLE)
    v, g = pair((3, 4, 2 * nr + 1, 2 * nc + 4), 22)
    v, g = v.cuda(), g.cuda()
    a, b = m.vjp(v, g), m.vjp(v, g)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    assert torch.equal(m.vjp(v, g, add_to=g, scale=1e-4), m.vjp(v, g, add_to=g, scale=1e-4))


def test_graph_replay_equals_eager():
    from cp_pre_amd.cns import last_backward_route
    nr, nc = tile()
    m = fused(H.TRUE_WRAP)
    sv, sg = pair((2, 4, nr + 1, nc + 4), 23)
    sv, sg = sv.cuda(), sg.cuda()
    out = torch.empty_like(sv)
    eager = m.vjp(sv, sg)                                                        # (also: the taps a capture is recorded with)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.vjp(sv, sg, out=out)
    assert last_backward_route() == "fused:cns_vjp"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    fv, fg = pair(tuple(sv.shape), 24)
    want = m.vjp(fv.cuda(), fg.cuda())
    sv.copy_(fv)
    sg.copy_(fg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_c_client(tmp_path):
    exe = tmp_path / "cnsvjp_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "FAIL" not in out.stdout and "no device" not in out.stdout, out.stdout + out.stderr
