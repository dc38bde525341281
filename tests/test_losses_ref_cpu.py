"""CPU tests of the float64 reference the seam and guard tests of the fused VJP kernels compare with
(tests/losses_helpers.py: ``Route``, ``ref64``, ``ref_vjp``, ``ref_loss``):
  * the restated residual expressions and their autograd gradients equal the fp32 oracle (oracle/residuals.py, the
    reference's own F.conv3d / F.conv2d arithmetic) and ITS autograd within TOL, at the small shapes of
    tests/test_gpu_losses.py: this pins the restatement to the reference-derived oracle;
  * the headroom of the GPU bound: the identical formulas evaluated in float32 on the CPU, at every shape the GPU tests
    run, differ from float64 by at most TOL / 4 - overall and per gradient channel - so a correct fp32 kernel is not
    expected anywhere near TOL.  The measured values are printed (pytest -s) and recorded in tests/LOSSES_TESTS.md."""
import pytest
import torch

from conftest import rel_err
from losses_helpers import (D, LOSS_SHAPES, ROUTES, SEAM_SHAPES, Dshift, Route, asym_star, channel_errs, ref64, ref_loss, ref_vjp,
                            seam_groups, seam_inputs)
from oracle import residuals as orr
from oracle.convops import ConvOperator1D as OracleOp1D
from oracle.convops import ConvOperator2D as OracleOp2D

TOL = 1e-5
SMALL = ((2, 6, 10, 16), (2, 5, 9, 13))
DT, DX, DY, NU = 0.01, 1 / 64, 1 / 32, 0.001


def _crop(r, boundary, nd):
    return r if boundary else r[(Ellipsis,) + (slice(1, -1),) * nd]


ORACLE = {
    "op3d": lambda x, b: _crop(OracleOp2D(("x", "y"), 2)(x), b, 3),
    "op2d": lambda x, b: _crop(OracleOp1D("x", 2)(x), b, 2),
    "wave": lambda x, b: orr.wave_residual(x, 1.0, 0.01, 0.02, boundary=b),
    "advection": lambda x, b: orr.advection_residual(x, 1.0, 2, 0.005, 0.01, boundary=b),
    "ns_continuity": lambda x, b: orr.ns_continuity(x, DX, DY, boundary=b),
    "ns_momentum": lambda x, b: orr.ns_momentum(x, DT, DX, DY, NU, boundary=b),
    "pre_ns": lambda x, b: orr.ns_momentum(x, DT, DX, DY, 0.001, boundary=b),
    "burgers": lambda x, b: orr.burgers_residual(x, 0.05, 0.01, 0.002, boundary=b),
}


def test_shifted_adds_are_the_zero_padded_cross_correlation():
    """``Dshift`` (what ``ref64`` is evaluated with) == ``D`` (the oracle's conv arithmetic) in fp64, dense and star kernels"""
    gen = torch.Generator().manual_seed(0)
    for nd, shape in ((3, (2, 5, 7, 9)), (2, (3, 6, 11)), (3, (1, 1, 1, 1)), (2, (2, 1, 2))):
        f = torch.randn(shape, generator=gen, dtype=torch.float64)
        for k in (torch.randn((3,) * nd, generator=gen, dtype=torch.float64), asym_star(nd).double(), torch.zeros((3,) * nd, dtype=torch.float64)):
            assert (Dshift(f, k) - D(f, k)).abs().max() <= 1e-13


def test_asymmetric_stars_have_no_equal_tap_pair():
    for name in ("op3d", "op2d", "wave", "advection", "ns_continuity_yfix"):
        for k in Route(name, asym=True).kernels(torch.float32):
            c = (1,) * k.dim()
            pairs = 0
            for ax in range(k.dim()):
                lo, hi = list(c), list(c)
                lo[ax], hi[ax] = 0, 2
                a, b = float(k[tuple(lo)]), float(k[tuple(hi)])
                if a != 0 or b != 0:
                    assert a != b, (name, ax)
                    pairs += 1
            assert pairs >= 1
    k = asym_star(3)
    assert len({abs(float(v)) for v in k[k != 0]}) == 7
    # y_axis_fix: D_y is D_x with its taps along Ny
    ns = Route("ns_momentum_yfix")
    assert torch.equal(ns.obj.D_y.kernel, ns.obj.D_x.kernel.transpose(1, 2)) and not Route("ns_continuity_yfix").has_t_taps()
    assert Route("ns_continuity").has_t_taps()                     # (the default D_y, like the reference's, lies along Nt)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("name", sorted(ORACLE))
def test_ref64_and_its_gradient_match_the_fp32_oracle(name, boundary):
    route = Route(name)
    for shape in SMALL:
        x, g = seam_inputs(route, shape, boundary, seed=1)
        with torch.no_grad():
            want = ORACLE[name](x, boundary)
        got = ref64(route, x.double(), boundary)
        assert got.shape == want.shape == g.shape
        xr = x.clone().requires_grad_(True)
        ORACLE[name](xr, boundary).backward(g)
        gref = ref_vjp(route, x.double(), g.double(), boundary)
        e_r, e_g = rel_err(want.numpy(), got.numpy()), rel_err(xr.grad.numpy(), gref.numpy())
        print(f"{name} {shape} boundary={boundary}: oracle vs ref64 residual {e_r:.2e}, gradient {e_g:.2e}")
        assert e_r <= TOL and e_g <= TOL
        # the loss: value and gradient
        xr = x.clone().requires_grad_(True)
        lo = ORACLE[name](xr, boundary).pow(2).mean()
        lo.backward()
        val, grad = ref_loss(route, x.double(), boundary)
        assert abs(float(lo.detach()) - val) <= TOL * abs(val) and rel_err(xr.grad.numpy(), grad.numpy()) <= TOL
        # ... and the conv form of D gives the same reference
        assert (ref64(route, x.double(), boundary, D) - got).abs().max() <= 1e-12 * max(1.0, float(got.abs().max()))


# ------------------------------------------------------------------ headroom of the GPU bounds
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("name", ROUTES)
def test_fp32_formula_headroom_of_the_vjp_bound(name, boundary):
    """the inputs of tests/test_gpu_losses_seams.py (same seeds, same asymmetric stars), the formulas in fp32 on the CPU"""
    route = Route(name, asym=True)
    worst = {}
    for group in seam_groups(name):
        for shape in SEAM_SHAPES[group]:
            x, g = seam_inputs(route, shape, boundary)
            errs = channel_errs(ref_vjp(route, x, g, boundary), ref_vjp(route, x.double(), g.double(), boundary))
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(errs.values()) <= TOL / 4, (name, shape, boundary, errs)
    print(f"headroom vjp {name} boundary={boundary}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("name", ["ns_momentum", "ns_continuity", "burgers", "wave", "advection"])
def test_fp32_formula_headroom_of_the_loss_bounds(name):
    route = Route(name, asym=True)
    for shape in LOSS_SHAPES:
        for boundary in (False, True):
            x, _ = seam_inputs(route, shape, True, seed=2)
            yy = x + 0.1 * torch.rand(x.shape, generator=torch.Generator().manual_seed(3))
            for what, y in (("pi", None), ("pisl", yy)):
                v32, g32 = ref_loss(route, x, boundary, y, 1000.0)
                v64, g64 = ref_loss(route, x.double(), boundary, None if y is None else y.double(), 1000.0)
                errs = channel_errs(g32, g64)
                ev = abs(v32 - v64) / abs(v64)
                print(f"headroom {what} {name} {shape} boundary={boundary}: value {ev:.2e}, gradient " +
                      ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
                assert ev <= TOL / 4 and max(errs.values()) <= TOL / 4, (name, shape, boundary, what, ev, errs)
