"""GPU tests of the ODE operators and fused ODE residuals (libcp_pre_ode.so through cp_pre_amd.convops_0d / cp_pre_amd.ode):
the reference-executed goldens (tests/golden/convops_0d.npz), a fuzz against F.conv1d in float64 on the CPU over strided and
permuted views, NaN / inf propagation, the fused script residuals, calibration on the residuals where they lie, gradients,
graph capture and one full-size case."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cp_pre_amd import _lib
from cp_pre_amd import inductive_cp as icp
from cp_pre_amd import ode, pipeline
from cp_pre_amd.convops_0d import ConvOperator, conv1d, stencil, wgrad
from oracle import conformal as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "convops_0d.npz"))
NTS = (1, 2, 3, 7, 100, 150)
KERNELS = {3: (2, 2), 5: (2, 4), 7: (2, 6)}


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(np.abs(want).max(), 1e-30) if want.size else 1.0
    return np.abs(got - want).max() / scale if want.size else 0.0


def conv_ref(x, taps):
    """F.conv1d in float64 on the CPU."""
    xd = torch.as_tensor(np.asarray(x, np.float64))
    k = torch.as_tensor(np.asarray(taps, np.float64))
    return F.conv1d(xd[:, None], k[None, None], padding=len(taps) // 2)[:, 0].numpy()


# ---------------------------------------------------------------- goldens
def test_golden_operators(gpu):
    for nt in NTS:
        x = G[f"x_nt{nt}"]
        for k, (d, t) in KERNELS.items():
            op = ConvOperator(order=d, taylor_order=t, scale=0.7)
            for dev in ("cpu", "cuda"):
                xt = torch.from_numpy(x).to(dev)
                got = op.convolution(xt)
                assert got.device.type == dev
                assert rel(got.cpu(), G[f"conv_nt{nt}_k{k}"]) <= 1e-5, (nt, k, dev)
                assert rel(op(xt).cpu(), G[f"conv_nt{nt}_k{k}"]) <= 1e-5
            xt = torch.from_numpy(x)
            if f"spec_nt{nt}_k{k}_error" in G.files:
                with pytest.raises(RuntimeError):
                    op.spectral_convolution(xt)
            else:
                assert rel(op.spectral_convolution(xt), G[f"spec_nt{nt}_k{k}"]) <= 1e-5, (nt, k)
            for corr in (False, True):
                for sp in (False, True):
                    tag = f"nt{nt}_k{k}_c{int(corr)}_s{int(sp)}"
                    # (integrate: the generator's eps, see make_golden_0d.gen_apply)
                    calls = (("diff", lambda: op.differentiate(xt, correlation=corr, slice_pad=sp), 1e-5),
                             ("integ", lambda: op.integrate(xt, correlation=corr, slice_pad=sp, eps=0.3), 1e-4))
                    if k == 3:
                        calls += (("integ_exact", lambda: ConvOperator(order=2).integrate(xt, correlation=corr, slice_pad=sp),
                                   1e-4),)
                    for name, fn, tol in calls:
                        if f"{name}_{tag}_error" in G.files:
                            with pytest.raises(RuntimeError):
                                fn()
                        else:
                            got = fn()
                            assert got.device.type == "cpu"
                            assert rel(got, G[f"{name}_{tag}"]) <= tol, (name, tag)


def test_golden_script_residuals(gpu):
    sol = torch.from_numpy(G["dho_sol"])[None]                   # [1, Nt, 2]: x, v
    m, c, k = (float(v) for v in G["dho_mck"])
    dt = float(G["dho_dt"])
    comb = ode.DHO(m, c, k, dt).residual(sol)
    assert comb.device.type == "cpu"
    assert rel(comb, G["dho_combined_direct"]) <= 1e-5
    assert rel(comb, G["dho_combined_spectral"]) <= 1e-5
    assert rel(ode.DHO(m, c, k, dt, split=True).residual(sol.to(gpu)).cpu(), G["dho_split"]) <= 1e-5
    assert rel(ode.DHO_kinematic(dt).residual(sol.numpy()), G["dho_kinematic"]) <= 1e-5
    t = G["sho_t"]
    assert rel(ode.SHO(float(G["sho_omega"]), t[1] - t[0]).residual(torch.from_numpy(G["sho_sol"])[None]),
               G["sho_direct"]) <= 1e-5
    x = G["bessel_x"]
    inner = np.zeros(x.size, bool)
    inner[1:-1] = np.abs(x[1:-1]) >= 1e-6                        # the loop leaves the ends and x = 0 at 0
    state = torch.from_numpy(G["bessel_sol"])[None].to(gpu)
    for n in (0, 1, 2):
        got = ode.Bessel(x, n, x[1] - x[0]).residual(state).cpu().numpy()
        want = G[f"bessel_res_n{n}"]
        assert rel(got[:, inner], want[:, inner]) <= 1e-5, n


# ---------------------------------------------------------------- fuzz against F.conv1d
def _view(kind, x, gpu):
    """A device view of the host [BS, Nt] array x laid out as ``kind``."""
    bs, nt = x.shape
    xt = torch.from_numpy(x)
    if kind == "dense":
        return xt.to(gpu)
    if kind.startswith("comp"):                                  # component c of a [BS, Nt, S] state
        S, c = int(kind[4]), int(kind[5])
        st = torch.randn(bs, nt, S).to(gpu)
        st[..., c] = xt.to(gpu)
        return st[..., c]
    if kind == "transpose":                                      # a [Nt, BS] buffer seen as [BS, Nt]
        return xt.t().contiguous().to(gpu).t()
    raise ValueError(kind)


KINDS = ("dense", "comp20", "comp21", "comp31", "comp32", "transpose")


def test_fuzz_against_conv1d(gpu):
    rng = np.random.default_rng(11)
    i = 0
    for bs in (0, 1, 3, 4097):
        for nt in (1, 2, 3, 7, 100, 1023, 4096):
            k = int(rng.choice([1, 3, 5, 7]))
            taps = rng.standard_normal(k).astype(np.float32)
            x = rng.standard_normal((bs, nt)).astype(np.float32)
            kinds = KINDS if bs * nt <= (1 << 16) else (KINDS[i % len(KINDS)], KINDS[(i + 3) % len(KINDS)])
            i += 1
            want = conv_ref(x, taps)
            for kind in kinds:
                v = _view(kind, x, gpu)
                assert torch.equal(v.cpu(), torch.from_numpy(x)), kind
                got = conv1d(v, torch.from_numpy(taps))
                assert got.shape == (bs, nt) and got.is_cuda
                assert rel(got.cpu(), want) <= 1e-5, (bs, nt, k, kind)
                # out written through strides: a transposed output buffer
                out = torch.empty(nt, bs, device=gpu).t()
                stencil(v, taps, out=out)
                assert rel(out.cpu(), want) <= 1e-5, (bs, nt, k, kind, "out^T")


def _raw_stencil(x_ptr, xs, out, taps, bs, nt):
    t = np.ascontiguousarray(taps, np.float32)
    rc = _lib.load_ode().pre_ode_stencil_f32(ctypes.c_void_p(x_ptr), _lib.iarr64(xs), _lib.ptr(out), _lib.iarr64(out.stride()),
                                             bs, nt, t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(t), 0, _lib.stream())
    _lib.check(rc, "pre_ode_stencil_f32")
    torch.cuda.synchronize()
    return out


def test_negative_and_zero_batch_strides(gpu):
    """torch views cannot carry a negative stride, so the C entry is called directly: rows read last to first, and one row
    broadcast over the batch."""
    rng = np.random.default_rng(3)
    for bs, nt in ((1, 5), (4097, 100), (3, 4096)):
        x = rng.standard_normal((bs, nt)).astype(np.float32)
        taps = rng.standard_normal(5).astype(np.float32)
        xd = torch.from_numpy(x).to(gpu)
        out = torch.empty(bs, nt, device=gpu)
        _raw_stencil(xd.data_ptr() + 4 * (bs - 1) * nt, (-nt, 1), out, taps, bs, nt)
        assert rel(out.cpu(), conv_ref(x[::-1], taps)) <= 1e-5, (bs, nt)
        _raw_stencil(xd.data_ptr(), (0, 1), out, taps, bs, nt)
        assert rel(out.cpu(), conv_ref(np.repeat(x[:1], bs, 0), taps)) <= 1e-5, (bs, nt)


def test_overlapping_output_is_rejected(gpu):
    x = torch.randn(4, 16, device=gpu)
    bad = torch.empty(16, device=gpu).as_strided((4, 16), (0, 1))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        stencil(x, np.ones(3, np.float32), out=bad)
    bad = torch.empty(40, device=gpu).as_strided((4, 16), (8, 1))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        stencil(x, np.ones(3, np.float32), out=bad)


def test_nonfinite_values_propagate_as_conv1d(gpu):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 40)).astype(np.float32)
    x[0, 5], x[1, 0], x[2, 39], x[3, 20], x[4, 21] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    x[5, 10] = np.nan
    for taps in (np.array([0, 1, 0], np.float32), np.array([1, -2, 1], np.float32),
                 np.array([1 / 90, -3 / 20, 3 / 2, -49 / 18, 3 / 2, -3 / 20, 1 / 90], np.float32), np.array([2.0], np.float32)):
        want = F.conv1d(torch.from_numpy(x)[:, None], torch.from_numpy(taps)[None, None], padding=len(taps) // 2)[:, 0].numpy()
        got = conv1d(torch.from_numpy(x).to(gpu), torch.from_numpy(taps)).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), taps
        assert np.array_equal(np.isposinf(got), np.isposinf(want)), taps
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), taps
        fin = np.isfinite(want)
        assert rel(got[fin], want[fin]) <= 1e-5


# ---------------------------------------------------------------- fused residuals
def test_fused_residuals_match_term_by_term(gpu):
    rng = np.random.default_rng(7)
    for bs, nt in ((1, 1), (3, 2), (5, 7), (257, 100), (33, 1023)):
        st = torch.from_numpy(rng.standard_normal((bs, nt, 2)).astype(np.float32)).to(gpu)
        x = np.linspace(-1.0, 4.0, nt)
        ops = [ode.SHO(1.7, 0.05), ode.DHO(1.5, 0.3, 2.0, 0.05), ode.DHO(1.5, 0.3, 2.0, 0.05, split=True),
               ode.DHO_kinematic(0.05), ode.Bessel(x, 1, (x[1] - x[0]) if nt > 1 else 1.0),
               ode.ODEResidual([(0, rng.standard_normal(7).astype(np.float32), rng.standard_normal(nt).astype(np.float32)),
                                (1, rng.standard_normal(1).astype(np.float32), None),
                                (1, rng.standard_normal(5).astype(np.float32), rng.standard_normal(nt).astype(np.float32)),
                                (0, rng.standard_normal(3).astype(np.float32), None)])]
        for j, op in enumerate(ops):
            fused = op.residual(st)
            comp = op.composed(st)
            want = np.zeros((bs, nt))
            for comp_i, kern, taps, c in op.terms:
                y = conv_ref(st[..., comp_i].cpu().numpy(), taps)
                want += (c.numpy().astype(np.float64)[None] * y) if c is not None else y
            assert rel(fused.cpu(), want) <= 1e-5, (bs, nt, j)
            assert rel(comp.cpu(), want) <= 1e-5, (bs, nt, j)
            assert torch.equal(op.residual(st, absolute=True), fused.abs()), (bs, nt, j)
            lst = [st[..., 0], st[..., 1]]
            assert torch.equal(op.residual(lst), fused), (bs, nt, j)


def test_absolute_into_row_padded_then_calibrate(gpu):
    rng = np.random.default_rng(9)
    n, nt = 300, 100
    st = torch.from_numpy(rng.standard_normal((n, nt, 2)).astype(np.float32)).to(gpu)
    op = ode.DHO(1.5, 0.3, 2.0, 0.05, split=True)
    buf = pipeline.row_padded(n, (nt,), device=gpu)
    assert buf.stride(0) == nt + 64
    got = op.residual(st, absolute=True, out=buf)
    assert got.data_ptr() == buf.data_ptr() and got.stride() == buf.stride()
    scores = buf.cpu().numpy()
    assert rel(scores, np.abs(op.residual(st).cpu().numpy())) == 0.0
    for alpha in (0.1, 0.5):
        q = icp.calibrate(buf, n, alpha).cpu().numpy()
        assert np.array_equal(q, oc.calibrate(scores, n, alpha)), alpha
    qs = icp.calibrate_multi(buf, n, [0.1, 0.3, 0.9])
    for a, q in zip([0.1, 0.3, 0.9], qs):
        assert np.array_equal(np.asarray(q.cpu() if isinstance(q, torch.Tensor) else q), oc.calibrate(scores, n, a))
    levels = [icp.calibrate(buf, n, a) for a in (0.1, 0.5)]
    cov = icp.emp_cov_levels(torch.stack(levels), buf)
    want = [oc.emp_cov([-lv.cpu().numpy(), lv.cpu().numpy()], scores) for lv in levels]
    assert np.array_equal(cov, np.array(want, np.float64))


def test_joint_cp_on_ode_residuals(gpu):
    rng = np.random.default_rng(13)
    n, nt = 400, 150
    st = torch.from_numpy(rng.standard_normal((n, nt, 2)).astype(np.float32)).to(gpu)
    r = ode.DHO(1.5, 0.3, 2.0, 0.05).residual(st)
    mod = icp.modulation_func(r, None)
    js = icp.ncf_metric_joint(r, None, mod)
    q = icp.calibrate(js, js.shape[0], 0.1)
    rn = r.cpu().numpy()
    mod_ref = oc.modulation_func(rn, np.zeros_like(rn))
    q_ref = oc.calibrate(oc.ncf_metric_joint(rn, np.zeros_like(rn), mod_ref), n, 0.1)
    assert abs(float(q) - float(q_ref)) <= 1e-6 * abs(float(q_ref))
    qf = np.float32(q.cpu().numpy() if isinstance(q, torch.Tensor) else q)
    m = mod.cpu().numpy()
    cov = icp.emp_cov_joint_levels(np.array([qf], np.float32), r, mod)
    want = oc.emp_cov_joint([-qf * m, qf * m], rn)
    assert np.array_equal(cov, np.array([want], np.float64))


# ---------------------------------------------------------------- gradients
def test_field_and_kernel_gradients(gpu):
    rng = np.random.default_rng(17)
    for bs, nt, k in ((3, 50, 3), (17, 1000, 5), (2, 7, 7), (4, 2, 3)):
        x = rng.standard_normal((bs, nt)).astype(np.float32)
        taps = rng.standard_normal(k).astype(np.float32)
        g = rng.standard_normal((bs, nt)).astype(np.float32)
        xd = torch.from_numpy(x).to(gpu).requires_grad_(True)
        kd = torch.from_numpy(taps).requires_grad_(True)
        ConvOperator(order=1).convolution(xd, kernel=kd).backward(torch.from_numpy(g).to(gpu))
        xr = torch.from_numpy(x).double().requires_grad_(True)
        kr = torch.from_numpy(taps).double().requires_grad_(True)
        F.conv1d(xr[:, None], kr[None, None], padding=k // 2)[:, 0].backward(torch.from_numpy(g).double())
        assert rel(xd.grad.cpu(), xr.grad) <= 1e-5, (bs, nt, k)
        assert rel(kd.grad, kr.grad) <= 1e-5, (bs, nt, k)
    x = torch.randn(4097, 1023, device=gpu)
    g = torch.randn(4097, 1023, device=gpu)
    a, b = wgrad(x, g, 7), wgrad(x, g, 7)
    assert torch.equal(a, b)
    xr = x.double().cpu()
    gr = g.double().cpu()
    ref = [float((gr[:, max(0, 3 - j):1023 - max(0, j - 3)] * xr[:, max(0, j - 3):1023 - max(0, 3 - j)]).sum()) for j in range(7)]
    assert rel(a.cpu(), np.array(ref)) <= 1e-5


def test_fused_residual_backward_recomputes(gpu):
    rng = np.random.default_rng(19)
    st = torch.from_numpy(rng.standard_normal((5, 60, 2)).astype(np.float32)).to(gpu).requires_grad_(True)
    op = ode.DHO(1.5, 0.3, 2.0, 0.05, split=True)
    g = torch.randn(5, 60, device=gpu)
    op.residual(st).backward(g)
    sr = st.detach().double().cpu().requires_grad_(True)
    want = None
    for comp, kern, taps, c in op.terms:
        y = F.conv1d(sr[..., comp][:, None], torch.from_numpy(taps).double()[None, None], padding=len(taps) // 2)[:, 0]
        want = y if want is None else want + y
    want.backward(g.double().cpu())
    assert rel(st.grad.cpu(), sr.grad) <= 1e-5


# ---------------------------------------------------------------- graph capture
def test_graph_capture_replays_eager(gpu):
    rng = np.random.default_rng(23)
    bs, nt = 1000, 300
    st = torch.from_numpy(rng.standard_normal((bs, nt, 2)).astype(np.float32)).to(gpu)
    taps = torch.from_numpy(rng.standard_normal(5).astype(np.float32))
    op = ode.DHO(1.5, 0.3, 2.0, 0.05, split=True)
    sco = pipeline.row_padded(bs, (nt,), device=gpu)
    out_s = torch.empty(bs, nt, device=gpu)
    out_r = torch.empty(bs, nt, device=gpu)
    tn = taps.numpy()

    def step():
        stencil(st[..., 0], tn, out=out_s)
        op.residual(st, out=out_r)
        op.residual(st, absolute=True, out=sco)

    step()
    torch.cuda.synchronize()
    e_s, e_r, e_a = out_s.clone(), out_r.clone(), sco.clone()
    for t in (out_s, out_r, sco):
        t.fill_(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in (out_s, out_r, sco):
        t.fill_(0)
    st.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_s, 2 * e_s) and torch.equal(out_r, 2 * e_r) and torch.equal(sco, 2 * e_a)


# ---------------------------------------------------------------- full size
def test_full_size_stencil_and_residual(gpu):
    bs, nt = 1 << 20, 1024
    gen = torch.Generator(device=gpu).manual_seed(0)
    st = torch.randn(bs, nt, 2, device=gpu, generator=gen)
    rows = torch.randint(0, bs, (64,), generator=torch.Generator().manual_seed(1))
    rows[0], rows[1] = 0, bs - 1
    taps = np.array([1 / 90, -3 / 20, 3 / 2, -49 / 18, 3 / 2, -3 / 20, 1 / 90], np.float32)
    out = conv1d(st[..., 1], torch.from_numpy(taps))
    want = conv_ref(st[rows, :, 1].cpu().numpy(), taps)
    assert rel(out[rows.to(gpu)].cpu(), want) <= 1e-5
    del out
    x = np.linspace(0.5, 8.0, nt)
    op = ode.Bessel(x, 1, x[1] - x[0])
    res = op.residual(st, absolute=True)
    sub = st[rows.to(gpu)].cpu().numpy()
    want = np.zeros((len(rows), nt))
    for comp, kern, taps_i, c in op.terms:
        want += c.numpy().astype(np.float64)[None] * conv_ref(sub[..., comp], taps_i)
    assert rel(res[rows.to(gpu)].cpu(), np.abs(want)) <= 1e-5
