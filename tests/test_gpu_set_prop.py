"""GPU tests of PRE set propagation (libcp_pre_setprop.so through cp_pre_amd.set_prop): both entry points against the
float64 numpy closed form over batch and row sizes (a table-tiling size included), strided, component and negative-stride
views, fp32 and fp64 inputs, q-hat shapes, both hulls, a NaN row, bitwise repeats and the script drop-ins."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cp_pre_amd import _lib
from cp_pre_amd import set_prop as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHO_K = np.array([1., -2., 1.]) + (10 / 99) ** 2 * np.array([0., 1., 0.])
K5 = np.array([-1 / 12, 4 / 3, -5 / 2, 4 / 3, -1 / 12])
K7 = np.array([1 / 90, -3 / 20, 3 / 2, -49 / 18, 3 / 2, -3 / 20, 1 / 90])
U = 2.0 ** -53


@pytest.fixture(scope="module")
def gpu():
    if not os.path.exists(_lib.SETPROP_SO_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cp_pre_amd", "csrc"), "../libcp_pre_setprop.so"])
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def H_of(n, seed):
    rng = np.random.default_rng(seed)
    return 1 / (np.fft.fft(np.r_[rng.standard_normal(3), np.zeros(n - 3)]) + 0.3)


def check_bounds(lo, hi, c, r, g, a, nterms, bad=None):
    """lo / hi (device) against the fp64 host closed form of the sets (c, r) within 8 * nterms * 2^-53 * sum|terms|."""
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    want_lo, want_hi = sp._bounds_host(c, r, g, a, bad)
    nan = np.isnan(want_lo)
    assert np.array_equal(np.isnan(lo), nan) and np.array_equal(np.isnan(hi), nan)
    if c.shape[0] == 0:
        return
    s = np.abs(c) @ np.abs(sp._circulant(g)) + np.abs(r) @ np.abs(sp._circulant(a))
    tol = 8 * nterms * U * s
    ok = ~nan
    assert np.all(np.abs(lo - want_lo)[ok] <= tol[ok]) and np.all(np.abs(hi - want_hi)[ok] <= tol[ok])


# ---------------------------------------------------------------- pre_setprop_bounds_f64
@pytest.mark.parametrize("B,N", [(0, 4), (1, 4), (3, 101), (4097, 101), (1, 1000), (3, 1000), (3, 4097), (4097, 4)])
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
@pytest.mark.parametrize("hull", sp.HULLS)
def test_bounds_against_the_closed_form(gpu, B, N, dtype, hull):
    torch.manual_seed(B * 7 + N)
    c = torch.randn(B, N, dtype=dtype)
    r = torch.rand(B, N, dtype=dtype)
    H = H_of(N, N)
    lo, hi = sp.propagate(c.to(gpu), r.to(gpu), H, hull=hull)
    assert lo.shape == (B, N) and lo.dtype == torch.float64 and lo.is_cuda
    g, a = sp.tables(H, hull)
    check_bounds(lo, hi, c.double().numpy(), r.double().numpy(), g, a, N)


def test_bounds_large_batch_and_tiled_table(gpu):
    B, N = 4097, 4097
    torch.manual_seed(1)
    c, r = torch.randn(B, N), torch.rand(B, N)
    H = H_of(N, 5)
    lo, hi = sp.propagate(c.to(gpu), r.to(gpu), H)
    check_bounds(lo, hi, c.double().numpy(), r.double().numpy(), *sp.tables(H), N)


def test_bounds_strided_component_and_negative_stride_views(gpu):
    B, N = 37, 101
    torch.manual_seed(2)
    sol = torch.randn(B, N, 2, device=gpu)
    rad = torch.rand(N, B, device=gpu, dtype=torch.float64).t()          # column-major [B, N]
    H = H_of(N, 9)
    g, a = sp.tables(H)
    lo, hi = sp.propagate(sol[..., 0], rad, H)
    check_bounds(lo, hi, sol[..., 0].double().cpu().numpy(), rad.cpu().numpy(), g, a, N)
    # negative strides through the ABI: rows read last to first and each row backwards
    c = torch.randn(B, N, device=gpu)
    r = torch.rand(B, N, device=gpu)
    gd, ad = (torch.from_numpy(t.copy()).to(gpu) for t in (g, a))
    lo2 = torch.empty(B, N, dtype=torch.float64, device=gpu)
    hi2 = torch.empty_like(lo2)
    last = ctypes.c_void_p(c.data_ptr() + ((B - 1) * N + N - 1) * 4)
    lastr = ctypes.c_void_p(r.data_ptr() + ((B - 1) * N + N - 1) * 4)
    rc = _lib.load_setprop().pre_setprop_bounds_f64(last, _lib.iarr64((-N, -1)), lastr, _lib.iarr64((-N, -1)), B, N,
                                                    _lib.ptr(gd), _lib.ptr(ad), _lib.ptr(lo2), _lib.ptr(hi2), 0, _lib.stream())
    _lib.check(rc, "pre_setprop_bounds_f64")
    check_bounds(lo2, hi2, c.flip(0, 1).double().cpu().numpy(), r.flip(0, 1).double().cpu().numpy(), g, a, N)


def test_bounds_nan_row_and_bitwise_repeat(gpu):
    B, N = 9, 101
    torch.manual_seed(3)
    c, r = torch.randn(B, N, device=gpu), torch.rand(B, N, device=gpu)
    c[4, 17] = float("nan")
    r[6, 3] = float("inf")
    H = H_of(N, 4)
    lo, hi = sp.propagate(c, r, H)
    assert torch.isnan(lo[[4, 6]]).all() and torch.isnan(hi[[4, 6]]).all()
    keep = [0, 1, 2, 3, 5, 7, 8]
    assert torch.isfinite(lo[keep]).all() and torch.isfinite(hi[keep]).all()
    lo2, hi2 = sp.propagate(c, r, H)
    assert torch.equal(lo.nan_to_num(), lo2.nan_to_num()) and torch.equal(hi.nan_to_num(), hi2.nan_to_num())
    with pytest.raises(ValueError, match=">= 0"):
        sp.propagate(c, -r.abs(), H)


# ---------------------------------------------------------------- pre_setprop_recipe_f32
def recipe_check(lo, hi, x, kernel, correlation, radius, hull, eps=1e-6):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
    B, nt = x.shape
    c, r, bad = sp.recipe_sets_host(x, kernel, correlation, radius)
    g, a = sp.tables(sp.recipe_key(kernel, nt, eps, correlation), hull)
    # sum|terms| includes the convolution's own products: the sets of |x| through |taps|
    ca, ra, _ = sp.recipe_sets_host(np.abs(np.nan_to_num(x)), np.abs(kernel), correlation,
                                    None if radius is None else radius)
    lo_h, hi_h = sp._bounds_host(c, r, g, a, bad)
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    nan = np.isnan(lo_h)
    assert np.array_equal(np.isnan(lo), nan) and np.array_equal(np.isnan(hi), nan)
    s = ca @ np.abs(sp._circulant(g)) + ra @ np.abs(sp._circulant(a))
    tol = 8 * (nt + 1 + len(kernel)) * U * s
    assert np.all(np.abs(lo - lo_h)[~nan] <= tol[~nan]) and np.all(np.abs(hi - hi_h)[~nan] <= tol[~nan])


@pytest.mark.parametrize("B,nt", [(0, 3), (1, 3), (3, 100), (4097, 100), (3, 999), (4, 4096), (4097, 3)])
@pytest.mark.parametrize("hull", sp.HULLS)
def test_recipe_on_component_views(gpu, B, nt, hull):
    torch.manual_seed(B + nt)
    t = torch.linspace(0, 10, nt)
    sol = torch.stack([torch.cos(t) + 0.05 * torch.randn(B, nt), torch.sin(t).expand(B, nt)], -1).to(gpu)   # [B, Nt, 2]
    x = sol[..., 0]
    lo, hi = sp.set_pre_bounds(x, SHO_K, hull=hull)
    assert lo.shape == (B, nt + 1) and lo.dtype == torch.float64
    recipe_check(lo, hi, x, SHO_K, False, None, hull)


@pytest.mark.parametrize("kernel,correlation", [(SHO_K, True), (K5, False), (K7, False), (K7, True),
                                                (np.array([0.3, -1.0, 0.5, 0.2]), False), (np.array([0.4, 1.1]), True)])
def test_recipe_kernels_and_correlation(gpu, kernel, correlation):
    torch.manual_seed(len(kernel))
    x = torch.randn(33, 150, device=gpu)
    lo, hi = sp.set_pre_bounds(x, kernel, correlation=correlation)
    recipe_check(lo, hi, x, kernel, correlation, None, "interval_fft")


def test_recipe_qhat_shapes(gpu):
    B, nt = 5, 100
    torch.manual_seed(6)
    x = torch.randn(B, nt, device=gpu)
    q = torch.rand(nt, device=gpu)
    qb = torch.rand(nt, B, device=gpu).t()                           # [B, Nt], strided
    for kernel, corr in ((SHO_K, False), (K7, False), (np.array([0.1, 1.0, -2.0, 0.7, 0.2]), True)):
        for radius in (0.25, torch.tensor(0.5, device=gpu), q, qb):
            lo, hi = sp.set_pre_bounds(x, kernel, correlation=corr, radius=radius)
            rq = radius.cpu().numpy() if isinstance(radius, torch.Tensor) else radius
            recipe_check(lo, hi, x, kernel, corr, rq, "interval_fft")
    with pytest.raises(ValueError, match="symmetric"):
        sp.set_pre_bounds(x, [1.0, -2.0, 0.5], radius=q)


def test_recipe_negative_strides_nan_row_and_bitwise_repeat(gpu):
    B, nt = 12, 100
    torch.manual_seed(8)
    buf = torch.randn(B, nt, device=gpu)
    buf[7, 50] = float("nan")
    buf[2, 0] = float("inf")
    key = sp.recipe_key(SHO_K, nt)
    g, a = sp._device_tables(key, "interval_fft", gpu)
    lo = torch.empty(B, nt + 1, dtype=torch.float64, device=gpu)
    hi = torch.empty_like(lo)
    last = ctypes.c_void_p(buf.data_ptr() + ((B - 1) * nt + nt - 1) * 4)
    taps = (ctypes.c_double * 3)(*SHO_K)
    rc = _lib.load_setprop().pre_setprop_recipe_f32(last, _lib.iarr64((-nt, -1)), B, nt, taps, 3, None, None, _lib.ptr(g),
                                                    _lib.ptr(a), _lib.ptr(lo), _lib.ptr(hi), 0, _lib.stream())
    _lib.check(rc, "pre_setprop_recipe_f32")
    x = buf.flip(0, 1)
    recipe_check(lo, hi, x, SHO_K, False, None, "interval_fft")
    assert torch.isnan(lo[B - 1 - 7]).all() and torch.isnan(lo[B - 1 - 2]).all()
    assert torch.isfinite(lo[0]).all()
    lq, hq = sp.set_pre_bounds(buf, SHO_K, radius=0.1)              # q-hat replaces every radius the NaN reaches
    assert torch.isnan(lq[7]).all() and torch.isfinite(lq[0]).all()
    lq2, hq2 = sp.set_pre_bounds(buf, SHO_K, radius=0.1)
    assert torch.equal(lq.nan_to_num(), lq2.nan_to_num()) and torch.equal(hq.nan_to_num(), hq2.nan_to_num())
    with pytest.raises(TypeError, match="fp32"):
        sp.set_pre_bounds(buf.double(), SHO_K)


def test_script_drop_ins_on_the_device(gpu):
    kernel = torch.tensor([1., -2., 1.]) + (10 / 99) ** 2 * torch.tensor([0, 1, 0])
    t = torch.linspace(0, 10, 100)
    x = torch.cos(t) + 0.05 * torch.randn(100)
    got = sp.set_PRE(x.to(gpu), kernel)
    want = sp.set_PRE(x, kernel)
    assert len(got) == len(want) == 101
    lo_g, lo_w = np.array([iv.inf for iv in got]), np.array([iv.inf for iv in want])
    hi_g, hi_w = np.array([iv.sup for iv in got]), np.array([iv.sup for iv in want])
    sc = np.abs(lo_w).max() + np.abs(hi_w).max()
    assert np.abs(lo_g - lo_w).max() <= 1e-12 * sc and np.abs(hi_g - hi_w).max() <= 1e-12 * sc
    code = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2]); import torch, numpy as np; "
            "from pre_set_prop import set_PRE; "
            "x = torch.stack([torch.cos(torch.linspace(0, 10, 100)), torch.sin(torch.linspace(0, 10, 100))], 1); "
            "a = set_PRE(x.cuda()); b = set_PRE(x.numpy()); "
            "d = max(max(abs(p.inf - q.inf), abs(p.sup - q.sup)) for p, q in zip(a, b)); "
            "s = max(max(abs(q.inf), abs(q.sup)) for q in b); print(len(a), len(b), d <= 1e-12 * s)")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "cp_pre_amd", "compat"), ROOT], cwd=ROOT,
                         capture_output=True, text=True, check=True).stdout.split()
    assert out == ["101", "101", "True"]
