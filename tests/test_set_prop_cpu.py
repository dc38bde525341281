"""CPU tests of PRE set propagation (cp_pre_amd.set_prop) and of libcp_pre_setprop.so's exported ABI.

The oracle is a literal float64 restatement, generator by generator, of the reference's Inverted_bounds/intervalFFT.py and
SHO.py:set_PRE (350-407): every interval becomes a 2-D zonotope, every rotation, complex product and Minkowski sum is built
explicitly, and the real-part interval hull is taken at the end.  The reference itself cannot execute (its
``from zonopy import zonotope, interval`` resolves to an empty package), so it is restated here rather than run.  The
device passes are covered by tests/test_gpu_set_prop.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cp_pre_amd import _lib
from cp_pre_amd import set_prop as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (5, 8, 13, 32, 101)
SHO_K = np.array([1., -2., 1.]) + (10 / 99) ** 2 * np.array([0., 1., 0.])
K5 = np.array([-1 / 12, 4 / 3, -5 / 2, 4 / 3, -1 / 12])
K7 = np.array([1 / 90, -3 / 20, 3 / 2, -49 / 18, 3 / 2, -3 / 20, 1 / 90])


def _ensure_lib():
    if not os.path.exists(_lib.SETPROP_SO_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cp_pre_amd", "csrc"), "../libcp_pre_setprop.so"])


# ---------------------------------------------------------------- the literal oracle
def _rot(theta):
    return np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])


def literal_propagate(lo, hi, H):
    """intervalFFT -> complex_prod with H -> inverse_intervalFFT -> Real, as the reference composes them (float64).
    A zonotope is (centre [2], generators [n, 2])."""
    N = len(lo)
    Z = []
    for x0, x1 in zip(lo, hi):                                        # convert_interval_to_zonotope
        rad = (x1 - x0) / 2
        Z.append((np.array([(x0 + x1) / 2, 0.0]), np.array([[rad, 0.0], [0.0, 0.0]])))
    F = []
    for h in range(N):                                                # intervalFFT_
        thetas = 2 * np.pi / N * np.arange(N) * h
        cs, gs = [], []
        for i in range(N):
            M = np.array([[np.cos(thetas[i]), 0.0], [-np.sin(thetas[i]), 0.0]])
            cs.append(M @ Z[i][0])
            gs.append(Z[i][1] @ M.T)
        F.append((np.sum(cs, axis=0), np.concatenate(gs)))
    P = []
    for (c, G), C in zip(F, H):                                       # complex_prod: the zip truncates H to N entries
        R = abs(C) * _rot(np.arctan2(C.imag, C.real))
        P.append((R @ c, G @ R.T))
    out = []
    for k in range(N):                                                # inverse_intervalFFT_, then Real
        thetas = 2 * np.pi / N * np.arange(N) * k
        c = sum(_rot(thetas[h]) @ P[h][0] for h in range(N)) / N
        G = np.concatenate([P[h][1] @ _rot(thetas[h]).T for h in range(N)]) / N
        w = np.abs(G[:, 0]).sum()
        out.append((c[0] - w, c[0] + w))
    return np.array(out)


def literal_recipe_sets(field, kernel, correlation=False):
    """SHO.py:360-396 up to the interval set (lower, upper lists) and the size-N inverse spectrum."""
    signal = np.concatenate(([0], np.asarray(field, np.float64), [0]))
    N = len(signal)
    kernel_fft = np.fft.fft(np.concatenate((np.asarray(kernel, np.float64), np.zeros(N - len(kernel)))))
    if correlation:
        kernel_fft.imag *= -1
    convolved = np.fft.ifft(np.fft.fft(signal) * kernel_fft)
    return convolved, kernel_fft


def literal_set_PRE(field, kernel, correlation=False, eps=1e-6):
    convolved, kernel_fft = literal_recipe_sets(field, kernel, correlation)
    inverse_kernel = 1 / (kernel_fft + eps)
    sets = [(x.real, x.real) for x in convolved[1:4]] + [(-abs(x.real), abs(x.real)) for x in convolved[4:-1]] \
        + [(convolved[-1].real, convolved[-1].real)]
    lo, hi = zip(*sets)
    return literal_propagate(lo, hi, inverse_kernel)


def scale(c, r, g, a):
    """sum_j |terms| per output: the yardstick of the agreement bound."""
    return np.abs(c) @ np.abs(sp._circulant(g)) + np.abs(r) @ np.abs(sp._circulant(a))


def noisy_cosine(nt, seed):
    rng = np.random.default_rng(seed)
    t = np.linspace(0, 10, nt)
    return (np.cos(t) + 0.05 * rng.standard_normal(nt)).astype(np.float32)


# ---------------------------------------------------------------- closed form == literal pipeline
@pytest.mark.parametrize("n", NS)
def test_closed_form_matches_the_literal_pipeline_on_random_sets(n):
    rng = np.random.default_rng(n)
    c, r = rng.standard_normal(n), rng.random(n)
    H = 1 / (np.fft.fft(np.r_[rng.standard_normal(3), np.zeros(n - 3)]) + 0.3)
    want = literal_propagate(c - r, c + r, H)
    lo, hi = sp.propagate(c, r, H)
    g, a = sp.tables(H)
    tol = 1e-12 * scale(c[None], r[None], g, a)[0]
    assert np.all(np.abs(lo - want[:, 0]) <= tol) and np.all(np.abs(hi - want[:, 1]) <= tol)


@pytest.mark.parametrize("n,kernel,correlation", [(n, k, cr) for n in NS for k, cr in ((SHO_K, False), (SHO_K, True),
                                                    (K5, False), (K7, True)) if len(k) <= n + 1])
def test_recipe_matches_the_literal_set_PRE(n, kernel, correlation):
    nt = n - 1
    x = noisy_cosine(nt, n)
    want = literal_set_PRE(x, kernel, correlation)
    lo, hi = sp.set_pre_bounds(torch.from_numpy(x), kernel, correlation=correlation)
    assert lo.shape == (nt + 1,)                                    # N' = Nt + 1
    c, r, _ = sp.recipe_sets_host(x[None], kernel, correlation)
    g, a = sp.tables(sp.recipe_key(kernel, nt, 1e-6, correlation))
    tol = 1e-12 * scale(c, r, g, a)[0]
    assert np.all(np.abs(lo - want[:, 0]) <= tol) and np.all(np.abs(hi - want[:, 1]) <= tol)


def test_sho_script_size():
    """The SHO recipe of the script: 100 steps, dt = 10/99, N' = 101, a torch fp32 kernel."""
    kernel = torch.tensor([1., -2., 1.]) + (10 / 99) ** 2 * torch.tensor([0, 1, 0])
    x = noisy_cosine(100, 7)
    want = literal_set_PRE(x, kernel.numpy())
    got = sp.set_PRE(torch.from_numpy(x), kernel)
    assert len(got) == 101 and all(isinstance(iv, sp.Interval) for iv in got)
    lo = np.array([iv.inf for iv in got])
    hi = np.array([float(iv.sup) for iv in got])
    assert np.abs(lo - want[:, 0]).max() <= 1e-12 * np.abs(want).max() * 101
    assert np.abs(hi - want[:, 1]).max() <= 1e-12 * np.abs(want).max() * 101
    mid = 0.5 * (got[50].inf + got[50].sup)
    assert mid in got[50] and got[50].sup + 1.0 not in got[50]


def test_compat_pre_set_prop_matches_its_script():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from pre_set_prop import set_PRE; import numpy as np; "
            "x = np.stack([np.cos(np.linspace(0, 10, 60)), np.sin(np.linspace(0, 10, 60))], 1); "
            "b = set_PRE(x); print(len(b)); print(' '.join(repr(v) for iv in b for v in (iv.inf, iv.sup)))")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "cp_pre_amd", "compat")], cwd=ROOT,
                         capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(out[0]) == 61
    got = np.array([float(v) for v in out[1].split()]).reshape(-1, 2)
    dt = 0.1010101
    kernel = np.array([1, -2, 1]) + dt ** 2 * np.array([0, 1, 0])
    want = literal_set_PRE(np.cos(np.linspace(0, 10, 60)), kernel, eps=1e-16)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() * 61


# ---------------------------------------------------------------- properties
@pytest.mark.parametrize("n", (8, 33, 101))
def test_exact_hull_is_inside_the_reference_hull_and_both_contain_the_image(n):
    rng = np.random.default_rng(100 + n)
    c, r = rng.standard_normal((4, n)), rng.random((4, n))
    H = sp.inverse_spectrum(SHO_K, n + 1, 1e-6)[:n]
    lo_i, hi_i = sp.propagate(c, r, H)
    lo_e, hi_e = sp.propagate(c, r, H, hull="exact")
    slack = 1e-9 * (np.abs(lo_i).max() + np.abs(hi_i).max())
    assert np.all(lo_e >= lo_i - slack) and np.all(hi_e <= hi_i + slack)
    assert np.median((hi_e - lo_e) / (hi_i - lo_i)) < 1.0
    G = sp._circulant(sp.tables(H)[0])                           # L(x) = Re(ifft(fft(x) * H)) = x @ G
    pts = [c + r * rng.uniform(-1, 1, (4, n)) for _ in range(8)] + [c + r * rng.choice([-1, 1], (4, n)) for _ in range(8)]
    for x in pts:
        y = x @ G
        assert np.all(y >= lo_e - slack) and np.all(y <= hi_e + slack)
        assert np.allclose(y[0], np.fft.ifft(np.fft.fft(x[0]) * H).real)


def test_spectrum_is_the_size_N_one_truncated():
    nt = 20
    x = noisy_cosine(nt, 3)[None]
    lo, hi = sp.set_pre_bounds(x, SHO_K)
    c, r, _ = sp.recipe_sets_host(x, SHO_K)
    H_trunc = sp.inverse_spectrum(SHO_K, nt + 2, 1e-6)[:nt + 1]
    lo2, hi2 = sp.propagate(c - 0, r, H_trunc)
    assert np.allclose(lo, lo2, rtol=0, atol=1e-13) and np.allclose(hi, hi2, rtol=0, atol=1e-13)
    lo3, _ = sp.propagate(c, r, sp.inverse_spectrum(SHO_K, nt + 1, 1e-6))
    assert np.abs(lo3 - lo).max() > 1e-6                           # a size-N' spectrum is a different operator


def test_correlation_conjugates_the_spectrum():
    K = np.array([0.3, -1.0, 0.5, 0.2])
    assert np.allclose(sp.inverse_spectrum(K, 16, 1e-6, correlation=True), np.conj(sp.inverse_spectrum(K, 16, 1e-6)),
                       rtol=0, atol=1e-15)
    x = noisy_cosine(30, 5)
    c0, _, _ = sp.recipe_sets_host(x[None], K)
    c1, _, _ = sp.recipe_sets_host(x[None], K, correlation=True)
    conv, _ = literal_recipe_sets(x, K, correlation=True)
    assert np.allclose(c1[0, :3], conv[1:4].real, atol=1e-13) and not np.allclose(c0, c1)


@pytest.mark.parametrize("kernel", (K5, K7))
def test_edge_points_are_three_whatever_the_kernel_length(kernel):
    x = noisy_cosine(40, 11)[None]
    c, r, _ = sp.recipe_sets_host(x, kernel)
    n = 41
    assert set(np.flatnonzero(c[0])) <= {0, 1, 2, n - 1} and np.all(c[0, [0, 1, 2, n - 1]] != 0)
    assert np.all(r[0, [0, 1, 2, n - 1]] == 0) and np.all(r[0, 3:n - 1] > 0)


def test_short_fields_and_bad_arguments_raise():
    for nt in (0, 1, 2):
        with pytest.raises(ValueError, match="Nt >= 3"):
            sp.set_pre_bounds(np.zeros((2, nt), np.float32), SHO_K)
    with pytest.raises(ValueError, match="does not fit"):
        sp.set_pre_bounds(np.zeros((1, 4), np.float32), K7)
    assert sp.set_pre_bounds(np.zeros((1, 3), np.float32), SHO_K)[0].shape == (1, 4)
    with pytest.raises(ValueError, match=">= 0"):
        sp.propagate(np.zeros(5), -np.ones(5), np.ones(5))
    with pytest.raises(ValueError, match="hull"):
        sp.propagate(np.zeros(5), np.ones(5), np.ones(5), hull="box")
    with pytest.raises(ValueError, match="odd kernel"):
        sp.set_pre_bounds(np.zeros((1, 10), np.float32), [1.0, -1.0], correlation=True, radius=0.1)
    with pytest.raises(ValueError, match="symmetric"):
        sp.set_pre_bounds(np.zeros((1, 10), np.float32), [1.0, -1.0, 0.5], radius=0.1)


def test_non_finite_row_is_nan_and_others_are_not():
    x = np.stack([noisy_cosine(30, s) for s in range(3)])
    x[1, 12] = np.nan
    lo, hi = sp.set_pre_bounds(x, SHO_K, radius=0.01)
    assert np.isnan(lo[1]).all() and np.isnan(hi[1]).all()
    assert np.isfinite(lo[[0, 2]]).all() and np.isfinite(hi[[0, 2]]).all()


def test_tables_are_keyed_by_value():
    kernel = torch.tensor([1., -2., 1.])
    x = noisy_cosine(30, 2)[None]
    lo1, _ = sp.set_pre_bounds(x, kernel)
    kernel[1] = -1.9                                                 # in place: same tensor, new values
    lo2, _ = sp.set_pre_bounds(x, kernel)
    lo3, _ = sp.set_pre_bounds(x, torch.tensor([1., -1.9, 1.]))
    assert not np.allclose(lo1, lo2) and np.array_equal(lo2, lo3)


# ---------------------------------------------------------------- calibrated mode: the q-hat index mapping
def residual(x, kernel):
    """Utils/ConvOps_0d.py's residual: cross-correlation with zero padding k//2, float64."""
    x = np.asarray(x, np.float64)
    k = len(kernel)
    xp = np.pad(x, ((0, 0), (k // 2, k // 2)))
    return sum(kernel[j] * xp[:, j:j + x.shape[1]] for j in range(k))


@pytest.mark.parametrize("kernel,correlation", [(SHO_K, False), (K5, False), (K7, False), (SHO_K, True),
                                                (np.array([0.5, -2.0, 1.0]), True), (np.array([0.1, 1.0, -2.0, 0.7, 0.2]), True),
                                                (np.array([0.3, 0.1, 1.0, -2.0, 0.7, 0.2, -0.4]), True), (np.array([2.0]), False)])
def test_qhat_index_mapping_against_the_literal_construction(kernel, correlation):
    nt = 40
    x = noisy_cosine(nt, 21).astype(np.float64)
    x[:4] = x[-4:] = 0                                              # no circular wrap reaches an in-range step
    conv, _ = literal_recipe_sets(x, kernel, correlation)
    res = residual(x[None], kernel)[0]
    shift = sp.qhat_shift(len(kernel), correlation)
    matched = 0
    for n in range(4, nt + 1):                                      # the interior indices 4 .. N-2
        t = n + shift
        if 0 <= t < nt:
            assert abs(conv[n].real - res[t]) <= 1e-12 * (np.abs(kernel).sum() * np.abs(x).max()), (n, t)
            matched += 1
    assert matched >= nt - 6
    # q-hat = |residual| reproduces the uncalibrated recipe exactly where the mapping covers it
    lo, hi = sp.set_pre_bounds(x[None].astype(np.float32), kernel, correlation=correlation)
    lq, hq = sp.set_pre_bounds(x[None].astype(np.float32), kernel, correlation=correlation,
                               radius=np.abs(residual(x[None].astype(np.float32), kernel)).astype(np.float32))
    assert np.allclose(lq, lo, rtol=0, atol=1e-6 * np.abs(lo).max()) and np.allclose(hq, hi, rtol=0, atol=1e-6 * np.abs(hi).max())


def test_qhat_shapes_replace_the_interior_radii_only():
    nt, B = 30, 3
    x = np.stack([noisy_cosine(nt, s) for s in range(B)])
    c0, r0, _ = sp.recipe_sets_host(x, SHO_K)
    q = np.linspace(0.1, 0.4, nt).astype(np.float32)
    for radius, want in ((0.25, np.full((B, nt), np.float32(0.25))), (q, np.broadcast_to(q, (B, nt))),
                         (np.stack([q, 2 * q, 3 * q]), np.stack([q, 2 * q, 3 * q]))):
        c, r, _ = sp.recipe_sets_host(x, SHO_K, radius=radius)
        assert np.array_equal(c, c0) and np.array_equal(r[:, [0, 1, 2, nt]], r0[:, [0, 1, 2, nt]])
        n = np.arange(4, nt + 1)
        assert np.array_equal(r[:, n - 1], want[:, n - 2].astype(np.float64))       # t = n - 2 for 3 symmetric taps
    with pytest.raises(ValueError, match="radius must be"):
        sp.set_pre_bounds(x, SHO_K, radius=np.zeros(nt + 1))


# ---------------------------------------------------------------- header <-> binding
def test_setprop_library_exports_what_its_header_declares():
    _ensure_lib()
    so = _lib.SETPROP_SO_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(os.path.join(ROOT, "include", "cp_pre_setprop.h")).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == {"pre_setprop_abi_version", "pre_setprop_bounds_f64", "pre_setprop_recipe_f32"}
    assert exported == declared and set(_lib.SETPROP_SIGNATURES) == declared
    for name, value in (("PRE_SETPROP_ABI_VERSION", _lib.PRE_SETPROP_ABI_VERSION),
                        ("PRE_SETPROP_MAX_TAPS", _lib.PRE_SETPROP_MAX_TAPS), ("PRE_SETPROP_FLAG_F64", _lib.PRE_SETPROP_FLAG_F64),
                        ("PRE_SETPROP_FLAG_CORRELATION", _lib.PRE_SETPROP_FLAG_CORRELATION)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == value, name
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from cp_pre_amd import _lib; "
            "print(_lib.load_setprop().pre_setprop_abi_version())")
    got = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, check=True).stdout.split()[-1]
    assert int(got) == _lib.PRE_SETPROP_ABI_VERSION


def test_c99_client_compiles_and_checks_arguments(tmp_path):
    """A C99 client of cp_pre_setprop.h: compiles pedantically, links against libcp_pre_setprop.so, and gets the argument
    errors back without a device (every check runs before a launch)."""
    _ensure_lib()
    src = tmp_path / "setprop_client.c"
    src.write_text(
        '#include <stdio.h>\n#include "cp_pre_setprop.h"\n'
        "int main(void) {\n"
        "  int64_t s[2] = {4, 1};\n  double taps[3] = {1, -2, 1}, asym[3] = {1, -2, 0.5};\n  float q = 1.0f;\n"
        "  printf(\"%d %d %d %d %d %d %d\\n\", pre_setprop_abi_version(),\n"
        "         pre_setprop_bounds_f64(0, s, 0, s, 0, 4, 0, 0, 0, 0, 0, 0),\n"
        "         pre_setprop_bounds_f64(0, s, 0, s, 1, 0, 0, 0, 0, 0, 0, 0),\n"
        "         pre_setprop_recipe_f32(0, s, 1, 2, taps, 3, 0, 0, 0, 0, 0, 0, 0, 0),\n"
        "         pre_setprop_recipe_f32(0, s, 1, 8, taps, 8, 0, 0, 0, 0, 0, 0, 0, 0),\n"
        "         pre_setprop_recipe_f32(0, s, 0, 8, asym, 3, &q, s, 0, 0, 0, 0, 0, 0),\n"
        "         pre_setprop_recipe_f32(0, s, 0, 8, asym, 3, &q, s, 0, 0, 0, 0, PRE_SETPROP_FLAG_CORRELATION, 0));\n"
        "  return 0;\n}\n")
    lib = os.path.join(ROOT, "cp_pre_amd")
    exe = tmp_path / "setprop_client"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           os.path.join(ROOT, "include", "cp_pre_setprop.h")])
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + lib, "-l:libcp_pre_setprop.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64", "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_lib.PRE_SETPROP_ABI_VERSION, _lib.PRE_OK, _lib.PRE_E_SHAPE, _lib.PRE_E_SHAPE, _lib.PRE_E_UNSUPPORTED,
                   _lib.PRE_E_UNSUPPORTED, _lib.PRE_OK]
    assert ctypes.sizeof(ctypes.c_int64) == 8
