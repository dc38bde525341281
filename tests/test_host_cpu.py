"""CPU-only checks: host logic of the drop-in surface, and that the C-ABI library loads and
exports every symbol include/cp_pre_hip.h declares (no compute calls without a GPU)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from cp_pre_amd import _dispatch, _lib
from cp_pre_amd import inductive_cp as icp
from cp_pre_amd.convops_1d import ConvOperator as Conv1D
from cp_pre_amd.convops_2d import ConvOperator as Conv2D
from cp_pre_amd.convops_2d import get_stencil, kernel_3d, pad_kernel
from oracle import conformal as oc


def _parse(key):
    tag, dom, order, taylor, scale = key.split("|")
    dom = {"none": None, "xy": ("x", "y"), "xyt": ("x", "y", "t"), "xt": ("x", "t")}.get(dom, dom)
    return tag, dom, int(order), int(taylor), float(scale)


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "cp_pre_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(pre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pre_abi_version() == _lib.PRE_ABI_VERSION == 8
    # the header's flag and error constants are the ones the ctypes mirror uses
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(PRE_(?:FLAG|E|OK)[A-Z_]*)\s+(-?\d+)", header)}
    assert consts["PRE_FLAG_HALO_X"] == 8 and len([k for k in consts if k.startswith("PRE_FLAG_")]) == 4
    for name, val in consts.items():
        assert getattr(_lib, name) == val, name
    # the spectral family's library (links hipFFT)
    header = open(os.path.join(ROOT, "include", "cp_pre_fft.h")).read()
    declared = set(re.findall(r"\bint\s+(pre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.FFT_SIGNATURES), declared ^ set(_lib.FFT_SIGNATURES)
    fft = _lib.load_fft()
    for name in declared:
        assert hasattr(fft, name), name
    assert fft.pre_fft_abi_version() == 1


def test_kernel_construction_matches_reference_bit_for_bit(golden):
    """The product's constructors against kernels dumped from the reference itself."""
    ks = golden["kernels"]
    for key in ks.files:
        tag, dom, order, taylor, scale = _parse(key)
        op = (Conv2D if tag == "2d" else Conv1D)(dom, order, scale=scale, taylor_order=taylor)
        ref = ks[key]
        if ref.size == 0:
            assert not hasattr(op, "kernel"), key
        else:
            assert hasattr(op, "kernel"), key
            assert np.array_equal(op.kernel.numpy(), ref), key


def test_constructor_error_behaviour():
    with pytest.raises(ValueError, match="Unknown Convolution Method"):
        Conv2D("x", 1, conv="fft")
    with pytest.raises(ValueError, match="Unknown Convolution Method"):
        Conv2D("x", 1, 1.0, 2, False)          # what Utils/VectorConvOps.py:33 does by accident
    D = Conv2D()                                # the 'empty' operator of the additive idiom
    assert not hasattr(D, "kernel") and D.conv == D.convolution
    with pytest.raises(AttributeError):
        D(torch.zeros(1, 3, 3, 3))
    assert not hasattr(Conv2D(("x", "y"), 1), "kernel")
    assert not hasattr(Conv1D("x", 3), "kernel")
    with pytest.raises(ValueError):
        get_stencil(3, 2)
    with pytest.raises(ValueError):
        kernel_3d(torch.zeros(3, 3), 5)
    assert Conv2D("t", 1, conv="spectral").conv.__name__ == "spectral_convolution"


def test_additive_kernel_idiom_and_taps():
    D_tt, D_l = Conv2D("t", 2), Conv2D(("x", "y"), 2)
    D = Conv2D()
    D.kernel = D_tt.kernel - 0.25 * D_l.kernel
    w, off = _dispatch.taps_of(_dispatch.host_kernel(D.kernel))
    got = {tuple(o): float(v) for o, v in zip(off.tolist(), w)}
    assert got == {(-1, 0, 0): 1.0, (1, 0, 0): 1.0, (0, 0, 0): -1.0, (0, -1, 0): -0.25, (0, 1, 0): -0.25,
                   (0, 0, -1): -0.25, (0, 0, 1): -0.25}
    # the y quirk: 'y' taps sit on the Nt axis; y_axis_fix moves them to Ny
    _, off_y = _dispatch.taps_of(_dispatch.host_kernel(Conv2D("y", 1).kernel))
    assert off_y.tolist() == [[-1, 0, 0], [1, 0, 0]]
    _, off_fix = _dispatch.taps_of(_dispatch.host_kernel(Conv2D("y", 1, y_axis_fix=True).kernel))
    assert off_fix.tolist() == [[0, 0, -1], [0, 0, 1]]
    # taylor-4: 5^3 kernel, all 9 taps one step before the centre in time
    _, off5 = _dispatch.taps_of(_dispatch.host_kernel(Conv2D(("x", "y"), 2, taylor_order=4).kernel))
    assert len(off5) == 9 and set(off5[:, 0].tolist()) == {-1}
    assert pad_kernel(torch.zeros(2, 5, 6, 7), D.kernel).shape == (5, 7, 6)


def test_dtype_and_shape_errors_before_any_gpu_work():
    D = Conv2D("x", 1)
    with pytest.raises(RuntimeError, match="Double"):
        D(torch.zeros(1, 3, 3, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        D(torch.zeros(3, 3, 3))
    with pytest.raises(NotImplementedError):
        D.convolution(torch.zeros(1, 3, 3, 3), torch.ones(2, 2, 2))


def test_no_cpu_fallback_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        Conv2D("x", 1)(torch.zeros(1, 3, 3, 3))
    with pytest.raises(RuntimeError, match="no HIP device"):
        icp.calibrate(np.zeros(5, np.float32), 5, 0.5)


def _build_c_client(out):
    """gcc -std=c99: the header and the library are consumable from plain C (no C++, no torch)."""
    import subprocess
    lib = os.path.join(ROOT, "cp_pre_amd")
    for h in ("cp_pre_hip.h", "cp_pre_fft.h"):
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                               os.path.join(ROOT, "include", h)])
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "c_abi", "abi_check.c"),
                           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-L" + lib, "-lcp_pre_hip", "-L/opt/rocm/lib",
                           "-lamdhip64", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    return str(out)


def test_c99_client_compiles_and_links(tmp_path):
    _lib.load()                                     # the library must exist (built by __graft_entry__.build())
    assert os.path.exists(_build_c_client(tmp_path / "abi_check"))
    # ... and calls every symbol the header declares (run on the GPU by test_gpu_parity.py::test_c_abi_client)
    header = open(os.path.join(ROOT, "include", "cp_pre_hip.h")).read()
    client = open(os.path.join(ROOT, "tests", "c_abi", "abi_check.c")).read()
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(pre_[a-z0-9_]+)\s*\(", header))
    assert len(declared) == 29 and not [d for d in declared if d + "(" not in client]


def test_graft_build_entry_point():
    """The driver's "does it build" check (`__graft_entry__.build()`: make + load + version assertions) must pass on an
    already-built tree too - round 4 bumped the ABI and left a literal 7 in it, which nothing here exercised."""
    import __graft_entry__
    assert __graft_entry__.build() is None


def test_missing_extension_fails_loudly(monkeypatch, tmp_path):
    """No silent fallback when libcp_pre_hip.so / libcp_pre_fft.so are absent: loading raises ImportError."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "libcp_pre_hip.so"))
    with pytest.raises(ImportError, match="no CPU fallback"):
        _lib.load()
    monkeypatch.setattr(_lib, "_fft", None)
    monkeypatch.setattr(_lib, "FFT_SO_PATH", str(tmp_path / "libcp_pre_fft.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_fft()


def test_library_of_another_abi_version_fails_loudly(monkeypatch):
    """A stale shared object (same symbol names, other signatures) must not load: every library of the table is checked
    against the version its signatures were written for, libcp_pre_fft.so included."""
    assert "fft" in _lib._LIBS and len(_lib._LIBS) == 8
    for key, (cache, _, _, version, _) in _lib._LIBS.items():
        monkeypatch.setattr(_lib, cache, None)
        monkeypatch.setattr(_lib, version, getattr(_lib, version) + 1)
        with pytest.raises(ImportError, match="ABI version"):
            _lib._load(key)
    with pytest.raises(ImportError, match="libcp_pre_fft.so has ABI version 1"):
        _lib.load_fft()


def test_compat_import_paths_resolve_to_the_product_classes():
    """cp_pre_amd/compat on sys.path gives the reference's own import lines (INTEGRATION.md level 1)."""
    import importlib
    import sys
    from cp_pre_amd import residuals
    compat = os.path.join(ROOT, "cp_pre_amd", "compat")
    sys.path.insert(0, compat)
    try:
        names = ["Utils.ConvOps_2d", "Utils.ConvOps_1d", "Utils.VectorConvOps", "Utils.ConvOps_Spatial", "Utils.boundary_conditions",
                 "Utils.VectorConvOps_Spatial", "Neural_PDE.UQ.inductive_cp", "ConvOps_2d", "ConvOps_1d", "PRE_estimations"]
        mods = {n: importlib.import_module(n) for n in names}
        assert mods["Utils.ConvOps_2d"].ConvOperator is Conv2D and mods["ConvOps_2d"].ConvOperator is Conv2D
        assert mods["Utils.ConvOps_1d"].ConvOperator is Conv1D and mods["ConvOps_1d"].ConvOperator is Conv1D
        assert mods["PRE_estimations"].PRE_NS is residuals.PRE_NS
        for fn in ("calibrate", "modulation_func", "ncf_metric_joint", "emp_cov", "emp_cov_joint"):
            assert getattr(mods["Neural_PDE.UQ.inductive_cp"], fn) is getattr(icp, fn)
        for cls in ("Divergence", "Gradient", "Curl", "Laplace", "dot", "cross", "vectorize"):
            assert hasattr(mods["Utils.VectorConvOps"], cls)
    finally:
        sys.path.remove(compat)
        for n in [k for k in sys.modules if k.split(".")[0] in ("Utils", "Neural_PDE", "ConvOps_2d", "ConvOps_1d", "PRE_estimations")]:
            del sys.modules[n]


def test_divergence_accepts_the_reference_spelling_require_grad():
    """``Utils/VectorConvOps.py:30`` spells the argument ``require_grad``; both spellings build the same two operators."""
    from cp_pre_amd import vector_convops as V
    a, b, c = V.Divergence(require_grad=True), V.Divergence(requires_grad=True), V.Divergence(("x", "y"), 1, 2.0, 2, require_grad=False)
    for op in ("grad_x", "grad_y"):
        assert torch.equal(getattr(a, op).kernel, getattr(b, op).kernel)
        assert torch.equal(getattr(c, op).kernel, 2.0 * getattr(a, op).kernel)
        assert vars(getattr(a, op)).keys() == vars(getattr(b, op)).keys()
    with pytest.raises(TypeError):
        V.Divergence(require_grads=True)


def test_rank_arithmetic_matches_numpy_higher():
    for n in (7, 100, 256, 4096, 8192, 65536):
        for a in oc.ALPHA_LEVELS:
            try:
                k = oc.kth_index(n, a)
            except ValueError:
                with pytest.raises(ValueError):
                    icp.kth_index(n, n, a)
                continue
            assert icp.kth_index(n, n, a) == k
            if n <= 256:
                s = np.random.default_rng(n).standard_normal(n).astype(np.float32)
                assert np.sort(s)[k] == oc.calibrate(s, n, a)


def test_spectral_family_has_no_cpu_fallback_either():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    D = Conv2D(("x", "y"), 2)
    for call in (lambda: D.spectral_convolution(torch.zeros(1, 4, 4, 4)), lambda: D.differentiate(torch.zeros(1, 4, 4, 4)),
                 lambda: D.integrate(torch.zeros(1, 4, 4, 4))):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
