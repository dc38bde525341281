"""CPU tests of the ODE operator drop-in (cp_pre_amd.convops_0d, cp_pre_amd.ode) and of libcp_pre_ode.so's exported ABI.
The stencil table and the constructor quirks are checked against tests/golden/convops_0d.npz (made by running the
reference's Utils/ConvOps_0d.py); the device passes are covered by tests/test_gpu_convops_0d.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cp_pre_amd import _lib, ode
from cp_pre_amd.convops_0d import ConvOperator, get_stencil, host_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "convops_0d.npz"))


def test_stencil_table_matches_the_reference():
    seen = 0
    for d in (0, 1, 2, 3, None):
        for t in (2, 4, 6, 8):
            key = f"stencil_d{d}_t{t}"
            if key + "_invalid" in G.files:
                with pytest.raises(ValueError, match="Invalid stencil parameters"):
                    get_stencil(d, t)
            else:
                got = get_stencil(d, t)
                assert got.dtype == torch.float32
                assert np.array_equal(got.numpy(), G[key])
                seen += 1
    assert seen == 9                                           # order 0 at every Taylor order, plus the five derivatives


def test_constructor_quirks():
    op = ConvOperator()                                        # order=None: the bare except swallows the ValueError
    assert hasattr(op, "kernel") == bool(G["ctor_default_has_kernel"])
    assert op.conv == op.convolution
    op = ConvOperator(order=2, scale=0.5, taylor_order=4, requires_grad=True)
    assert np.array_equal(op.kernel.numpy(), G["ctor_scaled_kernel"])
    assert op.kernel.requires_grad == bool(G["ctor_scaled_requires_grad"])        # an attribute, not autograd
    assert (op.kernel.requires_grad_ is True) == bool(G["ctor_scaled_requires_grad_attr"])
    assert ConvOperator(order=1, conv="spectral").conv.__name__ == "spectral_convolution"
    with pytest.raises(ValueError, match="Unknown Convolution Method"):
        ConvOperator(order=1, conv="fft")


@pytest.mark.parametrize("n", [2, 4, 9])
def test_kernels_the_library_does_not_serve_raise(n):
    with pytest.raises(NotImplementedError):
        ConvOperator(order=1).convolution(torch.zeros(2, 10), kernel=torch.ones(n))
    with pytest.raises(NotImplementedError):
        host_taps(torch.ones(n))


def test_a_kernel_argument_replaces_the_operator_kernel():
    op = ConvOperator(order=1)
    k = torch.ones(4)
    with pytest.raises(NotImplementedError):
        op.convolution(torch.zeros(1, 5), kernel=k)
    assert op.kernel is k


def test_ode_residual_validates_its_terms():
    k3 = [1.0, -2.0, 1.0]
    with pytest.raises(ValueError, match="1 to 6 terms"):
        ode.ODEResidual([(0, k3, None)] * 7)
    with pytest.raises(ValueError, match="1 to 6 terms"):
        ode.ODEResidual([])
    with pytest.raises(ValueError, match="odd length"):
        ode.ODEResidual([(0, [1.0, 1.0], None)])
    with pytest.raises(ValueError, match="odd length"):
        ode.ODEResidual([(0, np.ones(9, np.float32), None)])
    with pytest.raises(ValueError, match="odd length"):
        ode.ODEResidual([(0, np.ones((3, 3), np.float32), None)])
    with pytest.raises(IndexError):
        ode.ODEResidual([(-1, k3, None)])
    with pytest.raises(ValueError, match="component, kernel, coeff"):
        ode.ODEResidual([(0, k3)])
    r = ode.ODEResidual([(2, k3, None)])
    with pytest.raises(IndexError, match="out of range"):
        r.residual(torch.zeros(2, 5, 2))                        # validated before any device work
    r = ode.ODEResidual([(0, k3, np.ones(4, np.float32))])
    with pytest.raises(ValueError, match="coefficient row has 4 values"):
        r._coeff(0, "cpu", 5)
    with pytest.raises(ValueError, match="one shape"):
        ode.ODEResidual([(0, k3, None)]).residual([torch.zeros(2, 5), torch.zeros(2, 6)])


def test_script_constructors_restate_the_reference_kernels():
    m, c, k = (float(v) for v in G["dho_mck"])
    dt = float(G["dho_dt"])
    comb = ode.DHO(m, c, k, dt)
    assert np.array_equal(comb.terms[0][1].numpy(), G["dho_kernel_combined"])
    split = ode.DHO(m, c, k, dt, split=True)
    assert [t[0] for t in split.terms] == [1, 0]
    assert np.array_equal(split.terms[0][1].numpy(), G["dho_kernel_r1"])
    assert np.array_equal(split.terms[1][1].numpy(), G["dho_kernel_r2"])
    kin = ode.DHO_kinematic(dt)
    assert np.array_equal(kin.terms[0][1].numpy(), -G["dho_kernel_r4"])
    assert np.array_equal(kin.terms[1][1].numpy(), G["dho_kernel_r3"])
    t = G["sho_t"]
    sho = ode.SHO(float(G["sho_omega"]), t[1] - t[0])
    assert np.array_equal(sho.terms[0][1].numpy(), G["sho_kernel"])
    b = ode.Bessel(G["bessel_x"], 1, G["bessel_x"][1] - G["bessel_x"][0])
    assert len(b.terms) == 3 and all(term[0] == 0 for term in b.terms)


def test_compat_import_path():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from Utils.ConvOps_0d import ConvOperator, get_stencil; "
            "import cp_pre_amd.convops_0d as m; assert ConvOperator is m.ConvOperator and get_stencil is m.get_stencil")
    subprocess.check_call([sys.executable, "-c", code, os.path.join(ROOT, "cp_pre_amd", "compat")], cwd=ROOT)


def test_ode_library_exports_what_its_header_declares():
    so = _lib.ODE_SO_PATH
    assert os.path.exists(so), "libcp_pre_ode.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(os.path.join(ROOT, "include", "cp_pre_ode.h")).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == {"pre_ode_abi_version", "pre_ode_stencil_f32", "pre_ode_residual_f32", "pre_ode_wgrad_f32"}
    assert exported == declared and set(_lib.ODE_SIGNATURES) == declared
    for name, value in (("PRE_ODE_ABI_VERSION", _lib.PRE_ODE_ABI_VERSION), ("PRE_ODE_MAX_TAPS", _lib.PRE_ODE_MAX_TAPS),
                        ("PRE_ODE_MAX_TERMS", _lib.PRE_ODE_MAX_TERMS), ("PRE_ODE_FLAG_ABS", _lib.PRE_ODE_FLAG_ABS),
                        ("PRE_ODE_WGRAD_BLOCKS", _lib.PRE_ODE_WGRAD_BLOCKS)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == value, name
    assert _lib.load_ode().pre_ode_abi_version() == _lib.PRE_ODE_ABI_VERSION


def test_term_struct_layout_matches_the_header(tmp_path):
    """A C99 client of cp_pre_ode.h: compiles pedantically, links against libcp_pre_ode.so and agrees with the ctypes
    struct on the size and offsets of pre_ode_term_t."""
    src = tmp_path / "ode_client.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cp_pre_ode.h"\n'
        "int main(void) {\n"
        "  printf(\"%d %zu %zu %zu %zu %zu %zu\\n\", pre_ode_abi_version(), sizeof(pre_ode_term_t),\n"
        "         offsetof(pre_ode_term_t, sB), offsetof(pre_ode_term_t, sT), offsetof(pre_ode_term_t, c),\n"
        "         offsetof(pre_ode_term_t, k), offsetof(pre_ode_term_t, taps));\n"
        "  return 0;\n}\n")
    lib = os.path.join(ROOT, "cp_pre_amd")
    exe = tmp_path / "ode_client"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           os.path.join(ROOT, "include", "cp_pre_ode.h")])
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + lib, "-l:libcp_pre_ode.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64", "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = _lib.PreOdeTerm
    assert got == [_lib.PRE_ODE_ABI_VERSION, __import__("ctypes").sizeof(T), T.sB.offset, T.sT.offset, T.c.offset,
                   T.k.offset, T.taps.offset]


def test_no_gpu_means_an_error_not_a_fallback():
    if torch.cuda.is_available():                               # (on a GPU box the staged call simply runs)
        assert ConvOperator(order=1)(torch.zeros(1, 8)).device.type == "cpu"
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        ConvOperator(order=1)(torch.zeros(1, 8))
    with pytest.raises(RuntimeError, match="no HIP device"):
        ode.SHO(1.0, 0.1).residual(torch.zeros(1, 8, 1))
