"""CPU tests of the physics-informed residual losses (cp_pre_amd.losses, libcp_pre_vjp.so):
  * the closed-form vector-Jacobian products the kernels of csrc/residual_vjp.hip compute (include/cp_pre_vjp.h), restated
    with F.conv3d / F.conv2d and flipped kernels, against torch autograd of the oracle's expressions, in fp64;
  * the exported ABI against include/cp_pre_vjp.h and the ctypes binding, a C99 client;
  * the validation that happens before any device work.
The device passes are covered by tests/test_gpu_losses.py."""
import os
import re
import subprocess

import pytest
import torch

from conftest import rel_err
from losses_helpers import D, DT_, _k64, _mask, ns_kernels
from oracle import residuals as orr
from oracle.convops import ConvOperator1D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_vjp.h")
DT, DX, DY, NU = 0.01, 1 / 64, 1 / 32, 0.001


# ------------------------------------------------------------------ the formulas, in fp64, from the oracle's kernels
def ns_momentum64(vars, ks):
    Kt, Kx, Ky, KL = ks
    u, v, p = vars[:, 0], vars[:, 1], vars[:, 2]
    rx = D(u, Kt)*DX*DY + u*D(u, Kx)*DT*DY + v*D(u, Ky)*DT*DX - NU*D(u, KL)*DT + D(p, Kx)*DT*DY
    ry = D(v, Kt)*DX*DY + u*D(v, Kx)*DT*DX + v*D(v, Ky)*DT*DY - NU*D(v, KL)*DT + D(p, Ky)*DT*DX
    return rx + ry


def ns_momentum_vjp64(vars, g, ks):
    Kt, Kx, Ky, KL = ks
    u, v = vars[:, 0], vars[:, 1]
    a, b, c, n = DX * DY, DT * DY, DT * DX, NU * DT
    du = a*DT_(g, Kt) - n*DT_(g, KL) + g*(b*D(u, Kx) + c*D(v, Kx)) + b*DT_(g*u, Kx) + c*DT_(g*v, Ky)
    dv = a*DT_(g, Kt) - n*DT_(g, KL) + g*(c*D(u, Ky) + b*D(v, Ky)) + c*DT_(g*u, Kx) + b*DT_(g*v, Ky)
    dp = b*DT_(g, Kx) + c*DT_(g, Ky)
    return torch.stack([du, dv, dp], 1)


def burgers_kernels():
    return tuple(_k64(ConvOperator1D(d, o)) for d, o in (("t", 1), ("x", 1), ("x", 2)))


BDX, BDT, BNU = 0.05, 0.01, 0.002


def burgers64(u, ks):
    Kt, Kx, Kxx = ks
    return BDX*D(u, Kt) + BDT*u*D(u, Kx) - BNU*D(u, Kxx)*(2*BDT/BDX)


def burgers_vjp64(u, g, ks):
    Kt, Kx, Kxx = ks
    return BDX*DT_(g, Kt) + BDT*g*D(u, Kx) + BDT*DT_(g*u, Kx) - BNU*(2*BDT/BDX)*DT_(g, Kxx)


def _autograd(fn, x, g):
    x = x.clone().requires_grad_(True)
    fn(x).backward(g)
    return x.grad


@pytest.mark.parametrize("crop", [False, True])
def test_ns_momentum_vjp_formula_equals_autograd(crop):
    torch.manual_seed(0)
    ks = ns_kernels()
    v = torch.rand(2, 3, 5, 7, 9, dtype=torch.float64) + 0.5
    # the fp64 restatement IS the oracle's expression (fp32) to its rounding
    assert rel_err(ns_momentum64(v, ks).numpy(), orr.ns_momentum(v.float(), DT, DX, DY, NU, boundary=True).numpy()) <= 1e-5
    g = torch.randn(2, 5, 7, 9, dtype=torch.float64) * _mask((2, 5, 7, 9), crop)
    want = _autograd(lambda x: ns_momentum64(x, ks), v, g)
    assert (ns_momentum_vjp64(v, g, ks) - want).abs().max() <= 1e-10
    # the loss form: g = 2/N * 1000 * m * r
    m = _mask((2, 5, 7, 9), crop)
    want = _autograd(lambda x: 1000 * ((ns_momentum64(x, ks) ** 2 * m).sum() / m.sum()), v, torch.tensor(1.0, dtype=torch.float64))
    got = ns_momentum_vjp64(v, 2 / m.sum() * 1000 * m * ns_momentum64(v, ks), ks)
    assert (got - want).abs().max() <= 1e-10


@pytest.mark.parametrize("crop", [False, True])
def test_burgers_vjp_formula_equals_autograd(crop):
    torch.manual_seed(1)
    ks = burgers_kernels()
    u = torch.rand(3, 6, 11, dtype=torch.float64)
    assert rel_err(burgers64(u, ks).numpy(), orr.burgers_residual(u.float(), BDX, BDT, BNU, boundary=True).numpy()) <= 1e-5
    g = torch.randn(3, 6, 11, dtype=torch.float64) * _mask((3, 6, 11), crop)
    want = _autograd(lambda x: burgers64(x, ks), u, g)
    assert (burgers_vjp64(u, g, ks) - want).abs().max() <= 1e-10


@pytest.mark.parametrize("crop", [False, True])
def test_linear_vjp_formulas_equal_autograd(crop):
    """NS continuity, the wave kernel, the advection kernel: df = D^T(g)"""
    torch.manual_seed(2)
    _, Kx, Ky, _ = ns_kernels()
    ratio = DX / DY
    v = torch.rand(2, 2, 5, 7, 9, dtype=torch.float64)
    cont = lambda x: D(x[:, 0], Kx) + ratio * D(x[:, 1], Ky)
    assert rel_err(cont(v).numpy(), orr.ns_continuity(v.float(), DX, DY, boundary=True).numpy()) <= 1e-5
    g = torch.randn(2, 5, 7, 9, dtype=torch.float64) * _mask((2, 5, 7, 9), crop)
    want = _autograd(cont, v, g)
    assert (torch.stack([DT_(g, Kx), ratio * DT_(g, Ky)], 1) - want).abs().max() <= 1e-10
    Kw = orr.wave_kernel(1.0, 0.01, 0.02).double()
    f = torch.rand(2, 5, 7, 9, dtype=torch.float64)
    assert rel_err(D(f, Kw).numpy(), orr.wave_residual(f.float(), 1.0, 0.01, 0.02, boundary=True).numpy()) <= 1e-5
    assert (DT_(g, Kw) - _autograd(lambda x: D(x, Kw), f, g)).abs().max() <= 1e-10
    Ka = orr.advection_kernel(1.0, 2, 0.005, 0.01).double()
    f2 = torch.rand(3, 6, 11, dtype=torch.float64)
    g2 = torch.randn(3, 6, 11, dtype=torch.float64) * _mask((3, 6, 11), crop)
    assert rel_err(D(f2, Ka).numpy(), orr.advection_residual(f2.float(), 1.0, 2, 0.005, 0.01, boundary=True).numpy()) <= 1e-5
    assert (DT_(g2, Ka) - _autograd(lambda x: D(x, Ka), f2, g2)).abs().max() <= 1e-10


# ------------------------------------------------------------------ the ABI
DECLARED = {"pre_vjp_abi_version", "pre_vjp_stencil3d_f32", "pre_vjp_stencil2d_f32", "pre_vjp_linear2_f32",
            "pre_vjp_burgers_f32", "pre_vjp_ns_momentum_f32", "pre_vjp_sumsq_f32"}


def test_vjp_library_exports_what_its_header_declares():
    from cp_pre_amd import _lib
    so = _lib.VJP_SO_PATH
    assert os.path.exists(so), "libcp_pre_vjp.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.VJP_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_VJP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_VJP_ABI_VERSION
    assert _lib._load("vjp").pre_vjp_abi_version() == _lib.PRE_VJP_ABI_VERSION
    assert _lib.load_vjp() is _lib._load("vjp")
    for name in ("PRE_VJP_CROP", "PRE_VJP_VIEW3D", "PRE_VJP_SUMSQ_WORKSPACE"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == getattr(_lib, name)
    # every declaration cites the reference lines it serves
    for decl in re.split(r"\n(?=/\* )", header.split("int pre_vjp_abi_version(void);", 1)[1]):
        if "int pre_vjp_" in decl:
            assert re.search(r"\w+/\w+\.py:\d+", decl), decl[:80]
    # the first table keeps its eight rows; the new library's row lives next to it
    assert len(_lib._LIBS) == 8 and "vjp" not in _lib._LIBS and "vjp" in _lib._LIBS_MORE


def test_vjp_ctypes_signatures_have_the_header_arity():
    """number of parameters of every declaration == length of the binding's argtypes"""
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in re.findall(r"^int\s+(pre_vjp_\w+)\s*\(([^;]*)\);", header, flags=re.M):
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.VJP_SIGNATURES[name]), name


def test_vjp_wrong_abi_version_raises_import_error(monkeypatch):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_vjp", None)
    monkeypatch.setattr(_lib, "PRE_VJP_ABI_VERSION", _lib.PRE_VJP_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_vjp.so has ABI version 1"):
        _lib._load("vjp")


def test_vjp_missing_library_raises_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_vjp", None)
    monkeypatch.setattr(_lib, "VJP_SO_PATH", str(tmp_path / "libcp_pre_vjp.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_vjp()


def test_vjp_header_compiles_as_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", HEADER])


def test_vjp_c_client_builds_and_links(tmp_path):
    exe = tmp_path / "vjp_check"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "c_abi", "vjp_check.c"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_vjp.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)])
    assert exe.exists()


# ------------------------------------------------------------------ validation before any device work
def _methods():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_2d import ConvOperator
    v = torch.rand(2, 6, 5, 8, 12)
    u1 = torch.rand(3, 6, 10)
    ns = R.NavierStokes(0.1, 0.1, 0.1)
    return [
        (ns.residual_momentum, v[:, :3]),
        (ns.residual_continuity, v[:, :2]),
        (R.PRE_NS(0.1, 0.1, 0.1).residual, v[:, :3]),
        (R.PRE_MHD(0.1, 0.1, 0.1).residual, v),
        (R.MHD().residual_energy, v),
        (R.PRE_Wave(0.01, 0.02).residual, v[:, 0]),
        (R.Advection(1.0, 0.005, 0.01).residual, u1),
        (R.Burgers(0.1, 0.01, 0.002).residual, u1),
        (ConvOperator("x", 1), v[:, 0]),
    ]


@pytest.mark.parametrize("i", range(9))
def test_loss_validation_raises_before_device_work(i):
    from cp_pre_amd.losses import pi_loss, pisl_loss, residual_vjp
    method, like = _methods()[i]
    wrong = torch.zeros(tuple(like.shape[:-1]) + (like.shape[-1] + 1,))
    with pytest.raises(ValueError, match="shape"):
        pisl_loss(method, like, wrong)
    with pytest.raises(TypeError, match="dtype"):
        pisl_loss(method, like, like.double())
    with pytest.raises(TypeError, match="dtype"):
        pi_loss(method, like.double())
    with pytest.raises(TypeError):
        pi_loss(method, like.numpy())
    with pytest.raises(TypeError):
        pisl_loss(method, like, like.numpy())
    with pytest.raises(ValueError, match="shape"):
        residual_vjp(method, like, torch.zeros(3, 3))
    with pytest.raises(TypeError, match="dtype"):
        residual_vjp(method, like, torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        pi_loss(method, torch.zeros(4, 4))               # (a rank the method does not take)


def test_loss_validation_of_g_shape_device_and_method():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.losses import pi_loss, residual_vjp
    v = torch.rand(2, 3, 5, 8, 12)
    ns = R.NavierStokes(0.1, 0.1, 0.1)
    # g has the shape of the method's result: cropped unless boundary
    with pytest.raises(ValueError, match=r"expected \(2, 3, 6, 10\)"):
        residual_vjp(ns.residual_momentum, v, torch.zeros(2, 5, 8, 12))
    with pytest.raises(ValueError, match=r"expected \(2, 5, 8, 12\)"):
        residual_vjp(ns.residual_momentum, v, torch.zeros(2, 3, 6, 10), boundary=True)
    with pytest.raises(ValueError, match="is on"):
        residual_vjp(ns.residual_momentum, v, torch.zeros(2, 3, 6, 10, device="meta"))
    with pytest.raises(TypeError, match="residual_method"):
        pi_loss(lambda x, boundary=False: x, v)
    with pytest.raises(TypeError, match="residual_method"):
        pi_loss(ns.periodic_bc_residual, v)
