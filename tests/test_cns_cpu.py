"""CPU tests of ``cp_pre_amd.cns`` (``Euler_FV_OS_rhs``, libcp_pre_cns.so):
  * the restatement of tests/cns_helpers.py against ``tests/golden/cns.npz`` (the reference's own ``forward``), its fp32
    form against its fp64 form at every shape the GPU tests use (the headroom under ``TOL``), the quirks it pins;
  * the module on a CPU-only host: construction, attributes, ``count_params``, the import shim, the host-side route;
  * the exported ABI against include/cp_pre_cns.h and the ctypes binding, the C99 client compiled against the header, and
    the refusals of the entry, which are all decided on the host before anything touches a device.
The device pass is covered by tests/test_gpu_cns.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cns_helpers as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_cns.h")
DECLARED = {"pre_cns_abi_version", "pre_cns_rhs_f32"}
CONFIG = {"Physics": {"dx": H.DX, "dy": H.DX}}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "cns_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_cns.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


def module(**kw):
    """The module with CPU kernels in its gradient (``Gradient`` builds its sub-operators on 'cuda' whatever it is told, as
    the reference does: on a host without a device they end up without a kernel)."""
    from cp_pre_amd.cns import Euler_FV_OS_rhs
    m = Euler_FV_OS_rhs(CONFIG, "cpu", **kw)
    k = H.default_kernels()
    m.gradient.grad_x.kernel, m.gradient.grad_y.kernel = k["gx"].clone(), k["gy"].clone()
    return m


# ------------------------------------------------------------------ the restatement
def test_helper_reproduces_the_reference_forward():
    g = load_golden("cns.npz")
    for name in H.KERNEL_NAMES:
        assert np.array_equal(H.default_kernels(float(g["dx"]))[name].numpy(), g["kernel_" + name]), name
    assert np.array_equal(H.gamma32().numpy(), g["gamma"])
    for bc, value in zip(g["bcs"], g["bc_values"]):
        for i in range(2):
            got = H.rhs(torch.from_numpy(g[f"vars_{i}"]), H.sides(str(bc), float(value))).numpy()
            want = g[f"rhs_{bc}_{i}"]
            assert got.shape == want.shape == g[f"vars_{i}"].shape
            assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (bc, i)
            if bc == "periodic":
                assert np.array_equal(got, want), i


@pytest.mark.parametrize("bc", list(H.BC_KINDS) + ["mixed", "mixed_fusable", "true_wrap"])
def test_fp32_restatement_has_headroom_under_tol(bc):
    from cp_pre_amd.cns import TILE
    cond = {"mixed": H.MIXED, "mixed_fusable": H.MIXED_FUSABLE, "true_wrap": H.TRUE_WRAP}.get(bc) or H.sides(bc, 0.75 if bc == "dirichlet" else 0.0)
    nxs, nys = H.gpu_extents(*TILE)
    worst = 0.0
    for bs in (1, 3):
        for nx in nxs:
            for ny in nys:
                v = H.make_vars((bs, 4, nx, ny), seed=nx * 1000 + ny)
                for kernels in (None, H.asymmetric_kernels()):
                    worst = max(worst, H.channel_err(H.rhs(v, cond, kernels), H.rhs64(v, cond, kernels), H.zero_scale(v, kernels)))
    print(f"{bc}: fp32 against fp64 restatement, worst channel error {worst:.3e}")
    assert worst <= H.TOL / 4


def test_quirks_are_pinned():
    v = H.make_vars((2, 4, 9, 12), seed=3).double()
    k = {n: t.double() for n, t in H.default_kernels().items()}
    g, d, lap = H.make_ops(k, "periodic", torch.float64)
    r = H.expression(v, g, d, lap, H.gamma32().double())
    # the momentum channels differ exactly by (p_x - p_y) / rho: with the reference's kernels ('y' differences along Nx too)
    # that is zero, with a caller's kernels it is not
    gp = g(v[:, 3:4])
    assert torch.equal(r[:, 1:2] - r[:, 2:3], (1 / v[:, 0:1]) * gp[:, 0:1] - (1 / v[:, 0:1]) * gp[:, 1:2])
    assert torch.equal(k["gx"], k["gy"]) and torch.equal(r[:, 1], r[:, 2])
    ka = {n: t.double() for n, t in H.asymmetric_kernels().items()}
    ra = H.expression(v, *H.make_ops(ka, "periodic", torch.float64), H.gamma32().double())
    ga = H.make_ops(ka, "periodic", torch.float64)[0](v[:, 3:4])
    assert torch.allclose(ra[:, 1:2] - ra[:, 2:3], (ga[:, 0:1] - ga[:, 1:2]) / v[:, 0:1], rtol=1e-12, atol=1e-9)
    assert not torch.equal(ra[:, 1], ra[:, 2])
    # v does not enter the Laplacian term: doubling the Laplacian changes the momentum by lap(u) alone
    k2 = dict(ka, lap=2 * ka["lap"])
    r2 = H.expression(v, *H.make_ops(k2, "periodic", torch.float64), H.gamma32().double())
    lap_u = H.make_ops(ka, "periodic", torch.float64)[2](v[:, 1:2])
    assert torch.allclose(r2[:, 1:2] - ra[:, 1:2], lap_u, rtol=1e-9, atol=1e-6)
    assert torch.equal(r2[:, 0], ra[:, 0]) and torch.equal(r2[:, 3], ra[:, 3])
    # the energy line takes the gradient of rho: it does not move with p's neighbours
    vp = v.clone()
    vp[:, 3] += torch.linspace(0, 1, 12, dtype=torch.float64)
    rp = H.expression(vp, *H.make_ops(ka, "periodic", torch.float64), H.gamma32().double())
    d_a = H.make_ops(ka, "periodic", torch.float64)[1](v[:, 1:2], v[:, 2:3])
    assert torch.allclose(rp[:, 3:4] - ra[:, 3:4], -H.gamma32().double() * (vp[:, 3:4] - v[:, 3:4]) * d_a, rtol=1e-9, atol=1e-6)


# ------------------------------------------------------------------ the module on the host
def test_module_constructs_on_cpu_with_the_reference_attributes():
    from cp_pre_amd import vector_convops_spatial as V
    from cp_pre_amd.cns import Euler_FV_OS_rhs, TILE
    m = Euler_FV_OS_rhs(CONFIG, "cpu")
    assert isinstance(m, torch.nn.Module) and m.count_params() == 0 and list(m.parameters()) == []
    assert m.dx.dtype == m.dy.dtype == m.gamma.dtype == torch.float32 and m.dx.requires_grad and m.gamma.requires_grad
    assert float(m.dx) == float(torch.tensor(H.DX, dtype=torch.float32)) and float(m.gamma) == float(H.gamma32())
    assert isinstance(m.gradient, V.Gradient) and isinstance(m.laplace, V.Laplace) and isinstance(m.divergence, V.Divergence)
    assert m.laplace.scalar is True
    k = H.default_kernels()
    assert torch.equal(m.divergence.grad_x.kernel.detach(), k["dx"]) and torch.equal(m.divergence.grad_y.kernel.detach(), k["dy"])
    assert torch.equal(m.laplace.laplace.kernel.detach(), k["lap"])
    for op in (m.gradient, m.laplace, m.divergence):
        assert set(op.bc.boundary_types.values()) == {"periodic"}
    assert m.fused is True and m.param_grads is False and TILE == (16, 64)


def test_import_shim():
    sys.path.insert(0, os.path.join(ROOT, "cp_pre_amd", "compat"))
    try:
        import importlib
        shim = importlib.import_module("Active_Learning.CNS")
    finally:
        sys.path.pop(0)
    from cp_pre_amd.cns import Euler_FV_OS_rhs
    assert shim.Euler_FV_OS_rhs is Euler_FV_OS_rhs and not hasattr(shim, "CNS_residuals")


def test_route_reasons_come_from_the_host():
    from cp_pre_amd import convops_spatial as S
    from cp_pre_amd.cns import Euler_FV_OS_rhs
    v = H.make_vars((2, 4, 8, 16))
    assert module().plan(v) == "fused:cns_rhs"
    assert module(fused=False).plan(v) == "fallback:fused=False"
    assert Euler_FV_OS_rhs(CONFIG, "cpu").plan(v) in ("fused:cns_rhs", "fallback:operator without a kernel")
    m = module()
    del m.gradient.grad_y.kernel
    assert m.plan(v) == "fallback:operator without a kernel"
    assert module().plan(H.make_vars((2, 4, 8, 6))) == "fallback:Ny % 4 != 0"
    assert module().plan(H.make_vars((2, 4, 1, 8))) == "fallback:grid below 2 x 4 cells"
    assert module().plan(H.make_vars((2, 5, 8, 16))) == "fallback:channel count other than 4"
    assert module().plan(v[0]) == "fallback:channel count other than 4"
    assert module().plan(v.double()) == "fallback:dtype other than fp32"
    m = module()
    m.laplace.bc.set_all_boundaries("free_slip")
    assert m.plan(v) == "fallback:boundary condition without a fused mapping"
    m = module()
    for op in (m.gradient, m.laplace, m.divergence):
        op.bc.set_boundary_type("left", "symmetric")                 # under right 'periodic': the wrap lands on column 1
    assert m.plan(v) == "fallback:boundary condition without a fused mapping"
    m = module()
    m.divergence.bc.set_all_boundaries("neumann")
    assert m.plan(v) == "fallback:boundary conditions of the three operators differ"
    m = module()
    m.gradient.bc.set_all_boundaries("dirichlet", 0.5)
    m.divergence.bc.set_all_boundaries("dirichlet", 0.5)
    m.laplace.bc.set_all_boundaries("dirichlet", 0.25)
    assert m.plan(v) == "fallback:boundary conditions of the three operators differ"
    m = module()
    m.laplace.laplace = S.ConvOperator(("x", "y"), 2, 1.0, 4, "direct", "cpu")
    assert tuple(m.laplace.laplace.kernel.shape) == (5, 5) and m.plan(v) == "fallback:5x5 / 7x7 Taylor stencil"
    m = module()
    m.divergence.grad_x = S.ConvOperator("x", 1, 1.0, 2, "spectral", "cpu")
    assert m.plan(v) == "fallback:spectral operator"


def test_step_refuses_a_gradient():
    m = module()
    with pytest.raises(RuntimeError, match=r"vars \+ h\*forward\(vars\)"):
        m.step(H.make_vars((1, 4, 8, 16)).requires_grad_(), 1e-3)


# ------------------------------------------------------------------ the ABI
def test_cns_library_exports_exactly_its_entry_points():
    from cp_pre_amd import _lib
    so = _lib.CNS_SO_PATH
    assert os.path.exists(so), "libcp_pre_cns.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and exported == declared and set(_lib.CNS_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_CNS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_CNS_ABI_VERSION == 1
    assert int(re.search(r"#define\s+PRE_CNS_TILE_ROWS\s+(\d+)", header).group(1)) == _lib.PRE_CNS_TILE_ROWS
    assert int(re.search(r"#define\s+PRE_CNS_TILE_COLS\s+(\d+)", header).group(1)) == _lib.PRE_CNS_TILE_COLS
    assert _lib.load_cns().pre_cns_abi_version() == _lib.PRE_CNS_ABI_VERSION
    assert _lib.load_cns() is _lib._load("cns") and "cns" in _lib._LIBS_MORE and "cns" not in _lib._LIBS
    strip = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    args = re.search(r"int pre_cns_rhs_f32 ?\(([^;]*)\);", strip).group(1)
    assert len(args.split(",")) == len(_lib.CNS_SIGNATURES["pre_cns_rhs_f32"]) == 16
    mk = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "Makefile")).read()
    assert re.search(r"^cns_OBJS\s+:= cns_rhs\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bcns\b", mk, flags=re.M)


def test_cns_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "cns_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_refusals_are_decided_before_any_device_work():
    """Every refusal returns from the host-side checks: the addresses below are never dereferenced (they are not mapped), so a
    refusal that reached a launch, or a kernel, could not return its code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_cns()
    B, X, Y = 2, 8, 16
    base_in, base_out = 0x10000000, 0x20000000

    def planes(base, sb=4 * X * Y, sx=Y, shift=0):
        return (_lib.PreCnsPlane * 4)(*[_lib.PreCnsPlane(base + 4 * (c * X * Y + shift), sb, sx) for c in range(4)])

    k = [_lib.farr(t.reshape(-1).tolist()) for t in H.default_kernels().values()]
    bc = _lib.PreBC((ctypes.c_int * 4)(2, 1, 2, 1), (ctypes.c_float * 4)())

    def call(inp=None, out=None, kernels=k, bcs=bc, add=None, x=X, y=Y, flags=0, b=B):
        return lib.pre_cns_rhs_f32(planes(base_in) if inp is None else inp, planes(base_out) if out is None else out, *kernels,
                                   ctypes.byref(bcs) if bcs is not None else None, 5 / 3, add, 0.1, b, x, y, flags, None)

    assert call(bcs=None) == _lib.PRE_E_NULL
    assert call(kernels=k[:4] + [None]) == _lib.PRE_E_NULL
    assert call(inp=(_lib.PreCnsPlane * 4)()) == _lib.PRE_E_NULL                       # null plane pointers
    assert call(b=0) == _lib.PRE_E_NULL
    assert call(y=6) == _lib.PRE_E_UNSUPPORTED and call(y=0) == _lib.PRE_E_NULL
    assert call(x=1) == _lib.PRE_E_UNSUPPORTED
    assert call(flags=2) == _lib.PRE_E_UNSUPPORTED
    assert call(inp=planes(base_in, shift=1)) == _lib.PRE_E_UNSUPPORTED                                  # base off by one float
    assert call(inp=planes(base_in, sx=Y + 2)) == _lib.PRE_E_UNSUPPORTED
    assert call(out=planes(base_out, sb=4 * X * Y + 2)) == _lib.PRE_E_UNSUPPORTED
    assert call(add=planes(0x30000000, shift=2)) == _lib.PRE_E_UNSUPPORTED
    off = H.default_kernels()["lap"].clone()
    off[0, 2] = 1.0
    assert call(kernels=k[:4] + [_lib.farr(off.reshape(-1).tolist())]) == _lib.PRE_E_UNSUPPORTED
    assert call(bcs=_lib.PreBC((ctypes.c_int * 4)(2, 1, 9, 1), (ctypes.c_float * 4)())) == _lib.PRE_E_RANGE
    assert call(out=planes(base_in)) == _lib.PRE_E_RANGE                                                 # out on in
    assert call(out=planes(base_in + 4 * (4 * X * Y * B - Y))) == _lib.PRE_E_RANGE                       # out on in's last row
    assert call(add=planes(base_out, shift=Y)) == _lib.PRE_E_RANGE                                       # on out, one row down
    assert call(x=2 ** 31, inp=planes(base_in, sb=0, sx=0), out=planes(base_out, sb=0, sx=0)) == _lib.PRE_E_RANGE
    assert call(inp=planes(base_in, sx=2 ** 30)) == _lib.PRE_E_RANGE                                     # in-plane offsets beyond int32
    assert call(inp=planes(base_in, sb=2 ** 62)) == _lib.PRE_E_RANGE                                     # offsets beyond int64
