"""CPU tests of the data-driven scores (``minus=``, libcp_pre_pair.so): the exported ABI against include/cp_pre_pair.h and
the ctypes binding, a C99 client, and the ``minus=`` validation that happens before any device work.  The device passes
are covered by tests/test_gpu_pair.py."""
import os
import re
import subprocess

import pytest
import torch

from cp_pre_amd import _lib
from cp_pre_amd import residuals as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_pair.h")


def test_pair_library_exports_what_its_header_declares():
    so = _lib.PAIR_SO_PATH
    assert os.path.exists(so), "libcp_pre_pair.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == {"pre_pair_abi_version", "pre_pair_stencil3d_f32", "pre_pair_stencil2d_f32", "pre_pair_linear2_f32",
                        "pre_pair_ns_momentum_f32", "pre_pair_mhd_continuity_f32", "pre_pair_burgers_f32"}
    assert exported == declared and set(_lib.PAIR_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_PAIR_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_PAIR_ABI_VERSION
    assert _lib.load_pair().pre_pair_abi_version() == _lib.PRE_PAIR_ABI_VERSION
    # every declaration cites the reference lines it replaces
    for decl in re.split(r"\n(?=/\* )", header.split("int pre_pair_abi_version(void);", 1)[1]):
        if "int pre_pair_" in decl:
            assert re.search(r"\w+/\w+\.py:\d+", decl), decl[:80]


def test_pair_header_compiles_as_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", HEADER])


def test_pair_c_client_builds_and_links(tmp_path):
    exe = tmp_path / "pair_check"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "c_abi", "pair_check.c"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_pair.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    assert exe.exists()


def _cases():
    v = torch.rand(2, 6, 5, 8, 12)
    u1 = torch.rand(3, 6, 10)
    ns, mhd = R.NavierStokes(0.1, 0.1, 0.1), R.MHD()
    jorek = R.JOREK(torch.linspace(1, 2, 12))
    return [
        (lambda m, **k: ns.residual_momentum(v[:, :3], minus=m, **k), v[:, :3]),
        (lambda m, **k: ns.residual_continuity(v[:, :2], minus=m, **k), v[:, :2]),
        (lambda m, **k: R.PRE_NS(0.1, 0.1, 0.1).residual(v[:, :3], minus=m, **k), v[:, :3]),
        (lambda m, **k: R.PRE_MHD(0.1, 0.1, 0.1).residual(v, minus=m, **k), v),
        (lambda m, **k: mhd.residual_continuity(v, minus=m, **k), v),
        (lambda m, **k: mhd.residual_momentum(v, minus=m, **k), v),
        (lambda m, **k: mhd.residual_energy(v, minus=m, **k), v),
        (lambda m, **k: mhd.residual_induction(v, minus=m, **k), v),
        (lambda m, **k: mhd.residual_gauss(v, minus=m, **k), v),
        (lambda m, **k: R.PRE_Wave(0.01, 0.02).residual(v[:, :1], minus=m, **k), v[:, :1]),
        (lambda m, **k: R.Advection(1.0, 0.005, 0.01).residual(u1, minus=m, **k), u1),
        (lambda m, **k: R.Burgers(0.1, 0.01, 0.002).residual(u1, minus=m, **k), u1),
        (lambda m, **k: jorek.residual_continuity(v[:, :3].permute(0, 1, 3, 4, 2), minus=m, **k), v[:, :3].permute(0, 1, 3, 4, 2)),
        (lambda m, **k: jorek.residual_temperature(v[:, :3].permute(0, 1, 3, 4, 2), minus=m, **k), v[:, :3].permute(0, 1, 3, 4, 2)),
    ]


@pytest.mark.parametrize("i", range(14))
def test_minus_shape_and_dtype_mismatch_raise_before_device_work(i):
    fn, like = _cases()[i]
    with pytest.raises(ValueError, match="shape"):
        fn(torch.zeros(tuple(like.shape[:-1]) + (like.shape[-1] + 1,)))
    with pytest.raises(TypeError, match="dtype"):
        fn(like.double())
    with pytest.raises(TypeError):
        fn(like.numpy())


def test_halo_x_and_interior_out_need_a_device_view_of_minus():
    v = torch.rand(2, 3, 5, 8, 12)
    ns = R.NavierStokes(0.1, 0.1, 0.1)
    with pytest.raises(ValueError, match="minus"):
        ns.residual_momentum(v, minus=v.clone(), halo_x=True)
    with pytest.raises(ValueError, match="minus"):
        ns.residual_momentum(v, minus=v.clone(), skip_t_rim=True, out=torch.empty(2, 3, 8, 12))
    with pytest.raises(ValueError, match="minus"):
        R.MHD().residual_induction(torch.rand(2, 6, 5, 8, 12), minus=torch.rand(2, 6, 5, 8, 12), halo_x=True)
    with pytest.raises(ValueError, match="minus"):
        R.PRE_Wave(0.01, 0.02).residual(v[:, :1], minus=v[:, :1].clone(), halo_x=True)
