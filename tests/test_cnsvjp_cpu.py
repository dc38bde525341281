"""CPU tests of the fused backward of ``cp_pre_amd.cns`` (libcp_pre_cnsvjp.so, include/cp_pre_cnsvjp.h):
  * the header's mathematics (tests/cnsvjp_helpers.gather_vjp: per-cell formulas, transposed crosses as gathers with folds)
    against fp64 autograd through the pinned restatement of the reference's expression, to 1e-12;
  * fp32 autograd against fp64 at every shape the GPU tests use: the headroom under ``TOL``;
  * the exported ABI against the header and the ctypes binding, the C99 client compiled against the header, and the
    refusals of the entry, all decided on the host before anything touches a device;
  * the host-side routes: ``plan_backward``, the constructor's argument, ``step`` under the default.
The device pass is covered by tests/test_gpu_cnsvjp.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import cns_helpers as H
import cnsvjp_helpers as V
from test_cns_cpu import module
from test_gpu_cns import CONDITIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_cnsvjp.h")
DECLARED = {"pre_cnsvjp_abi_version", "pre_cns_vjp_f32"}
# every condition of the forward's GPU tests that has a pre_bc_t mapping, and a constant side of value 0
FUSED_CONDITIONS = {k: c for k, c in CONDITIONS.items() if k != "mixed"}
FUSED_CONDITIONS["dirichlet0"] = V.DIRICHLET0


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "cnsvjp_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_cnsvjp.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


def tile():
    from cp_pre_amd import _lib
    return _lib.PRE_CNSVJP_TILE_ROWS, _lib.PRE_CNSVJP_TILE_COLS


def cases():
    nxs, nys = H.gpu_extents(*tile())
    for bs in (1, 3):
        for nx in nxs:
            for ny in nys:
                seed = nx * 1000 + ny
                yield H.make_vars((bs, 4, nx, ny), seed=seed), V.make_cot((bs, 4, nx, ny), seed=seed)


# ------------------------------------------------------------------ the mathematics
def test_mixed_is_the_only_condition_without_a_mapping():
    assert V.bc_struct(CONDITIONS["mixed"]) is None
    assert all(V.bc_struct(c) is not None for c in FUSED_CONDITIONS.values())


@pytest.mark.parametrize("bc", list(FUSED_CONDITIONS))
def test_gather_with_folds_is_the_gradient(bc):
    cond = FUSED_CONDITIONS[bc]
    st = V.bc_struct(cond)
    worst = 0.0
    for v, g in cases():
        for kernels in (None, H.asymmetric_kernels()):
            want = V.vjp64(v, g, cond, kernels)
            worst = max(worst, V.channel_err(V.gather_vjp(v, g, st, kernels), want, V.zero(v, g, kernels)))
    print(f"{bc}: gather with folds against fp64 autograd, worst channel error {worst:.3e}")
    assert worst <= 1e-12


def test_zero_channels_exist():
    """Nx = 2 under 'symmetric' rows with the constructor's kernels: d_rho, d_v and d_p are exactly zero (why ``zero`` exists)."""
    v, g = H.make_vars((1, 4, 2, 8), seed=1), V.make_cot((1, 4, 2, 8), seed=1)
    want = V.vjp64(v, g, CONDITIONS["symmetric"])
    assert [float(want[:, c].abs().max()) == 0.0 for c in range(4)] == [True, False, True, True]


@pytest.mark.parametrize("bc", list(FUSED_CONDITIONS))
def test_fp32_autograd_has_headroom_under_tol(bc):
    cond = FUSED_CONDITIONS[bc]
    worst = 0.0
    for v, g in cases():
        for kernels in (None, H.asymmetric_kernels()):
            got = V.vjp_autograd(v, g, cond, kernels, torch.float32)
            worst = max(worst, V.channel_err(got, V.vjp64(v, g, cond, kernels), V.zero(v, g, kernels)))
    print(f"{bc}: fp32 against fp64 autograd, worst channel error {worst:.3e}")
    assert worst <= H.TOL / 4


# ------------------------------------------------------------------ the ABI
def test_cnsvjp_library_exports_exactly_its_entry_points():
    from cp_pre_amd import _lib
    so = _lib.CNSVJP_SO_PATH
    assert os.path.exists(so), "libcp_pre_cnsvjp.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and exported == declared and set(_lib.CNSVJP_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_CNSVJP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_CNSVJP_ABI_VERSION == 1
    assert int(re.search(r"#define\s+PRE_CNSVJP_TILE_ROWS\s+(\d+)", header).group(1)) == _lib.PRE_CNSVJP_TILE_ROWS
    assert int(re.search(r"#define\s+PRE_CNSVJP_TILE_COLS\s+(\d+)", header).group(1)) == _lib.PRE_CNSVJP_TILE_COLS
    assert _lib.load_cnsvjp().pre_cnsvjp_abi_version() == _lib.PRE_CNSVJP_ABI_VERSION
    assert _lib.load_cnsvjp() is _lib._load("cnsvjp") and "cnsvjp" in _lib._LIBS_MORE and "cnsvjp" not in _lib._LIBS
    strip = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    args = re.search(r"int pre_cns_vjp_f32 ?\(([^;]*)\);", strip).group(1)
    assert len(args.split(",")) == len(_lib.CNSVJP_SIGNATURES["pre_cns_vjp_f32"]) == 17
    mk = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "Makefile")).read()
    assert re.search(r"^cnsvjp_OBJS\s+:= cns_vjp\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bcnsvjp\b", mk, flags=re.M)
    # the forward's library is not touched by its backward
    assert re.search(r"^cns_OBJS\s+:= cns_rhs\.o", mk, flags=re.M)


def test_cnsvjp_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "cnsvjp_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_refusals_are_decided_before_any_device_work():
    """Every refusal returns from the host-side checks: the addresses below are never dereferenced (they are not mapped), so a
    refusal that reached a launch, or a kernel, could not return its code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_cnsvjp()
    B, X, Y = 2, 8, 16
    base_in, base_cot, base_out = 0x10000000, 0x18000000, 0x20000000

    def planes(base, sb=4 * X * Y, sx=Y, shift=0):
        return (_lib.PreCnsPlane * 4)(*[_lib.PreCnsPlane(base + 4 * (c * X * Y + shift), sb, sx) for c in range(4)])

    k = [_lib.farr(t.reshape(-1).tolist()) for t in H.default_kernels().values()]
    bc = _lib.PreBC((ctypes.c_int * 4)(2, 1, 2, 1), (ctypes.c_float * 4)())

    def call(inp=None, cot=None, out=None, kernels=k, bcs=bc, add=None, x=X, y=Y, flags=0, b=B):
        return lib.pre_cns_vjp_f32(planes(base_in) if inp is None else inp, planes(base_cot) if cot is None else cot,
                                   planes(base_out) if out is None else out, *kernels,
                                   ctypes.byref(bcs) if bcs is not None else None, 5 / 3, add, 0.1, b, x, y, flags, None)

    assert call(bcs=None) == _lib.PRE_E_NULL
    assert call(kernels=k[:4] + [None]) == _lib.PRE_E_NULL
    assert call(inp=(_lib.PreCnsPlane * 4)()) == _lib.PRE_E_NULL                       # null plane pointers
    assert call(cot=(_lib.PreCnsPlane * 4)()) == _lib.PRE_E_NULL
    assert call(out=(_lib.PreCnsPlane * 4)()) == _lib.PRE_E_NULL
    assert call(add=(_lib.PreCnsPlane * 4)()) == _lib.PRE_E_NULL
    assert call(b=0) == _lib.PRE_E_NULL
    assert call(y=6) == _lib.PRE_E_UNSUPPORTED and call(y=0) == _lib.PRE_E_NULL
    assert call(x=1) == _lib.PRE_E_UNSUPPORTED
    assert call(flags=2) == _lib.PRE_E_UNSUPPORTED
    assert call(inp=planes(base_in, shift=1)) == _lib.PRE_E_UNSUPPORTED                                  # base off by one float
    assert call(cot=planes(base_cot, shift=1)) == _lib.PRE_E_UNSUPPORTED
    assert call(cot=planes(base_cot, sx=Y + 2)) == _lib.PRE_E_UNSUPPORTED
    assert call(out=planes(base_out, sb=4 * X * Y + 2)) == _lib.PRE_E_UNSUPPORTED
    assert call(add=planes(0x30000000, shift=2)) == _lib.PRE_E_UNSUPPORTED
    off = H.default_kernels()["lap"].clone()
    off[0, 2] = 1.0
    assert call(kernels=k[:4] + [_lib.farr(off.reshape(-1).tolist())]) == _lib.PRE_E_UNSUPPORTED
    assert call(bcs=_lib.PreBC((ctypes.c_int * 4)(2, 1, 9, 1), (ctypes.c_float * 4)())) == _lib.PRE_E_RANGE
    assert call(out=planes(base_in)) == _lib.PRE_E_RANGE                                                 # gin on in
    assert call(out=planes(base_in + 4 * (4 * X * Y * B - Y))) == _lib.PRE_E_RANGE                       # gin on in's last row
    assert call(out=planes(base_cot)) == _lib.PRE_E_RANGE                                                # gin on cot
    assert call(out=planes(base_cot + 4 * (4 * X * Y * B - Y))) == _lib.PRE_E_RANGE                      # gin on cot's last row
    assert call(add=planes(base_out, shift=Y)) == _lib.PRE_E_RANGE                                       # on gin, one row down
    assert call(x=2 ** 31, inp=planes(base_in, sb=0, sx=0), cot=planes(base_cot, sb=0, sx=0),
                out=planes(base_out, sb=0, sx=0)) == _lib.PRE_E_RANGE
    assert call(cot=planes(base_cot, sx=2 ** 30)) == _lib.PRE_E_RANGE                                    # in-plane offsets beyond int32
    assert call(cot=planes(base_cot, sb=2 ** 62)) == _lib.PRE_E_RANGE                                    # offsets beyond int64


# ------------------------------------------------------------------ the host-side routes
def test_plan_backward_answers_from_the_host():
    v = H.make_vars((2, 4, 8, 16))
    assert module().plan_backward(v) == "fallback:backward='recompute'"
    assert module(backward="fused").plan_backward(v) == "fused:cns_vjp"
    assert module(backward="fused", param_grads=True).plan_backward(v) == "fallback:param_grads=True"
    assert module(backward="fused", fused=False).plan_backward(v) == "fallback:fused=False"
    assert module(backward="fused").plan_backward(H.make_vars((2, 4, 8, 6))) == "fallback:Ny % 4 != 0"
    assert module(backward="fused").plan_backward(H.make_vars((2, 4, 1, 8))) == "fallback:grid below 2 x 4 cells"
    assert module(backward="fused").plan_backward(v.double()) == "fallback:dtype other than fp32"
    m = module(backward="fused")
    m.laplace.bc.set_all_boundaries("free_slip")
    assert m.plan_backward(v) == "fallback:boundary condition without a fused mapping"
    # the forward's plan does not depend on the backward's
    assert module(backward="fused").plan(v) == module().plan(v) == "fused:cns_rhs"


def test_backward_argument():
    from cp_pre_amd.cns import Euler_FV_OS_rhs
    assert module().backward == "recompute" and module(backward="fused").backward == "fused"
    with pytest.raises(ValueError, match="'recompute' or 'fused'"):
        Euler_FV_OS_rhs(V.CONFIG, "cpu", backward="autograd")


def test_step_still_refuses_a_gradient_under_the_default():
    v = H.make_vars((1, 4, 8, 16))
    for m in (module(), module(backward="recompute"), module(backward="fused", param_grads=True)):
        with pytest.raises(RuntimeError, match=r"vars \+ h\*forward\(vars\)"):
            m.step(v.clone().requires_grad_(), 1e-3)
        with pytest.raises(RuntimeError, match=r"vars \+ h\*forward\(vars\)"):
            m.step(v, 1e-3, base=v.clone().requires_grad_())


def test_vjp_refuses_what_the_fused_pass_does_not_take():
    v = H.make_vars((2, 4, 8, 6))
    with pytest.raises(ValueError, match="Ny % 4 != 0"):
        module().vjp(v, torch.ones_like(v))
    with pytest.raises(ValueError, match="fused=False"):
        module(fused=False).vjp(v, torch.ones_like(v))
