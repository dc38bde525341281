"""CPU tests of the residuals under boundary conditions on the x-y rim (``bc=``, libcp_pre_bcres.so):
  * the restatement of tests/bcres_helpers.py and the package's COMPOSED route (pad, composed operators, crop - run here with
    torch stand-ins for the HIP operators) against ``tests/golden/bcres.npz``, the reference's own ``pad_signal`` followed by
    the reference's own residual code;
  * ``bc='wrap'`` against circular padding, shapes, the ``boundary=False`` crop, the refusals and their ``last_route()``;
  * ``bc=None`` leaves the library unloaded; the exported ABI against include/cp_pre_bcres.h and the ctypes binding, the C99
    client compiled against the header, and the refusals of the entries, all decided on the host before any device work.
The device pass is covered by tests/test_gpu_bcres.py (rows and branches: tests/BCRES_TESTS.md)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bcres_helpers as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_bcres.h")
DECLARED = {"pre_bcres_abi_version", "pre_bcres_linear1_f32", "pre_bcres_linear2_f32", "pre_bcres_ns_momentum_f32",
            "pre_bcres_mhd_f32", "pre_bcres_burgers_f32", "pre_bcres_linear1_rows_f32"}
GOLDEN_KIND = {"PRE_Wave": "wave", "PRE_NS": "ns_momentum", "PRE_MHD": "mhd_energy"}
CASES = {"dirichlet": H.sides("dirichlet", 0.75), "mixed": H.MIXED}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "bcres_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_bcres.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


def golden_rows():
    g = load_golden("bcres.npz")
    v6, u1 = torch.from_numpy(g["vars6"]), torch.from_numpy(g["u1d"])
    for key in g.files:
        if "|" in key:
            k, case = key.split("|")
            kind = GOLDEN_KIND.get(k, k)
            yield key, kind, CASES.get(case, case), (u1 if kind in H.KINDS_1D else v6), torch.from_numpy(g[key])


def composed(kind, vars, bc, **kw):
    """The package's residual with torch stand-ins for its operators: on CPU tensors it takes the composed route."""
    obj, name = H.module(kind, bc)
    return getattr(H.with_torch_ops(obj), name)(H.package_input(kind, vars), **kw)


# ------------------------------------------------------------------ the semantics, pinned to the reference
def test_fixture_covers_the_kinds_and_the_conditions():
    g = load_golden("bcres.npz")
    assert list(g["cases"]) == list(H.BC_KINDS) + ["mixed"]
    assert g["vars6"].shape == (2, 6, 4, 6, 8) and g["u1d"].shape == (2, 6, 8)
    kinds = {GOLDEN_KIND.get(k.split("|")[0], k.split("|")[0]) for k in g.files if "|" in k}
    assert kinds == set(H.KINDS_2D) | set(H.KINDS_1D)
    assert np.allclose(g["coef"], [H.DT, H.DX, H.DY]) and np.allclose(g["burgers_coef"], H.BURGERS)
    assert np.array_equal(g["advection_kernel"], H.default_ops()["advection"].kernel.numpy())
    assert sum(1 for _ in golden_rows()) == 11 * 6                      # (PRE_MHD repeats mhd_energy under its own key)


def test_restatement_reproduces_the_reference_composition():
    worst = 0.0
    for key, kind, bc, v, want in golden_rows():
        got = H.residual(kind, v, bc)
        assert got.shape == want.shape, key
        worst = max(worst, H.err(got, want))
    print(f"restatement against the reference's pad + residual: worst tensor-scale error {worst:.3e}")
    assert worst <= H.TOL


def test_composed_route_on_cpu_tensors_reproduces_the_fixture():
    from cp_pre_amd import residuals as R
    worst = 0.0
    for key, kind, bc, v, want in golden_rows():
        got = composed(kind, v, bc, boundary=True)
        assert R.last_route() == "fallback:CPU inputs", key
        assert got.shape == want.shape and got.dtype == torch.float32, key
        worst = max(worst, H.err(got, want))
    print(f"composed route against the reference's pad + residual: worst tensor-scale error {worst:.3e}")
    assert worst <= H.TOL


def test_manager_and_name_forms_agree_with_the_dict_form():
    from cp_pre_amd.boundary_conditions import BoundaryManager
    v = H.make_vars((2, 3, 4, 6, 8), seed=2)
    m = BoundaryManager(3)
    for s, (t, val) in H.MIXED.items():
        m.set_boundary_type(s, t, val)
    assert torch.equal(composed("ns_momentum", v, m), composed("ns_momentum", v, H.MIXED))
    assert torch.equal(composed("ns_momentum", v, "neumann"), composed("ns_momentum", v, H.sides("neumann")))
    assert torch.equal(composed("ns_momentum", v, {"left": "neumann"}),
                       composed("ns_momentum", v, dict(H.sides("periodic"), left=("neumann", 0.0))))
    with pytest.raises(TypeError):
        H.module("ns_momentum", 3.0)
    with pytest.raises(ValueError, match="kernel_size=3"):
        H.module("ns_momentum", BoundaryManager(5))
    with pytest.raises(ValueError):
        H.module("ns_momentum", "no_such_condition")


@pytest.mark.parametrize("kind", H.KINDS_2D + H.KINDS_1D)
def test_wrap_is_circular_padding_then_composed(kind):
    nd = 2 if kind in H.KINDS_1D else 3
    v = H.make_vars((2, 6, 8) if nd == 2 else (2, 6, 3, 5, 8), seed=4)

    def circular(f, bc, n):
        return torch.nn.functional.pad(f, (1, 1, 1, 1) if n == 3 else (1, 1), mode="circular")
    want = H.residual(kind, v, "wrap", padder=circular)
    got = composed(kind, v, "wrap", boundary=True)
    assert torch.equal(got, want)
    # the quirk of the parity form is not the wrap: under 'periodic' the high sides read the last cell itself
    assert not torch.equal(got, composed(kind, v, "periodic", boundary=True))


@pytest.mark.parametrize("kind", H.KINDS_2D + H.KINDS_1D)
def test_shapes_and_the_boundary_false_crop(kind):
    nd = 2 if kind in H.KINDS_1D else 3
    v = H.make_vars((2, 5, 8) if nd == 2 else (2, 6, 5, 3, 4), seed=6)
    full = composed(kind, v, "symmetric", boundary=True)
    assert tuple(full.shape) == ((2, 5, 8) if nd == 2 else (2, 5, 3, 4))
    cropped = composed(kind, v, "symmetric")
    assert torch.equal(cropped, full[:, 1:-1])                       # the time rim only: the x-y rim is valid
    assert torch.equal(composed(kind, v, "symmetric", boundary=True, absolute=True), full.abs())


def test_minus_composes_as_the_difference():
    from cp_pre_amd import residuals as R
    a, b = H.make_vars((2, 6, 3, 5, 8), seed=7), H.make_vars((2, 6, 3, 5, 8), seed=8)
    for kind in ("ns_momentum", "mhd_induction", "wave"):
        d = composed(kind, a, "neumann", boundary=True, absolute=True, minus=H.package_input(kind, b))
        want = (composed(kind, a, "neumann", boundary=True) - composed(kind, b, "neumann", boundary=True)).abs()
        assert torch.equal(d, want), kind
    ar = a.clone().requires_grad_()
    d = composed("ns_momentum", ar, "neumann", boundary=True, minus=b)
    assert R.last_route() == "fallback:minus= with a field that requires grad" and d.requires_grad
    with pytest.raises(ValueError, match="minus has shape"):
        composed("ns_momentum", a, "neumann", minus=b[:1])


def test_refusals_and_their_routes():
    from cp_pre_amd import residuals as R
    v = H.make_vars((2, 6, 3, 6, 8), seed=9)

    def route(kind, vars, bc, edit=None, ctor=None, **kw):
        obj, name = H.module(kind, bc, **(ctor or {}))
        H.with_torch_ops(obj)
        if edit:
            edit(obj)
        getattr(obj, name)(H.package_input(kind, vars), boundary=True, **kw)
        return R.last_route()
    assert route("ns_momentum", v, "free_slip") == "fallback:'free_slip' has no padding rule"
    assert route("ns_momentum", v, H.MIXED_INEXPRESSIBLE) == "fallback:mixed condition without a fused mapping"
    assert route("ns_momentum", v, "periodic", ctor={"fused": False}) == "fallback:fused=False"
    assert route("ns_momentum", v[..., :6], "periodic") == "fallback:Ny % 4 != 0"
    assert route("burgers", v[:, 0, 0, :, :6], "periodic") == "fallback:Nx % 4 != 0"
    nt_fastest = v.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert nt_fastest.shape == v.shape and nt_fastest.stride(-1) != 1
    assert route("ns_momentum", nt_fastest, "periodic") == "fallback:no unit stride on Ny"
    assert route("wave", nt_fastest, "wrap") == "fallback:no unit stride on Ny"

    def off_star(o):
        o.D_x.kernel = o.D_x.kernel.clone()
        o.D_x.kernel[0, 0, 0] = 1.0
    assert route("ns_momentum", v, "periodic", off_star) == "fallback:operator kernel off the 7-point star"

    def taylor4(o):
        o.D_xx_yy.kernel = torch.zeros(5, 5, 5)
    assert route("ns_momentum", v, "periodic", taylor4) == "fallback:operator kernel off the 7-point star"

    def trainable(o):
        o.D_t.kernel = o.D_t.kernel.clone().requires_grad_()
    assert route("mhd_energy", v, "periodic", trainable) == "fallback:operator kernel requires grad"
    assert route("ns_momentum", v, ["periodic", ("dirichlet"), {"left": ("dirichlet", 1.0)}]) == "fallback:per-field boundary conditions"
    assert route("ns_momentum", v, "periodic") == "fallback:CPU inputs"
    assert route("mhd_gauss", v, "wrap") == "fallback:CPU inputs"
    # a call without bc resets the report (it needs a device to compute: the report is reset before that)
    obj, name = H.module("ns_momentum")
    try:
        getattr(obj, name)(v)
    except RuntimeError:
        pass
    assert R.last_route() is None


def test_combinations_that_raise():
    v = H.make_vars((2, 6, 4, 6, 8), seed=10)
    for kind in ("ns_momentum", "mhd_energy", "wave"):
        with pytest.raises(ValueError, match="bc with halo_x"):
            composed(kind, v, "periodic", halo_x=True)
    with pytest.raises(ValueError, match="interior-plane out"):
        composed("ns_momentum", v, "periodic", skip_t_rim=True, out=torch.empty(2, 2, 6, 8))
    with pytest.raises(ValueError, match="out with bc"):
        composed("ns_momentum", v, "periodic", out=torch.empty(2, 4, 6, 8))            # (not a device tensor)


def test_apply_bc_on_a_bare_operator():
    from cp_pre_amd import residuals as R
    v = H.make_vars((2, 4, 6, 8), seed=11)
    ops = H.default_ops()
    got = R.apply_bc(ops["wave"], v, "symmetric")
    assert torch.equal(got, H.residual("wave", v[:, None], "symmetric")) and got.shape == v.shape
    u = H.make_vars((2, 6, 8), seed=12)
    assert torch.equal(R.apply_bc(ops["advection"], u, "wrap"), H.residual("advection", u, "wrap"))
    with pytest.raises(RuntimeError, match="expected a"):
        R.apply_bc(ops["wave"], v[0, 0], "wrap")


def test_screens_and_losses_decline_an_object_with_bc():
    """Out of scope: no fused screen or backward evaluates the rim under ``bc`` - their shared gate says so, so that none
    launches the zero-pad functor on the operators of such an object."""
    from cp_pre_amd import losses, screen
    v = H.make_vars((2, 3, 4, 8, 8), seed=13)
    for mod in (screen, losses):
        obj, name = H.module("ns_momentum", "wrap")
        assert mod._Spec(getattr(obj, name)).declined(v).startswith("bc=")
        obj, name = H.module("ns_momentum")
        assert mod._Spec(getattr(obj, name)).declined(v) is None


def test_bc_none_leaves_the_library_unloaded():
    """Constructing every class with and without ``bc``, and composing under ``bc`` on the host, maps no libcp_pre_bcres.so:
    it is loaded by the first fused launch alone.  (The bits of ``bc=None`` against a call without the keyword: the GPU
    tests.)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import torch, bcres_helpers as H\n"
            "from cp_pre_amd import residuals as R, _lib\n"
            "v = H.make_vars((2, 6, 3, 6, 8))\n"
            "for kind in H.KINDS_2D + H.KINDS_1D:\n"
            "    H.module(kind); H.module(kind, None); H.module(kind, 'periodic')\n"
            "obj, name = H.module('ns_momentum', 'periodic'); getattr(H.with_torch_ops(obj), name)(v)\n"
            "assert R.last_route() == 'fallback:CPU inputs' and _lib._bcres is None\n"
            "assert 'libcp_pre_bcres' not in open('/proc/self/maps').read()\n"
            "print('unloaded')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("unloaded"), r.stdout + r.stderr


# ------------------------------------------------------------------ the ABI
def test_bcres_library_exports_exactly_the_headers_entries():
    from cp_pre_amd import _lib
    so = _lib.BCRES_SO_PATH
    assert os.path.exists(so), "libcp_pre_bcres.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and exported == declared and set(_lib.BCRES_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_BCRES_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_BCRES_ABI_VERSION == 1
    assert _lib.load_bcres().pre_bcres_abi_version() == _lib.PRE_BCRES_ABI_VERSION
    assert _lib.load_bcres() is _lib._load("bcres") and "bcres" in _lib._LIBS_MORE and "bcres" not in _lib._LIBS
    strip = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for name, sig in _lib.BCRES_SIGNATURES.items():
        args = re.search(r"int %s ?\(([^;]*)\);" % name, strip).group(1)
        assert (0 if args.strip() == "void" else len(args.split(","))) == len(sig), name
    hip = open(os.path.join(ROOT, "include", "cp_pre_hip.h")).read()
    for mode in ("CONSTANT", "REPLICATE", "PERIODIC", "REFLECT"):
        assert int(re.search(r"#define\s+PRE_BC_%s\s+(\d+)" % mode, hip).group(1)) == getattr(_lib, "PRE_BC_" + mode)
    mk = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "Makefile")).read()
    assert re.search(r"^bcres_OBJS\s+:= residual_bc\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bbcres\b", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS :=(.*\\\n)*.*\$\(bcres_OBJS\)", mk, flags=re.M)


def test_bcres_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    exe = tmp_path / "bcres_check"
    subprocess.check_call(c_client_command(exe))
    assert exe.exists()


def test_refusals_are_decided_before_any_device_work():
    """Every refusal returns from the host-side checks: the addresses below are never dereferenced (they are not mapped), so a
    refusal that reached a launch, or a kernel, could not return its code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_bcres()
    B, T, X, Y = 2, 3, 8, 16
    base_in, base_out = 0x10000000, 0x20000000

    def view(base, sx=Y, sy=1):
        return _lib.PreField(base, T * X * Y, X * Y, sx, sy)
    k27 = H.default_ops()["wave"].kernel.reshape(-1).tolist()
    K = _lib.farr(k27)
    k9 = _lib.farr(H.default_ops()["advection"].kernel.reshape(-1).tolist())

    def bc(modes=(2, 2, 0, 3), values=(0, 0, 2.5, 0)):
        return _lib.PreBC((ctypes.c_int * 4)(*modes), (ctypes.c_float * 4)(*values))

    def call(inp=None, out=None, kernel=K, bcs=bc(), x=X, y=Y, flags=0, b=B):
        return lib.pre_bcres_linear1_f32(ctypes.byref(inp or view(base_in)), ctypes.byref(out or view(base_out)), kernel,
                                         ctypes.byref(bcs) if bcs is not None else None, b, T, x, y, flags, None)
    assert call(bcs=None) == _lib.PRE_E_NULL and call(kernel=None) == _lib.PRE_E_NULL
    assert call(inp=view(0)) == _lib.PRE_E_NULL and call(out=view(0)) == _lib.PRE_E_NULL
    assert call(b=0) == _lib.PRE_E_NULL and call(y=0) == _lib.PRE_E_NULL
    assert call(bcs=bc(modes=(2, 9, 0, 3))) == _lib.PRE_E_RANGE                          # unknown mode
    assert call(x=1) == _lib.PRE_E_RANGE                                                 # X < 2 under PRE_BC_REFLECT
    assert call(inp=view(base_in, sx=2 ** 30)) == _lib.PRE_E_RANGE                       # in-plane offsets beyond 32 bits
    assert call(y=6) == _lib.PRE_E_UNSUPPORTED
    assert call(inp=view(base_in, sx=1, sy=X)) == _lib.PRE_E_UNSUPPORTED                 # no relabelling: Ny must be the unit axis
    assert call(out=view(base_out, sy=2)) == _lib.PRE_E_UNSUPPORTED
    assert call(flags=_lib.PRE_FLAG_HALO_X) == _lib.PRE_E_UNSUPPORTED
    assert call(flags=_lib.PRE_FLAG_OUT_INTERIOR_T) == _lib.PRE_E_UNSUPPORTED
    off = list(k27)
    off[0] = 1.0
    assert call(kernel=_lib.farr(off)) == _lib.PRE_E_UNSUPPORTED
    # the other entries share the checks
    f, o, b4 = view(base_in), view(base_out), bc()
    six = (_lib.PreField * 6)(*[view(base_in + 4 * i * B * T * X * Y) for i in range(6)])
    assert lib.pre_bcres_mhd_f32(5, six, ctypes.byref(o), K, K, K, 5 / 3, ctypes.byref(b4), B, T, X, Y, 0, None) == _lib.PRE_E_RANGE
    assert lib.pre_bcres_mhd_f32(1, six, ctypes.byref(o), K, K, K, 5 / 3, ctypes.byref(b4), B, T, X, 6, 0, None) == _lib.PRE_E_UNSUPPORTED
    assert lib.pre_bcres_mhd_f32(1, six, ctypes.byref(o), K, K, K, 5 / 3, None, B, T, X, Y, 0, None) == _lib.PRE_E_NULL
    # (the general star of MHD momentum / energy is not built: the wave kernel has taps on all three axes)
    assert lib.pre_bcres_mhd_f32(1, six, ctypes.byref(o), K, K, K, 5 / 3, ctypes.byref(b4), B, T, X, Y, 0, None) == _lib.PRE_E_UNSUPPORTED
    assert lib.pre_bcres_mhd_f32(2, six, ctypes.byref(o), K, K, K, 5 / 3, ctypes.byref(b4), B, T, X, Y, 0, None) == _lib.PRE_E_UNSUPPORTED
    assert lib.pre_bcres_linear2_f32(ctypes.byref(f), ctypes.byref(f), ctypes.byref(o), K, None, 1.0, ctypes.byref(b4), B, T, X, Y, 0,
                                     None) == _lib.PRE_E_NULL
    assert lib.pre_bcres_ns_momentum_f32(ctypes.byref(f), ctypes.byref(f), ctypes.byref(f), ctypes.byref(o), K, K, K, K, .1, .1, .1, .1,
                                         ctypes.byref(bc(modes=(0, 0, 0, 4))), B, T, X, Y, 0, None) == _lib.PRE_E_RANGE
    s3 = _lib.iarr64((T * X, X, 1))
    rows = lambda strides=s3, x=X, flags=0, bcs=b4: lib.pre_bcres_linear1_rows_f32(
        base_in, strides, base_out, s3, k9, ctypes.byref(bcs), B, T, x, flags, None)
    assert rows(x=6) == _lib.PRE_E_UNSUPPORTED and rows(strides=_lib.iarr64((T * X, 1, T))) == _lib.PRE_E_UNSUPPORTED
    assert rows(flags=_lib.PRE_FLAG_HALO_X) == _lib.PRE_E_UNSUPPORTED and rows(bcs=bc(modes=(7, 0, 0, 0))) == _lib.PRE_E_RANGE
    assert lib.pre_bcres_burgers_f32(base_in, s3, base_out, s3, k9, k9, None, .1, .1, .1, .1, ctypes.byref(b4), B, T, X, 0,
                                     None) == _lib.PRE_E_NULL
    assert lib.pre_bcres_burgers_f32(base_in, s3, base_out, s3, k9, k9, k9, .1, .1, .1, .1, ctypes.byref(b4), B, T, 6, 0,
                                     None) == _lib.PRE_E_UNSUPPORTED
