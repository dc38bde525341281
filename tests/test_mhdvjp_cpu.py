"""CPU tests of the fused backward for the ideal-MHD residual losses (``mhd=True`` of cp_pre_amd.losses,
libcp_pre_vjpmhd.so):
  * the exported ABI against include/cp_pre_vjpmhd.h and the ctypes binding, a C99 client compiled against the header;
  * the default (``mhd=False``) decides what it decided before and never loads the new library; every refusal of
    ``mhd=True`` has its reason;
  * the restated fp64 expressions of tests/mhdvjp_helpers.py and their gradients against oracle/residuals.py ``mhd_*``;
  * the header's closed forms, evaluated with shifted adds in fp64, against fp64 autograd;
  * headroom: the same expressions in float32 on the CPU within TOL / 4 of float64 at every shape the GPU file runs.
The device passes are covered by tests/test_gpu_mhdvjp.py."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import mhdvjp_helpers as mh
from losses_helpers import channel_errs, ref_vjp, seam_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_vjpmhd.h")
ENTRIES = {"pre_vjpmhd_%s_f32" % e for e in ("continuity", "induction", "momentum", "energy")}
DECLARED = ENTRIES | {"pre_vjpmhd_abi_version", "pre_vjpmhd_supported"}
TOL = mh.TOL


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "vjpmhd_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_vjpmhd.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


def dev(t, requires_grad=False):
    """a stand-in for a device tensor without storage: what the host decisions read of it"""
    return type("Dev", (), {"is_cuda": True, "numel": t.numel, "stride": t.stride, "dim": t.dim, "shape": t.shape,
                            "requires_grad": requires_grad})()


# ------------------------------------------------------------------ the ABI
def test_vjpmhd_library_exports_exactly_its_entry_points():
    from cp_pre_amd import _lib
    so = _lib.VJPMHD_SO_PATH
    assert os.path.exists(so), "libcp_pre_vjpmhd.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.VJPMHD_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_VJPMHD_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_VJPMHD_ABI_VERSION == 1
    assert _lib._load("vjpmhd").pre_vjpmhd_abi_version() == _lib.PRE_VJPMHD_ABI_VERSION
    assert _lib.load_vjpmhd() is _lib._load("vjpmhd")
    assert len(_lib._LIBS) == 8 and "vjpmhd" not in _lib._LIBS and "vjpmhd" in _lib._LIBS_MORE
    # every entry mirrors pre_vjp_ns_momentum_f32: g, fields, outputs, the dense kernels, [gamma,] the two scales, B, T, X, Y,
    # flags, stream
    strip = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for name in ENTRIES:
        args = [a.strip() for a in re.search(r"int %s ?\(([^;]*)\);" % name, strip).group(1).split(",")]
        assert len(args) == len(_lib.VJPMHD_SIGNATURES[name]) == (15 if name.endswith("energy_f32") else 14), name
        assert args[0] == "const pre_field_t *g" and args[1].startswith("const pre_field_t fields[") and args[2].startswith("const pre_out_t out[")
        assert args[3:6] == ["const float *K_t", "const float *K_x", "const float *K_y"]
        assert args[-8:] == ["float host_scale", "const float *dev_scale", "int64_t B", "int64_t T", "int64_t X", "int64_t Y", "int flags", "void *stream"]


def test_vjpmhd_wrong_abi_version_and_missing_library_raise(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_vjpmhd", None)
    monkeypatch.setattr(_lib, "PRE_VJPMHD_ABI_VERSION", _lib.PRE_VJPMHD_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_vjpmhd.so has ABI version 1"):
        _lib._load("vjpmhd")
    monkeypatch.setattr(_lib, "VJPMHD_SO_PATH", str(tmp_path / "libcp_pre_vjpmhd.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_vjpmhd()


def test_vjpmhd_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "vjpmhd_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()
    exe = tmp_path / "vjpmhd_check"
    subprocess.check_call(c_client_command(exe))
    assert exe.exists()


def test_the_march_is_shared_not_copied():
    csrc = os.path.join(ROOT, "cp_pre_amd", "csrc")
    march = open(os.path.join(csrc, "vjp_march.h")).read()
    assert march.count("vjp_march_kernel(const VGeom g") == 1 and "atomic" not in march.split("namespace {")[1]
    for name in ("residual_vjp.hip", "vjp_mhd.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "vjp_march.h"' in src and "__global__ void __launch_bounds__(NR" not in src, name
    assert "atomic" not in open(os.path.join(csrc, "vjp_mhd.hip")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^vjpmhd_OBJS\s+:= vjp_mhd\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bvjpmhd\b", mk, flags=re.M)
    shared = re.search(r"^SHARED_OBJS := ((?:.*\\\n)*.*)$", mk, flags=re.M).group(1)
    assert "$(vjpmhd_OBJS)" in shared and "$(vjp_OBJS)" in shared
    assert re.search(r"^SHARED_HDRS := .*\bvjp_functors\.h\b.*\bvjp_march\.h\b", mk, flags=re.M)
    assert re.search(r"^\$\(vjpmhd_OBJS\): \$\(INC\)/cp_pre_vjpmhd\.h \$\(INC\)/cp_pre_vjp\.h$", mk, flags=re.M)
    assert "fast-math" not in mk


def test_supported_says_which_tap_structures_are_built():
    """general stars: momentum is built (no scratch in either pass), the other three are declined; the reference's
    construction and y_axis_fix are built for all four"""
    from cp_pre_amd import _dispatch, _lib
    lib = _lib.load_vjpmhd()

    def ask(route, eq):
        ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in route.ops]
        return lib.pre_vjpmhd_supported(eq, *ks)
    for opset in mh.OPSETS:
        assert [ask(mh.MHDRoute("momentum", opset), eq) for eq in range(4)] == [0, 0, 0, 0], opset
    stars = mh.MHDRoute("momentum", "stars")
    assert [ask(stars, eq) for eq in range(4)] == [_lib.PRE_E_UNSUPPORTED, 0, _lib.PRE_E_UNSUPPORTED, _lib.PRE_E_UNSUPPORTED]
    stars.ops[1].kernel[0, 0, 0] = 1.0                             # weight off the star
    assert ask(stars, 1) == _lib.PRE_E_UNSUPPORTED
    assert ask(stars, 4) == _lib.PRE_E_RANGE and ask(stars, -1) == _lib.PRE_E_RANGE
    assert lib.pre_vjpmhd_supported(0, None, None, None) == _lib.PRE_E_NULL


def test_refusals_are_decided_before_any_device_work():
    """Every refusal returns from the host-side checks: the addresses below are not mapped, so a refusal that reached a
    launch could not return its code here."""
    import ctypes
    from cp_pre_amd import _dispatch, _lib
    lib = _lib.load_vjpmhd()
    B, T, X, Y = 2, 5, 9, 20
    n = B * T * X * Y
    route = mh.MHDRoute("momentum")
    ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in route.ops]
    star_ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in mh.MHDRoute("energy", "stars").ops]

    def view(base, i=0, sY=1):
        return _lib.PreField(base + 4 * n * i, T * X * Y, X * Y, Y, sY)

    def call(name, nf, g=None, fields=None, outs=None, kernels=ks, dims=(B, T, X, Y)):
        g = view(0x10000000) if g is None else g
        fields = [view(0x20000000, i) for i in range(nf)] if fields is None else fields
        outs = [view(0x40000000, i) for i in range(nf)] if outs is None else outs
        extra = (5.0 / 3.0,) if name == "energy" else ()
        fn = getattr(lib, "pre_vjpmhd_%s_f32" % name)
        return fn(ctypes.byref(g), (_lib.PreField * nf)(*fields), (_lib.PreField * nf)(*outs), *kernels, *extra, 1.0, None,
                  *dims, 0, None)
    for name, nf in (("continuity", 3), ("induction", 4), ("momentum", 6), ("energy", 6)):
        assert call(name, nf, dims=(B, 0, X, Y)) == _lib.PRE_E_NULL, name
        assert call(name, nf, g=view(0)) == _lib.PRE_E_NULL, name
        assert call(name, nf, fields=[view(0x20000000, i) for i in range(nf - 1)] + [view(0)]) == _lib.PRE_E_NULL, name
        assert call(name, nf, kernels=[ks[0], None, ks[2]]) == _lib.PRE_E_NULL, name
        assert call(name, nf, g=view(0x10000000, sY=2)) == _lib.PRE_E_UNSUPPORTED, name
        assert call(name, nf, outs=[view(0x40000000, i, sY=(2 if i == nf - 1 else 1)) for i in range(nf)]) == _lib.PRE_E_UNSUPPORTED, name
        # the last output over the first field: whichever launch reads that field (momentum: d By over rho - d By is
        # written by the launch that reads rho; energy: over rho, which no launch reads - its view is checked all the same)
        over = [view(0x40000000, i) for i in range(nf - 1)] + [view(0x20000000 + 4 * Y)]
        assert call(name, nf, outs=over) == _lib.PRE_E_SHAPE, name
        over_g = [view(0x10000000 + 4 * Y)] + [view(0x40000000, i) for i in range(1, nf)]
        assert call(name, nf, outs=over_g) == _lib.PRE_E_SHAPE, name
        assert call(name, nf, outs=[view(0x40000000)] * nf) == _lib.PRE_E_SHAPE, name
        want = 0 if name == "momentum" else _lib.PRE_E_UNSUPPORTED
        if want:                                                  # (momentum with general stars would launch)
            assert call(name, nf, kernels=star_ks) == want, name
    # momentum: an output of launch A (du) over an input of launch B only (p)
    outs = [view(0x40000000, i) for i in range(6)]
    outs[1] = view(0x20000000 + 4 * n * 3 + 8)
    assert call("momentum", 6, outs=outs) == _lib.PRE_E_SHAPE


# ------------------------------------------------------------------ host decisions
def test_the_default_decides_what_it_decided_before(monkeypatch):
    from cp_pre_amd import _lib, losses
    for fn in (losses.pi_loss, losses.pisl_loss, losses.residual_vjp):
        assert inspect.signature(fn).parameters["mhd"].default is False

    def boom():
        raise AssertionError("the default keyword loaded libcp_pre_vjpmhd.so")
    monkeypatch.setattr(_lib, "load_vjpmhd", boom)
    # (no device here: the composed expression the fallback evaluates is stood in for by the formulas of mhdvjp_helpers)
    now = {}
    monkeypatch.setattr(losses._Spec, "call", lambda self, x, boundary, minus=None: now["route"].residual(x, boundary))
    x = torch.rand(2, 6, 5, 8, 12) + 0.5
    for eq in mh.EQS:
        route = now["route"] = mh.MHDRoute(eq)
        for spec in (losses._Spec(route.method), losses._Spec(route.method, False)):
            assert spec.kind is None and spec.chan == () and spec.ops == ()
            assert spec.prepare(x) == ("no fused VJP for MHD", ()) == spec.prepare(dev(x))
            assert spec.prepare_flat(dev(x)) == ("no fused VJP for MHD", ())
        g = torch.randn(2, 3, 6, 10)
        a = losses.residual_vjp(route.method, x, g)
        assert losses.last_route() == "fallback:no fused VJP for MHD"
        b = losses.residual_vjp(route.method, x, g, mhd=False)
        assert losses.last_route() == "fallback:no fused VJP for MHD" and torch.equal(a, b)
    pre = mh.MHDRoute("induction", pre=True)
    assert losses._Spec(pre.method).prepare(x) == ("no fused VJP for PRE_MHD", ())
    # the other families do not see the keyword
    from losses_helpers import Route
    ns = Route("ns_momentum")
    s = losses._Spec(ns.method, True)
    assert s.kind == "ns_momentum" and not s.mhd


def test_every_refusal_of_mhd_true_has_its_reason(monkeypatch):
    from cp_pre_amd import losses
    x = torch.rand(2, 6, 5, 8, 12) + 0.5
    S = losses._Spec
    for eq in mh.EQS:
        route = mh.MHDRoute(eq)
        spec = S(route.method, True)
        assert spec.mhd and spec.kind == mh.KIND[eq] and spec.chan == mh.CHAN[eq] and spec.why is None
        assert len(spec.ops) == (2 if eq == "gauss" else 3)
        assert spec.prepare(x) == ("input on the CPU", ())
        assert spec.prepare(dev(torch.empty((0, 6, 5, 8, 12), device="meta"))) == ("empty input", ())
        nt = torch.empty_strided((2, 6, 5, 8, 12), (6 * 480, 480, 1, 60, 5), device="meta")
        assert spec.prepare(dev(nt)) == ("no unit stride on the last axis", ())
        assert spec.wants_flat(dev(nt)) and spec.prepare_flat(dev(nt)) == ("no flat VJP for MHD", ())
        ok = dev(torch.empty((2, 6, 5, 8, 12), device="meta"))
        why, ks = spec.prepare(ok)
        assert why is None and len(ks) == len(spec.ops)
        off = mh.MHDRoute(eq)
        off.obj.fused = False
        assert S(off.method, True).prepare(ok) == ("fused=False", ())
        live = mh.MHDRoute(eq)
        live.obj.D_x.kernel.requires_grad_(True)
        assert S(live.method, True).prepare(ok) == ("operator kernel requires grad", ())
        assert S(route.method, True).prepare(ok, dev(x, True)) == ("yy requires grad", ())
        box = mh.MHDRoute(eq)
        box.obj.D_x.kernel[0, 0, 0] = 1.0
        assert S(box.method, True).prepare(ok) == ("operator kernel off the 7-point star", ())
        stars = mh.MHDRoute(eq, "stars")
        want = None if eq in ("momentum", "gauss") else "declined by the library"
        assert S(stars.method, True).prepare(ok)[0] == want, eq
    pre = S(mh.MHDRoute("induction", pre=True).method, True)
    assert pre.kind == "mhd_induction" and pre.chan == (1, 2, 4, 5)
    other = S(mh.MHDRoute("energy").obj.D_x, True)                 # an operator is not an MHD residual
    assert not other.mhd and other.kind == "stencil3d"
    # CPU inputs: the fallback, whatever the keyword
    route = mh.MHDRoute("energy")
    monkeypatch.setattr(S, "call", lambda self, x, boundary, minus=None: route.residual(x, boundary))
    g = torch.randn(2, 3, 6, 10)
    a = losses.residual_vjp(route.method, x, g, mhd=True)
    assert losses.last_route() == "fallback:input on the CPU"
    assert torch.equal(a, losses.residual_vjp(route.method, x, g))
    with pytest.raises(ValueError, match="F>=6"):
        losses.residual_vjp(route.method, x[:, :5], g, mhd=True)


# ------------------------------------------------------------------ the reference is the reference's
@pytest.mark.parametrize("shape", [(2, 6, 10, 16), (2, 5, 9, 13)])
@pytest.mark.parametrize("eq", mh.EQS)
def test_restated_expressions_and_gradients_equal_the_oracle(eq, shape):
    from oracle import residuals as orr
    fn = getattr(orr, "mhd_" + eq)
    route = mh.MHDRoute(eq)
    for boundary in (False, True):
        x, g = seam_inputs(route, shape, boundary, seed=3)
        xo = x.clone().requires_grad_(True)
        want = fn(xo, boundary=boundary)
        got = route.residual(x.double(), boundary)
        assert float((got - want.detach().double()).abs().max()) <= TOL * float(want.detach().abs().max()), (eq, boundary)
        want.backward(g)
        errs = channel_errs(ref_vjp(route, x.double(), g.double(), boundary), xo.grad)
        assert max(errs.values()) <= TOL, (eq, boundary, errs)
        for c in mh.unread(route):
            assert not xo.grad[:, c].any()


# ------------------------------------------------------------------ the header's formulas are the gradient
@pytest.mark.parametrize("opset", mh.OPSETS + ("stars",))
@pytest.mark.parametrize("eq", mh.EQS)
def test_closed_forms_equal_fp64_autograd(eq, opset):
    route = mh.MHDRoute(eq, opset)
    for shape in [(2, 6, 10, 16), (2, 5, 9, 13), (1, 3, 3, 3), (1, 1, 1, 1)]:
        for boundary in (False, True):
            x, g = seam_inputs(route, shape, boundary, seed=4)
            want = ref_vjp(route, x.double(), g.double(), boundary)
            got = mh.closed_form(route, x.double(), mh.pad_g(g.double(), boundary, shape))
            scale = max(float(want.abs().max()), 1.0)
            assert float((got - want).abs().max()) <= 1e-13 * scale, (eq, opset, shape, boundary)


# ------------------------------------------------------------------ headroom of the tolerance
@pytest.mark.parametrize("opset", mh.OPSETS)
@pytest.mark.parametrize("eq", mh.EQS)
def test_fp32_headroom_at_every_gpu_shape(eq, opset):
    """What a correct fp32 evaluation may differ from fp64 by, measured on the CPU: at most TOL / 4 per channel, so that the
    bound the GPU file applies has a factor 4 of slack for another order of the sums."""
    route = mh.MHDRoute(eq, opset)
    worst = 0.0
    for shape in mh.seam_shapes(eq, opset):
        for boundary in (False, True):
            x, g = seam_inputs(route, shape, boundary, seed=5)
            errs = channel_errs(ref_vjp(route, x, g, boundary), ref_vjp(route, x.double(), g.double(), boundary))
            worst = max(worst, max(errs.values()))
            assert max(errs.values()) <= TOL / 4, (eq, opset, shape, boundary, errs)
    print(f"{eq} {opset}: fp32 against fp64 worst {worst:.2e}")
