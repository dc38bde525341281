"""CPU tests of the fused backward of the ideal-MHD residual losses for Nt-fastest views (``mhd="flat"`` of
cp_pre_amd.losses, libcp_pre_vjpflatmhd.so):
  * the exported ABI against include/cp_pre_vjpflatmhd.h, include/cp_pre_vjpmhd.h and the ctypes binding, a C99 client
    compiled against the header;
  * the unit includes csrc/vjp_flat.hip and defines no second march; the Makefile target;
  * ``mhd=True`` decides what it decided before; every host decision of ``mhd="flat"`` with its reason, on meta tensors;
  * the built-set constants of the unit against ``pre_vjpflatmhd_supported``;
  * every refusal of the entries, decided on unmapped addresses;
  * headroom: the closed forms of the header in float32 on the CPU within TOL / 4 of float64 at every GPU shape.
The device passes are covered by tests/test_gpu_vjpflatmhd.py."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import vjpflatmhd_helpers as fh
from losses_helpers import channel_errs, ref_vjp, seam_inputs
from mhdvjp_helpers import pad_g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cp_pre_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "cp_pre_vjpflatmhd.h")
ENTRIES = {"pre_vjpflatmhd_%s_f32" % e for e in fh.EQ4}
DECLARED = ENTRIES | {"pre_vjpflatmhd_abi_version", "pre_vjpflatmhd_supported"}
TOL = fh.TOL


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "vjpflatmhd_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_vjpflatmhd.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


def view(B, F, Nt, Nx, Ny, pitch_t=None):
    """an Nt-fastest [B,F,Nt,Nx,Ny] tensor without storage (``pitch_t`` > Nt: a t-slab of a larger tensor, rows not dense)"""
    Tp = pitch_t or Nt
    plane = Nx * Ny * Tp
    return torch.empty_strided((B, F, Nt, Nx, Ny), (F * plane, plane, 1, Ny * Tp, Tp), device="meta")


def dev(t, requires_grad=False):
    """a stand-in for a device tensor without storage: what the host decisions read of it"""
    return type("Dev", (), {"is_cuda": True, "numel": t.numel, "stride": t.stride, "dim": t.dim, "shape": t.shape,
                            "requires_grad": requires_grad, "__getitem__": lambda s, i: dev(t[i])})()


def strip_comments(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


# ------------------------------------------------------------------ the ABI
def test_vjpflatmhd_library_exports_exactly_its_entry_points():
    from cp_pre_amd import _lib
    so = _lib.VJPFLATMHD_SO_PATH
    assert os.path.exists(so), "libcp_pre_vjpflatmhd.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.VJPFLATMHD_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_VJPFLATMHD_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_VJPFLATMHD_ABI_VERSION == 1
    assert _lib._load("vjpflatmhd").pre_vjpflatmhd_abi_version() == _lib.PRE_VJPFLATMHD_ABI_VERSION
    assert _lib.load_vjpflatmhd() is _lib._load("vjpflatmhd")
    assert len(_lib._LIBS) == 8 and "vjpflatmhd" not in _lib._LIBS and "vjpflatmhd" in _lib._LIBS_MORE


def test_entries_mirror_the_tiled_library_argument_for_argument():
    from cp_pre_amd import _lib
    for name in DECLARED - {"pre_vjpflatmhd_abi_version"}:
        assert _lib.VJPFLATMHD_SIGNATURES[name] == _lib.VJPMHD_SIGNATURES[name.replace("vjpflatmhd", "vjpmhd")], name
    tiled = strip_comments(open(os.path.join(ROOT, "include", "cp_pre_vjpmhd.h")).read())
    found = re.findall(r"int (pre_vjpflatmhd_\w+) ?\(([^;]*)\);", strip_comments(open(HEADER).read()))
    assert {n for n, _ in found} == DECLARED
    for name, args in found:
        if name != "pre_vjpflatmhd_abi_version":
            assert "int %s(%s);" % (name.replace("vjpflatmhd", "vjpmhd"), args) in tiled, name


def test_vjpflatmhd_wrong_abi_version_and_missing_library_raise(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_vjpflatmhd", None)
    monkeypatch.setattr(_lib, "PRE_VJPFLATMHD_ABI_VERSION", _lib.PRE_VJPFLATMHD_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_vjpflatmhd.so has ABI version 1"):
        _lib._load("vjpflatmhd")
    monkeypatch.setattr(_lib, "VJPFLATMHD_SO_PATH", str(tmp_path / "libcp_pre_vjpflatmhd.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_vjpflatmhd()


def test_vjpflatmhd_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "vjpflatmhd_check.o"
    subprocess.check_call(c_client_command(obj, link=False), stderr=subprocess.DEVNULL)
    assert obj.exists()
    exe = tmp_path / "vjpflatmhd_check"
    subprocess.check_call(c_client_command(exe), stderr=subprocess.DEVNULL)
    assert exe.exists()


def test_the_march_is_included_not_copied_and_the_makefile_target():
    src = open(os.path.join(CSRC, "vjp_flat_mhd.hip")).read()
    assert '#include "vjp_flat.hip"' in src and '#include "../../include/cp_pre_vjpflatmhd.h"' in src
    before = src.split('#include "vjp_flat.hip"')[0]
    assert re.search(r"^#define VF_MAXIN 5$", before, flags=re.M) and re.search(r"^#define VF_MAXOUT 4$", before, flags=re.M)
    assert re.search(r"^#define PRE_VJPFLAT_NO_ENTRIES\b", before, flags=re.M)
    assert "__global__" not in src and "__shared__" not in src and "atomic" not in src      # no second march
    flat = open(os.path.join(CSRC, "vjp_flat.hip")).read()
    assert flat.count("__global__") == 1 and "vjp_flat_kernel" in flat
    for macro, value in (("VF_MAXIN", 3), ("VF_MAXOUT", 3)):
        assert re.search(r"^#ifndef %s\n#define %s %d\n#endif$" % (macro, macro, value), flat, flags=re.M), macro
    guard = flat.index("#ifndef PRE_VJPFLAT_NO_ENTRIES")
    assert guard < flat.index('extern "C" {') and flat.rstrip().endswith("#endif")
    assert "VjpMHD" in src and "VjpMHD" not in flat                                         # the functors are vjp_functors.h's
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^vjpflatmhd_OBJS\s+:= vjp_flat_mhd\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bvjpflatmhd\b", mk, flags=re.M)
    shared = re.search(r"^SHARED_OBJS := ((?:.*\\\n)*.*)$", mk, flags=re.M).group(1)
    assert "$(vjpflatmhd_OBJS)" in shared and "$(vjpflat_OBJS)" in shared
    assert mk.count("-disable-vector-combine") == 1
    line = next(ln for ln in mk.splitlines() if "-disable-vector-combine" in ln and not ln.startswith("#"))
    targets = line.split(":")[0].split()
    assert "vjp_flat.o" in targets and "vjp_flat_mhd.o" in targets
    assert re.search(r"^vjp_flat_mhd\.o:.*\bvjp_flat\.hip\b", mk, flags=re.M)              # the included unit is a dependency
    assert re.search(r"^\$\(vjpflatmhd_OBJS\): \$\(INC\)/cp_pre_vjpflatmhd\.h\b", mk, flags=re.M)
    assert "fast-math" not in mk


# ------------------------------------------------------------------ what is built
def built_constants():
    src = open(os.path.join(CSRC, "vjp_flat_mhd.hip")).read()
    return {e: int(re.search(r"^#define VJPFLATMHD_MODE2_%s (\d)$" % e.upper(), src, flags=re.M).group(1)) for e in fh.EQ4}


def test_built_set_constants_agree_with_supported():
    """the reference's construction, y_axis_fix and the rescaled set serve all four equations; general stars those the
    unit's constants name"""
    from cp_pre_amd import _dispatch, _lib
    from cp_pre_amd._method import MHD_EQ
    lib = _lib.load_vjpflatmhd()
    built = built_constants()
    assert set(built.values()) <= {0, 1}

    def ask(route, eq):
        ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in route.ops]
        return lib.pre_vjpflatmhd_supported(eq, *ks)
    for opset in fh.OPSETS:
        assert [ask(fh.MHDRoute("momentum", opset), eq) for eq in range(4)] == [0, 0, 0, 0], opset
    stars = fh.MHDRoute("momentum", "stars")
    assert [ask(stars, eq) for eq in range(4)] == [0 if built[e] else _lib.PRE_E_UNSUPPORTED for e in MHD_EQ]
    stars.ops[1].kernel[0, 0, 0] = 1.0                             # weight off the star
    assert ask(stars, 0) == _lib.PRE_E_UNSUPPORTED
    assert ask(stars, 4) == _lib.PRE_E_RANGE and ask(stars, -1) == _lib.PRE_E_RANGE
    assert lib.pre_vjpflatmhd_supported(0, None, None, None) == _lib.PRE_E_NULL


def test_refusals_are_decided_before_any_device_work():
    """Every refusal returns from the host-side checks: the addresses below are not mapped, so a refusal that reached a
    launch could not return its code here."""
    from cp_pre_amd import _dispatch, _lib
    lib = _lib.load_vjpflatmhd()
    built = built_constants()
    B, T, X, Y = 2, 10, 9, 6
    n = B * T * X * Y
    ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in fh.MHDRoute("momentum").ops]
    star_ks = [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in fh.MHDRoute("energy", "stars").ops]

    def v(base, i=0, sT=1, sY=None, sX=None, t=T):
        return _lib.PreField(base + 4 * n * i, X * Y * t, sT, Y * t if sX is None else sX, t if sY is None else sY)

    def call(name, nf, g=None, fields=None, outs=None, kernels=ks, dims=(B, T, X, Y), flags=0):
        g = v(0x10000000) if g is None else g
        fields = [v(0x20000000, i) for i in range(nf)] if fields is None else fields
        outs = [v(0x40000000, i) for i in range(nf)] if outs is None else outs
        extra = (5.0 / 3.0,) if name == "energy" else ()
        fn = getattr(lib, "pre_vjpflatmhd_%s_f32" % name)
        return fn(ctypes.byref(g), (_lib.PreField * nf)(*fields), (_lib.PreField * nf)(*outs), *kernels, *extra, 1.0, None,
                  *dims, flags, None)
    for name, nf in (("continuity", 3), ("induction", 4), ("momentum", 6), ("energy", 6)):
        last = nf - 1
        assert call(name, nf, dims=(B, 0, X, Y)) == _lib.PRE_E_NULL, name
        assert call(name, nf, g=v(0)) == _lib.PRE_E_NULL, name
        assert call(name, nf, fields=[v(0x20000000, i) for i in range(last)] + [v(0)]) == _lib.PRE_E_NULL, name
        assert call(name, nf, kernels=[ks[0], None, ks[2]]) == _lib.PRE_E_NULL, name
        # the layout conditions of cp_pre_vjpflat.h, on g, on the LAST field and on the LAST output (momentum, energy: views
        # of the second launch, refused before the first)
        ylast = _lib.PreField(0x10000000, T * X * Y, X * Y, Y, 1)                  # unit stride on Y: the tiled library's
        assert call(name, nf, g=ylast) == _lib.PRE_E_UNSUPPORTED, name
        assert call(name, nf, g=v(0x10000000, sT=2)) == _lib.PRE_E_UNSUPPORTED, name
        for bad in (dict(sY=T + 2), dict(sX=Y * T + 4), dict(sT=2)):
            assert call(name, nf, fields=[v(0x20000000, i, **(bad if i == last else {})) for i in range(nf)]) == _lib.PRE_E_UNSUPPORTED, (name, bad)
            assert call(name, nf, outs=[v(0x40000000, i, **(bad if i == last else {})) for i in range(nf)]) == _lib.PRE_E_UNSUPPORTED, (name, bad)
        t96 = dict(t=96)
        assert call(name, nf, g=v(0x10000000, **t96), fields=[v(0x20000000, i, **t96) for i in range(nf)],
                    outs=[v(0x40000000, i, **t96) for i in range(nf)], dims=(B, 96, X, Y)) == _lib.PRE_E_UNSUPPORTED, name
        t7 = dict(t=7)                                                             # Y * T = 63
        assert call(name, nf, g=v(0x10000000, **t7), fields=[v(0x20000000, i, **t7) for i in range(nf)],
                    outs=[v(0x40000000, i, **t7) for i in range(nf)], dims=(B, 7, X, 9)) == _lib.PRE_E_UNSUPPORTED, name
        assert call(name, nf, flags=2) == _lib.PRE_E_UNSUPPORTED, name            # any flag but PRE_VJP_CROP
        # the overlap rules of cp_pre_vjpmhd.h: the last output over the first field, whichever launch reads that field
        # (energy: over rho, which no launch reads - its view is checked all the same); an output over g; one base twice
        over = [v(0x40000000, i) for i in range(last)] + [v(0x20000000 + 4 * Y * T)]
        assert call(name, nf, outs=over) == _lib.PRE_E_SHAPE, name
        over_g = [v(0x10000000 + 4 * Y * T)] + [v(0x40000000, i) for i in range(1, nf)]
        assert call(name, nf, outs=over_g) == _lib.PRE_E_SHAPE, name
        assert call(name, nf, outs=[v(0x40000000)] * nf) == _lib.PRE_E_SHAPE, name
        box = fh.MHDRoute("momentum")
        box.ops[1].kernel[0, 0, 0] = 1.0
        assert call(name, nf, kernels=[_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in box.ops]) == _lib.PRE_E_UNSUPPORTED, name
        if not built[name]:                                        # (a built general-star instantiation would launch)
            assert call(name, nf, kernels=star_ks) == _lib.PRE_E_UNSUPPORTED, name
    assert not built["momentum"] or not built["energy"] or built["continuity"], "nothing general is declined: restate the case"
    # momentum: an output of launch A (du) over an input of launch B only (p)
    outs = [v(0x40000000, i) for i in range(6)]
    outs[1] = v(0x20000000 + 4 * n * 3 + 8)
    assert call("momentum", 6, outs=outs) == _lib.PRE_E_SHAPE


# ------------------------------------------------------------------ host decisions
def test_mhd_true_decides_what_it_decided_before(monkeypatch):
    """``mhd=True`` never loads the new library; with ``flat=True`` an Nt-fastest input keeps its reason"""
    from cp_pre_amd import _lib, losses

    def boom():
        raise AssertionError("mhd=True loaded libcp_pre_vjpflatmhd.so")
    monkeypatch.setattr(_lib, "load_vjpflatmhd", boom)
    for fn in (losses.pi_loss, losses.pisl_loss, losses.residual_vjp):
        assert inspect.signature(fn).parameters["mhd"].default is False
    nt = dev(view(2, 6, 8, 10, 16))
    ok = dev(torch.empty((2, 6, 5, 8, 12), device="meta"))
    for eq in fh.EQS:
        route = fh.MHDRoute(eq)
        for flag in (True, 1):
            spec = losses._Spec(route.method, flag)
            assert spec.mhd and not spec.mhd_flat
            assert spec.wants_flat(nt) and spec.prepare_flat(nt) == ("no flat VJP for MHD", ())
            assert spec.prepare(nt) == ("no unit stride on the last axis", ())
            why, ks = spec.prepare(ok)
            assert why is None and len(ks) == len(spec.ops)
        plain = losses._Spec(route.method)
        assert not plain.mhd and not plain.mhd_flat and plain.prepare_flat(nt) == ("no fused VJP for MHD", ())
    # the other families do not see the keyword
    from losses_helpers import Route
    s = losses._Spec(Route("ns_momentum").method, "flat")
    assert s.kind == "ns_momentum" and not s.mhd and not s.mhd_flat
    assert not losses._Spec(fh.MHDRoute("energy").obj.D_x, "flat").mhd_flat


def test_every_host_decision_of_mhd_flat_has_its_reason():
    from cp_pre_amd import losses
    S = losses._Spec
    for eq in fh.EQS:
        route = fh.MHDRoute(eq)
        spec = S(route.method, "flat")
        assert spec.mhd and spec.mhd_flat and spec.chan == fh.CHAN[eq] and spec.why is None
        nonlinear = eq != "gauss"
        assert spec.kind == ("mhd_" + eq if nonlinear else "linear2")
        ok = dev(view(2, 6, 8, 10, 16))
        assert spec.wants_flat(ok)
        why, ks = spec.prepare_flat(ok)
        assert why is None and len(ks) == len(spec.ops) == (3 if nonlinear else 2)
        assert spec.prepare_flat(dev(view(2, 8, 8, 10, 16)))[0] is None                     # F = 8: channels 6, 7 not read
        # a unit-stride input is not offered to the flat route at all: prepare() decides, as with mhd=True
        dense = dev(torch.empty((2, 6, 5, 8, 12), device="meta"))
        assert not spec.wants_flat(dense) and spec.prepare(dense)[0] is None
        assert spec.prepare_flat(dev(view(2, 6, 96, 5, 12))) == ("Nt >= 96", ())
        assert spec.prepare_flat(dev(view(2, 6, 7, 5, 9))) == ("merged row Ny*Nt not a multiple of 4", ())
        odd = dev(torch.empty_strided((2, 6, 8, 10, 16), (6 * 1280, 1280, 160, 1, 10), device="meta"))
        assert spec.wants_flat(odd) and spec.prepare_flat(odd) == ("the unit-stride axis is not Nt", ())
        # rows that are not dense: the launches of the non-linear equations read the fields there; gauss reads none
        slab = dev(view(2, 6, 6, 10, 16, pitch_t=8))
        if nonlinear:
            assert spec.prepare_flat(slab) == ("rows of the fields not dense", ())
        else:
            assert spec.prepare_flat(slab)[0] is None
        # what declines in any layout, each before the layout is looked at
        off = fh.MHDRoute(eq)
        off.obj.fused = False
        assert S(off.method, "flat").prepare_flat(slab) == ("fused=False", ())
        live = fh.MHDRoute(eq)
        live.obj.D_x.kernel.requires_grad_(True)
        assert S(live.method, "flat").prepare_flat(ok) == ("operator kernel requires grad", ())
        assert spec.prepare_flat(ok, dev(view(2, 6, 8, 10, 16), True)) == ("yy requires grad", ())
        box = fh.MHDRoute(eq)
        box.obj.D_x.kernel[0, 0, 0] = 1.0
        assert S(box.method, "flat").prepare_flat(ok) == ("operator kernel off the 7-point star", ())
        stars = fh.MHDRoute(eq, "stars")
        want = None if (not nonlinear or built_constants()[eq]) else "declined by the library"
        assert S(stars.method, "flat").prepare_flat(ok)[0] == want, eq
    pre = S(fh.MHDRoute("induction", pre=True).method, "flat")
    assert pre.kind == "mhd_induction" and pre.mhd_flat and pre.prepare_flat(dev(view(2, 6, 8, 10, 16)))[0] is None


def test_cpu_inputs_take_the_fallback_whatever_the_keyword(monkeypatch):
    from cp_pre_amd import losses
    route = fh.MHDRoute("energy")
    monkeypatch.setattr(losses._Spec, "call", lambda self, x, boundary, minus=None: route.residual(x, boundary))
    x = (torch.rand(2, 6, 8, 12, 5) + 0.5).permute(0, 1, 4, 2, 3)                        # Nt fastest, on the CPU
    g = torch.randn(2, 3, 6, 10)
    a = losses.residual_vjp(route.method, x, g, mhd="flat")
    assert losses.last_route() == "fallback:input on the CPU"
    assert torch.equal(a, losses.residual_vjp(route.method, x, g, mhd=True)) and torch.equal(a, losses.residual_vjp(route.method, x, g))


# ------------------------------------------------------------------ layouts and shapes of the GPU file
def test_layout_helpers_and_gpu_shapes():
    x = torch.rand(2, 6, 10, 5, 6)
    a, b = fh.nt_fastest(x, "cpu"), fh.nt_fastest_exact(x, "cpu")
    assert a.stride() == b.stride() and torch.equal(a, b) and torch.equal(b, x)
    for shape in fh.GPU_SHAPES:
        B, Nt, Nx, Ny = shape
        v = fh.nt_fastest_exact(torch.zeros(B, 6, Nt, Nx, Ny), "cpu")
        assert v.stride()[2:] == (1, Ny * Nt, Nt) and (Ny * Nt) % 4 == 0 and Nt < 96
        assert fh.is_flat_view(v) == (Nt > 1), shape                # Nt = 1: the view is Ny-fastest as well
    assert [s for s in fh.DEGENERATE if s[1] == 1] == [(2, 1, 3, 4)]


# ------------------------------------------------------------------ headroom of the tolerance
@pytest.mark.parametrize("opset", fh.OPSETS + ("stars",))
@pytest.mark.parametrize("eq", fh.EQS)
def test_fp32_headroom_of_the_closed_forms_at_every_gpu_shape(eq, opset):
    """What a correct fp32 evaluation of the header's formulas may differ from fp64 autograd by, measured on the CPU: at most
    TOL / 4 per channel, so that the bound the GPU file applies has a factor 4 of slack for another order of the sums."""
    route = fh.MHDRoute(eq, opset)
    worst = 0.0
    for shape in fh.GPU_SHAPES:
        for boundary in (False, True):
            x, g = seam_inputs(route, shape, boundary)
            want = ref_vjp(route, x.double(), g.double(), boundary)
            got = fh.closed_form(route, x, pad_g(g, boundary, shape))
            errs = channel_errs(got, want)
            worst = max(worst, max(errs.values()))
            assert max(errs.values()) <= TOL / 4, (eq, opset, shape, boundary, errs)
    print(f"{eq} {opset}: fp32 closed form against fp64 autograd worst {worst:.2e}")
