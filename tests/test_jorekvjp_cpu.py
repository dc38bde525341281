"""CPU tests of the fused backward of the reduced-MHD (JOREK) residual losses (``jorek=True`` of cp_pre_amd.losses,
libcp_pre_vjpjorek.so):
  * the exported ABI against include/cp_pre_vjpjorek.h and the ctypes binding, a C99 client compiled against the header;
  * the unit includes csrc/vjp_flat.hip for its geometry and host side; the Makefile lines;
  * every refusal of the entry, decided on unmapped addresses;
  * every host decision of ``jorek=True`` with its reason, on tensors without storage; ``jorek=False`` decides what it
    decided before and never loads the library;
  * the reference: ``JorekRoute`` against ``oracle.residuals.jorek_*`` in float64; every term of the closed forms counts;
  * headroom: the closed forms of the header in float32 on the CPU within TOL / 4 of float64 autograd at every GPU shape.
The device passes are covered by tests/test_gpu_jorekvjp.py."""
import ctypes
import functools
import inspect
import os
import re
import subprocess

import pytest
import torch

import jorekvjp_helpers as jh
from losses_helpers import channel_errs, ref_vjp, seam_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cp_pre_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "cp_pre_vjpjorek.h")
DECLARED = {"pre_vjpjorek_abi_version", "pre_vjpjorek_supported", "pre_vjpjorek_flat_f32"}
TOL = jh.TOL


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "vjpjorek_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_vjpjorek.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


def vars_view(B, F, Nx, Ny, Nt, pitch_t=None, ny_fastest=False):
    """``vars`` [B,F,Nx,Ny,Nt] without storage: dense; ``pitch_t`` > Nt: a t-slab of a longer tensor (rows not dense);
    ``ny_fastest``: the permuted view of memory [B,F,Nt,Nx,Ny]"""
    if ny_fastest:
        return torch.empty((B, F, Nt, Nx, Ny), device="meta").permute(0, 1, 3, 4, 2)
    Tp = pitch_t or Nt
    return torch.empty_strided((B, F, Nx, Ny, Nt), (F * Nx * Ny * Tp, Nx * Ny * Tp, Ny * Tp, Tp, 1), device="meta")


def dev(t, requires_grad=False):
    """a stand-in for a device tensor without storage: what the host decisions read of it"""
    return type("Dev", (), {"is_cuda": True, "numel": t.numel, "stride": t.stride, "dim": t.dim, "shape": t.shape,
                            "requires_grad": requires_grad, "__getitem__": lambda s, i: dev(t[i]),
                            "permute": lambda s, *p: dev(t.permute(*p))})()


def host_kernels(route):
    from cp_pre_amd import _dispatch, _lib
    return [_lib.farr(_dispatch.host_kernel(op.kernel).reshape(-1)) for op in route.ops]


# ------------------------------------------------------------------ the ABI
def test_vjpjorek_library_exports_exactly_its_entry_points():
    from cp_pre_amd import _lib
    so = _lib.VJPJOREK_SO_PATH
    assert os.path.exists(so), "libcp_pre_vjpjorek.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.VJPJOREK_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_VJPJOREK_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_VJPJOREK_ABI_VERSION == 1
    assert _lib._load("vjpjorek").pre_vjpjorek_abi_version() == _lib.PRE_VJPJOREK_ABI_VERSION
    assert _lib.load_vjpjorek() is _lib._load("vjpjorek")
    assert len(_lib._LIBS) == 8 and "vjpjorek" not in _lib._LIBS and "vjpjorek" in _lib._LIBS_MORE
    # the arguments of pre_screenjorek_flat_f32 with g, out and the gradient plumbing of the MHD entries
    sig, scr, mhd = (_lib.VJPJOREK_SIGNATURES["pre_vjpjorek_flat_f32"], _lib.SCREENJOREK_SIGNATURES["pre_screenjorek_flat_f32"],
                     _lib.VJPFLATMHD_SIGNATURES["pre_vjpflatmhd_continuity_f32"])
    assert sig[0] == scr[0] and sig[2:4] == scr[1:3] and sig[5:11] == scr[3:9] and sig[11:] == mhd[6:]
    assert sig[1] == mhd[0] and sig[4] == mhd[2]


def test_vjpjorek_wrong_abi_version_and_missing_library_raise(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_vjpjorek", None)
    monkeypatch.setattr(_lib, "PRE_VJPJOREK_ABI_VERSION", _lib.PRE_VJPJOREK_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_vjpjorek.so has ABI version 1"):
        _lib._load("vjpjorek")
    monkeypatch.setattr(_lib, "VJPJOREK_SO_PATH", str(tmp_path / "libcp_pre_vjpjorek.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_vjpjorek()


def test_vjpjorek_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "vjpjorek_check.o"
    subprocess.check_call(c_client_command(obj, link=False), stderr=subprocess.DEVNULL)
    assert obj.exists()
    exe = tmp_path / "vjpjorek_check"
    subprocess.check_call(c_client_command(exe), stderr=subprocess.DEVNULL)
    assert exe.exists()


def test_the_host_side_is_included_and_the_makefile_lines():
    src = open(os.path.join(CSRC, "vjp_flat_jorek.hip")).read()
    assert '#include "vjp_flat.hip"' in src and '#include "../../include/cp_pre_vjpjorek.h"' in src
    before = src.split('#include "vjp_flat.hip"')[0]
    assert re.search(r"^#define VF_MAXIN 4$", before, flags=re.M) and re.search(r"^#define VF_MAXOUT 3$", before, flags=re.M)
    assert re.search(r"^#define PRE_VJPFLAT_NO_ENTRIES\b", before, flags=re.M)
    assert src.count("__global__") == 1 and "vjp_jorek_kernel" in src and "atomicAdd" not in src      # ONE plane loop of its own
    for name in ("check_vjp_flat", "prepare_vjp_flat", "flat_chunk", "flat_split", "lds_barrier"):
        assert name in src, name                                   # taken from vjp_flat.hip / star_march.h, not restated
    assert "int check_vjp_flat" not in src and "int flat_chunk" not in src
    assert re.search(r"^#define VJPJOREK_TEMP_ONE_LAUNCH 0$", src, flags=re.M)     # (one launch needs scratch: DESIGN 4.22)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^vjpjorek_OBJS\s+:= vjp_flat_jorek\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bvjpjorek\b", mk, flags=re.M)
    shared = re.search(r"^SHARED_OBJS := ((?:.*\\\n)*.*)$", mk, flags=re.M).group(1)
    assert "$(vjpjorek_OBJS)" in shared
    assert mk.count("-disable-vector-combine") == 1
    line = next(ln for ln in mk.splitlines() if "-disable-vector-combine" in ln and not ln.startswith("#"))
    targets = line.split(":")[0].split()
    assert "vjp_flat.o" in targets and "vjp_flat_jorek.o" in targets
    assert re.search(r"^vjp_flat_jorek\.o:.*\bvjp_flat\.hip\b", mk, flags=re.M)            # the included unit is a dependency
    assert re.search(r"^\$\(vjpjorek_OBJS\): \$\(INC\)/cp_pre_vjpjorek\.h\b", mk, flags=re.M)
    assert "fast-math" not in mk


# ------------------------------------------------------------------ what is built
def test_supported_says_what_is_built():
    from cp_pre_amd import _lib
    lib = _lib.load_vjpjorek()
    for eq in (0, 1):
        for opset in jh.OPSETS:
            assert lib.pre_vjpjorek_supported(eq, *host_kernels(jh.JorekRoute(jh.EQS[eq], 12, opset))) == 0, (eq, opset)
        for opset in jh.DECLINED_SETS:
            assert lib.pre_vjpjorek_supported(eq, *host_kernels(jh.JorekRoute(jh.EQS[eq], 12, opset))) == _lib.PRE_E_UNSUPPORTED, (eq, opset)
        for i in range(5):                                         # weight off the star, on each operator in turn
            box = jh.JorekRoute(jh.EQS[eq], 12)
            box.ops[i].kernel[0, 0, 0] = 1.0
            assert lib.pre_vjpjorek_supported(eq, *host_kernels(box)) == _lib.PRE_E_UNSUPPORTED, (eq, i)
        ks = host_kernels(jh.JorekRoute(jh.EQS[eq], 12))
        for i in range(5):
            assert lib.pre_vjpjorek_supported(eq, *[None if j == i else k for j, k in enumerate(ks)]) == _lib.PRE_E_NULL
    ks = host_kernels(jh.JorekRoute("continuity", 12))
    assert lib.pre_vjpjorek_supported(2, *ks) == _lib.PRE_E_RANGE and lib.pre_vjpjorek_supported(-1, *ks) == _lib.PRE_E_RANGE
    # D_RR with a tap off D_R's axis, D_ZZ off D_Z's: every operator would be a general star
    for name, idx in (("D_RR", (0, 1, 1)), ("D_RR", (1, 1, 2)), ("D_ZZ", (1, 0, 1)), ("D_ZZ", (1, 1, 0))):
        r = jh.JorekRoute("temperature", 12)
        getattr(r.obj, name).kernel[idx] = 0.5
        assert lib.pre_vjpjorek_supported(1, *host_kernels(r)) == _lib.PRE_E_UNSUPPORTED, (name, idx)


def test_refusals_are_decided_before_any_device_work():
    """Every refusal returns from the host-side checks: the addresses below are not mapped, so a refusal that reached a
    launch could not return its code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_vjpjorek()
    B, T, X, Y = 2, 10, 9, 6
    n = B * T * X * Y
    ks = host_kernels(jh.JorekRoute("temperature", Y))
    coef = _lib.farr([1.0, 1.0, 2.0, 3.4])

    def v(base, i=0, sT=1, sY=None, sX=None, t=T):
        return _lib.PreField(base + 4 * n * i, X * Y * t, sT, Y * t if sX is None else sX, t if sY is None else sY)

    def Rv(t=T, **kw):
        s = dict(sB=0, sT=1, sX=0, sY=t)
        s.update(kw)
        return _lib.PreField(0x08000000, s["sB"], s["sT"], s["sX"], s["sY"])

    def call(eq, g=None, fields=None, Rb=None, outs=None, kernels=ks, coef=coef, dims=(B, T, X, Y), flags=0):
        g = v(0x10000000) if g is None else g
        fields = [v(0x20000000, i) for i in range(3)] if fields is None else fields
        outs = [v(0x40000000, i) for i in range(3)] if outs is None else outs
        Rb = Rv() if Rb is None else Rb
        fa = None if fields == "null" else (_lib.PreField * 3)(*fields)
        oa = None if outs == "null" else (_lib.PreField * 3)(*outs)
        return lib.pre_vjpjorek_flat_f32(eq, ctypes.byref(g), fa, None if Rb == "null" else ctypes.byref(Rb), oa, *kernels, coef,
                                         1.0, None, *dims, flags, None)
    assert call(2) == _lib.PRE_E_RANGE and call(-1) == _lib.PRE_E_RANGE
    for eq in (0, 1):
        last = 1 + eq                                              # the last field read, the last output written
        assert call(eq, dims=(B, 0, X, Y)) == _lib.PRE_E_NULL
        assert call(eq, g=v(0)) == _lib.PRE_E_NULL
        assert call(eq, fields="null") == _lib.PRE_E_NULL and call(eq, outs="null") == _lib.PRE_E_NULL
        assert call(eq, Rb="null") == _lib.PRE_E_NULL and call(eq, Rb=_lib.PreField(0, 0, 1, 0, T)) == _lib.PRE_E_NULL
        assert call(eq, coef=None) == _lib.PRE_E_NULL
        assert call(eq, fields=[v(0x20000000, i) if i != last else v(0) for i in range(3)]) == _lib.PRE_E_NULL
        assert call(eq, outs=[v(0x40000000, i) if i != last else v(0) for i in range(3)]) == _lib.PRE_E_NULL
        for i in range(5):
            assert call(eq, kernels=[None if j == i else k for j, k in enumerate(ks)]) == _lib.PRE_E_NULL
        # the layout conditions of cp_pre_vjpflat.h, on g, on the LAST field read and on the LAST output written
        ylast = _lib.PreField(0x10000000, T * X * Y, X * Y, Y, 1)                  # unit stride on Y: Ny-fastest
        assert call(eq, g=ylast) == _lib.PRE_E_UNSUPPORTED
        assert call(eq, g=v(0x10000000, sT=2)) == _lib.PRE_E_UNSUPPORTED
        for bad in (dict(sY=T + 2), dict(sX=Y * T + 4), dict(sT=2)):
            assert call(eq, g=v(0x10000000, **bad)) == _lib.PRE_E_UNSUPPORTED, (eq, bad)
            assert call(eq, fields=[v(0x20000000, i, **(bad if i == last else {})) for i in range(3)]) == _lib.PRE_E_UNSUPPORTED, (eq, bad)
            assert call(eq, outs=[v(0x40000000, i, **(bad if i == last else {})) for i in range(3)]) == _lib.PRE_E_UNSUPPORTED, (eq, bad)
        # R: a [Y][T] array behind every sample and plane
        for bad in (dict(sT=2), dict(sY=T + 1), dict(sX=Y * T), dict(sB=Y * T)):
            assert call(eq, Rb=Rv(**bad)) == _lib.PRE_E_UNSUPPORTED, (eq, bad)
        t96 = dict(t=96)
        assert call(eq, g=v(0x10000000, **t96), fields=[v(0x20000000, i, **t96) for i in range(3)], Rb=Rv(96),
                    outs=[v(0x40000000, i, **t96) for i in range(3)], dims=(B, 96, X, Y)) == _lib.PRE_E_UNSUPPORTED
        t7 = dict(t=7)                                                             # Y * T = 63
        assert call(eq, g=v(0x10000000, **t7), fields=[v(0x20000000, i, **t7) for i in range(3)], Rb=Rv(7),
                    outs=[v(0x40000000, i, **t7) for i in range(3)], dims=(B, 7, X, 9)) == _lib.PRE_E_UNSUPPORTED
        assert call(eq, flags=2) == _lib.PRE_E_UNSUPPORTED                        # any flag but PRE_VJP_CROP
        # the overlap rules: the last output over the first field; an output over g; over R; one base twice
        over = [v(0x40000000, i) for i in range(3)]
        over[last] = v(0x20000000 + 4 * Y * T)
        assert call(eq, outs=over) == _lib.PRE_E_SHAPE
        over_g = [v(0x10000000 + 4 * Y * T)] + [v(0x40000000, i) for i in range(1, 3)]
        assert call(eq, outs=over_g) == _lib.PRE_E_SHAPE
        over_R = [v(0x40000000, i) for i in range(3)]
        over_R[last] = v(0x08000000 + 4 * (Y * T - 1))
        assert call(eq, outs=over_R) == _lib.PRE_E_SHAPE
        assert call(eq, outs=[v(0x40000000)] * 3) == _lib.PRE_E_SHAPE
        # weight off the star, y_axis_fix, general stars
        box = jh.JorekRoute(jh.EQS[eq], Y)
        box.ops[1].kernel[0, 0, 0] = 1.0
        assert call(eq, kernels=host_kernels(box)) == _lib.PRE_E_UNSUPPORTED
        for opset in jh.DECLINED_SETS:
            assert call(eq, kernels=host_kernels(jh.JorekRoute(jh.EQS[eq], Y, opset))) == _lib.PRE_E_UNSUPPORTED, (eq, opset)


# ------------------------------------------------------------------ host decisions
def test_without_the_keyword_jorek_decides_what_it_decided_before(monkeypatch):
    from cp_pre_amd import _lib, losses

    def boom():
        raise AssertionError("jorek=False loaded libcp_pre_vjpjorek.so")
    monkeypatch.setattr(_lib, "load_vjpjorek", boom)
    for fn in (losses.pi_loss, losses.pisl_loss, losses.residual_vjp):
        params = list(inspect.signature(fn).parameters)
        assert params[-1] == "jorek" and params[-2] == "mhd" and inspect.signature(fn).parameters["jorek"].default is False
    assert list(inspect.signature(losses._Spec.__init__).parameters)[-2:] == ["mhd", "jorek"]
    ok = dev(vars_view(2, 3, 10, 16, 8))
    for eq in jh.EQS:
        route = jh.JorekRoute(eq, 16)
        for spec in (losses._Spec(route.method), losses._Spec(route.method, False, False), losses._Spec(route.method, "flat")):
            assert not spec.jorek and spec.kind is None and spec.why == "no fused VJP for JOREK"
            assert spec.prepare(ok) == ("no fused VJP for JOREK", ()) and spec.prepare_flat(ok) == ("no fused VJP for JOREK", ())
    with pytest.raises(TypeError):                                 # a partial is a method only under the keyword
        losses._Spec(functools.partial(jh.JorekRoute("continuity", 16).obj.residual_continuity, norms=True))
    # on the CPU: the parent's answer and the composed gradient (the method itself needs the device: its expression here)
    route = jh.JorekRoute("temperature", 6, K=jh.K_BIG)
    monkeypatch.setattr(losses._Spec, "call", lambda self, v, boundary, minus=None: route.residual(jh.to_logical(v), boundary))
    x, g = seam_inputs(route, (2, 10, 5, 6), False)
    got = losses.residual_vjp(route.method, jh.to_vars(x), g)
    assert losses.last_route() == "fallback:no fused VJP for JOREK"
    assert torch.equal(got, losses.residual_vjp(route.method, jh.to_vars(x), g, False, False, False, False))
    errs = channel_errs(jh.to_logical(got), ref_vjp(route, x.double(), g.double(), False))
    assert max(errs.values()) <= TOL, errs
    # the other families do not see the keyword
    from losses_helpers import Route
    s = losses._Spec(Route("ns_momentum").method, False, True)
    assert s.kind == "ns_momentum" and not s.jorek
    assert not losses._Spec(route.obj.D_R, False, True).jorek


def test_cpu_inputs_take_the_fallback_under_the_keyword(monkeypatch):
    from cp_pre_amd import losses
    route = jh.JorekRoute("continuity", 6, norms=True)
    monkeypatch.setattr(losses._Spec, "call", lambda self, v, boundary, minus=None: route.residual(jh.to_logical(v), boundary))
    x, g = seam_inputs(route, (2, 10, 5, 6), True)
    a = losses.residual_vjp(route.method, jh.to_vars(x), g, boundary=True, jorek=True)
    assert losses.last_route() == "fallback:input on the CPU"
    errs = channel_errs(jh.to_logical(a), ref_vjp(route, x.double(), g.double(), True))
    assert max(errs.values()) <= TOL, errs


def test_every_host_decision_of_the_keyword_has_its_reason():
    from cp_pre_amd import losses
    S = losses._Spec
    for eq in jh.EQS:
        route = jh.JorekRoute(eq, 16)
        spec = S(route.method, False, True)
        assert spec.jorek and spec.kind == "jorek_" + eq and spec.why is None and spec.eq == jh.EQS.index(eq) and not spec.norms
        assert len(spec.ops) == 5
        ok = dev(vars_view(2, 3, 10, 16, 8))
        why, ks = spec.prepare_jorek(ok)
        assert why is None and len(ks) == 5
        assert spec.prepare_jorek(dev(vars_view(2, 5, 10, 16, 8)))[0] is None                  # F = 5: channels 3, 4 not read
        assert spec.prepare_jorek(dev(vars_view(2, 2, 10, 16, 8))) == ("fewer than three JOREK channels", ())
        assert spec.prepare_jorek(dev(vars_view(2, 3, 5, 12, 96))) == ("Nt >= 96", ())
        assert spec.prepare_jorek(dev(vars_view(2, 3, 5, 9, 7))) == ("merged row Ny*Nt not a multiple of 4", ())
        assert spec.prepare_jorek(dev(vars_view(2, 3, 10, 16, 8, ny_fastest=True))) == ("fields not Nt-fastest", ())
        assert spec.prepare_jorek(dev(vars_view(2, 3, 10, 16, 6, pitch_t=8))) == ("rows of the fields not dense", ())
        assert spec.prepare_jorek(dev(vars_view(2, 3, 10, 12, 8))) == ("len(R) is not Ny", ())
        cpu = dev(vars_view(2, 3, 10, 16, 8))
        cpu.is_cuda = False
        assert spec.prepare_jorek(cpu) == ("input on the CPU", ())
        assert spec.prepare_jorek(dev(vars_view(0, 3, 10, 16, 8))) == ("empty input", ())
        # what declines in any layout, each before the layout is looked at
        slab = dev(vars_view(2, 3, 10, 16, 6, pitch_t=8))
        off = jh.JorekRoute(eq, 16)
        off.obj.fused = False
        assert S(off.method, False, True).prepare_jorek(slab) == ("fused=False", ())
        for i in range(5):
            live = jh.JorekRoute(eq, 16)
            live.ops[i].kernel.requires_grad_(True)
            assert S(live.method, False, True).prepare_jorek(slab) == ("operator kernel requires grad", ())
        assert spec.prepare_jorek(ok, dev(vars_view(2, 3, 10, 16, 8), True)) == ("yy requires grad", ())
        box = jh.JorekRoute(eq, 16)
        box.obj.D_ZZ.kernel[0, 0, 0] = 1.0
        assert S(box.method, False, True).prepare_jorek(ok) == ("operator kernel off the 7-point star", ())
        for opset in jh.DECLINED_SETS:
            assert S(jh.JorekRoute(eq, 16, opset).method, False, True).prepare_jorek(ok) == ("declined by the library", ())
        assert S(jh.JorekRoute(eq, 16, "rescaled").method, False, True).prepare_jorek(ok)[0] is None
    n = S(jh.JorekRoute("continuity", 16, norms=True).method, False, True)
    assert n.jorek and n.norms and n.kind == "jorek_continuity"
    assert n.obj._coef(0, True) == [2 * jh.NORM_DX * jh.NORM_DY, jh.NORM_DT, 4 * jh.NORM_DT * jh.NORM_DY, 4 * jh.NORM_DT * float(torch.tensor(3.4))]
    with pytest.raises(TypeError):                                 # any other keyword is not the equation's
        S(functools.partial(jh.JorekRoute("continuity", 16).obj.residual_continuity, absolute=True), False, True)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("eq", jh.EQS)
def test_the_restated_expressions_are_the_oracles_in_fp64(eq):
    """``JorekRoute.full`` against ``oracle.residuals.jorek_continuity`` / ``jorek_temperature`` in float64, with the
    oracle's operators carrying the same kernels: default and rescaled, both K, norms"""
    import screen_helpers as sh
    from oracle import residuals as orr
    shape = (2, 10, 5, 6)
    for opset in jh.OPSETS:
        for K in (None, jh.K_BIG):
            for norms in ((False, True) if eq == "continuity" else (False,)):
                route = jh.JorekRoute(eq, shape[3], opset, K=K, norms=norms)
                x, _ = seam_inputs(route, shape, True)
                ops = orr.OpsJorek()
                for name in jh.RESCALE:
                    getattr(ops, name).kernel = getattr(route.obj, name).kernel.clone()
                with sh.oracle_fp64():
                    R = jh.radius(shape[3]).double()
                    if eq == "continuity":
                        kw = dict(norms=True, dx=jh.NORM_DX, dy=jh.NORM_DY, dt=jh.NORM_DT) if norms else {}
                        want = orr.jorek_continuity(jh.to_vars(x.double()), R, boundary=True, ops=ops, **kw)
                    else:
                        want = orr.jorek_temperature(jh.to_vars(x.double()), R, K=route.obj.K, boundary=True, ops=ops)
                got = route.full(x.double())
                err = float((got - want).abs().max() / want.abs().max())
                assert err <= 1e-13, (eq, opset, K, norms, err)


BIG_SHAPES = [s for s in jh.GPU_SHAPES if min(s[1:]) > 1]


@pytest.mark.parametrize("eq", jh.EQS)
def test_every_term_of_the_closed_forms_counts(eq):
    """At every GPU shape with more than one cell per axis and K = 0.75, dropping any one term of the closed forms moves
    some channel by more than 100 TOL: a kernel that left one out could not pass."""
    assert len(BIG_SHAPES) == len(jh.SEAM_SHAPES) + 1
    least = 1e300
    for shape in BIG_SHAPES:
        route = jh.JorekRoute(eq, shape[3], "rescaled", K=jh.K_BIG)
        x, g = seam_inputs(route, shape, True)
        want = ref_vjp(route, x.double(), g.double(), True)
        parts = jh.terms(route, x.double(), g.double())
        assert sorted(parts) == list(range(route.nread))
        for c, ts in parts.items():
            for i in range(len(ts)):
                errs = channel_errs(jh.closed_form(route, x.double(), g.double(), drop=(c, i)), want)
                least = min(least, errs["ch%d" % c])
                assert errs["ch%d" % c] > 100 * TOL, (eq, shape, c, i, errs)
    print(f"{eq}: the least a dropped term moves its channel by is {least:.2e}")


@pytest.mark.parametrize("K", [None, jh.K_BIG])
@pytest.mark.parametrize("opset", jh.OPSETS)
@pytest.mark.parametrize("eq", jh.EQS)
def test_fp32_headroom_of_the_closed_forms_at_every_gpu_shape(eq, opset, K):
    """What a correct fp32 evaluation of the header's formulas may differ from fp64 autograd by, measured on the CPU: at most
    TOL / 4 per channel, so that the bound the GPU file applies has a factor 4 of slack for another order of the sums."""
    worst = 0.0
    for shape in jh.GPU_SHAPES:
        for norms in ((False, True) if eq == "continuity" else (False,)):
            route = jh.JorekRoute(eq, shape[3], opset, K=K, norms=norms)
            for boundary in (False, True):
                x, g = seam_inputs(route, shape, boundary)
                want = ref_vjp(route, x.double(), g.double(), boundary)
                got = jh.closed_form(route, x, jh.pad_g(g, boundary, shape))
                errs = channel_errs(got, want)
                worst = max(worst, max(errs.values()))
                assert max(errs.values()) <= TOL / 4, (eq, opset, K, shape, boundary, errs)
                assert not got[:, route.nread:].any()
    print(f"{eq} {opset} K={K}: fp32 closed form against fp64 autograd worst {worst:.2e}")
