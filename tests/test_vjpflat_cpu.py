"""CPU tests of the fused loss backward for Nt-fastest views (``flat=True`` of cp_pre_amd.losses, libcp_pre_vjpflat.so):
  * the exported ABI against include/cp_pre_vjpflat.h and the ctypes binding, a C99 client compiled against the header;
  * the default (``flat=False``) decides what it decided before and never loads the new library;
  * every host reason ``flat=True`` falls back for, with its exact string;
  * the split rule's seams as tests/vjpflat_helpers.py names them;
  * the formulas in float32 on the CPU within TOL / 4 of float64 at every shape the GPU file runs.
The device passes are covered by tests/test_gpu_vjpflat.py."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import vjpflat_helpers as vf
from losses_helpers import Route, asym_star, channel_errs, ref_loss, ref_vjp, seam_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_vjpflat.h")
DECLARED = {"pre_vjpflat_abi_version", "pre_vjpflat_stencil3d_f32", "pre_vjpflat_linear2_f32", "pre_vjpflat_ns_momentum_f32"}
TOL = vf.TOL


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "vjpflat_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_vjpflat.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


def full_star_route(name):
    """``name`` with every operator an asymmetric star, all taps non-zero and distinct per operator"""
    route = Route(name)
    for i, op in enumerate(route.ops):
        op.kernel = asym_star(3) * (1.0 + 0.25 * i)
    return route


def routes():
    """(label, Route) of every case family the GPU file runs: asymmetric stars on the linear routes, the reference's
    operators and full asymmetric stars on the NS routes"""
    return [("wave", Route("wave", asym=True)), ("op3d", Route("op3d", asym=True)), ("ns_continuity", Route("ns_continuity")),
            ("ns_continuity_stars", full_star_route("ns_continuity")), ("ns_momentum", Route("ns_momentum")),
            ("ns_momentum_stars", full_star_route("ns_momentum"))]


# ------------------------------------------------------------------ the ABI
def test_vjpflat_library_exports_exactly_its_entry_points():
    from cp_pre_amd import _lib
    so = _lib.VJPFLAT_SO_PATH
    assert os.path.exists(so), "libcp_pre_vjpflat.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.VJPFLAT_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_VJPFLAT_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_VJPFLAT_ABI_VERSION == 1
    assert _lib._load("vjpflat").pre_vjpflat_abi_version() == _lib.PRE_VJPFLAT_ABI_VERSION
    assert _lib.load_vjpflat() is _lib._load("vjpflat")
    assert "vjpflat" not in _lib._LIBS and "vjpflat" in _lib._LIBS_MORE
    # the entries mirror cp_pre_vjp.h argument for argument
    for name in DECLARED - {"pre_vjpflat_abi_version"}:
        assert _lib.VJPFLAT_SIGNATURES[name] == _lib.VJP_SIGNATURES[name.replace("vjpflat", "vjp")], name
    strip = lambda text: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    tiled = strip(open(os.path.join(ROOT, "include", "cp_pre_vjp.h")).read())
    for name, args in re.findall(r"int (pre_vjpflat_\w+_f32) ?\(([^;]*)\);", strip(header)):
        assert "int %s(%s);" % (name.replace("vjpflat", "vjp"), args) in tiled.replace("f32 (", "f32("), name


def test_vjpflat_wrong_abi_version_and_missing_library_raise(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_vjpflat", None)
    monkeypatch.setattr(_lib, "PRE_VJPFLAT_ABI_VERSION", _lib.PRE_VJPFLAT_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_vjpflat.so has ABI version 1"):
        _lib._load("vjpflat")
    monkeypatch.setattr(_lib, "VJPFLAT_SO_PATH", str(tmp_path / "libcp_pre_vjpflat.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_vjpflat()


def test_vjpflat_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "vjpflat_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_vjpflat_translation_unit_and_makefile_target():
    src = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "vjp_flat.hip")).read()
    assert '#include "vjp_functors.h"' in src and "PRE_STAR_MARCH_TEMPLATES_ONLY" not in src and "star_march.hip" not in src
    assert '#include "star_march.h"' in open(os.path.join(ROOT, "cp_pre_amd", "csrc", "vjp_functors.h")).read()
    march = src.split("// ---")[1]
    assert "vjp_flat_kernel" in march and "lds_barrier" in march and "atomic" not in march
    assert '#include "../../include/cp_pre_vjpflat.h"' in src
    mk = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "Makefile")).read()
    assert "vjpflat_OBJS := vjp_flat.o" in mk and re.search(r"^LIBS\s+:=.*\bvjpflat\b", mk, flags=re.M)
    shared = re.search(r"^SHARED_OBJS := ((?:.*\\\n)*.*)$", mk, flags=re.M).group(1)
    assert "$(vjpflat_OBJS)" in shared and re.search(r"^\$\(SHARED_OBJS\): \$\(SHARED_HDRS\)$", mk, flags=re.M)
    assert re.search(r"^SHARED_HDRS := .*\bstar_march\.h\b.*\bvjp_functors\.h\b", mk, flags=re.M)
    assert "star_march.hip" not in mk and mk.count("-disable-vector-combine") == 1      # (no hand-written line, flags once)
    assert re.search(r"^\$\(vjpflat_OBJS\): \$\(INC\)/cp_pre_vjpflat\.h \$\(INC\)/cp_pre_vjp\.h$", mk, flags=re.M)


# ------------------------------------------------------------------ host decisions
def view(B, F, Nt, Nx, Ny, pitch_t=None, chan_gap=0):
    """an Nt-fastest [B,(F),Nt,Nx,Ny] tensor without storage (``pitch_t`` > Nt: a t-slab of a larger tensor, rows not
    dense); F = 0: a field"""
    Tp = pitch_t or Nt
    plane = Nx * Ny * Tp + chan_gap
    if F == 0:
        return torch.empty_strided((B, Nt, Nx, Ny), (plane, 1, Ny * Tp, Tp), device="meta")
    return torch.empty_strided((B, F, Nt, Nx, Ny), (F * plane, plane, 1, Ny * Tp, Tp), device="meta")


def test_the_default_decides_what_it_decided_before(monkeypatch):
    """``flat`` defaults to False on the three entry points; with the default (and with ``flat=False`` spelled out) an input
    takes the route it took, the reason string included, and the new library is never loaded"""
    from cp_pre_amd import _lib, losses
    for fn in (losses.pi_loss, losses.pisl_loss, losses.residual_vjp):
        assert inspect.signature(fn).parameters["flat"].default is False

    def boom():
        raise AssertionError("the default keyword loaded libcp_pre_vjpflat.so")
    monkeypatch.setattr(_lib, "load_vjpflat", boom)
    ns, wave = Route("ns_momentum"), Route("wave")
    S = losses._Spec
    # the host decision of an Nt-fastest view is the one line it was, whatever else holds
    for spec, v in ((S(ns.method), view(2, 3, 8, 10, 16)), (S(wave.method), view(2, 0, 8, 10, 16)), (S(wave.method), view(2, 0, 96, 5, 12))):
        x = type("Dev", (), {"is_cuda": True, "numel": v.numel, "stride": v.stride, "dim": v.dim, "shape": v.shape})()
        assert spec.prepare(x) == ("no unit stride on the last axis", ())
    # CPU inputs: the same fallback, value and gradient with and without the keyword (no device here: the composed
    # expression the fallback evaluates is stood in for by the fp32 formulas of losses_helpers)
    monkeypatch.setattr(S, "call", lambda self, x, boundary, minus=None: ns.residual(x, boundary))
    x, _ = seam_inputs(ns, (2, 8, 10, 16), True)
    xt = x.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    got = []
    for kw in ({}, {"flat": False}, {"flat": True}):
        xr = xt.clone().requires_grad_(True)
        loss = losses.pi_loss(ns.method, xr, **kw)
        assert losses.last_route() == "fallback:input on the CPU"
        loss.backward()
        got.append((loss.detach().clone(), xr.grad.clone()))
        g = torch.ones(2, 6, 8, 14)
        v = losses.residual_vjp(ns.method, xt, g, **kw)
        assert losses.last_route() == "fallback:input on the CPU"
        got[-1] += (v,)
    for other in got[1:]:
        assert all(torch.equal(a, b) for a, b in zip(got[0], other))
    # the unit-stride chain of prepare() is unchanged: same strings, same order
    dev = lambda t: type("Dev", (), {"is_cuda": True, "numel": t.numel, "stride": t.stride, "dim": t.dim, "shape": t.shape,
                                     "requires_grad": False})()
    dense = dev(torch.empty((2, 3, 8, 10, 16), device="meta"))
    from cp_pre_amd import residuals as R
    assert S(R.NavierStokes(0.01, 0.1, 0.1, fused=False).residual_momentum).prepare(dense) == ("fused=False", ())
    live = R.NavierStokes(0.01, 0.1, 0.1)
    live.D_x.kernel.requires_grad_(True)
    assert S(live.residual_momentum).prepare(dense) == ("operator kernel requires grad", ())
    why, ks = S(ns.method).prepare(dense)
    assert why is None and len(ks) == 4
    assert S(R.MHD().residual_continuity).prepare(dense) == ("no fused VJP for MHD", ())


def test_flat_host_refusals_and_their_reasons():
    """every reason ``flat=True`` takes the fallback for, before anything is launched"""
    from cp_pre_amd import losses
    from cp_pre_amd import residuals as R
    S = losses._Spec
    ns, cont, wave = S(Route("ns_momentum").method), S(Route("ns_continuity").method), S(Route("wave").method)
    ok5, ok4 = view(2, 3, 8, 10, 16), view(2, 0, 8, 10, 16)
    for spec, v, n in ((ns, ok5, 4), (cont, ok5, 2)):
        why, ks = spec.prepare_flat(v)
        assert why is None and len(ks) == n
    why, (w, off) = wave.prepare_flat(ok4)
    assert why is None and len(w) == len(off) == 7
    assert wave.prepare_flat(view(2, 1, 8, 10, 16))[0] is None                       # [BS,1,Nt,Nx,Ny]
    for spec, five in ((ns, 3), (cont, 3), (wave, 0)):
        assert spec.prepare_flat(view(2, five, 96, 5, 12)) == ("Nt >= 96", ())
        assert spec.prepare_flat(view(2, five, 7, 5, 9)) == ("merged row Ny*Nt not a multiple of 4", ())
    # rows that are not dense: NS momentum reads u and v there; the linear routes read no field
    slab = view(2, 3, 6, 10, 16, pitch_t=8)
    assert ns.prepare_flat(slab) == ("rows of u, v not dense", ())
    assert cont.prepare_flat(slab)[0] is None and wave.prepare_flat(view(2, 0, 6, 10, 16, pitch_t=8))[0] is None
    # a last axis without unit stride whose unit-stride axis is not Nt either
    odd = torch.empty_strided((2, 8, 10, 16), (2560, 160, 1, 10), device="meta")
    assert wave.prepare_flat(odd) == ("the unit-stride axis is not Nt", ())
    # the 1-D family and Burgers, MHD, JOREK
    v3 = torch.empty_strided((4, 8, 10), (80, 1, 8), device="meta")
    assert S(Route("burgers").method).prepare_flat(v3) == ("no flat VJP for the 1-D family", ())
    assert S(Route("advection").method).prepare_flat(v3) == ("no flat VJP for the 1-D family", ())
    assert S(Route("op2d").method).prepare_flat(v3) == ("no flat VJP for the 1-D family", ())
    assert S(R.MHD().residual_continuity).prepare_flat(view(2, 6, 8, 10, 16)) == ("no fused VJP for MHD", ())
    # what falls back whatever the layout
    assert S(R.NavierStokes(0.01, 0.1, 0.1, fused=False).residual_momentum).prepare_flat(ok5) == ("fused=False", ())
    live = R.NavierStokes(0.01, 0.1, 0.1)
    live.D_x.kernel.requires_grad_(True)
    assert S(live.residual_momentum).prepare_flat(ok5) == ("operator kernel requires grad", ())
    yy = view(2, 3, 8, 10, 16).requires_grad_(True)
    assert ns.prepare_flat(ok5, yy) == ("yy requires grad", ())
    assert wave.prepare_flat(view(2, 2, 8, 10, 16)) == ("multi-channel wave input", ())
    box = R.NavierStokes(0.01, 0.1, 0.1)
    box.D_x.kernel.data[0, 0, 0] = 0.5
    assert S(box.residual_momentum).prepare_flat(ok5)[0] == "operator kernel off the 7-point star"
    # a unit-stride input is not offered to the flat route at all
    assert not ns.wants_flat(type("Dev", (), {"is_cuda": True, "numel": lambda s: 1, "dim": lambda s: 5, "stride": lambda s, d: 1})())


# ------------------------------------------------------------------ the split rule and the seams named from it
def test_vjpflat_seam_shapes_cross_the_seams_they_are_named_for():
    sp = {k: vf.split(s) for k, s in vf.SEAM_SHAPES.items()}
    for k, s in vf.SEAM_SHAPES.items():
        # fewer workgroups than resident slots whatever the device: the split of these shapes does not depend on it
        assert s[0] * sp[k]["nCh"] * sp[k]["nTSeg"] < vf.MIN_SLOTS and sp[k] == vf.split(s, 1 << 20), k
    assert sp["one_chunk_one_march"] == dict(nt=256, nCh=1, last=32, hq=2, tSeg=10, nTSeg=1, last_planes=10)
    for k in ("straddle_10", "straddle_6"):
        B, Nt, Nx, Ny = vf.SEAM_SHAPES[k]
        assert Nt % 4 == 2 and Ny * Nt == 60 and sp[k]["nCh"] == 1, k
    assert 60 * 36 > 2048 and (sp["chunk_seam"]["nt"], sp["chunk_seam"]["nCh"], sp["chunk_seam"]["last"], sp["chunk_seam"]["hq"]) == (320, 2, 220, 15)
    assert vf.SEAM_SHAPES["bound"][1] == 92 and 92 < vf.FLAT_MAX_Y <= 96 and sp["bound"]["hq"] == 23 and sp["bound"]["nCh"] == 2
    # the marched axis: 16 planes are one march, 17 the first cut
    B, Nt, _, Ny = vf.SEAM_SHAPES["two_marches"]
    assert vf.split((B, Nt, 16, Ny))["nTSeg"] == 1
    assert (sp["two_marches"]["tSeg"], sp["two_marches"]["nTSeg"], sp["two_marches"]["last_planes"]) == (9, 2, 8)
    assert (sp["full_last_march"]["tSeg"], sp["full_last_march"]["nTSeg"], sp["full_last_march"]["last_planes"]) == (9, 2, 9)
    assert (sp["one_plane_last_march"]["tSeg"], sp["one_plane_last_march"]["nTSeg"], sp["one_plane_last_march"]["last_planes"]) == (9, 16, 1)
    for shape in vf.DECLINED:
        assert shape[1] >= vf.FLAT_MAX_Y or (shape[3] * shape[1]) % 4


# ------------------------------------------------------------------ headroom of the GPU bounds
@pytest.mark.parametrize("boundary", [False, True])
def test_fp32_formulas_stay_within_a_quarter_of_tol_at_the_gpu_shapes(boundary):
    """the inputs of tests/test_gpu_vjpflat.py (same seeds, same stars), the formulas in fp32 on the CPU against fp64"""
    for label, route in routes():
        worst = {}
        for shape in vf.SEAM_SHAPES.values():
            x, g = seam_inputs(route, shape, boundary)
            errs = channel_errs(ref_vjp(route, x, g, boundary), ref_vjp(route, x.double(), g.double(), boundary))
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(errs.values()) <= TOL / 4, (label, shape, boundary, errs)
        print(f"headroom vjp {label} boundary={boundary}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_fp32_loss_formulas_stay_within_a_quarter_of_tol_at_the_script_view():
    route = Route("wave", asym=True)
    for shape in ((2, 8, 10, 16), (2, 10, 17, 6)):                 # the interior of the preds of the script's-view test
        x, _ = seam_inputs(route, shape, True, seed=2)
        yy = x + 0.1 * torch.rand(x.shape, generator=torch.Generator().manual_seed(3))
        for boundary in (False, True):
            for y in (None, yy):
                v32, g32 = ref_loss(route, x, boundary, y, 1000.0)
                v64, g64 = ref_loss(route, x.double(), boundary, None if y is None else y.double(), 1000.0)
                assert abs(v32 - v64) <= TOL / 4 * abs(v64) and max(channel_errs(g32, g64).values()) <= TOL / 4
