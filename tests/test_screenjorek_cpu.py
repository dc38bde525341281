"""CPU tests of the opt-in fused screen of the JOREK residuals (cp_pre_amd.screen with ``jorek=True``,
libcp_pre_screenjorek.so):
  * the exported ABI against include/cp_pre_screenjorek.h and the ctypes binding, a C99 client compiled against the header;
  * what ``_Spec`` resolves with and without the keyword, and the host reasons for the three-pass route;
  * both entry points refusing, from ctypes with unmapped addresses, before any launch;
  * the caps the GPU tests' tolerances rest on, from the oracle alone, for every case tests/test_gpu_screenjorek.py uses.
The device passes are covered by tests/test_gpu_screenjorek.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import screenjorek_helpers as sj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screenjorek.h")
DECLARED = {"pre_screenjorek_abi_version", "pre_screenjorek_f32", "pre_screenjorek_flat_f32"}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screenjorek_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screenjorek.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_screenjorek_library_exports_exactly_its_three_symbols():
    from cp_pre_amd import _lib
    so = _lib.SCREENJOREK_SO_PATH
    assert os.path.exists(so), "libcp_pre_screenjorek.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and len(DECLARED) == 3
    assert exported == declared and set(_lib.SCREENJOREK_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREENJOREK_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREENJOREK_ABI_VERSION == 1
    assert _lib._load("screenjorek").pre_screenjorek_abi_version() == _lib.PRE_SCREENJOREK_ABI_VERSION
    assert _lib.load_screenjorek() is _lib._load("screenjorek")
    # every declaration cites the reference lines it serves
    for decl in re.split(r"\n(?=/\* )", header.split("pre_screenjorek_abi_version(void);", 1)[1]):
        if "int pre_screenjorek_" in decl:
            assert re.search(r"Joint/JOREK_residuals_CP\.py:210-243", decl) and "297-308" in decl, decl[:80]
    assert len(_lib._LIBS) == 8 and "screenjorek" not in _lib._LIBS and "screenjorek" in _lib._LIBS_MORE


def test_screenjorek_ctypes_signatures_have_the_header_arity():
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^int\s+(pre_screenjorek_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    assert {n for n, _ in found} == DECLARED
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREENJOREK_SIGNATURES[name]), name
    # the argument list of pre_residual_jorek_f32 with the set descriptor in place of `out`
    res = _lib.SIGNATURES["pre_residual_jorek_f32"]
    for name, desc in (("pre_screenjorek_f32", _lib.PreScreen), ("pre_screenjorek_flat_f32", _lib.PreScreenFlat)):
        sig = _lib.SCREENJOREK_SIGNATURES[name]
        assert len(sig) == len(res) and sig[9] is ctypes.POINTER(desc) and sig[10:] == res[10:]


def test_screenjorek_wrong_abi_version_raises_import_error(monkeypatch):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screenjorek", None)
    monkeypatch.setattr(_lib, "PRE_SCREENJOREK_ABI_VERSION", _lib.PRE_SCREENJOREK_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_screenjorek.so has ABI version 1"):
        _lib._load("screenjorek")


def test_screenjorek_missing_library_raises_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screenjorek", None)
    monkeypatch.setattr(_lib, "SCREENJOREK_SO_PATH", str(tmp_path / "libcp_pre_screenjorek.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_screenjorek()


def test_screenjorek_header_compiles_as_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])


def test_screenjorek_c_client_compiles_against_the_header(tmp_path):
    obj = tmp_path / "screenjorek_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_screenjorek_translation_unit_and_makefile_target():
    """the kernels reach the new translation unit through two headers that the existing two include as well"""
    csrc = os.path.join(ROOT, "cp_pre_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in ("screen_jorek.hip", "screen_march.hip", "screen_flat.hip",
                                                             "screen_march.h", "screen_flat.h")}
    assert '#include "screen_march.h"' in src["screen_jorek.hip"] and '#include "screen_flat.h"' in src["screen_jorek.hip"]
    assert '#include "../../include/cp_pre_screenjorek.h"' in src["screen_jorek.hip"]
    assert '#include "screen_march.h"' in src["screen_march.hip"] and '#include "screen_flat.h"' in src["screen_flat.hip"]
    assert "screen_march_kernel(const SGeom g" in src["screen_march.h"] and "__global__" not in src["screen_march.hip"]
    assert "screen_flat_kernel(const FGeom g" in src["screen_flat.h"] and "__global__" not in src["screen_flat.hip"]
    assert "__global__" not in src["screen_jorek.hip"]                    # nothing new runs on the device
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^screenjorek_OBJS\s+:= screen_jorek\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bscreenjorek\b", mk, flags=re.M)
    assert re.search(r"^SHARED_HDRS\s+:=.*\bscreen_march\.h\b.*\bscreen_flat\.h\b", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS\s+:=(.|\\\n)*\$\(screenjorek_OBJS\)", mk, flags=re.M)
    assert "$(screenjorek_OBJS): $(INC)/cp_pre_screenjorek.h $(INC)/cp_pre_screen.h $(INC)/cp_pre_screenflat.h" in mk


# ------------------------------------------------------------------ what the keyword resolves, on the host
def test_screenjorek_spec_resolves_the_opt_in_kinds():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _Spec
    jo = sj.jorek_of()
    x = sj.to_vars(torch.rand(3, 3, 10, 5, 12))                          # [BS,F,Nx,Ny,Nt], dense in the logical order
    for eq, name in enumerate(sj.EQS):
        method = getattr(jo, "residual_" + name)
        # without the keyword nothing changed, and nothing changes by asking
        for plain in (_Spec(method), _Spec(method, jorek=False)):
            assert plain.kind is None and plain.why == "no fused screen for JOREK" and plain.chan == () and plain.ops == ()
            assert plain.prepare(x, None, torch.ones(2), None) == ("no fused screen for JOREK", ())
            assert not plain.nt_fastest(sj.to_vars(torch.rand(3, 3, 5, 12, 10).permute(0, 1, 4, 2, 3)))
        spec = _Spec(method, jorek=True)
        assert spec.kind == "jorek_" + name and spec.why is None and spec.eq == eq and spec.rows_kind is None
        assert len(spec.ops) == 5 and all(a is b for a, b in zip(spec.ops, jo._ops()))
        fs = spec.fields(x)
        assert len(fs) == 2 + eq and all(tuple(f.shape) == (3, 10, 5, 12) for f in fs)
        assert all(f.data_ptr() == g.data_ptr() and f.stride() == g.stride() for f, g in zip(fs, R.JOREK.unstack_fields(x)))
        assert spec.field_shape(x) == (3, 10, 5, 12) and not spec.reads_halo()
        assert spec.entry("") == "pre_screenjorek_f32" and spec.entry("flat") == "pre_screenjorek_flat_f32"
        assert spec.route("") == "fused:jorek_" + name and spec.route("flat") == "fused:flat_jorek_" + name
        coef, = spec.scalars()
        assert list(coef) == [ctypes.c_float(v).value for v in jo._coef(eq)]
    assert jo._coef(0) == [1.0, 1.0, 2.0, float(torch.tensor(3.4, dtype=torch.float32))]
    assert jo._coef(1) == [float(2 * torch.tensor(5 / 3, dtype=torch.float32)), 0.0, 0.0, float(torch.tensor(2.25e-7, dtype=torch.float32))]
    # the keyword on anything but the two JOREK equations is an error, not a silent three-pass route
    for other in (R.MHD().residual_continuity, jo.unstack_fields):
        with pytest.raises(TypeError):
            _Spec(other, jorek=True)


def test_screenjorek_layout_decisions_are_taken_on_the_field_views():
    from cp_pre_amd.screen import _Spec
    spec = _Spec(sj.jorek_of().residual_temperature, jorek=True)
    dense = torch.rand(3, 3, 5, 12, 10)                                   # the script's vars: Nt-fastest field views
    assert spec.nt_fastest(dense) and spec._layout_flat(spec.view(dense)) is None
    assert spec._layout(spec.view(dense)) == "no unit stride on the last axis"
    ny = sj.to_vars(torch.rand(3, 3, 10, 5, 12))                          # a view of memory [BS,F,Nt,Nx,Ny]
    assert not spec.nt_fastest(ny) and spec._layout(spec.view(ny)) is None
    assert spec._layout(spec.view(sj.to_vars(torch.rand(3, 3, 10, 5, 13)))) == "row width not a multiple of 4"
    assert spec._layout_flat(spec.view(torch.rand(3, 3, 5, 12, 96))) == "Nt >= 96"
    assert spec._layout_flat(spec.view(torch.rand(3, 3, 5, 13, 10))) == "merged row Ny*Nt not a multiple of 4"
    assert spec._layout_flat(spec.view(torch.rand(3, 3, 5, 12, 10)[..., 2:8])) == "rows not dense"
    # the reasons that come before and after the layout, with their strings
    q = torch.tensor([0.5, 1.0])
    assert spec.prepare_flat(dense, dense, q, None) == ("minus=", ())
    assert spec.prepare_flat(dense, None, q, None) == ("input on the CPU", ())
    assert spec.prepare(ny, None, q, None) == ("input on the CPU", ())
    # the R view and its length
    jo = sj.jorek_of()
    f = jo.unstack_fields(dense)[0]
    Rb = jo._R_view(f)
    assert tuple(Rb.shape) == tuple(f.shape) and Rb.stride() == (0, 1, 0, 10) and torch.equal(Rb[2, :, 3], sj.radius(12)[None].expand(10, 12))
    g = jo.unstack_fields(ny)[0]
    assert jo._R_view(g).stride() == (0, 0, 0, 1) and jo._R_view(g.transpose(2, 3).contiguous().transpose(2, 3)) is None
    with pytest.raises(RuntimeError, match="R has 12 points"):
        jo._R_view(jo.unstack_fields(torch.rand(3, 3, 5, 16, 10))[0])


@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_cpu_tensors_take_the_fallback_and_meet_the_reference(kind):
    """``jorek=True`` on CPU tensors: staged, three-pass, and the case's reference is met (on a machine with a GPU; without
    one the staging raises as everywhere else in the package)"""
    from cp_pre_amd import screen
    if not torch.cuda.is_available():
        from cp_pre_amd.screen import _Spec
        c = sj.case(kind, sj.FLAT_BASE)
        why, _ = _Spec(sj.method_of(kind), jorek=True).prepare_flat(sj.to_vars(c.x), None, c.q, c.mod)
        assert why == "input on the CPU"
        with pytest.raises(RuntimeError):
            screen.screen(sj.method_of(kind), sj.to_vars(c.x).contiguous(), c.q, c.mod, jorek=True)
        return
    c = sj.case(kind, sj.FLAT_BASE)
    s = screen.screen(sj.method_of(kind), sj.to_vars(c.x).contiguous(), c.q, c.mod, jorek=True)
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    err = (s.score.double() - c.s_ref).abs()
    assert bool((err <= c.tol_s + 1.2e-7 * c.s_ref).all()) and bool(((s.inside - c.count_ref).abs() <= c.undecided).all())
    assert torch.equal(s.accept(), c.accept_ref)


# ------------------------------------------------------------------ refusals before any launch, from ctypes
def test_screenjorek_entry_points_refuse_before_any_launch():
    """The addresses are not mapped and nothing is dereferenced: a refusal that reached a launch could not return its
    code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_screenjorek()
    B, T, X, Y = 2, 6, 5, 12
    a0, r0, q0, s0, c0 = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000

    def dense(base):                     # [B,T,X,Y], Y fastest
        return _lib.PreField(base, T * X * Y, X * Y, Y, 1)

    def nt_fast(base):                   # the same logical view with memory [B,X,Y,T]
        return _lib.PreField(base, T * X * Y, 1, Y * T, T)

    def three(mk):
        return (_lib.PreField * 3)(mk(a0), mk(a0 + 0x01000000), mk(a0 + 0x02000000))

    k27 = [0.0] * 27
    k27[13] = 1.0
    K = [_lib.farr(k27) for _ in range(5)]
    coef = _lib.farr([1.0, 1.0, 2.0, 3.4])
    Ry, Rt = _lib.PreField(r0, 0, 0, 0, 1), _lib.PreField(r0, 0, 1, 0, T)
    sy = _lib.PreScreen(q0, 3, None, 0, 0, 1, 1, 1, s0, c0, B)
    st = _lib.PreScreenFlat(q0, 3, None, 0, 0, 0, 1, 1, 1, s0, c0, B)
    ny, flat = lib.pre_screenjorek_f32, lib.pre_screenjorek_flat_f32
    tail = (B, T, X, Y, 0, None)
    for fn, mk, Rb, s in ((ny, dense, Ry, sy), (flat, nt_fast, Rt, st)):
        f = three(mk)
        # a null pointer: the fields, R, a kernel, the scalars, the set descriptor, a view's ptr, the levels
        assert fn(0, None, ctypes.byref(Rb), *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(0, f, None, *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(1, f, ctypes.byref(Rb), *K[:4], None, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(1, f, ctypes.byref(Rb), *K, None, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(1, f, ctypes.byref(Rb), *K, coef, None, *tail) == _lib.PRE_E_NULL
        assert fn(1, f, ctypes.byref(_lib.PreField(None, 0, 0, 0, 1)), *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        noq = type(s).from_buffer_copy(s)
        noq.q = None
        assert fn(0, f, ctypes.byref(Rb), *K, coef, ctypes.byref(noq), *tail) == _lib.PRE_E_NULL
        # eq outside 0..1
        assert fn(2, f, ctypes.byref(Rb), *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_RANGE
        assert fn(-1, f, ctypes.byref(Rb), *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_RANGE
    # a flat call whose R view has sT != 1; fields of the other layout
    assert flat(0, three(nt_fast), ctypes.byref(Ry), *K, coef, ctypes.byref(st), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(1, three(nt_fast), ctypes.byref(_lib.PreField(r0, 0, 2, 0, T)), *K, coef, ctypes.byref(st), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(1, three(dense), ctypes.byref(Rt), *K, coef, ctypes.byref(st), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(0, three(nt_fast), ctypes.byref(Rt), *K, coef, ctypes.byref(st), B, T, X, Y, _lib.PRE_FLAG_HALO_X, None) == _lib.PRE_E_UNSUPPORTED
    # an Ny-fastest call with Y % 4 != 0; an R view without unit stride on Y; fields of the other layout
    assert ny(0, three(dense), ctypes.byref(Ry), *K, coef, ctypes.byref(sy), B, T, X, 10, 0, None) == _lib.PRE_E_UNSUPPORTED
    assert ny(1, three(dense), ctypes.byref(Rt), *K, coef, ctypes.byref(sy), *tail) == _lib.PRE_E_UNSUPPORTED
    assert ny(0, three(nt_fast), ctypes.byref(Ry), *K, coef, ctypes.byref(sy), *tail) == _lib.PRE_E_UNSUPPORTED
    # operator weight off the 7-point star, after every layout check passed
    box = list(k27)
    box[0] = 0.5
    assert ny(0, three(dense), ctypes.byref(Ry), K[0], _lib.farr(box), *K[2:], coef, ctypes.byref(sy), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(1, three(nt_fast), ctypes.byref(Rt), *K[:4], _lib.farr(box), coef, ctypes.byref(st), *tail) == _lib.PRE_E_UNSUPPORTED


# ------------------------------------------------------------------ the caps of the GPU tests, from the oracle alone
@pytest.mark.parametrize("kind", sj.KINDS)
def test_screenjorek_reference_values_meet_the_caps(kind):
    """Every case tests/test_gpu_screenjorek.py runs: at most 1 % of the counted cells undecided for every (level, sample),
    every level further than tau / m_min from every per-sample score, a level that accepts some samples and rejects
    others, m_min > 0 - at the first seed in 0..5 that gives all of it."""
    worst, seeds, n = (0.0, float("inf")), {}, 0
    for key in sj.gpu_cases():
        if key[0] != kind:
            continue
        c = sj.case(*key)
        share, dist, split = c.caps()
        assert c.m_min > 0 and c.q.dtype == torch.float32 and c.q.shape == (key[4],)
        assert share <= 0.01 and dist > 1.0 and split, (key, share, dist, split)
        assert tuple(c.x.shape) == (key[1][0], 3) + tuple(key[1][1:]) and float(c.x.min()) > 0
        worst, n = (max(worst[0], share), min(worst[1], dist)), n + 1
        if c.seed:
            seeds[key[1:]] = c.seed
    assert n == 61
    print(f"{kind}: {n} cases, largest undecided share {worst[0]:.4f}, closest level {worst[1]:.1f} x tau/m_min from a score; "
          f"seeds other than 0: {seeds}")
