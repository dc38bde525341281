"""CPU tests of the opt-in per-cell screen of the JOREK residuals (``cp_pre_amd.screen.screen_cells`` / ``ScreenCells`` with
``jorek=True``, libcp_pre_screenjorekcells.so) and of ``norms=True`` through ``functools.partial`` on both JOREK screens:
  * the exported ABI against include/cp_pre_screenjorekcells.h and the ctypes binding, a C99 client compiled against the header,
    the translation unit and its Makefile lines;
  * what ``_Spec`` resolves from the partial, the entry and route names, the host reasons for the three-pass route;
  * both entry points refusing, from ctypes with unmapped addresses, before any launch;
  * every error of the host side raised before device work, cropped against padded level fields;
  * the caps the GPU tests' tolerances rest on, from the oracle alone, for every case tests/test_gpu_screenjorekcells.py uses.
The device passes are covered by tests/test_gpu_screenjorekcells.py; tests/SCREENJOREKCELLS_TESTS.md says which test reaches
which branch."""
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

import screen_helpers as sh
import screenjorek_helpers as sj
import screenjorekcells_helpers as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screenjorekcells.h")
DECLARED = {"pre_screenjorekcells_abi_version", "pre_screenjorekcells_sample_group", "pre_screenjorekcells_f32",
            "pre_screenjorekcells_flat_f32"}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screenjorekcells_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screenjorekcells.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_screenjorekcells_library_exports_exactly_its_four_symbols():
    from cp_pre_amd import _lib
    so = _lib.SCREENJOREKCELLS_SO_PATH
    assert os.path.exists(so), "libcp_pre_screenjorekcells.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.SCREENJOREKCELLS_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREENJOREKCELLS_ABI_VERSION\s+(\d+)", header).group(1)) == \
        _lib.PRE_SCREENJOREKCELLS_ABI_VERSION == 1
    lib = _lib._load("screenjorekcells")
    assert lib.pre_screenjorekcells_abi_version() == _lib.PRE_SCREENJOREKCELLS_ABI_VERSION
    assert _lib.load_screenjorekcells() is lib and lib.pre_screenjorekcells_sample_group() >= 1
    assert "screenjorekcells" in _lib._LIBS_MORE and "screenjorekcells" not in _lib._LIBS
    # both entries cite the reference lines they serve
    for decl in re.split(r"\n(?=/\* )", header.split("pre_screenjorekcells_sample_group(void);", 1)[1]):
        if "int pre_screenjorekcells_" in decl:
            assert "Marginal/JOREK_residuals_CP.py:210-243" in decl and "297-311" in decl, decl[:80]


def test_screenjorekcells_ctypes_signatures_follow_the_header_prototypes():
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^int\s+(pre_screenjorekcells_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    assert {n for n, _ in found} == DECLARED
    table = (("pre_screencellsflat_t", ctypes.POINTER(_lib.PreScreenCellsFlat)), ("pre_screencells_t", ctypes.POINTER(_lib.PreScreenCells)),
             ("pre_field_t", ctypes.POINTER(_lib.PreField)), ("float", ctypes.POINTER(ctypes.c_float)), ("void *", ctypes.c_void_p),
             ("int64_t", ctypes.c_int64), ("int ", ctypes.c_int))
    for name, args in found:
        want = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            a = " ".join(a.split())
            assert ("*" in a or "[" in a) == any(w in a for w in ("_t *", "_t f", "float", "void")), a     # pointers are pointers
            want.append(next(t for word, t in table if word in a))
        assert want == _lib.SCREENJOREKCELLS_SIGNATURES[name], name
    # the joint twin's arguments with the set descriptor swapped
    for name, twin, desc in (("pre_screenjorekcells_f32", "pre_screenjorek_f32", _lib.PreScreenCells),
                             ("pre_screenjorekcells_flat_f32", "pre_screenjorek_flat_f32", _lib.PreScreenCellsFlat)):
        sig, tw = _lib.SCREENJOREKCELLS_SIGNATURES[name], _lib.SCREENJOREK_SIGNATURES[twin]
        assert len(sig) == len(tw) and sig[9] is ctypes.POINTER(desc) and sig[:9] == tw[:9] and sig[10:] == tw[10:]


def test_screenjorekcells_wrong_abi_version_and_missing_library_raise_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screenjorekcells", None)
    monkeypatch.setattr(_lib, "PRE_SCREENJOREKCELLS_ABI_VERSION", _lib.PRE_SCREENJOREKCELLS_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_screenjorekcells.so has ABI version 1"):
        _lib._load("screenjorekcells")
    monkeypatch.setattr(_lib, "SCREENJOREKCELLS_SO_PATH", str(tmp_path / "libcp_pre_screenjorekcells.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_screenjorekcells()


def test_screenjorekcells_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "screenjorekcells_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_screenjorekcells_translation_unit_and_makefile_lines():
    """no kernel of its own; the view assembly stated once; the Makefile's line, dependencies and variants"""
    csrc = os.path.join(ROOT, "cp_pre_amd", "csrc")
    unit = open(os.path.join(csrc, "screen_jorek_cells.hip")).read()
    joint = open(os.path.join(csrc, "screen_jorek.hip")).read()
    entries = open(os.path.join(csrc, "screen_entries.h")).read()
    assert "__global__" not in unit and "asm" not in unit
    for inc in ("screen_march.h", "screen_flat.h", "../../include/cp_pre_screenjorekcells.h", "screen_entries.h"):
        assert '#include "%s"' % inc in unit
    assert unit.count("jorek<NyForm, Single, CellSets>") == 1 and unit.count("jorek<FlatForm, Single, CellSets>") == 1
    assert entries.count("Views jorek_views(") == 1 and "Views jorek_views(" not in unit + joint
    assert "jorek_views(eq, fields, Rb)" in unit and "jorek_views(eq, fields, Rb)" in joint
    for fn in ("JorekContinuity", "JorekTemperature"):
        assert "struct CellsBatch<%s<M>, void> { static constexpr int value = PRE_SCREENJOREKCELLS_BATCH; };" % fn in unit
    assert "CellsLate<" not in unit                                        # (the later batches have the first one's size)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^screenjorekcells_OBJS\s+:= screen_jorek_cells\.o", mk, flags=re.M)
    assert re.search(r"^LIBS\s+:=.*\bscreenjorekcells\b", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS\s+:=(.|\\\n)*\$\(screenjorekcells_OBJS\)", mk, flags=re.M)
    assert "$(screenjorekcells_OBJS): $(INC)/cp_pre_screenjorekcells.h $(INC)/cp_pre_screencells.h" in mk
    assert "each of its seven objects" in mk
    for var, macro in (("SCREENJOREKCELLS_GROUP", "PRE_SCREENCELLS_GROUP"), ("SCREENJOREKCELLS_BATCH", "PRE_SCREENJOREKCELLS_BATCH")):
        assert "ifdef %s\nscreen_jorek_cells.o: FLAGS += -D%s=$(%s)\nendif" % (var, macro, var) in mk
    # the flags are star_march.o's: no per-object flag but the measurement variants
    assert not re.search(r"^screen_jorek_cells\.o: FLAGS \+= (?!-DPRE_SCREEN)", mk, flags=re.M)


# ------------------------------------------------------------------ what the keyword and the partial resolve, on the host
def test_screenjorekcells_spec_entries_and_routes():
    from cp_pre_amd.screen import _Spec
    jo = sj.jorek_of()
    for eq, name in enumerate(jc.EQS):
        spec = _Spec(getattr(jo, "residual_" + name), jorek=True)
        assert spec.entry("", cells=True) == "pre_screenjorekcells_f32"
        assert spec.entry("flat", cells=True) == "pre_screenjorekcells_flat_f32"
        assert spec.route("", cells=True) == "fused:cells_jorek_" + name == jc.route("jorek_" + name, "ny")
        assert spec.route("flat", cells=True) == "fused:flat_cells_jorek_" + name == jc.route("jorek_" + name, "flat")
        # the joint screen's names are what they were
        assert spec.entry("") == "pre_screenjorek_f32" and spec.route("flat") == "fused:flat_jorek_" + name
        assert spec.norms is False and spec.pair_declined() == "no paired screen for jorek_" + name
        # without the keyword: no fused kind, as before
        plain = _Spec(getattr(jo, "residual_" + name))
        assert plain.kind is None and plain.why == "no fused screen for JOREK"
        assert plain.prepare(sj.to_vars(torch.rand(3, 3, 10, 5, 12)), None, torch.ones(2, 10, 5, 12), None) == \
            ("no fused screen for JOREK", ())


def test_screenjorekcells_spec_takes_norms_from_a_partial():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _Spec
    jo = sj.jorek_of(coef=jc.NORMS)
    bound = jo.residual_continuity
    for norms in (True, False):
        part = functools.partial(bound, norms=norms)
        spec = _Spec(part, jorek=True)
        assert spec.kind == "jorek_continuity" and spec.eq == 0 and spec.norms is norms and spec.method is part
        assert spec.obj is jo and len(spec.ops) == 5 and spec.route("flat", cells=True) == "fused:flat_cells_jorek_continuity"
        coef, = spec.scalars()
        assert list(coef) == [ctypes.c_float(v).value for v in jo._coef(0, norms)]
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    dx, dy, dt = (t(jc.NORMS[k]) for k in ("dx", "dy", "dt"))
    assert jo._coef(0, True) == [float(2 * dx * dy), float(dt), float((2 * dt * dy) * 2), float((4 * dt) * t(3.4))]
    assert jo._coef(0, True) != jo._coef(0, False)
    # a partial without keywords is the bound method; the bound method evaluates norms=False
    assert _Spec(functools.partial(bound), jorek=True).norms is False and _Spec(bound, jorek=True).norms is False
    # norms=True without the grid steps: the method's ValueError; on temperature: the reference's exception
    with pytest.raises(ValueError, match="norms=True needs dx, dy, dt"):
        _Spec(functools.partial(sj.jorek_of().residual_continuity, norms=True), jorek=True)
    with pytest.raises(Exception, match="Norm not implemented yet"):
        _Spec(functools.partial(jo.residual_temperature, norms=True), jorek=True)
    assert _Spec(functools.partial(jo.residual_temperature, norms=False), jorek=True).eq == 1
    # foreign keywords, positional arguments, a partial of another class's method, and any partial without the keyword
    x = sj.to_vars(torch.rand(3, 3, 10, 5, 12))
    for bad in (functools.partial(bound, boundary=True), functools.partial(bound, norms=True, absolute=True),
                functools.partial(bound, x), functools.partial(R.MHD().residual_continuity, norms=True)):
        with pytest.raises(TypeError):
            _Spec(bad, jorek=True)
    with pytest.raises(TypeError):
        _Spec(functools.partial(bound, norms=True))
    with pytest.raises(TypeError, match="jorek=True"):
        _Spec(R.MHD().residual_continuity, jorek=True)


# ------------------------------------------------------------------ refusals before any launch, from ctypes
def test_screenjorekcells_entry_points_refuse_before_any_launch():
    """The addresses are not mapped and nothing is dereferenced: a refusal that reached a launch could not return its
    code here.  The order is the body's: nulls, eq, the joint descriptor's checks, the level strides, the star."""
    from cp_pre_amd import _lib
    lib = _lib.load_screenjorekcells()
    B, T, X, Y, NK = 2, 6, 5, 12, 3
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
    sy = _lib.PreScreenCells(q0, NK, T * X * Y, X * Y, Y, None, 0, 0, 1, 1, 1, s0, c0, B)
    st = _lib.PreScreenCellsFlat(q0, NK, T * X * Y, 1, Y * T, T, None, 0, 0, 0, 1, 1, 1, s0, c0, B)
    ny, flat = lib.pre_screenjorekcells_f32, lib.pre_screenjorekcells_flat_f32
    tail = (B, T, X, Y, 0, None)

    def changed(s, **kw):
        c = type(s).from_buffer_copy(s)
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)
    for fn, mk, Rb, s in ((ny, dense, Ry, sy), (flat, nt_fast, Rt, st)):
        f, R_ = three(mk), ctypes.byref(Rb)
        assert fn(0, None, R_, *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(0, f, None, *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(1, f, R_, *K[:4], None, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(1, f, R_, *K, None, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(1, f, R_, *K, coef, None, *tail) == _lib.PRE_E_NULL
        assert fn(1, f, ctypes.byref(_lib.PreField(None, 0, 0, 0, 1)), *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_NULL
        assert fn(0, f, R_, *K, coef, changed(s, levels=None), *tail) == _lib.PRE_E_NULL
        assert fn(0, f, R_, *K, coef, changed(s, score=None), *tail) == _lib.PRE_E_NULL
        assert fn(0, f, R_, *K, coef, changed(s, count_ld=B - 1), *tail) == _lib.PRE_E_NULL
        assert fn(0, f, R_, *K, coef, ctypes.byref(s), 0, T, X, Y, 0, None) == _lib.PRE_E_NULL
        # eq comes before the descriptor: a null descriptor with eq out of range is a range error
        assert fn(2, f, R_, *K, coef, None, *tail) == _lib.PRE_E_RANGE
        assert fn(-1, f, R_, *K, coef, ctypes.byref(s), *tail) == _lib.PRE_E_RANGE
        assert fn(0, f, R_, *K, coef, changed(s, nk=0), *tail) == _lib.PRE_E_RANGE
        assert fn(0, f, R_, *K, coef, changed(s, nk=17), *tail) == _lib.PRE_E_RANGE
        assert fn(0, f, R_, *K, coef, changed(s, cx=-1), *tail) == _lib.PRE_E_RANGE
        # the level strides
        assert fn(0, f, R_, *K, coef, changed(s, lK=-1), *tail) == _lib.PRE_E_SHAPE
        assert fn(1, f, R_, *K, coef, changed(s, lX=-1), *tail) == _lib.PRE_E_SHAPE
    assert flat(0, three(nt_fast), ctypes.byref(Rt), *K, coef, changed(st, lT=T, lY=1), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(0, three(nt_fast), ctypes.byref(Rt), *K, coef, changed(st, lY=T + 1), *tail) == _lib.PRE_E_UNSUPPORTED
    # layouts the forms do not take, R's view included; the flag the flat form does not take
    assert flat(0, three(nt_fast), ctypes.byref(Ry), *K, coef, ctypes.byref(st), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(1, three(dense), ctypes.byref(Rt), *K, coef, ctypes.byref(st), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(0, three(nt_fast), ctypes.byref(Rt), *K, coef, ctypes.byref(st), B, T, X, Y, _lib.PRE_FLAG_HALO_X, None) == _lib.PRE_E_UNSUPPORTED
    assert ny(0, three(dense), ctypes.byref(Ry), *K, coef, ctypes.byref(sy), B, T, X, 10, 0, None) == _lib.PRE_E_UNSUPPORTED
    assert ny(1, three(dense), ctypes.byref(Rt), *K, coef, ctypes.byref(sy), *tail) == _lib.PRE_E_UNSUPPORTED
    assert ny(0, three(nt_fast), ctypes.byref(Ry), *K, coef, ctypes.byref(sy), *tail) == _lib.PRE_E_UNSUPPORTED
    # operator weight off the 7-point star, after every layout check passed
    box = list(k27)
    box[0] = 0.5
    assert ny(0, three(dense), ctypes.byref(Ry), K[0], _lib.farr(box), *K[2:], coef, ctypes.byref(sy), *tail) == _lib.PRE_E_UNSUPPORTED
    assert flat(1, three(nt_fast), ctypes.byref(Rt), *K[:4], _lib.farr(box), coef, ctypes.byref(st), *tail) == _lib.PRE_E_UNSUPPORTED


# ------------------------------------------------------------------ the host side of screen_cells, without a device
def test_screenjorekcells_every_error_is_raised_before_device_work():
    from cp_pre_amd import screen
    c = jc.case("jorek_temperature", jc.FLAT_BASE)
    x, q, mod = sj.to_vars(c.x).contiguous(), c.q, c.mod
    method = sj.method_of(c.kind)
    kw = dict(jorek=True)
    s = screen.ScreenCells(3, c.nk, "cpu")
    for bad in (lambda: s.add_slab(method, x, q[:3], mod, **kw),                      # another nk
                lambda: s.add_slab(method, x, q[:, 1:], mod, **kw),                   # levels of other extents
                lambda: s.add_slab(method, x, c.q_cropped(), mod, **kw),              # (cropped levels: screen_cells only)
                lambda: s.add_slab(method, x, q, mod[1:], **kw),                      # a modulation of other extents
                lambda: s.add_slab(method, x[:2], q, mod, **kw),                      # another sample count
                lambda: s.add_slab(method, x[:, 0], q, mod, **kw),                    # not [BS,F,Nx,Ny,Nt]
                lambda: s.add_slab(method, x, q, mod, crop=(9, 1, 1), **kw),          # a crop that leaves nothing
                lambda: s.add_slab(method, x, q, mod, minus=x[:2], **kw),             # a second set of another shape
                lambda: s.add_slab(method, x[:, :, 1:-1], q[:, :, 1:-1], mod[:, 1:-1], crop=(1, 0, 1), halo_x=True, **kw),
                lambda: screen.screen_cells(method, x, c.q_cropped(), mod, boundary=True, **kw),
                lambda: screen.screen_cells(method, x, q[:, :-1], mod, **kw),
                lambda: screen.screen_cells(functools.partial(sj.jorek_of().residual_continuity, norms=True), x, q, mod, **kw)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: s.add_slab(method, x.double(), q, mod, **kw), lambda: s.add_slab(method, x, q.half(), mod, **kw),
                lambda: s.add_slab(sh.method_of("ns_momentum"), torch.rand(3, 3, 10, 5, 12), q, mod, **kw),
                lambda: screen.screen_cells(sh.method_of("ns_momentum"), torch.rand(3, 3, 10, 5, 12), q, mod, **kw),
                lambda: screen.screen_cells(functools.partial(method, absolute=True), x, q, mod, **kw),
                lambda: screen.screen_cells(functools.partial(sj.jorek_of(coef=jc.NORMS).residual_continuity, norms=True), x, q, mod)):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(Exception, match="Norm not implemented yet"):
        screen.screen_cells(functools.partial(method, norms=True), x, q, mod, **kw)
    assert s.acc is None and s.cells == 0


def test_screenjorekcells_cropped_levels_are_padded_once_with_nan_in_the_fields_layout():
    from cp_pre_amd.screen import _pad_levels
    c = jc.case("jorek_continuity", jc.FLAT_BASE)
    full = tuple(c.shape[1:])
    for nt_fastest in (False, True):
        p = _pad_levels(c.q_cropped(), full, nt_fastest)
        assert tuple(p.shape) == (c.nk,) + full and p.dtype == torch.float32
        assert torch.equal(p[:, 1:-1, 1:-1, 1:-1], c.q[:, 1:-1, 1:-1, 1:-1])
        rim = torch.ones(full, dtype=torch.bool)
        rim[1:-1, 1:-1, 1:-1] = False
        assert bool(torch.isnan(p[:, rim]).all()) and not bool(torch.isnan(p[:, ~rim]).any())
        if nt_fastest:                   # memory [nk,X,Y,T]: what the flat entry takes without a copy
            assert p.stride(1) == 1 and p.stride(3) == full[0] and p.stride(2) == full[0] * full[2]
        else:
            assert p.is_contiguous()


@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_cpu_tensors_take_the_fallback_and_meet_the_reference(kind):
    """``jorek=True`` on CPU tensors: staged, three-pass, and the float64 counts are met (on a machine with a GPU; without
    one the staging raises as everywhere else in the package, after the route was decided)"""
    from cp_pre_amd import screen
    from cp_pre_amd.screen import _Spec
    c = jc.case(kind, jc.FLAT_BASE)
    x = sj.to_vars(c.x).contiguous()
    why, _ = _Spec(sj.method_of(kind), jorek=True).prepare_flat(x, None, c.q, c.mod)
    assert why == "input on the CPU"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            screen.screen_cells(sj.method_of(kind), x, c.q, c.mod, jorek=True)
        assert screen.last_route() == "fallback:input on the CPU"
        # without the keyword the route is what it was
        with pytest.raises(RuntimeError):
            screen.screen_cells(sj.method_of(kind), x, c.q, c.mod)
        assert screen.last_route() == "fallback:no fused screen for JOREK"
        return
    s = screen.screen_cells(sj.method_of(kind), x, c.q, c.mod, jorek=True)
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    jc.check(c, s, "CPU inputs")
    s2 = screen.screen_cells(sj.method_of(kind), x, c.q_cropped(), c.mod, jorek=True)
    assert torch.equal(s2.inside, s.inside) and torch.equal(s2.score, s.score)
    screen.screen_cells(sj.method_of(kind), x, c.q, c.mod)
    assert screen.last_route() == "fallback:no fused screen for JOREK"


# ------------------------------------------------------------------ the caps of the GPU tests, from the oracle alone
@pytest.mark.parametrize("kind", jc.KINDS)
def test_screenjorekcells_reference_values_meet_the_caps(kind):
    """Every case tests/test_gpu_screenjorekcells.py compares with the reference: at most SHARE_CAP of the counted cells
    undecided for every (level, sample), and a level that splits a sample's cells - at the first seed in 0..5 that gives
    both."""
    from cp_pre_amd import screen
    worst, seeds, n = 0.0, {}, 0
    for key in jc.gpu_cases(screen.sample_group_jorek()):
        if key[0] != kind:
            continue
        c = jc.case(*key)
        share, split = c.caps()
        B = key[6] or key[1][0]
        assert c.q.dtype == torch.float32 and tuple(c.q.shape) == (key[4],) + tuple(key[1][1:])
        assert share <= jc.SHARE_CAP and split, (key, share, split)
        assert tuple(c.x.shape) == (B, 3) + tuple(key[1][1:]) and (B > 3 or float(c.x.min()) > 0)
        worst, n = max(worst, share), n + 1
        if c.seed:
            seeds[key[1:]] = c.seed
    assert n >= 60
    print(f"{kind}: {n} cases, largest undecided share {worst:.4f}; seeds other than 0: {seeds}")
    # norms=True (continuity): the two cases of the partial tests, per-cell and joint
    if kind == "jorek_continuity":
        for shape in (jc.FLAT_BASE, jc.NY_BASE):
            c = jc.case(kind, shape, norms=True)
            assert c.caps()[0] <= jc.SHARE_CAP and c.caps()[1]
            assert not torch.allclose(c.r_ref, jc.case(kind, shape).r_ref)
            j = jc.joint_norms_case(shape)
            assert sj.caps_hold(j)
