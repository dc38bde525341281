"""CPU tests of the opt-in paired screen of the 1-D family (cp_pre_amd.screen with ``minus=`` and ``pair="rows"``,
libcp_pre_screen1dpair.so):
  * the exported ABI against include/cp_pre_screen1dpair.h and the ctypes binding, a C99 client compiled against the header;
  * the Makefile and loader facts: one statement of the row march, the Burgers entry in an object without contraction;
  * the host reasons for the three-pass route, in order, on stub layouts; ``pair=True`` unchanged; ``pair="rows"`` without
    ``minus`` inert;
  * the entry points refusing, from ctypes with unmapped addresses, before any launch;
  * the caps the GPU tests' tolerances rest on, from the oracle alone, for every case tests/test_gpu_screen1dpair.py uses.
The device passes are covered by tests/test_gpu_screen1dpair.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import screen1d_helpers as s1
import screen1dpair_helpers as p1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screen1dpair.h")
DECLARED = {"pre_screen1dpair_abi_version", "pre_screen1dpair_stencil2d_f32", "pre_screen1dpair_burgers_f32"}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screen1dpair_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screen1dpair.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_screen1dpair_library_exports_exactly_its_three_symbols():
    from cp_pre_amd import _lib
    so = _lib.SCREEN1DPAIR_SO_PATH
    assert os.path.exists(so), "libcp_pre_screen1dpair.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.SCREEN1DPAIR_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREEN1DPAIR_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREEN1DPAIR_ABI_VERSION == 1
    assert _lib._load("screen1dpair").pre_screen1dpair_abi_version() == _lib.PRE_SCREEN1DPAIR_ABI_VERSION
    assert _lib.load_screen1dpair() is _lib._load("screen1dpair")
    # every declaration cites the reference lines it serves; the header says what the test is and is not
    for decl in re.split(r"\n(?=/\* )", header.split("pre_screen1dpair_abi_version(void);", 1)[1]):
        if "int pre_screen1dpair_" in decl:
            assert re.search(r"Joint/\w+_Residuals_CP\.py:\d+", decl), decl[:80]
    assert "NOT the reference's two-sided form" in header
    # the single-set library keeps its export list
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SCREEN1D_SO_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)} == set(_lib.SCREEN1D_SIGNATURES)


def test_screen1dpair_ctypes_signatures_have_the_header_arity_and_the_twins_tails():
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^int\s+(pre_screen1dpair_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    assert {n for n, _ in found} == DECLARED
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREEN1DPAIR_SIGNATURES[name]), name
    # the twin's arguments after its field (pointer, strides), unchanged; two (pointer, strides) pairs in front
    for kind in ("stencil2d", "burgers"):
        sig, tw = _lib.SCREEN1DPAIR_SIGNATURES["pre_screen1dpair_%s_f32" % kind], _lib.SCREEN1D_SIGNATURES["pre_screen1d_%s_f32" % kind]
        assert sig[4:] == tw[2:] and sig[:2] == sig[2:4] == tw[:2], kind
        assert sig[-6] is ctypes.POINTER(_lib.PreScreen)


def test_screen1dpair_wrong_abi_version_and_missing_library_raise_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screen1dpair", None)
    monkeypatch.setattr(_lib, "PRE_SCREEN1DPAIR_ABI_VERSION", _lib.PRE_SCREEN1DPAIR_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_screen1dpair.so has ABI version 1"):
        _lib._load("screen1dpair")
    monkeypatch.setattr(_lib, "SCREEN1DPAIR_SO_PATH", str(tmp_path / "libcp_pre_screen1dpair.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_screen1dpair()


def test_screen1dpair_header_compiles_as_c99_and_the_c_client_compiles_and_links(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "screen1dpair_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()
    exe = tmp_path / "screen1dpair_check"
    subprocess.check_call(c_client_command(exe))
    assert exe.exists()
    # the client's slabs cut the plane's ROWS in both layouts (the contiguous axis would have to keep a multiple of 4)
    src = open(os.path.join(ROOT, "tests", "c_abi", "screen1dpair_check.c")).read()
    assert "a + 6 * sa[1]" in src and "a + 14 * sa[2]" in src


def test_screen1dpair_makefile_and_loader_facts():
    from cp_pre_amd import _lib
    assert len(_lib._LIBS) == 8 and "screen1dpair" not in _lib._LIBS and "screen1dpair" in _lib._LIBS_MORE
    csrc = os.path.join(ROOT, "cp_pre_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^LIBS\s+:=.*\bscreen1dpair\b", mk, flags=re.M)
    assert re.search(r"^screen1dpair_OBJS\s+:= screen_rows_pair\.o screen_rows_pair_nc\.o", mk, flags=re.M)
    assert re.search(r"^screen1d_OBJS\s+:= screen_rows\.o\s", mk, flags=re.M)
    assert re.search(r"^SHARED_HDRS\s+:=.*\bscreen_rows\.h\b", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS\s+:=(.|\\\n)*\$\(screen1dpair_OBJS\)", mk, flags=re.M)
    assert "$(screen1dpair_OBJS): $(INC)/cp_pre_screen1dpair.h $(INC)/cp_pre_screen.h" in mk
    # the Burgers entry is built as pair_march_nc.o is: a part macro and no contraction; the tap-list entry keeps star_march.o's flags
    assert re.search(r"^screen_rows_pair_nc\.o: FLAGS \+= -DPRE_SCREEN1DPAIR_PART=2 -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^screen_rows_pair\.o: FLAGS \+= -DPRE_SCREEN1DPAIR_PART=1$", mk, flags=re.M)
    assert not re.search(r"^screen_rows\.o:.*FLAGS", mk, flags=re.M)
    # the march is stated once, in the shared header; both units include it and neither restates a kernel
    src = {f: open(os.path.join(csrc, f)).read() for f in ("screen_rows.h", "screen_rows.hip", "screen_rows_pair.hip")}
    assert src["screen_rows.h"].count("__global__") == 1 and "screen_rows_kernel" in src["screen_rows.h"]
    assert "RSplit rows_split(" in src["screen_rows.h"] and "int prepare_rows(" in src["screen_rows.h"]
    for f in ("screen_rows.hip", "screen_rows_pair.hip"):
        assert '#include "screen_rows.h"' in src[f] and "__global__" not in src[f] and "rows_split(" not in src[f], f
    assert '#include "paired_functor.h"' in src["screen_rows_pair.hip"] and "struct Paired" not in src["screen_rows_pair.hip"]
    part2 = src["screen_rows_pair.hip"].split("#if PRE_SCREEN1DPAIR_PART == 2", 1)[1]
    assert "pre_screen1dpair_burgers_f32" in part2 and "pre_screen1dpair_stencil2d_f32" not in part2
    assert "one-sided test" in src["screen_rows_pair.hip"]
    # the split rule the helpers restate is the header's
    assert "while (B * s.nCT * ((R + rc - 1) / rc) < slots && rc > ROWS_MINSEG * nseg) rc = (rc + 1) / 2;" in src["screen_rows.h"]
    assert s1.split(8192, 200, 512, 2048) == dict(ws=2, nseg=2, nCT=1, rc=200, nChunk=1, rSeg=100)


# ------------------------------------------------------------------ the host routing, on stub layouts
class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the layout reasons come after the device check."""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def _nt(t):
    """the logical [B,Nt,Nx] tensor with unit stride on Nt"""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def test_screen1dpair_pair_true_is_unchanged_and_rows_without_minus_is_inert():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _Spec, _pair_mode
    q = torch.ones(2)
    for method in (R.Burgers(0.01, 0.01, 0.01).residual, R.Advection(1.0, 0.01, 0.01).residual, s1.method_of("dxx")):
        rows, u = _Spec(method), torch.rand(3, 8, 16)
        assert rows.pair_declined() == "no paired screen for the 1-D family" and rows.pair_declined(rows=True) is None
        assert rows.prepare(u, u, q, None, pair=True) == ("no paired screen for the 1-D family", ())
        assert rows.prepare_rows(_dev(u), _dev(u), q, None, pair=True) == ("no paired screen for the 1-D family", ())
        assert rows.prepare_rows(_dev(u), _dev(u), q, None, pair=1) == ("no paired screen for the 1-D family", ())
        assert rows.prepare_rows(_dev(u), _dev(u), q, None, pair="yes") == ("no paired screen for the 1-D family", ())
        assert rows.prepare_rows(_dev(u), _dev(u), q, None) == ("minus=", ())
        assert rows.prepare_rows(_dev(u), _dev(u), q, None, pair="") == ("minus=", ())
        # pair="rows" without minus: the single-set screen's answer
        assert rows.prepare_rows(u, None, q, None, pair="rows") == rows.prepare_rows(u, None, q, None) == ("input on the CPU", ())
        why, ks = rows.prepare_rows(_dev(u), None, q, None, pair="rows")
        assert why is None and len(ks) == len(rows.prepare_rows(_dev(u), None, q, None)[1])
    assert _pair_mode("rows", None) is False and _pair_mode("rows", q) == "rows" and _pair_mode(True, q) is True
    assert _pair_mode("flat", q) is True and _pair_mode(0, q) is False and _pair_mode(None, q) is False


def test_screen1dpair_rows_does_everything_pair_true_does_for_the_2d_kinds():
    import screen_helpers as sh
    from cp_pre_amd.screen import _Spec
    q = torch.ones(2)
    x = torch.rand(3, 3, 10, 5, 12)
    ns = _Spec(sh.method_of("ns_momentum"))
    for pair in (True, "rows"):
        why, ks = ns.prepare(_dev(x), _dev(x), q, None, pair=pair)
        assert why is None and len(ks) == 4
    assert ns.prepare(_dev(x[..., :8]), _dev(x[..., ::2][..., :8]), q, None, pair="rows") == ("minus: no unit stride on the last axis", ())
    assert _Spec(sh.method_of("mhd_energy")).prepare(_dev(x), _dev(x), q, None, pair="rows") == ("no paired screen for mhd_energy", ())


def test_screen1dpair_host_reasons_in_order():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_1d import ConvOperator as C1
    from cp_pre_amd.screen import _Spec
    q, q64 = torch.ones(2), torch.ones(2, dtype=torch.float64)
    x, y = torch.rand(3, 8, 16), torch.rand(3, 8, 16)
    bg = _Spec(R.Burgers(s1.DX, s1.DT, s1.NU).residual)
    kw = dict(pair="rows")
    assert bg.entry("rows", True) == "pre_screen1dpair_burgers_f32" and bg.route("rows", True) == "fused:rows_pair_burgers"
    assert bg.entry("rows") == "pre_screen1d_burgers_f32" and bg.route("rows") == "fused:rows_burgers"
    for kind in p1.KINDS:
        sp = _Spec(s1.method_of(kind))
        assert sp.route("rows", True) == p1.ROUTE[kind]
        assert sp.entry("rows", True) == "pre_screen1dpair_" + ("burgers" if kind == "burgers" else "stencil2d") + "_f32"
    # the input: either set on the CPU, float64 levels or modulation
    assert bg.prepare_rows(x, y, q, None, **kw) == ("input on the CPU", ())
    assert bg.prepare_rows(_dev(x), y, q, None, **kw) == ("input on the CPU", ())
    assert bg.prepare_rows(x, _dev(y), q, None, **kw) == ("input on the CPU", ())
    assert bg.prepare_rows(_dev(x), _dev(y), q64, None, **kw) == ("float64 levels or modulation", ())
    assert bg.prepare_rows(_dev(x), _dev(y), q, torch.ones(8, 16, dtype=torch.float64), **kw) == ("float64 levels or modulation", ())
    # the layout of vars, as on the single-set rows route
    assert bg.prepare_rows(_dev(x[:, None]), _dev(y[:, None]), q, None, **kw) == ("[BS,1,Nt,Nx] input", ())
    wide = torch.rand(3, 16, 32)
    assert bg.prepare_rows(_dev(wide[:, ::2, ::2]), _dev(y), q, None, **kw) == ("no unit-stride axis", ())
    odd = torch.rand(3, 8, 14)
    assert bg.prepare_rows(_dev(odd), _dev(odd), q, None, **kw) == ("contiguous-axis length not a multiple of 4", ())
    oddt = _nt(torch.rand(3, 14, 8))
    assert bg.prepare_rows(_dev(oddt), _dev(oddt), q, None, **kw) == ("contiguous-axis length not a multiple of 4", ())
    # the second set: the other layout, then its own reasons
    assert bg.prepare_rows(_dev(x), _dev(_nt(y)), q, None, **kw) == ("field sets in different layouts", ())
    assert bg.prepare_rows(_dev(_nt(x)), _dev(y), q, None, **kw) == ("field sets in different layouts", ())
    assert bg.prepare_rows(_dev(x), _dev(wide[:, ::2, ::2]), q, None, **kw) == ("minus: no unit-stride axis", ())
    assert bg.prepare_rows(_dev(_nt(x)), _dev(wide[:, ::2, ::2]), q, None, **kw) == ("minus: no unit-stride axis", ())
    # a spectral operator has no rows kind: the reason it gives today
    spec = _Spec(C1("x", 2, conv="spectral"))
    assert spec.rows_kind is None and spec.prepare(_dev(x), _dev(y), q, None, **kw) == ("spectral operator", ())
    # what declines whatever the layout, then the kernels
    assert _Spec(R.Burgers(s1.DX, s1.DT, s1.NU, fused=False).residual).prepare_rows(_dev(x), _dev(y), q, None, **kw) == ("fused=False", ())
    live = R.Burgers(s1.DX, s1.DT, s1.NU)
    live.D_x.kernel.requires_grad_(True)
    assert _Spec(live.residual).prepare_rows(_dev(x), _dev(y), q, None, **kw) == ("operator kernel requires grad", ())
    box = R.Burgers(s1.DX, s1.DT, s1.NU)
    box.D_t.kernel.data[2, 2] = 0.5
    assert _Spec(box.residual).prepare_rows(_dev(x), _dev(y), q, None, **kw) == ("operator kernel off the 5-point star", ())
    op = C1("x", 2)
    op.kernel.data[0, 0] = 0.5
    assert _Spec(op).prepare_rows(_dev(x), _dev(y), q, None, **kw) == ("operator kernel off the 5-point star", ())
    # all of it passes, in both layouts and with pitched sets: the kernels come back
    for a, b in ((x, y), (_nt(x), _nt(y)), (wide[:, :8, :16], y), (_nt(x), _nt(torch.rand(3, 8, 20))[:, :, :16])):
        why, ks = bg.prepare_rows(_dev(a), _dev(b), q, None, **kw)
        assert why is None and len(ks) == 3, (a.stride(), b.stride(), why)


def test_screen1dpair_validation_and_halo_x_raise_before_any_device_work():
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    m = R.Burgers(s1.DX, s1.DT, s1.NU).residual
    x, q = torch.rand(3, 8, 16), torch.ones(2)
    with pytest.raises(ValueError, match="minus has shape"):
        screen.screen(m, x, q, minus=x[:2], pair="rows")
    with pytest.raises(TypeError, match="minus has dtype"):
        screen.screen(m, x, q, minus=x.double(), pair="rows")
    s = screen.Screen(3, 2, "cpu")
    with pytest.raises(ValueError, match="halo_x"):
        s.add_slab(m, x, q, None, crop=(1, 1), halo_x=True, minus=x, pair="rows")     # (a host tensor has no halo rows)
    with pytest.raises(RuntimeError, match="halo_x"):
        s.add_slab(m, _dev(x), q, None, crop=(1, 1), halo_x=True, minus=_dev(x), pair="rows")
    assert s.acc is None and s.cells == 0


@pytest.mark.parametrize("kind", ["burgers", "advection"])
def test_screen1dpair_cpu_tensors_take_the_fallback_and_meet_the_reference(kind):
    """``pair="rows"`` on CPU tensors: staged, three-pass, and the case's reference is met (on a machine with a GPU; without
    one the staging raises as everywhere else in the package)"""
    from cp_pre_amd import screen
    c = p1.case(kind, *p1.BASE, "nx")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            screen.screen(s1.method_of(kind), c.x, c.q, c.mod, minus=c.y, pair="rows")
        return
    s = screen.screen(s1.method_of(kind), c.x, c.q, c.mod, minus=c.y, pair="rows")
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    err = (s.score.double() - c.s_ref).abs()
    assert bool((err <= c.tol_s + 1.2e-7 * c.s_ref).all()) and bool(((s.inside - c.count_ref).abs() <= c.undecided).all())
    assert torch.equal(s.accept(), c.accept_ref)


# ------------------------------------------------------------------ refusals before any launch, from ctypes
def test_screen1dpair_entry_points_refuse_before_any_launch():
    """The addresses are not mapped and nothing is dereferenced on the host but the stride arrays and the set descriptor: a
    refusal that reached a launch could not return its code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_screen1dpair()
    B, T, X = 2, 8, 16
    a0, b0, q0, s0, c0, m0 = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000
    nx, nt, none = _lib.iarr64([T * X, X, 1]), _lib.iarr64([T * X, 1, T]), _lib.iarr64([4 * T * X, 2 * X, 2])
    pitched = _lib.iarr64([T * (X + 4) + 8, X + 4, 1])
    sc = _lib.PreScreen(q0, 3, None, 0, 0, 1, 1, 0, s0, c0, B)
    ref = ctypes.byref(sc)
    tw, on, corner, far = _lib.farr([1.0, 2.0]), _lib.iarr32([0, 0, 0, 1]), _lib.iarr32([0, 0, 1, 1]), _lib.iarr32([0, 0, 0, 4])
    k9 = [0.0] * 9
    k9[4] = 1.0
    K = [_lib.farr(k9) for _ in range(3)]
    box = list(k9)
    box[0] = 0.5
    scal = (0.01, 0.02, 0.001, 1.0)
    tail = (B, T, X, 0, None)
    st, bg = lib.pre_screen1dpair_stencil2d_f32, lib.pre_screen1dpair_burgers_f32
    P = ctypes.c_void_p
    assert st(None, nx, P(b0), nx, tw, on, 2, ref, *tail) == _lib.PRE_E_NULL and st(P(a0), nx, None, nx, tw, on, 2, ref, *tail) == _lib.PRE_E_NULL
    assert st(P(a0), None, P(b0), nx, tw, on, 2, ref, *tail) == _lib.PRE_E_NULL and st(P(a0), nx, P(b0), None, tw, on, 2, ref, *tail) == _lib.PRE_E_NULL
    assert st(P(a0), nx, P(b0), nx, None, on, 2, ref, *tail) == _lib.PRE_E_NULL and st(P(a0), nx, P(b0), nx, tw, on, 2, None, *tail) == _lib.PRE_E_NULL
    assert bg(P(a0), nx, None, nx, *K, *scal, ref, *tail) == _lib.PRE_E_NULL and bg(P(a0), nx, P(b0), nx, K[0], None, K[2], *scal, ref, *tail) == _lib.PRE_E_NULL
    assert st(P(a0), nx, P(b0), nx, tw, on, 2, ref, B, 0, X, 0, None) == _lib.PRE_E_NULL
    many = _lib.PreScreen.from_buffer_copy(sc)
    many.nk = 17
    assert st(P(a0), nx, P(b0), nx, tw, on, 2, ctypes.byref(many), *tail) == _lib.PRE_E_RANGE
    cy = _lib.PreScreen.from_buffer_copy(sc)
    cy.cy = 1
    assert bg(P(a0), nx, P(b0), nx, *K, *scal, ctypes.byref(cy), *tail) == _lib.PRE_E_RANGE
    assert st(P(a0), nx, P(b0), nx, tw, on, 50, ref, *tail) == _lib.PRE_E_SHAPE
    assert st(P(a0), nx, P(b0), nx, tw, far, 2, ref, *tail) == _lib.PRE_E_SHAPE
    assert bg(P(a0), nx, P(b0), nx, *K, *scal, ref, B, 1 << 17, 1 << 16, 0, None) == _lib.PRE_E_SHAPE          # (T * X = 2^33)
    # PRE_E_UNSUPPORTED: sets with different unit-stride axes (either way round), none, the modulation's axis, C % 4, the
    # star, flags
    for fn, mid in ((st, (tw, on, 2)), (bg, (*K, *scal))):
        assert fn(P(a0), nx, P(b0), nt, *mid, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert fn(P(a0), nt, P(b0), nx, *mid, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert fn(P(a0), nx, P(b0), none, *mid, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert fn(P(a0), none, P(b0), nx, *mid, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert fn(P(a0), nx, P(b0), pitched, *mid, ref, B, T, X - 2, 0, None) == _lib.PRE_E_UNSUPPORTED
        assert fn(P(a0), nt, P(b0), nt, *mid, ref, B, T - 2, X, 0, None) == _lib.PRE_E_UNSUPPORTED
        assert fn(P(a0), nx, P(b0), pitched, *mid, ref, B, T, X, _lib.PRE_FLAG_ABS, None) == _lib.PRE_E_UNSUPPORTED
        assert fn(P(a0), nx, P(b0), pitched, *mid, ref, B, T, X, _lib.PRE_FLAG_HALO_X, None) == _lib.PRE_E_UNSUPPORTED
        modt = _lib.PreScreen(q0, 3, m0, 1, T, 1, 1, 0, s0, c0, B)                 # modulation Nt-fastest, sets Nx-fastest
        assert fn(P(a0), nx, P(b0), nx, *mid, ctypes.byref(modt), *tail) == _lib.PRE_E_UNSUPPORTED
    assert st(P(a0), nx, P(b0), pitched, tw, corner, 2, ref, *tail) == _lib.PRE_E_UNSUPPORTED
    assert bg(P(a0), nx, P(b0), pitched, K[0], _lib.farr(box), K[2], *scal, ref, *tail) == _lib.PRE_E_UNSUPPORTED


# ------------------------------------------------------------------ the caps of the GPU tests, from the oracle alone
@pytest.mark.parametrize("kind", p1.KINDS)
def test_screen1dpair_reference_values_meet_the_caps(kind):
    """Every case tests/test_gpu_screen1dpair.py compares with the reference: at most max(1 cell, 1 %) of the counted cells
    undecided for every (level, sample), every level further than 2 tau / m_min from every per-sample score, a level that
    accepts some samples and rejects others, m_min > 0 - at the seed ``screen1dpair_helpers.SEEDS`` names (default 0)."""
    worst, n = (0.0, float("inf")), 0
    for key in p1.gpu_cases():
        if key[0] != kind:
            continue
        c = p1.case(*key)
        ok, (und, cells, dist, split) = c.caps_hold()
        assert c.q.dtype == torch.float32 and c.q.shape == (key[6],) and tuple(c.x.shape) == tuple(c.y.shape)
        assert c.seed == p1.SEEDS.get(p1.key_of(*key), 0)
        assert ok, (key, c.seed, und, cells, dist, split)
        if cells >= 100:
            worst = (max(worst[0], und / cells), worst[1])
        worst, n = (worst[0], min(worst[1], dist)), n + 1
    assert n >= 24 and worst[0] <= 0.01
    print(f"{kind}: {n} cases, largest undecided share {worst[0]:.4f} (regions of 100 cells and more), closest level "
          f"{worst[1]:.1f} x tau/m_min from a score")
    used = {p1.key_of(*k) for k in p1.gpu_cases()}
    assert all(k in used for k in p1.SEEDS), "a seed for a case that no test uses"


def test_screen1dpair_gpu_cases_cover_what_the_issue_names():
    cases = p1.gpu_cases()
    base = {(k, lay, b, m, nk) for k, B, pl, lay, b, m, nk in cases if (B, pl) == p1.BASE}
    assert base >= {(k, lay, b, m, nk) for k in p1.KINDS for lay in p1.LAYOUTS for b in (False, True) for m in (False, True) for nk in (1, 10, 16)}
    for kind in p1.SEAM_KINDS:
        for lay in p1.LAYOUTS:
            assert {(B, pl) for k, B, pl, l2, *_ in cases if k == kind and l2 == lay} >= set(s1.SEAM_PLANES.values()) | set(s1.ODD_PLANES)
