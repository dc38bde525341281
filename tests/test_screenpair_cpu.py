"""CPU tests of the opt-in paired screen of the data-driven scores (cp_pre_amd.screen with ``minus=`` and ``pair=True``,
libcp_pre_screenpair.so):
  * the exported ABI against include/cp_pre_screenpair.h and the ctypes binding, a C99 client compiled against the header;
  * the Makefile and loader facts;
  * the host reasons for the three-pass route, on CPU tensors and stub layouts, and the unchanged answer without ``pair``;
  * the entry points refusing, from ctypes with unmapped addresses, before any launch;
  * the caps the GPU tests' tolerances rest on, from the oracle alone, for every case tests/test_gpu_screenpair.py uses.
The device passes are covered by tests/test_gpu_screenpair.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import screen_helpers as sh
import screenflat_helpers as sf
import screenpair_helpers as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screenpair.h")
KIND_NAMES = ("stencil3d", "linear2", "ns_momentum", "mhd_continuity")
DECLARED = {"pre_screenpair_abi_version"} | {"pre_screenpair_%s%s_f32" % (f, k) for f in ("", "flat_") for k in KIND_NAMES}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screenpair_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screenpair.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_screenpair_library_exports_exactly_its_nine_symbols():
    from cp_pre_amd import _lib
    so = _lib.SCREENPAIR_SO_PATH
    assert os.path.exists(so), "libcp_pre_screenpair.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and len(DECLARED) == 9
    assert exported == declared and set(_lib.SCREENPAIR_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREENPAIR_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREENPAIR_ABI_VERSION == 1
    assert _lib._load("screenpair").pre_screenpair_abi_version() == _lib.PRE_SCREENPAIR_ABI_VERSION
    assert _lib.load_screenpair() is _lib._load("screenpair")
    # every declaration cites the reference lines it serves; the header says what the test is and is not
    for decl in re.split(r"\n(?=/\* )", header.split("pre_screenpair_abi_version(void);", 1)[1]):
        if "int pre_screenpair_" in decl:
            assert re.search(r"(Joint/\w+_Residuals_CP\.py:289-290, 307-313|Other_UQ/Evaluation/Eval\.py:278-281)", decl), decl[:80]
    assert "NOT the reference's two-sided form" in header


def test_screenpair_ctypes_signatures_have_the_header_arity_and_the_twins_tails():
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^int\s+(pre_screenpair_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    assert {n for n, _ in found} == DECLARED
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREENPAIR_SIGNATURES[name]), name
    # the twin's arguments after its field views, unchanged: kernels, scalars, the set descriptor, shape, flags, stream
    twins = {"stencil3d": ("stencil3d", 1), "linear2": ("linear2", 2), "ns_momentum": ("ns_momentum", 3)}
    for kind, (twin, nviews) in twins.items():
        for form, table, prefix in (("", _lib.SCREEN_SIGNATURES, "pre_screen_"), ("flat_", _lib.SCREENFLAT_SIGNATURES, "pre_screenflat_")):
            sig, tw = _lib.SCREENPAIR_SIGNATURES["pre_screenpair_%s%s_f32" % (form, kind)], table[prefix + twin + "_f32"]
            assert sig[2:] == tw[nviews:], (kind, form)
    for form, desc in (("", _lib.PreScreen), ("flat_", _lib.PreScreenFlat)):
        sig = _lib.SCREENPAIR_SIGNATURES["pre_screenpair_%smhd_continuity_f32" % form]
        assert sig[5] is ctypes.c_double and sig[6] is ctypes.POINTER(desc)


def test_screenpair_wrong_abi_version_and_missing_library_raise_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screenpair", None)
    monkeypatch.setattr(_lib, "PRE_SCREENPAIR_ABI_VERSION", _lib.PRE_SCREENPAIR_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_screenpair.so has ABI version 1"):
        _lib._load("screenpair")
    monkeypatch.setattr(_lib, "SCREENPAIR_SO_PATH", str(tmp_path / "libcp_pre_screenpair.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_screenpair()


def test_screenpair_header_compiles_as_c99_and_the_c_client_compiles_against_it(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "screenpair_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_screenpair_c_client_links(tmp_path):
    exe = tmp_path / "screenpair_check"
    subprocess.check_call(c_client_command(exe))
    assert exe.exists()


def test_screenpair_makefile_and_loader_facts():
    from cp_pre_amd import _lib
    assert len(_lib._LIBS) == 8 and "screenpair" not in _lib._LIBS and "screenpair" in _lib._LIBS_MORE
    csrc = os.path.join(ROOT, "cp_pre_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^LIBS\s+:=.*\bscreenpair\b", mk, flags=re.M) and re.search(r"^screenpair_OBJS\s+:= screen_pair\.o", mk, flags=re.M)
    assert re.search(r"^SHARED_HDRS\s+:=.*\bpaired_functor\.h\b", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS\s+:=(.|\\\n)*\$\(screenpair_OBJS\)", mk, flags=re.M)
    assert "$(screenpair_OBJS): $(INC)/cp_pre_screenpair.h $(INC)/cp_pre_screen.h $(INC)/cp_pre_screenflat.h" in mk
    assert not re.search(r"^screen_pair\.o:.*FLAGS", mk, flags=re.M)          # star_march.o's flags
    # Paired<Fn> is stated once, in the shared header; nothing new runs on the device
    src = {f: open(os.path.join(csrc, f)).read() for f in ("screen_pair.hip", "pair_march.hip", "paired_functor.h")}
    assert "struct Paired {" in src["paired_functor.h"] and all("struct Paired" not in src[f] for f in ("screen_pair.hip", "pair_march.hip"))
    assert all('#include "paired_functor.h"' in src[f] for f in ("screen_pair.hip", "pair_march.hip"))
    assert "__global__" not in src["screen_pair.hip"]
    assert '#include "screen_march.h"' in src["screen_pair.hip"] and '#include "screen_flat.h"' in src["screen_pair.hip"]


# ------------------------------------------------------------------ the host routing, on CPU tensors and stub layouts
class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the layout reasons come after the device check."""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def _nt_fast(t):
    """the logical tensor ``t`` [..., T, X, Y] as the permute view of a contiguous [..., X, Y, T] one"""
    n = t.dim()
    return t.permute(*range(n - 3), n - 2, n - 1, n - 3).contiguous().permute(*range(n - 3), n - 1, n - 3, n - 2)


def test_screenpair_without_the_keyword_prepare_still_declines_minus():
    from cp_pre_amd.screen import _Spec
    q = torch.ones(2)
    x = torch.rand(3, 3, 10, 5, 12)
    spec = _Spec(sh.method_of("ns_momentum"))
    for prep, v in ((spec.prepare, x), (spec.prepare_flat, _nt_fast(x))):
        assert prep(_dev(v), _dev(v), q, None) == ("minus=", ())
        assert prep(_dev(v), _dev(v), q, None, pair=False) == ("minus=", ())
        assert prep(v, None, q, None, pair=True) == ("input on the CPU", ())       # pair without minus: no effect
    b = _Spec(sh.method_of("wave"))
    assert b.prepare(_dev(x[:, 0]), _dev(x[:, 0]), q, None) == ("minus=", ())
    from cp_pre_amd import residuals as R
    rows = _Spec(R.Burgers(0.01, 0.01, 0.01).residual)
    assert rows.prepare_rows(_dev(torch.rand(3, 8, 16)), _dev(torch.rand(3, 8, 16)), q, None) == ("minus=", ())


def test_screenpair_host_reasons_in_order():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _PAIR_KINDS, _Spec
    assert _PAIR_KINDS == KIND_NAMES
    q, q64 = torch.ones(2), torch.ones(2, dtype=torch.float64)
    x, y = torch.rand(3, 6, 10, 5, 12), torch.rand(3, 6, 10, 5, 12)
    ns = _Spec(sh.method_of("ns_momentum"))
    assert ns.pair_declined() is None and ns.entry("", True) == "pre_screenpair_ns_momentum_f32"
    assert ns.entry("flat", True) == "pre_screenpair_flat_ns_momentum_f32"
    assert ns.route("", True) == "fused:pair_ns_momentum" and ns.route("flat", True) == "fused:flat_pair_ns_momentum"
    assert ns.entry("") == "pre_screen_ns_momentum_f32" and ns.route("flat") == "fused:flat_ns_momentum"
    for kind in sp.KINDS:
        assert _Spec(sh.method_of(kind)).route("", True) == sp.route(kind, "ny")
        assert _Spec(sh.method_of(kind)).route("flat", True) == sp.route(kind, "flat")
    # no paired screen for the method, before anything about the input
    for kind, why in sp.UNPAIRED.items():
        assert _Spec(sh.method_of(kind)).prepare(x, y, q, None, pair=True) == (why, ())
        assert _Spec(sh.method_of(kind)).prepare_flat(_dev(_nt_fast(x)), _dev(_nt_fast(y)), q, None, pair=True) == (why, ())
    import screenjorek_helpers as sj
    jo = _Spec(sj.jorek_of().residual_temperature, jorek=True)
    v = torch.rand(3, 3, 5, 12, 10)
    assert jo.prepare_flat(_dev(v), _dev(v), q, None, pair=True) == ("no paired screen for jorek_temperature", ())
    assert _Spec(sj.jorek_of().residual_continuity).prepare(v, v, q, None, pair=True) == ("no fused screen for JOREK", ())
    for method, u in ((R.Burgers(0.01, 0.01, 0.01).residual, torch.rand(3, 8, 16)), (R.Advection(1.0, 0.01, 0.01).residual, torch.rand(3, 8, 16))):
        rows = _Spec(method)
        assert rows.prepare(u, u, q, None, pair=True) == ("no paired screen for the 1-D family", ())
        assert rows.prepare_rows(_dev(u), _dev(u), q, None, pair=True) == ("no paired screen for the 1-D family", ())
    # the input: either set on the CPU, float64 levels or modulation
    assert ns.prepare(x, y, q, None, pair=True) == ("input on the CPU", ())
    assert ns.prepare(_dev(x), y, q, None, pair=True) == ("input on the CPU", ())
    assert ns.prepare(x, _dev(y), q, None, pair=True) == ("input on the CPU", ())
    assert ns.prepare(_dev(x), _dev(y), q64, None, pair=True) == ("float64 levels or modulation", ())
    assert ns.prepare(_dev(x), _dev(y), q, torch.ones(10, 5, 12, dtype=torch.float64), pair=True) == ("float64 levels or modulation", ())
    # the layout of vars, as today; then the same of minus
    odd = torch.rand(3, 3, 10, 5, 13)
    assert ns.prepare(_dev(odd), _dev(odd), q, None, pair=True) == ("row width not a multiple of 4", ())
    assert ns.prepare(_dev(x[..., ::2]), _dev(y[..., ::2]), q, None, pair=True) == ("no unit stride on the last axis", ())
    assert ns.prepare(_dev(x[..., :8]), _dev(y[..., ::2]), q, None, pair=True) == ("minus: no unit stride on the last axis", ())
    xt, yt = _nt_fast(x), _nt_fast(y)
    assert ns.nt_fastest(xt) and not ns.nt_fastest(x)
    assert ns.prepare_flat(_dev(xt[:, :, 2:8]), _dev(yt[:, :, 2:8]), q, None, pair=True) == ("rows not dense", ())
    slab = _nt_fast(torch.rand(3, 6, 6, 5, 12))
    assert ns.prepare_flat(_dev(slab), _dev(yt[:, :, 2:8]), q, None, pair=True) == ("minus: rows not dense", ())
    big = _nt_fast(torch.rand(3, 3, 96, 5, 12))
    assert ns.prepare_flat(_dev(big), _dev(big), q, None, pair=True) == ("Nt >= 96", ())
    oddt = _nt_fast(odd)
    assert ns.prepare_flat(_dev(oddt), _dev(oddt), q, None, pair=True) == ("merged row Ny*Nt not a multiple of 4", ())
    # one set Ny-fastest, the other Nt-fastest
    assert ns.prepare(_dev(x), _dev(yt), q, None, pair=True) == ("field sets in different layouts", ())
    assert ns.prepare_flat(_dev(xt), _dev(y), q, None, pair=True) == ("field sets in different layouts", ())
    # what declines whatever the layout, then the kernels
    off = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, fused=False)
    assert _Spec(off.residual_momentum).prepare(_dev(x), _dev(y), q, None, pair=True) == ("fused=False", ())
    live = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU)
    live.D_x.kernel.requires_grad_(True)
    assert _Spec(live.residual_momentum).prepare(_dev(x), _dev(y), q, None, pair=True) == ("operator kernel requires grad", ())
    box = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU)
    box.D_y.kernel.data[0, 0, 0] = 0.5
    assert _Spec(box.residual_momentum).prepare(_dev(x), _dev(y), q, None, pair=True) == ("operator kernel off the 7-point star", ())
    # all of it passes: the kernels come back, and three MHD channels are enough for the paired continuity
    why, ks = ns.prepare(_dev(x), _dev(y), q, None, pair=True)
    assert why is None and len(ks) == 4
    mc = _Spec(sh.method_of("mhd_continuity"))
    assert mc.prepare(_dev(x[:, :3]), _dev(y[:, :3]), q, None, pair=True)[0] is None
    assert mc.prepare(_dev(x[:, :3]), None, q, None)[0] == "fewer than six MHD channels"


def test_screenpair_bad_second_set_raises_before_any_device_work():
    from cp_pre_amd import screen
    m = sh.method_of("ns_momentum")
    x, q = torch.rand(3, 3, 6, 5, 12), torch.ones(2)
    with pytest.raises(ValueError, match="minus has shape"):
        screen.screen(m, x, q, minus=x[:2], pair=True)
    with pytest.raises(TypeError, match="minus has dtype"):
        screen.screen(m, x, q, minus=x.double(), pair=True)
    with pytest.raises(TypeError):
        screen.screen(m, x, q, minus=x, pair=True, nonsense=True)


@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_screenpair_cpu_tensors_take_the_fallback_and_meet_the_reference(kind):
    """``pair=True`` on CPU tensors: staged, three-pass, and the case's reference is met (on a machine with a GPU; without
    one the staging raises as everywhere else in the package)"""
    from cp_pre_amd import screen
    c = sp.case(kind, sp.NY_BASE)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            screen.screen(sh.method_of(kind), c.x, c.q, c.mod, minus=c.y, pair=True)
        return
    s = screen.screen(sh.method_of(kind), c.x, c.q, c.mod, minus=c.y, pair=True)
    assert screen.last_route() == "fallback:input on the CPU" and not s.score.is_cuda
    err = (s.score.double() - c.s_ref).abs()
    assert bool((err <= c.tol_s + 1.2e-7 * c.s_ref).all()) and bool(((s.inside - c.count_ref).abs() <= c.undecided).all())
    assert torch.equal(s.accept(), c.accept_ref)


# ------------------------------------------------------------------ refusals before any launch, from ctypes
def test_screenpair_entry_points_refuse_before_any_launch():
    """The addresses are not mapped and nothing is dereferenced: a refusal that reached a launch could not return its
    code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_screenpair()
    B, T, X, Y = 2, 6, 5, 12
    a0, b0, q0, s0, c0 = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000

    def dense(base):                     # [B,T,X,Y], Y fastest
        return _lib.PreField(base, T * X * Y, X * Y, Y, 1)

    def nt_fast(base):                   # the same logical view with memory [B,X,Y,T]
        return _lib.PreField(base, T * X * Y, 1, Y * T, T)

    def three(mk, base):
        return (_lib.PreField * 3)(mk(base), mk(base + 0x01000000), mk(base + 0x02000000))

    k27 = [0.0] * 27
    k27[13] = 1.0
    K = [_lib.farr(k27) for _ in range(4)]
    box, gen = list(k27), [0.0] * 27
    box[0] = 0.5
    gen[4] = gen[10] = gen[12] = 1.0                                # weight on all three axes: the general star
    sy = _lib.PreScreen(q0, 3, None, 0, 0, 1, 1, 1, s0, c0, B)
    st = _lib.PreScreenFlat(q0, 3, None, 0, 0, 0, 1, 1, 1, s0, c0, B)
    tail = (B, T, X, Y, 0, None)
    sc = (0.01, 0.02, 0.03, 0.001)
    for form, mk, other, s in (("", dense, nt_fast, sy), ("flat_", nt_fast, dense, st)):
        ns = getattr(lib, "pre_screenpair_%sns_momentum_f32" % form)
        mhd = getattr(lib, "pre_screenpair_%smhd_continuity_f32" % form)
        l2 = getattr(lib, "pre_screenpair_%slinear2_f32" % form)
        s3 = getattr(lib, "pre_screenpair_%sstencil3d_f32" % form)
        a, b = three(mk, a0), three(mk, b0)
        ref = ctypes.byref(s)
        assert ns(None, b, *K, *sc, ref, *tail) == _lib.PRE_E_NULL and ns(a, None, *K, *sc, ref, *tail) == _lib.PRE_E_NULL
        assert ns(a, b, *K[:3], None, *sc, ref, *tail) == _lib.PRE_E_NULL and ns(a, b, *K, *sc, None, *tail) == _lib.PRE_E_NULL
        nullb = three(mk, b0)
        nullb[2].ptr = None                                         # a null view of the SECOND set
        assert ns(a, nullb, *K, *sc, ref, *tail) == _lib.PRE_E_NULL
        assert mhd(a, nullb, *K[:3], 5 / 3, ref, *tail) == _lib.PRE_E_NULL
        assert l2(a, None, K[0], K[1], 1.0, ref, *tail) == _lib.PRE_E_NULL
        noq = type(s).from_buffer_copy(s)
        noq.q = None
        assert mhd(a, b, *K[:3], 5 / 3, ctypes.byref(noq), *tail) == _lib.PRE_E_NULL
        many = type(s).from_buffer_copy(s)
        many.nk = 17
        assert l2(a, b, K[0], K[1], 1.0, ctypes.byref(many), *tail) == _lib.PRE_E_RANGE
        # the layout of either set; flags the form does not take
        assert ns(three(other, a0), b, *K, *sc, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert ns(a, three(other, b0), *K, *sc, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert s3(ctypes.byref(mk(a0)), ctypes.byref(other(b0)), _lib.farr([1.0]), _lib.iarr32([0, 0, 0]), 1, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert ns(a, b, *K, *sc, ref, B, T, X, Y, _lib.PRE_FLAG_ABS, None) == _lib.PRE_E_UNSUPPORTED
        # operator weight off the star, and the general stars of the six-view functors, after every layout check passed
        assert ns(a, b, K[0], _lib.farr(box), *K[2:], *sc, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert ns(a, b, K[0], _lib.farr(gen), *K[2:], *sc, ref, *tail) == _lib.PRE_E_UNSUPPORTED
        assert mhd(a, b, K[0], _lib.farr(gen), K[2], 5 / 3, ref, *tail) == _lib.PRE_E_UNSUPPORTED
    flat_ns = lib.pre_screenpair_flat_ns_momentum_f32
    assert flat_ns(three(nt_fast, a0), three(nt_fast, b0), *K, *sc, ctypes.byref(st), B, T, X, Y, _lib.PRE_FLAG_HALO_X, None) == _lib.PRE_E_UNSUPPORTED
    assert lib.pre_screenpair_ns_momentum_f32(three(dense, a0), three(dense, b0), *K, *sc, ctypes.byref(sy), B, T, X, 10, 0, None) == _lib.PRE_E_UNSUPPORTED


# ------------------------------------------------------------------ the caps of the GPU tests, from the oracle alone
@pytest.mark.parametrize("kind", sp.KINDS + tuple(sp.UNPAIRED))
def test_screenpair_reference_values_meet_the_caps(kind):
    """Every case tests/test_gpu_screenpair.py compares with the reference: at most max(1 cell, 1 %) of the counted cells
    undecided for every (level, sample), every level further than 2 tau / m_min from every per-sample score, a level that
    accepts some samples and rejects others, m_min > 0 - at the seed ``screenpair_helpers.SEEDS`` names (default 0)."""
    worst, n = (0.0, float("inf")), 0
    for key in sp.gpu_cases():
        if key[0] != kind:
            continue
        c = sp.case(*key)
        ok, (und, cells, dist, split) = c.caps_hold()
        assert c.q.dtype == torch.float32 and c.q.shape == (key[4],) and tuple(c.x.shape) == tuple(c.y.shape)
        assert ok, (key, c.seed, und, cells, dist, split)
        if cells >= 100:
            worst = (max(worst[0], und / cells), worst[1])
        worst, n = (worst[0], min(worst[1], dist)), n + 1
    assert n > 0 and worst[0] <= 0.01
    print(f"{kind}: {n} cases, largest undecided share {worst[0]:.4f} (regions of 100 cells and more), closest level "
          f"{worst[1]:.1f} x tau/m_min from a score")
    assert all(k[:4] in {c[:4] for c in sp.gpu_cases()} for k in sp.SEEDS), "a seed for a case that no test uses"
