"""The per-cell screen of the data-driven scores without a GPU: the reference's own caps for every case the GPU files run,
the argument errors (all before any device work), the route reasons that shapes and strides alone decide and their order,
the ABI facts of libcp_pre_screencellspair.so and its C client, the Makefile and source facts of the unit.  Helpers and the
reference: tests/screencellspair_helpers.py."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import screen_helpers as sh
import screencellspair_helpers as cp
import screenpair_helpers as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cp_pre_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "cp_pre_screencellspair.h")
KINDS4 = ("stencil3d", "linear2", "ns_momentum", "mhd_continuity")
DECLARED = {"pre_screencellspair_abi_version", "pre_screencellspair_sample_group"} | \
    {"pre_screencellspair_%s%s_f32" % (form, k) for form in ("", "flat_") for k in KINDS4}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screencellspair_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screencellspair.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the layout reasons come after the device check."""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def _nt_fast(t):
    n = t.dim()
    return t.permute(*range(n - 3), n - 2, n - 1, n - 3).contiguous().permute(*range(n - 3), n - 1, n - 3, n - 2)


# ------------------------------------------------------------------ the reference's own caps
def test_screencellspair_reference_caps_hold_for_every_gpu_case():
    from cp_pre_amd import screen
    G = screen.sample_group_pair()
    assert isinstance(G, int) and G >= 1
    cases = cp.gpu_cases(G)
    worst, curve_lo, curve_hi = 0.0, 1.0, 0.0
    for key in cases:
        c = cp.case(*key)
        ok, (und, cells, (rank, want, differ), split) = c.caps_hold()
        worst = max(worst, und / cells)
        cov = c.count_ref.double().sum(dim=1) / (c.cells * c.shape[0])
        curve_lo, curve_hi = min(curve_lo, float(cov.min())), max(curve_hi, float(cov.max()))
        assert und <= (int(0.01 * cells) if cells >= 100 else 1), (key, und, cells)
        assert rank == want == (12 if key[4] == 16 else key[4]) and differ > 0.5, (key, rank, want, differ)
        assert split and ok, key
        assert tuple(c.q.shape) == (key[4],) + tuple(key[1][1:]) and c.q.dtype == torch.float32
        assert c.tau > 0 and c.tol_s > 0
    assert not set(cp.SEEDS) - set(cases)                            # (no seed is tabled for a case no test uses)
    print(f"{len(cases)} cases: largest undecided share {worst:.4f}, coverage curve from {curve_lo:.3f} to {curve_hi:.3f}")


def test_screencellspair_cases_are_those_of_the_two_helper_modules():
    """the field sets, the modulation and tau are the paired joint case's; the ranks the per-cell case's"""
    import screencells_helpers as ch
    c = cp.case("ns_momentum", sp.NY_BASE, False, True, 10)
    p = sp.PairCase("ns_momentum", sp.NY_BASE, False, True, 6, seed=0)
    assert torch.equal(c.x, p.x) and torch.equal(c.y, p.y) and torch.equal(c.mod, p.mod) and c.tau == p.tau
    assert torch.equal(c.s_ref, p.s_ref) and c.cells == p.cells and not torch.equal(c.x, c.y)
    assert cp.ranks(10) == ch.ranks(10) and cp.ranks(16) == ch.ranks(16) and cp.ranks(1) == ch.ranks(1)
    for nk in cp.ONE_LIVE:
        assert len(cp.ranks(nk)) == len(set(cp.ranks(nk))) == nk and set(cp.ranks(nk)) <= set(ch.ranks(10))
    assert isinstance(c, ch.CellCase) and cp.check is ch.check


# ------------------------------------------------------------------ argument errors, before any device work
def test_screencellspair_argument_errors():
    from cp_pre_amd import screen
    m = sh.method_of("ns_momentum")
    x, y = torch.rand(3, 3, 6, 9, 12), torch.rand(3, 3, 6, 9, 12)
    q = torch.rand(10, 6, 9, 12)
    kw = dict(minus=y, pair=True)
    with pytest.raises(TypeError, match="qcells must be a torch.Tensor"):
        screen.screen_cells(m, x, [1.0], **kw)
    with pytest.raises(TypeError, match="float32 fields"):
        screen.screen_cells(m, x.double(), q, **kw)
    with pytest.raises(ValueError, match="1 <= nk <= 16"):
        screen.screen_cells(m, x, torch.rand(17, 6, 9, 12), **kw)
    with pytest.raises(ValueError, match="or the cropped"):
        screen.screen_cells(m, x, torch.rand(10, 5, 9, 12), **kw)
    with pytest.raises(ValueError, match="modulation has shape"):
        screen.screen_cells(m, x, q, torch.rand(4, 7, 10), **kw)
    with pytest.raises(ValueError):                                   # the second set: shape, then dtype
        screen.screen_cells(m, x, q, minus=y[:2], pair=True)
    with pytest.raises(ValueError):
        screen.screen_cells(m, x, q, minus=y[:, :2], pair=True)
    with pytest.raises(TypeError):
        screen.screen_cells(m, x, q, minus=y.double(), pair=True)
    with pytest.raises(TypeError):
        screen.screen_cells(m, x, q, minus=[1.0], pair=True)
    s = screen.ScreenCells(3, 10, "cpu")
    with pytest.raises(ValueError, match="expected n_local = 3"):
        s.add_slab(m, x[:2], q, minus=y[:2], pair=True)
    with pytest.raises(ValueError, match="leaves no cell"):
        s.add_slab(m, x, q, crop=(3, 1, 1), **kw)
    with pytest.raises(ValueError, match="uncropped extents"):
        s.add_slab(m, x, torch.rand(10, 4, 7, 10), **kw)
    assert s.acc is None and s.cells == 0
    # the keyword is the last one of both signatures, and False by default
    for fn in (screen.screen_cells, screen.ScreenCells.add_slab):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "pair" and params[-1].default is False and params[-2].name == "rows"


# ------------------------------------------------------------------ the route reasons, in order
def test_screencellspair_route_reasons_in_order():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _Spec
    x, y = torch.rand(3, 3, 10, 5, 12), torch.rand(3, 3, 10, 5, 12)
    q, q64 = torch.rand(4, 10, 5, 12), torch.rand(4, 10, 5, 12).double()
    spec = _Spec(sh.method_of("ns_momentum"))
    # without the keyword: minus= first, whatever else is wrong
    assert spec.prepare(_dev(x), _dev(y), q, None) == ("minus=", ())
    assert spec.prepare(x, y, q64, None, False) == ("minus=", ())
    # with it: no paired screen for the kind, CPU inputs, float64, the layouts of vars, different layouts, minus: <reason>
    x6 = torch.rand(3, 6, 10, 5, 12)
    for kind, why in sp.UNPAIRED.items():
        assert _Spec(sh.method_of(kind)).prepare(x6, x6, q64, None, True) == (why, ())
    assert spec.prepare(x, _dev(y), q64, None, True) == ("input on the CPU", ())
    assert spec.prepare(_dev(x), y, q64, None, True) == ("input on the CPU", ())
    assert spec.prepare(_dev(x)[..., ::2], _dev(y), q64, None, True) == ("float64 levels or modulation", ())
    assert spec.prepare(_dev(x), _dev(y), q, torch.rand(10, 5, 12).double(), True) == ("float64 levels or modulation", ())
    assert spec.prepare(_dev(x)[..., ::2], _dev(_nt_fast(y)), q, None, True) == ("no unit stride on the last axis", ())
    assert spec.prepare(_dev(torch.rand(3, 3, 10, 5, 13)), _dev(_nt_fast(torch.rand(3, 3, 10, 5, 13))), q, None, True) == \
        ("row width not a multiple of 4", ())
    assert spec.prepare(_dev(x), _dev(_nt_fast(y)), q, None, True) == ("field sets in different layouts", ())
    assert spec.prepare(_dev(x), _dev(y)[..., ::2], q, None, True) == ("minus: no unit stride on the last axis", ())
    xf, yf = _nt_fast(x), _nt_fast(y)
    assert spec.nt_fastest(xf)
    assert spec.prepare_flat(xf, _dev(yf), q, None, True) == ("input on the CPU", ())
    assert spec.prepare_flat(_dev(_nt_fast(torch.rand(3, 3, 96, 5, 12))), _dev(y), q, None, True) == ("Nt >= 96", ())
    assert spec.prepare_flat(_dev(xf), _dev(y), q, None, True) == ("field sets in different layouts", ())
    assert spec.prepare_flat(_dev(xf), _dev(_nt_fast(torch.rand(3, 3, 16, 5, 12)))[:, :, 2:12], q, None, True) == ("minus: rows not dense", ())
    off = _Spec(R.NavierStokes(0.01, 0.1, 0.1, fused=False).residual_momentum)
    assert off.prepare(_dev(x), _dev(y)[..., ::2], q, None, True)[0] == "minus: no unit stride on the last axis"
    assert off.prepare(_dev(x), _dev(y), q, None, True)[0] == "fused=False"
    assert spec.prepare(_dev(x), _dev(y), q, None, True)[0] is None
    assert spec.prepare_flat(_dev(xf), _dev(yf), q, None, True)[0] is None
    # pair=True without minus: the one-set question
    assert spec.prepare(_dev(x), None, q, None, True)[0] is None
    # the routes and the entries
    assert spec.route("", True, cells=True) == "fused:cells_pair_ns_momentum"
    assert spec.route("flat", True, cells=True) == "fused:flat_cells_pair_ns_momentum"
    assert spec.entry("", True, cells=True) == "pre_screencellspair_ns_momentum_f32"
    assert spec.entry("flat", True, cells=True) == "pre_screencellspair_flat_ns_momentum_f32"
    for kind in sp.KINDS:
        s = _Spec(sh.method_of(kind))
        assert s.route("", True, cells=True) == cp.route(kind) and s.route("flat", True, cells=True) == cp.route(kind, flat=True)
        assert s.entry("", True, cells=True) in DECLARED and s.entry("flat", True, cells=True) in DECLARED
    assert _Spec(sh.method_of("mhd_continuity")).entry("flat", True, cells=True) == "pre_screencellspair_flat_mhd_continuity_f32"
    # the routes that were there are spelled as they were
    assert spec.route("", cells=True) == "fused:cells_ns_momentum" and spec.entry("", cells=True) == "pre_screencells_ns_momentum_f32"
    assert spec.route("", True) == "fused:pair_ns_momentum" and spec.entry("flat", True) == "pre_screenpair_flat_ns_momentum_f32"
    bu = _Spec(R.Burgers(0.01, 0.01, 0.01).residual)
    assert bu.route("rows", True, cells=True) == "fused:rows_cells_pair_burgers"
    assert bu.entry("rows", True, cells=True) == "pre_screen1dcells_pair_burgers_f32"


def test_screencellspair_cpu_inputs_reach_the_fallback_without_loading_the_library():
    """on CPU tensors the call reaches the three-pass route (which stages to the device): without a device it fails loudly
    in the staging, not in the argument checks; the route is named first, and the library is not loaded on the way"""
    from cp_pre_amd import _lib, screen
    c = cp.case("ns_momentum", sp.NY_BASE, False, True, 10)
    loaded = _lib._screencellspair
    for pair, why in ((True, "fallback:input on the CPU"), (False, "fallback:minus=")):
        if torch.cuda.is_available():
            got = screen.screen_cells(sh.method_of("ns_momentum"), c.x, c.q, c.mod, minus=c.y, pair=pair)
            cp.check(c, got, why)
        else:
            with pytest.raises((RuntimeError, AssertionError)):
                screen.screen_cells(sh.method_of("ns_momentum"), c.x, c.q, c.mod, minus=c.y, pair=pair)
        assert screen.last_route() == why
    assert _lib._screencellspair is loaded


# ------------------------------------------------------------------ the ABI
def test_screencellspair_library_exports_exactly_its_symbols_and_the_sample_group():
    from cp_pre_amd import _lib, screen
    so = _lib.SCREENCELLSPAIR_SO_PATH
    assert os.path.exists(so), "libcp_pre_screencellspair.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and len(DECLARED) == 10
    assert exported == declared and set(_lib.SCREENCELLSPAIR_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREENCELLSPAIR_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREENCELLSPAIR_ABI_VERSION == 1
    lib = _lib.load_screencellspair()
    assert lib.pre_screencellspair_abi_version() == 1
    G = lib.pre_screencellspair_sample_group()
    assert G >= 1 and screen.sample_group_pair() == G
    assert "screencellspair" in _lib._LIBS_MORE and len(_lib._LIBS) == 8
    # the header defines no struct and includes the per-cell one
    assert "typedef struct" not in header and '#include "cp_pre_screencells.h"' in header
    # the twins' arguments in libcp_pre_screenpair.so, with the per-cell descriptor in the place of theirs
    for form, desc in (("", _lib.PreScreenCells), ("flat_", _lib.PreScreenCellsFlat)):
        for k in KINDS4:
            sig = _lib.SCREENCELLSPAIR_SIGNATURES["pre_screencellspair_%s%s_f32" % (form, k)]
            tw = _lib.SCREENPAIR_SIGNATURES["pre_screenpair_%s%s_f32" % (form, k)]
            assert len(sig) == len(tw)
            diff = [i for i, (a, b) in enumerate(zip(sig, tw)) if a is not b]
            assert len(diff) == 1 and sig[diff[0]] is ctypes.POINTER(desc), (form, k)


def test_screencellspair_header_and_c_client_compile_and_link(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "screencellspair_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    exe = tmp_path / "screencellspair_check"
    subprocess.check_call(c_client_command(exe))
    assert obj.exists() and exe.exists()


def test_screencellspair_makefile_and_source_facts():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^LIBS\s+:=.*\bscreencellspair\b", mk, flags=re.M)
    assert re.search(r"^screencellspair_OBJS\s+:= screen_cells_pair\.o", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS\s+:=(.|\\\n)*\$\(screencellspair_OBJS\)", mk, flags=re.M)
    assert "$(screencellspair_OBJS): $(INC)/cp_pre_screencellspair.h $(INC)/cp_pre_screencells.h $(INC)/cp_pre_screen.h $(INC)/cp_pre_screenflat.h" in mk
    for var, macro in (("SCREENCELLSPAIR_GROUP", "PRE_SCREENCELLS_GROUP"), ("SCREENCELLSPAIR_BATCH", "PRE_SCREENCELLSPAIR_BATCH"),
                       ("SCREENCELLSPAIR_LATE", "PRE_SCREENCELLSPAIR_LATE")):
        assert "ifdef %s\nscreen_cells_pair.o: FLAGS += -D%s=$(%s)\nendif" % (var, macro, var) in mk
    assert not re.search(r"^screen_cells_pair\.o: FLAGS \+= -f", mk, flags=re.M)      # star_march.o's flags: no contraction switch
    src = open(os.path.join(CSRC, "screen_cells_pair.hip")).read()
    assert "__global__" not in src                                   # the marches are not copied
    for inc in ("screen_march.h", "screen_flat.h", "paired_functor.h", "screen_entries.h", "../../include/cp_pre_screencellspair.h"):
        assert '#include "%s"' % inc in src
    assert src.count("Paired, CellSets>(") == 8 and "ScalarSets>(" not in src and "Single, " not in src.split("#include")[-1]
    # pair_views is stated once, next to mhd_views, and used by both paired units
    entries = open(os.path.join(CSRC, "screen_entries.h")).read()
    pair = open(os.path.join(CSRC, "screen_pair.hip")).read()
    assert entries.count("Views pair_views(") == 1 and entries.index("Views mhd_views(") < entries.index("Views pair_views(")
    assert "Views pair_views(" not in pair and "Views pair_views(" not in src
    assert pair.count("pair_views<") == 6 and src.count("pair_views<") == 6
    # what is not built is in the table, false rows for CellSets on the paired functors
    for row in ("template <class Form> struct Built<Form, CellSets, PairedNS<2>> : std::false_type {};",
                "template <class Form> struct Built<Form, CellSets, PairedMHDContinuity<2>> : std::false_type {};",
                "template <> struct Built<NyForm, CellSets, PairedNS<1>> : std::false_type {};",
                "template <> struct Built<FlatForm, CellSets, PairedNS<4>> : std::false_type {};"):
        assert row in entries


def test_screencellspair_late_batch_defaults_to_the_first_batch():
    """read from the header text: CellsLate<Fn> is CellsBatch<Fn> unless a unit says otherwise, and only the new unit does"""
    plane = open(os.path.join(CSRC, "screen_plane.h")).read()
    assert "template <class Fn, class = void> struct CellsLate { static constexpr int value = CellsBatch<Fn>::value; };" in plane
    assert "template <class Fn, class = void> struct CellsBatch { static constexpr int value = PRE_SCREENCELLS_BATCH; };" in plane
    users = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) and "struct CellsLate<" in open(os.path.join(CSRC, f)).read())
    assert users == ["screen_cells_pair.hip"]
    for march in ("screen_march.h", "screen_flat.h"):
        text = open(os.path.join(CSRC, march)).read()
        assert "constexpr int LL = CellsLate<Fn>::value;" in text and "load_late(t, k0);" in text
        assert "screen_plane_count<LL>(ac, sv, k0, g.nk, qm, cnt);" in text
    rows = open(os.path.join(CSRC, "screen_rows.h")).read()
    assert "CellsLate" not in rows


def test_screencellspair_resource_listing_has_no_scratch():
    """profiles/screencellspair/resources.txt, the listing of the unit as committed: every row spill-free, scratch 0; the
    listings of the five existing units at the parent and at the head have the same rows"""
    prof = os.path.join(ROOT, "profiles", "screencellspair")
    rows = [ln for ln in open(os.path.join(prof, "resources.txt")).read().splitlines() if "v=" in ln]
    assert len(rows) == 20 and all("Paired<" in ln for ln in rows)
    for ln in rows:
        m = re.search(r"v=(\d+)\s+spill=(\S*)\s+scratch=(\d+)", ln)
        assert m and int(m.group(1)) <= 256 and m.group(2) in ("", "0") and int(m.group(3)) == 0, ln
    assert open(os.path.join(prof, "resources_existing_parent.txt")).read() == open(os.path.join(prof, "resources_existing_head.txt")).read()


def test_screencellspair_library_is_not_loaded_by_any_other_route():
    """screen.py reaches the library in two places only: the paired branch of the one launcher under ``cells``, and
    ``sample_group_pair``; ``Screen.add_slab`` never passes ``cells``"""
    from cp_pre_amd import screen
    src = inspect.getsource(screen)
    assert src.count('_load("screencellspair")') == 2
    users = {name for name, fn in inspect.getmembers(screen, inspect.isfunction) if "screencellspair\")" in inspect.getsource(fn)}
    assert users == {"sample_group_pair"}
    launch = inspect.getsource(screen._Spec.launch)
    assert '_lib._load("screencellspair") if cells else _lib.load_screenpair()' in launch
    assert "cells=True" not in inspect.getsource(screen.Screen.add_slab)
    assert "pair" in inspect.signature(screen.ScreenCells.add_slab).parameters
    # nothing else in the package names it
    pkg = os.path.join(ROOT, "cp_pre_amd")
    others = [f for f in os.listdir(pkg) if f.endswith(".py") and f not in ("screen.py", "_lib.py") and
              "screencellspair" in open(os.path.join(pkg, f)).read()]
    assert others == []
