"""The per-cell screen of the 1-D family without a GPU: the reference's own caps for every case the GPU file runs, the
argument errors (all before any device work), the reasons of the opt-in route in ``prepare_rows``' order, the unchanged route
without ``rows=True``, the NaN padding of cropped levels in both layouts, the ABI facts of libcp_pre_screen1dcells.so and its C
client, the Makefile facts and the block order restated.  Helpers and the reference: tests/screen1dcells_helpers.py."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import screen1d_helpers as s1
import screen1dcells_helpers as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screen1dcells.h")
DECLARED = {"pre_screen1dcells_abi_version", "pre_screen1dcells_sample_group", "pre_screen1dcells_stencil2d_f32",
            "pre_screen1dcells_burgers_f32", "pre_screen1dcells_pair_stencil2d_f32", "pre_screen1dcells_pair_burgers_f32"}
FIELDS = ["levels", "nk", "lK", "lT", "lX", "modulation", "mT", "mX", "ct", "cx", "score", "count", "count_ld"]


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screen1dcells_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screen1dcells.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the layout reasons come after the device check."""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def _nt(t):
    """the logical [..,Nt,Nx] tensor with unit stride on Nt"""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def _burgers():
    from cp_pre_amd import residuals as R
    return R.Burgers(s1.DX, s1.DT, s1.NU).residual


# ------------------------------------------------------------------ the reference's own caps
def test_screen1dcells_reference_caps_hold_for_every_gpu_case():
    """a condition on the INPUTS, from the float64 reference alone: at most 1 % of a sample's counted cells undecided at any
    level, and a level that splits a sample's cells"""
    from cp_pre_amd import screen
    G = screen.sample_group_rows()
    assert isinstance(G, int) and G >= 1
    cases = h.gpu_cases(G)
    worst = 0.0
    for key in cases:
        c = h.case(*key)
        share, split = c.caps()
        worst = max(worst, share)
        assert share <= h.SHARE_CAP == 0.01, (key, share)
        assert split, key
        assert tuple(c.q.shape) == (c.nk,) + c.shape[1:] and c.q.dtype == torch.float32
    print(f"{len(cases)} cases: largest undecided share {worst:.4f}")
    assert not set(h.SEEDS) - {(k, s1.logical_shape(B, tuple(p), lay), bool(b), bool(m), nk, bool(pr))
                               for k, B, p, lay, b, m, nk, pr in cases}, "a SEEDS entry names a case no test uses"
    # what the issue names is in the list
    planes = {(B, tuple(p)) for _, B, p, *_ in cases}
    assert set(s1.SEAM_PLANES.values()) <= planes
    assert {(G + 1, (12, 64)), (2 * G - 1, (12, 64))} <= planes or G == 1
    assert {(k, lay, b, m, nk) for k, _, _, lay, b, m, nk, pr in cases if not pr} >= {
        (k, lay, b, m, nk) for k in s1.KINDS for lay in s1.LAYOUTS for b in (False, True) for m in (False, True) for nk in (1, 10, 16)}
    assert {(k, lay) for k, _, _, lay, _, _, _, pr in cases if pr} == {(k, lay) for k in h.PAIR_KINDS for lay in s1.LAYOUTS}


def test_screen1dcells_levels_have_full_rank():
    """a kernel that reads one level field for every k, or one level per k for every cell, cannot pass"""
    for pair in (False, True):
        c = h.case("burgers", *s1.SEAM_PLANES["wave_segments"], "nx", nk=10, pair=pair)
        assert int(torch.linalg.matrix_rank(c.q.reshape(10, -1).double())) == 10
    c = h.case("dxx", *s1.SEAM_PLANES["partial_last_strip"], "nt", nk=16)
    assert int(torch.linalg.matrix_rank(c.q.reshape(16, -1).double())) == 16
    assert h.ranks(10) == [(i, i) for i in (11, 10, 8, 7, 6, 5, 4, 2, 1, 0)]
    assert len(set(h.ranks(16))) == 16 and h.ranks(1) == [(5, 6)]


# ------------------------------------------------------------------ argument errors, before any device work
def test_screen1dcells_argument_errors():
    from cp_pre_amd import screen
    m = _burgers()
    x, q, qc = torch.rand(3, 8, 16), torch.rand(10, 8, 16), torch.rand(10, 6, 14)
    kw = dict(rows=True)
    with pytest.raises(TypeError, match="qcells must be a torch.Tensor"):
        screen.screen_cells(m, x, [1.0], **kw)
    with pytest.raises(TypeError, match="dtype"):
        screen.screen_cells(m, x, q.half(), **kw)
    with pytest.raises(TypeError, match="float32 fields"):
        screen.screen_cells(m, x.double(), q, **kw)
    with pytest.raises(ValueError, match="1 <= nk <= 16"):
        screen.screen_cells(m, x, torch.rand(17, 8, 16), **kw)
    with pytest.raises(ValueError, match="1 <= nk <= 16"):
        screen.screen_cells(m, x, torch.rand(10), **kw)
    with pytest.raises(ValueError, match="or the cropped"):
        screen.screen_cells(m, x, torch.rand(10, 7, 16), **kw)
    with pytest.raises(ValueError, match=r"expected \[nk, \*\(8, 16\)\]$"):
        screen.screen_cells(m, x, qc, boundary=True, **kw)            # cropped extents with boundary=True
    with pytest.raises(ValueError, match="is on"):
        screen.screen_cells(m, x, q.to("meta"), **kw)
    with pytest.raises(ValueError, match="modulation has shape"):
        screen.screen_cells(m, x, q, torch.rand(6, 14), **kw)
    with pytest.raises(ValueError, match="minus has shape"):
        screen.screen_cells(m, x, q, minus=x[:2], **kw)
    with pytest.raises(TypeError, match="minus has dtype"):
        screen.screen_cells(m, x, q, minus=x.double(), **kw)
    s = screen.ScreenCells(3, 10, "cpu")
    with pytest.raises(ValueError, match="expected n_local = 3"):
        s.add_slab(m, x[:2], q, crop=(1, 1), **kw)
    with pytest.raises(ValueError, match="crop"):
        s.add_slab(m, x, q, **kw)                                    # (the default crop has three axes)
    with pytest.raises(ValueError, match="leaves no cell"):
        s.add_slab(m, x, q, crop=(4, 1), **kw)
    with pytest.raises(ValueError, match=r"expected \(10,\)"):
        s.add_slab(m, x, q[:4], crop=(1, 1), **kw)
    with pytest.raises(ValueError, match="uncropped extents"):
        s.add_slab(m, x, qc, crop=(1, 1), **kw)
    # halo_x raises for this family as it does without rows=True
    with pytest.raises(ValueError, match="halo_x"):
        s.add_slab(m, x, q, crop=(1, 1), halo_x=True, **kw)
    for rows in (False, True):
        with pytest.raises(RuntimeError, match="halo_x"):
            s.add_slab(m, _dev(x), q, crop=(1, 1), halo_x=True, rows=rows)
    assert s.acc is None and s.cells == 0


# ------------------------------------------------------------------ the routes
def test_screen1dcells_reasons_come_in_prepare_rows_order():
    """what ``ScreenCells.add_slab(rows=True)`` asks: ``prepare_rows`` with the level fields in the place of the levels, and
    ``pair="rows"`` when there is a ``minus``"""
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_1d import ConvOperator as C1
    from cp_pre_amd.screen import _Spec
    q, q64 = torch.rand(4, 8, 16), torch.rand(4, 8, 16).double()
    x, y = torch.rand(3, 8, 16), torch.rand(3, 8, 16)
    bg = _Spec(_burgers())
    for kind in s1.KINDS:
        sp, k = _Spec(s1.method_of(kind)), "burgers" if kind == "burgers" else "stencil2d"
        assert sp.route("rows", cells=True) == h.ROUTE[kind] == "fused:rows_cells_" + k
        assert sp.route("rows", True, cells=True) == h.ROUTE_PAIR[kind] == "fused:rows_cells_pair_" + k
        assert sp.entry("rows", cells=True) == "pre_screen1dcells_" + k + "_f32"
        assert sp.entry("rows", True, cells=True) == "pre_screen1dcells_pair_" + k + "_f32"
        # the other forms keep their names
        assert sp.entry("rows") == "pre_screen1d_" + k + "_f32" and sp.entry("rows", True) == "pre_screen1dpair_" + k + "_f32"
    # _Spec.prepare still gives the family's reason: the route is opt-in
    assert bg.prepare(_dev(x), None, q, None) == ("1-D family: the marched axis is the batch", ())
    # one set
    assert bg.prepare_rows(x, None, q, None) == ("input on the CPU", ())
    assert bg.prepare_rows(_dev(x), None, q64, None) == ("float64 levels or modulation", ())
    assert bg.prepare_rows(_dev(x), None, q, torch.ones(8, 16).double()) == ("float64 levels or modulation", ())
    assert bg.prepare_rows(_dev(x[:, None]), None, q, None) == ("[BS,1,Nt,Nx] input", ())
    wide = torch.rand(3, 16, 32)
    assert bg.prepare_rows(_dev(wide[:, ::2, ::2]), None, q, None) == ("no unit-stride axis", ())
    assert bg.prepare_rows(_dev(torch.rand(3, 8, 14)), None, q, None) == ("contiguous-axis length not a multiple of 4", ())
    assert bg.prepare_rows(_dev(_nt(torch.rand(3, 14, 8))), None, q, None) == ("contiguous-axis length not a multiple of 4", ())
    live = R.Burgers(s1.DX, s1.DT, s1.NU)
    live.D_x.kernel.requires_grad_(True)
    assert _Spec(live.residual).prepare_rows(_dev(x), None, q, None) == ("operator kernel requires grad", ())
    # the order: input before layout before what declines whatever the layout
    assert _Spec(live.residual).prepare_rows(x[:, None], None, q64, None) == ("input on the CPU", ())
    assert _Spec(live.residual).prepare_rows(_dev(x[:, None]), None, q64, None) == ("float64 levels or modulation", ())
    assert _Spec(live.residual).prepare_rows(_dev(x[:, None]), None, q, None) == ("[BS,1,Nt,Nx] input", ())
    # two sets
    kw = dict(pair="rows")
    assert bg.prepare_rows(_dev(x), y, q, None, **kw) == ("input on the CPU", ())
    assert bg.prepare_rows(_dev(x), _dev(_nt(y)), q, None, **kw) == ("field sets in different layouts", ())
    assert bg.prepare_rows(_dev(_nt(x)), _dev(y), q, None, **kw) == ("field sets in different layouts", ())
    assert bg.prepare_rows(_dev(x), _dev(wide[:, ::2, ::2]), q, None, **kw) == ("minus: no unit-stride axis", ())
    for a, b in ((x, None), (_nt(x), None), (x, y), (_nt(x), _nt(y)), (wide[:, :8, :16], y)):
        why, ks = bg.prepare_rows(_dev(a), None if b is None else _dev(b), q, None, **kw)
        assert why is None and len(ks) == 3
    # a method outside the family: rows=True has no effect on what is asked of it
    assert _Spec(C1("x", 2, conv="spectral")).rows_kind is None
    src = inspect.getsource(__import__("cp_pre_amd.screen", fromlist=["x"]).ScreenCells.add_slab)
    assert "rows = bool(rows) and spec.rows_kind is not None" in src and src.count("spec.launch(") == 1


def test_screen1dcells_without_rows_the_route_is_unchanged_and_the_library_is_not_loaded():
    from cp_pre_amd import _lib, screen
    saved = _lib._screen1dcells
    _lib._screen1dcells = None
    try:
        c = h.case("burgers", *s1.SEAM_PLANES["wave_segments"], "nx")
        m = s1.method_of("burgers")
        for kw in ({}, dict(rows=False), dict(rows=True)):             # (CPU inputs: every one reaches the three-pass route)
            if torch.cuda.is_available():
                got = screen.screen_cells(m, c.x, c.q, c.mod, **kw)
                h.check(c, got, "CPU inputs %r" % kw)
            else:
                with pytest.raises((RuntimeError, AssertionError)):
                    screen.screen_cells(m, c.x, c.q, c.mod, **kw)
            want = "fallback:input on the CPU" if kw.get("rows") else h.FALLBACK
            assert screen.last_route() == want, kw
        assert _lib._screen1dcells is None, "libcp_pre_screen1dcells.so was loaded without a launch of the new route"
    finally:
        _lib._screen1dcells = saved
    # screen.py names the loader in the launcher's rows branches and in sample_group_rows only
    src = inspect.getsource(screen)
    users = {name for name, fn in inspect.getmembers(screen, inspect.isfunction) if "load_screen1dcells" in inspect.getsource(fn)}
    assert users == {"sample_group_rows"}
    assert src.count("load_screen1dcells") == 3 and inspect.getsource(screen._Spec.launch).count("load_screen1dcells") == 2
    assert "rows" not in inspect.signature(screen.screen).parameters
    assert inspect.signature(screen.screen_cells).parameters["rows"].default is False
    assert inspect.signature(screen.ScreenCells.add_slab).parameters["rows"].default is False


def test_screen1dcells_cropped_levels_are_padded_with_nan_in_both_layouts():
    from cp_pre_amd.screen import _pad_levels
    qc = torch.rand(3, 6, 14)
    for nt_fastest in (False, True):
        full = _pad_levels(qc, (8, 16), nt_fastest)
        assert tuple(full.shape) == (3, 8, 16) and full.dtype == qc.dtype
        assert torch.equal(full[:, 1:-1, 1:-1], qc)
        rim = torch.ones(8, 16, dtype=torch.bool)
        rim[1:-1, 1:-1] = False
        assert bool(torch.isnan(full[:, rim]).all())
        assert (full.stride(1) == 1 and full.stride(2) == 8) if nt_fastest else full.is_contiguous()      # memory [nk,Nx,Nt]


# ------------------------------------------------------------------ the ABI
def test_screen1dcells_library_exports_exactly_its_symbols_and_the_sample_group():
    from cp_pre_amd import _lib, screen
    so = _lib.SCREEN1DCELLS_SO_PATH
    assert os.path.exists(so), "libcp_pre_screen1dcells.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and len(DECLARED) == 6
    assert exported == declared and set(_lib.SCREEN1DCELLS_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREEN1DCELLS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREEN1DCELLS_ABI_VERSION == 1
    lib = _lib.load_screen1dcells()
    assert lib.pre_screen1dcells_abi_version() == 1
    G = lib.pre_screen1dcells_sample_group()
    assert G >= 1 and screen.sample_group_rows() == G
    assert "screen1dcells" in _lib._LIBS_MORE and "screen1dcells" not in _lib._LIBS and len(_lib._LIBS) == 8
    # the twins' arguments, with the per-cell descriptor in the place of pre_screen_t
    for name, tw in (("stencil2d", _lib.SCREEN1D_SIGNATURES["pre_screen1d_stencil2d_f32"]),
                     ("burgers", _lib.SCREEN1D_SIGNATURES["pre_screen1d_burgers_f32"]),
                     ("pair_stencil2d", _lib.SCREEN1DPAIR_SIGNATURES["pre_screen1dpair_stencil2d_f32"]),
                     ("pair_burgers", _lib.SCREEN1DPAIR_SIGNATURES["pre_screen1dpair_burgers_f32"])):
        sig = _lib.SCREEN1DCELLS_SIGNATURES["pre_screen1dcells_%s_f32" % name]
        assert len(sig) == len(tw)
        diff = [i for i, (a, b) in enumerate(zip(sig, tw)) if a is not b]
        assert len(diff) == 1 and sig[diff[0]] is ctypes.POINTER(_lib.PreScreen1dCells) and tw[diff[0]] is ctypes.POINTER(_lib.PreScreen), name
        # the header's arity
        decl = re.search(r"int\s+pre_screen1dcells_%s_f32\s*\(([^;]*)\);" % name, header).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == len(sig), name


def test_screen1dcells_descriptor_has_the_header_layout(tmp_path):
    """sizeof / offsetof of the descriptor in C against the ctypes structure"""
    from cp_pre_amd import _lib
    t, st = "pre_screen1dcells_t", _lib.PreScreen1dCells
    body = 'printf("%%zu", sizeof(%s)); %s printf("\\n");\n' % (t, " ".join('printf(" %%zu", offsetof(%s, %s));' % (t, f) for f in FIELDS))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cp_pre_screen1dcells.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, *offs = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [f for f, _ in st._fields_] == FIELDS
    assert int(size) == ctypes.sizeof(st) and [int(o) for o in offs] == [getattr(st, f).offset for f in FIELDS]


def test_screen1dcells_header_and_c_client_compile_and_link(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "screen1dcells_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    exe = tmp_path / "screen1dcells_check"
    subprocess.check_call(c_client_command(exe))
    assert obj.exists() and exe.exists()


def test_screen1dcells_entry_points_refuse_before_any_launch():
    """the host checks of the entries need no device: null pointers, ranges, shapes, layouts, in the twins' order"""
    from cp_pre_amd import _lib
    lib = _lib.load_screen1dcells()
    B, T, X = 3, 8, 16
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    sx, st_ = _lib.iarr64((T * X, X, 1)), _lib.iarr64((T * X, 1, T))
    tw, off = _lib.farr([1.0, 2.0]), (ctypes.c_int32 * 4)(0, 0, 0, 1)
    K = _lib.farr([0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])

    def desc(**kw):
        d = dict(levels=p, nk=4, lK=T * X, lT=X, lX=1, modulation=None, mT=0, mX=0, ct=1, cx=1, score=p, count=p, count_ld=B)
        d.update(kw)
        return ctypes.byref(_lib.PreScreen1dCells(*[d[f] for f in FIELDS]))

    def st2(u=p, s=sx, d=None, Tn=T, Xn=X, flags=0, n=2):
        return lib.pre_screen1dcells_stencil2d_f32(u, s, tw, off, n, d or desc(), B, Tn, Xn, flags, None)

    def bgp(a=p, sa=sx, b=p, sb=sx, d=None, flags=0):
        return lib.pre_screen1dcells_pair_burgers_f32(a, sa, b, sb, K, K, K, 0.1, 0.1, 0.1, 1.0, d or desc(), B, T, X, flags, None)

    assert st2(u=None) == _lib.PRE_E_NULL and st2(n=-1) == _lib.PRE_E_NULL and st2(Tn=0) == _lib.PRE_E_NULL
    assert st2(d=desc(levels=None)) == _lib.PRE_E_NULL and st2(d=desc(score=None)) == _lib.PRE_E_NULL
    assert st2(d=desc(count_ld=B - 1)) == _lib.PRE_E_NULL
    assert st2(d=desc(nk=0)) == _lib.PRE_E_RANGE and st2(d=desc(nk=17)) == _lib.PRE_E_RANGE and st2(d=desc(ct=-1)) == _lib.PRE_E_RANGE
    assert st2(n=50) == _lib.PRE_E_SHAPE
    assert st2(flags=_lib.PRE_FLAG_HALO_X) == _lib.PRE_E_UNSUPPORTED
    assert st2(Xn=X - 2) == _lib.PRE_E_UNSUPPORTED                                   # a contiguous axis that is no multiple of 4
    assert st2(s=_lib.iarr64((T * X, 2 * X, 2))) == _lib.PRE_E_UNSUPPORTED           # no unit-stride axis
    assert st2(d=desc(modulation=p, mT=1, mX=T)) == _lib.PRE_E_UNSUPPORTED           # the modulation on the other axis
    assert st2(d=desc(lT=1, lX=T)) == _lib.PRE_E_UNSUPPORTED                         # the levels on the other axis
    assert st2(s=st_, d=desc(lT=X, lX=1)) == _lib.PRE_E_UNSUPPORTED
    assert st2(d=desc(lX=2)) == _lib.PRE_E_UNSUPPORTED
    assert st2(d=desc(lK=-1)) == _lib.PRE_E_SHAPE and st2(d=desc(lT=-X)) == _lib.PRE_E_SHAPE
    # the order: a null pointer before a range, a range before a layout, the fields' layout before the levels'
    assert st2(u=None, d=desc(nk=17, lX=2)) == _lib.PRE_E_NULL and st2(d=desc(nk=17, lX=2)) == _lib.PRE_E_RANGE
    assert st2(Xn=X - 2, d=desc(lK=-1)) == _lib.PRE_E_UNSUPPORTED
    assert bgp(b=None) == _lib.PRE_E_NULL and bgp(sb=None) == _lib.PRE_E_NULL
    assert bgp(sb=st_) == _lib.PRE_E_UNSUPPORTED and bgp(sa=st_, sb=st_) == _lib.PRE_E_UNSUPPORTED      # (levels Nx-fastest)
    assert bgp(d=desc(lK=-1)) == _lib.PRE_E_SHAPE
    assert lib.pre_screen1dcells_burgers_f32(p, sx, K, None, K, 0.1, 0.1, 0.1, 1.0, desc(), B, T, X, 0, None) == _lib.PRE_E_NULL
    corner = _lib.farr([1.0] + [0.0] * 8)
    assert lib.pre_screen1dcells_burgers_f32(p, sx, K, corner, K, 0.1, 0.1, 0.1, 1.0, desc(), B, T, X, 0, None) == _lib.PRE_E_UNSUPPORTED
    assert lib.pre_screen1dcells_pair_stencil2d_f32(p, sx, p, sx, tw, (ctypes.c_int32 * 4)(0, 0, 1, 1), 2, desc(), B, T, X, 0, None) == \
        _lib.PRE_E_UNSUPPORTED


# ------------------------------------------------------------------ the build and the source
def test_screen1dcells_makefile_and_source_facts():
    csrc = os.path.join(ROOT, "cp_pre_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^LIBS\s+:=.*\bscreen1dcells\b", mk, flags=re.M)
    assert re.search(r"^screen1dcells_OBJS\s+:= screen_rows_cells\.o screen_rows_cells_nc\.o", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS\s+:=(.|\\\n)*\$\(screen1dcells_OBJS\)", mk, flags=re.M)
    assert "$(screen1dcells_OBJS): $(INC)/cp_pre_screen1dcells.h $(INC)/cp_pre_screen.h" in mk
    assert "screen_rows_cells.o: FLAGS += -DPRE_SCREEN1DCELLS_PART=1\n" in mk
    assert "screen_rows_cells_nc.o: FLAGS += -DPRE_SCREEN1DCELLS_PART=2 -ffp-contract=off\n" in mk
    assert "ifdef SCREEN1DCELLS_GROUP\nscreen_rows_cells.o screen_rows_cells_nc.o: FLAGS += -DPRE_SCREEN1DCELLS_GROUP=$(SCREEN1DCELLS_GROUP)\nendif" in mk
    src = open(os.path.join(csrc, "screen_rows_cells.hip")).read()
    assert "__global__" not in src                                   # the march is not copied
    assert '#include "screen_rows.h"' in src and '#include "paired_functor.h"' in src
    assert src.count("prepare_rows(") == 1 and src.count("prepare_rows_cells(") == 5      # the host checks stated once
    rows = open(os.path.join(csrc, "screen_rows.h")).read()
    assert rows.count("__global__") == 1 and "template <class Fn, class Sets = ScalarSets>" in rows
    assert "#define PRE_SCREEN1DCELLS_GROUP 16" in rows
    assert "screen_plane_score(" in rows and "screen_plane_count<LB>(" in rows
    # every row step evaluates the functor through RowsFn (the stated operation order of Burgers<3>), and nothing else does
    assert rows.count("RowsFn<Fn>::eval(n, prm)") == 1 and "Fn::eval(n, prm)" not in rows.replace("RowsFn<Fn>::eval(n, prm)", "")
    assert "struct RowsFn<Burgers<3>>" in rows and rows.count("struct RowsFn<") == 1
    for f in ("screen_rows.hip", "screen_rows_pair.hip"):            # the joint screens do not name the policy: its default
        assert "CellSets" not in open(os.path.join(csrc, f)).read()
    for f in ("resources.txt", "resources_existing_parent.txt", "resources_existing_head.txt"):
        assert os.path.exists(os.path.join(ROOT, "profiles", "screen1dcells", f)), f
    before = open(os.path.join(ROOT, "profiles", "screen1dcells", "resources_existing_parent.txt")).read()
    after = open(os.path.join(ROOT, "profiles", "screen1dcells", "resources_existing_head.txt")).read()
    figures = lambda s: [ln.split("void")[0].split() for ln in s.splitlines() if "screen_rows_kernel" in ln]
    assert figures(before) == figures(after) and len(figures(before)) == 8
    built = [ln for ln in open(os.path.join(ROOT, "profiles", "screen1dcells", "resources.txt")).read().splitlines() if "screen_rows_kernel" in ln]
    assert len(built) == 8 and all("scratch=0 " in ln and re.search(r"spill=\s", ln) for ln in built)


# ------------------------------------------------------------------ the block order
@pytest.mark.parametrize("plane", [(12, 64), (130, 12), (9, 1028), (40, 516)])
def test_screen1dcells_block_order_visits_every_workgroup_once(plane):
    """the decode of screen_rows_kernel under CellSets, restated: sample of a group fastest, then column tile, chunk, group"""
    from cp_pre_amd import screen
    G = screen.sample_group_rows()
    for Gs in sorted({G, 1, 2, 8, 16}):
        for B in sorted({1, max(Gs - 1, 1), Gs, Gs + 1, 2 * Gs - 1}):
            got, sp = h.visits(B, *plane, Gs)
            live = [v for v in got if v is not None]
            want = {(b, ch, ct) for b in range(B) for ch in range(sp["nChunk"]) for ct in range(sp["nCT"])}
            assert len(live) == len(want) and set(live) == want, (plane, Gs, B)
            assert len(got) - len(live) == ((B + Gs - 1) // Gs * Gs - B) * sp["nChunk"] * sp["nCT"]
            assert sp == s1.split(B, *plane)                          # rows_split does not know of the group
            # the workgroups that are contiguous in the logical order share their (chunk, tile): one set of level quads
            for i in range(0, len(got), Gs):
                assert len({v[1:] for v in got[i:i + Gs] if v is not None}) <= 1
