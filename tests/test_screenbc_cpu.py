"""CPU tests of the screens and statistics under boundary conditions on the x-y rim (``bc=`` of cp_pre_amd.screen,
libcp_pre_screenbc.so):
  * the conditions every GPU case must meet, on the float64 reference alone (tests/screenbc_helpers.py);
  * the keyword's errors, the crop rule, every fallback reason in its order, the gate with and without the keyword;
  * a keyword-less call on a ``bc`` object maps no libcp_pre_screenbc.so;
  * the exported ABI against include/cp_pre_screenbc.h and the ctypes binding, the Makefile rows, a C99 client;
  * every error return of every entry, decided on unmapped addresses, and the host-only workspace query."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import bcres_helpers as bh
import screenbc_helpers as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screenbc.h")
KINDS4 = ("stencil3d", "linear2", "ns_momentum", "mhd")
DECLARED = {"pre_screenbc_abi_version", "pre_screenbc_stats_workspace_len"} | \
    {"pre_screenbc_" + s + k + "_f32" for s in ("", "stats_") for k in KINDS4}


def c_client_command(exe):
    return ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
            os.path.join(ROOT, "tests", "c_abi", "screenbc_check.c"), "-I" + os.path.join(ROOT, "include"),
            "-I/opt/rocm/include", "-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screenbc.so",
            "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm",
            "-o", str(exe)]


def method(kind, cond=None, **kw):
    obj, name = bh.module(kind, cond, **kw)
    return getattr(obj, name)


# ------------------------------------------------------------------ the conditions of the GPU cases, on the reference alone
def test_every_gpu_case_meets_the_conditions_on_the_reference_alone():
    worst_share, worst_dist, missed = 0.0, float("inf"), []
    for key in sb.gpu_cases():
        c = sb.case(*key)
        ok, text = c.conditions()
        share, dist, _ = c.caps()
        worst_share, worst_dist = max(worst_share, share), min(worst_dist, dist)
        if not ok:
            missed.append(text)
    print(f"{len(sb.gpu_cases())} cases: worst undecided share {worst_share:.4f}, smallest distance {worst_dist:.2f} tau / m_min")
    assert not missed, missed


def test_the_reference_is_the_padded_zero_pad_residual():
    """``Case.r_ref`` is r_zero_pad(pad(f))[..., 1:-1, 1:-1]: equal to the zero-pad oracle wherever the star stays inside the
    grid, different on the rim (else the bc cases would show nothing the zero-pad screens do not)."""
    c = sb.case("ns_momentum", (3, 3, 9, 8), "wrap", (1, 0, 0))
    zero = bh.residual64("ns_momentum", c.x.double(), {s: ("dirichlet", 0.0) for s in bh.SIDES})
    assert torch.equal(c.r_ref[..., 1:-1, 1:-1], zero[..., 1:-1, 1:-1])
    assert float((c.r_ref - zero)[..., 0, :].abs().max()) > 100 * c.tau and float((c.r_ref - zero)[..., :, -1].abs().max()) > 100 * c.tau


# ------------------------------------------------------------------ the keyword
def test_bc_keyword_errors_are_raised_before_any_device_work():
    from cp_pre_amd import screen
    from cp_pre_amd.convops_2d import ConvOperator
    x = sb.fields("ns_momentum", (2, 3, 5, 8))
    q = torch.ones(1)
    with pytest.raises(TypeError, match="built without bc="):
        screen.screen(method("ns_momentum"), x, q, bc=True)
    with pytest.raises(TypeError, match="built without bc="):
        screen.screen_stats(method("wave"), x[:, 0], bc=True)
    with pytest.raises(TypeError, match="bare ConvOperator"):
        screen.screen(method("ns_momentum", "wrap"), x, q, bc="wrap")
    with pytest.raises(TypeError, match="bare ConvOperator"):
        screen._Spec(method("mhd_induction", "periodic"), bc={"left": "neumann"})
    lap = ConvOperator(("x", "y"), 2)
    with pytest.raises(TypeError, match="bc=True takes a bound"):
        screen.screen(lap, x[:, 0], q, bc=True)
    with pytest.raises(TypeError, match="bc must be"):
        screen.screen(lap, x[:, 0], q, bc=3.5)
    import screenjorek_helpers as sj
    for kw in (dict(bc=True), dict(jorek=True, bc=True), dict(bc="wrap")):
        with pytest.raises(TypeError, match="JOREK"):
            screen._Spec(sj.method_of("jorek_continuity"), **kw)
    # halo_x with bc raises as the residuals do, whatever the route would have been
    for args in ((screen.Screen(2, 1, "cpu"), (method("ns_momentum", "wrap"), x, q)), (screen.ScreenStats(2, "cpu"), (method("ns_momentum", "wrap"), x))):
        with pytest.raises(ValueError, match="bc with halo_x=True"):
            args[0].add_slab(*args[1], crop=(1, 0, 0), halo_x=True, bc=True)
    # per-cell sets are out of scope: a spec made with bc= is refused there
    with pytest.raises(TypeError, match="per-cell sets"):
        screen.ScreenCells(2, 1, "cpu").add_slab(screen._Spec(method("ns_momentum", "wrap"), bc=True), x, torch.ones(1, 3, 5, 8))
    # without the keyword nothing changed: False and None are "not asked for"
    assert screen._Spec(method("ns_momentum", "wrap")).bc is None and screen._Spec(lap, bc=False).bc is None


def test_the_gate_with_and_without_the_keyword():
    from cp_pre_amd import screen
    v = bh.make_vars((2, 3, 4, 8, 8), seed=13)
    m = method("ns_momentum", "wrap")
    assert screen._Spec(m).declined(v).startswith("bc=")
    assert screen._Spec(m, bc=True).declined(v) is None
    assert screen._Spec(m, bc=True).bc is m.__self__.bc                 # the object's own condition, held and not copied


def test_crop_rule_of_screen_and_screen_stats(monkeypatch):
    """With ``bc`` set ``boundary=False`` counts crop (1, 0, 0), ``boundary=True`` every cell; without it (1, 1, 1) as before.
    The stored residual is the reference's, so the counts say which cells were counted."""
    from cp_pre_amd import screen
    c = sb.case("ns_momentum", (3, 5, 9, 8), "mixed", (1, 0, 0))
    stored = c.r_ref.float()
    monkeypatch.setattr(screen._Spec, "full", lambda self, v, minus, halo_x: stored)
    seen = []

    def fallback(self, spec, vars, qhats, modulation, crop, halo_x, minus):      # (the three passes need a device: the crop is recorded)
        seen.append(crop)
        self._buffers(vars.device)
    monkeypatch.setattr(screen.Screen, "_fallback", fallback)
    big = torch.full((1,), 1e30)
    B, T, X, Y = c.shape
    for kw, crop, cells in ((dict(bc=True), (1, 0, 0), (T - 2) * X * Y), (dict(bc=True, boundary=True), (0, 0, 0), T * X * Y),
                            (dict(), (1, 1, 1), (T - 2) * (X - 2) * (Y - 2)), (dict(boundary=True), (0, 0, 0), T * X * Y)):
        m = method("ns_momentum", c.bc)
        why = "fallback:input on the CPU"                     # (the input's reasons come first, with and without the keyword)
        s = screen.screen(m, c.x, big, **kw)
        assert s.cells == cells and seen[-1] == crop and screen.last_route() == why, (kw, s.cells, seen[-1])
        st = screen.screen_stats(m, c.x, **kw)
        assert st.cells == cells and screen.last_route() == why
        # the statistics of exactly that region of the stored residual
        reg = stored[(slice(None),) + tuple(slice(k, n - k) for k, n in zip(crop, stored.shape[1:]))].double().flatten(1)
        assert torch.equal(st.sum_abs, reg.abs().sum(dim=1)) and torch.equal(st.max_abs, reg.abs().max(dim=1).values.float())
    # the modulation keeps the uncropped extents
    screen.screen(method("ns_momentum", c.bc), c.x, c.q, c.mod, bc=True)
    with pytest.raises(ValueError, match="modulation has shape"):
        screen.screen(method("ns_momentum", c.bc), c.x, c.q, c.mod[1:-1], bc=True)
    # add_slab keeps its explicit crop
    acc = screen.Screen(3, 1, "cpu")
    acc.add_slab(method("ns_momentum", c.bc), c.x, big, crop=(0, 2, 1), bc=True)
    assert acc.finish().cells == T * (X - 4) * (Y - 2) and seen[-1] == (0, 2, 1)
    st = screen.ScreenStats(3, "cpu")
    st.add_slab(method("ns_momentum", c.bc), c.x, crop=(0, 2, 1), bc=True)
    assert st.finish().cells == T * (X - 4) * (Y - 2)


class OnDevice:
    """Stands in for a device tensor in ``_Spec.prepare``: the reasons are decided on the host, from shape, strides and
    ``is_cuda`` alone."""

    def __init__(self, t):
        self.t, self.is_cuda, self.shape, self.dtype = t, True, t.shape, t.dtype

    def dim(self):
        return self.t.dim()

    def stride(self, *a):
        return self.t.stride(*a)

    def __getitem__(self, i):
        return OnDevice(self.t[i])

    def permute(self, *a):
        return OnDevice(self.t.permute(*a))


def test_every_fallback_reason_in_its_order():
    """Each reason with everything after it in the order ALSO wrong: the earlier one is the one named."""
    from cp_pre_amd import residuals as R, screen
    from cp_pre_amd.convops_2d import ConvOperator
    q32, q64 = torch.ones(1), torch.ones(1, dtype=torch.float64)
    x = sb.fields("ns_momentum", (2, 3, 5, 8))

    def why(spec, v, minus=None, q=q32):
        return spec.prepare(v, minus, q, None)[0]
    per_field = ["periodic", "neumann", "periodic"]
    grad = method("ns_momentum", per_field, fused=False)
    grad.__self__.D_t.kernel.requires_grad_(True)
    odd = x[..., :6]                                            # Ny % 4 != 0
    ntf = x.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)[..., :6]      # Nt-fastest, and a ragged width
    # 1. the input's reasons, each before everything else
    s = screen._Spec(grad, bc=True)
    assert why(s, odd, minus=odd) == "minus="
    assert why(s, odd) == "input on the CPU"
    assert why(s, OnDevice(odd), q=q64) == "float64 levels or modulation"
    # 2. the 1-D family (an object with bc, and a bare 1-D operator with a condition)
    bur = screen._Spec(method("burgers", "periodic", fused=False), bc=True)
    assert why(bur, OnDevice(bh.make_vars((2, 5, 6)))) == "no fused screen under bc for the 1-D family"
    from cp_pre_amd.convops_1d import ConvOperator as Conv1
    assert why(screen._Spec(Conv1(("t", "x"), 1), bc="wrap"), OnDevice(bh.make_vars((2, 5, 6)))) == \
        "no fused screen under bc for the 1-D family"
    # 3. an Nt-fastest view, 4. the layout, 5. fused=False, 6. the condition, 7. the kernels
    assert why(s, OnDevice(ntf)) == "Nt-fastest view: the merged-row march has no BC form"
    assert why(s, OnDevice(odd)) == "row width not a multiple of 4"
    assert why(s, OnDevice(x[..., ::2])) == "no unit stride on the last axis"
    assert why(s, OnDevice(x)) == "fused=False"
    grad.__self__.fused = True
    assert why(s, OnDevice(x)) == "per-field boundary conditions"
    m = method("ns_momentum", bh.MIXED_INEXPRESSIBLE)
    m.__self__.D_t.kernel.requires_grad_(True)
    assert why(screen._Spec(m, bc=True), OnDevice(x)) == "mixed condition without a fused mapping"
    # 'free_slip' has no padding rule: the residual under it has not the field's extents, so the keyword raises before any
    # device work, whatever else would decline (without the keyword such an object keeps the route it had)
    slip = method("ns_momentum", {"left": "free_slip"}, fused=False)
    for v in (odd, OnDevice(x)):
        with pytest.raises(ValueError, match="free_slip"):
            why(screen._Spec(slip, bc=True), v)
    with pytest.raises(ValueError, match="free_slip"):
        screen.screen_stats(method("ns_momentum", "free_slip"), x, bc=True)
    # ... in any member of a per-field list too (whose reason would otherwise be "per-field boundary conditions")
    for cond in (["free_slip"] * 3, ["periodic", {"bottom": "free_slip"}, "periodic"]):
        with pytest.raises(ValueError, match="free_slip"):
            screen.screen_stats(method("ns_momentum", cond), x, bc=True)
        with pytest.raises(ValueError, match="free_slip"):
            why(screen._Spec(method("ns_momentum", cond), bc=True), OnDevice(x))
    from cp_pre_amd import residuals as R
    assert not R._BC("wrap").free_slip() and not R._BC(["periodic", "neumann"]).free_slip() and R._BC({"top": "free_slip"}).free_slip()
    assert not R._BC({"top": "free_slip"}).free_slip(2) and R._BC({"right": "free_slip"}).free_slip(2)     # (the 1-D family pads left / right)
    with pytest.raises(ValueError, match="free_slip"):
        screen.screen(method("ns_momentum", "free_slip"), x, q32, bc=True)
    assert screen._Spec(slip).declined(x) == "fused=False"
    m = method("ns_momentum", "wrap")
    m.__self__.D_t.kernel.requires_grad_(True)
    assert why(screen._Spec(m, bc=True), OnDevice(x)) == "operator kernel requires grad"
    m = method("ns_momentum", "wrap")
    m.__self__.D_x.kernel.data[0, 0, 0] = 0.5
    assert why(screen._Spec(m, bc=True), OnDevice(x)) == "operator kernel off the 7-point star"
    lap = ConvOperator(("x", "y"), 2)
    lap.kernel.data[0, 0, 0] = 0.5
    assert why(screen._Spec(lap, bc="symmetric"), OnDevice(x[:, 0])) == "operator kernel off the 7-point star"
    # nothing declines: the kernels come back (8., ``declined by the library``, is the library's answer: the GPU tests)
    w, ks = screen._Spec(method("ns_momentum", bh.MIXED), bc=True).prepare(OnDevice(x), None, q32, None)
    assert w is None and len(ks) == 4
    assert why(screen._Spec(method("mhd_energy", "wrap"), bc=True), OnDevice(x)) == "fewer than six MHD channels"
    # routes and entries
    for kind, route, entry in (("wave", "stencil3d", "stencil3d"), ("ns_continuity", "linear2", "linear2"), ("mhd_gauss", "linear2", "linear2"),
                               ("ns_momentum", "ns_momentum", "ns_momentum"), ("mhd_energy", "mhd_energy", "mhd")):
        sp = screen._Spec(method(kind, "wrap"), bc=True)
        assert sp.route("") == "fused:bc_" + route and sp.route("", stats=True) == "fused:bc_stats_" + route
        assert sp.entry("") == "pre_screenbc_%s_f32" % entry and sp.entry("", stats=True) == "pre_screenbc_stats_%s_f32" % entry
    assert screen._Spec(method("ns_momentum", "wrap")).route("") == "fused:ns_momentum"


def test_fallback_on_the_cpu_is_the_reductions_of_the_bc_residual():
    """No device: ``fallback:input on the CPU`` and the statistics of the bc residual - the object's own composed pass with
    torch operators - against the fp64 reference.  (The three passes of ``Screen`` need a device: the GPU tests.)"""
    from cp_pre_amd import screen
    from cp_pre_amd.convops_2d import ConvOperator
    for kind, cond in (("ns_momentum", "mixed"), ("wave", "symmetric"), ("mhd_induction", "wrap")):
        c = sb.case(kind, (3, 5, 9, 8), cond, (1, 0, 0))
        obj, name = bh.module(kind, c.bc)
        m = getattr(bh.with_torch_ops(obj), name)
        st = screen.screen_stats(m, sb.package_input(kind, c.x), bc=True)
        assert screen.last_route() == "fallback:input on the CPU" and st.cells == c.cells
        tol = sb.stats_tolerances(c)
        assert bool(((st.max_abs.double() - c.ref["max_abs"]).abs() <= tol["max_abs"]).all())
        assert bool(((st.mean() - c.ref["sum"] / c.cells).abs() <= tol["mean"]).all())
        assert bool(((st.mean_abs() - c.ref["sum_abs"] / c.cells).abs() <= tol["mean_abs"]).all())
        assert bool(((st.mean_sq() - c.ref["sum_sq"] / c.cells).abs() <= tol["mean_sq"]).all())
    spec = screen._Spec(ConvOperator(("x", "y"), 2), bc="symmetric")
    assert spec.bc is not None and spec.kind == "stencil3d" and spec.route("") == "fused:bc_stencil3d"


def test_keyword_less_call_on_a_bc_object_maps_no_new_library():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import torch, bcres_helpers as H, screenbc_helpers as sb\n"
            "from cp_pre_amd import screen, _lib\n"
            "obj, name = H.module('ns_momentum', 'periodic'); m = getattr(H.with_torch_ops(obj), name)\n"
            "x = sb.fields('ns_momentum', (2, 3, 5, 8))\n"
            "assert screen._Spec(m).prepare(x, None, torch.ones(2), None)[0] == 'input on the CPU'\n"
            "assert screen._Spec(m).declined(x).startswith('bc= (')\n"
            "screen.screen_stats(m, x); assert screen.last_route() == 'fallback:input on the CPU', screen.last_route()\n"
            "assert _lib._screenbc is None and 'libcp_pre_screenbc' not in open('/proc/self/maps').read()\n"
            "print('unloaded')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("unloaded"), r.stdout + r.stderr


# ------------------------------------------------------------------ the ABI
def test_screenbc_library_exports_exactly_the_headers_entries():
    from cp_pre_amd import _lib
    so = _lib.SCREENBC_SO_PATH
    assert os.path.exists(so), "libcp_pre_screenbc.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^(?:int|int64_t)\s+(pre_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    declared = {n for n, _ in found}
    assert declared == DECLARED and len(DECLARED) == 10
    assert exported == declared and set(_lib.SCREENBC_SIGNATURES) == declared
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREENBC_SIGNATURES[name]), name
    # each entry is its zero-pad twin with a pre_bc_t before the extents
    for k in KINDS4:
        for mine, twin in (("pre_screenbc_%s_f32" % k, _lib.SCREEN_SIGNATURES["pre_screen_%s_f32" % k]),
                           ("pre_screenbc_stats_%s_f32" % k, _lib.SCREENSTATS_SIGNATURES["pre_screenstats_%s_f32" % k])):
            sig = _lib.SCREENBC_SIGNATURES[mine]
            assert sig[:-7] + sig[-6:] == twin and sig[-7] is ctypes.POINTER(_lib.PreBC), mine
    assert int(re.search(r"#define\s+PRE_SCREENBC_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREENBC_ABI_VERSION == 1
    lib = _lib.load_screenbc()
    assert lib.pre_screenbc_abi_version() == _lib.PRE_SCREENBC_ABI_VERSION and lib is _lib._load("screenbc")
    assert "screenbc" in _lib._LIBS_MORE and "screenbc" not in _lib._LIBS and len(_lib._LIBS) == 8
    mk = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "Makefile")).read()
    assert re.search(r"^screenbc_OBJS\s+:= screen_bc\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bscreenbc\b", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS :=(.*\\\n)*.*\$\(screenbc_OBJS\)", mk, flags=re.M)
    assert re.search(r"^\$\(screenbc_OBJS\):.*cp_pre_screenbc\.h", mk, flags=re.M)


def test_screenbc_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    exe = tmp_path / "screenbc_check"
    subprocess.check_call(c_client_command(exe))
    assert exe.exists()


def test_workspace_query_is_host_only():
    from cp_pre_amd import _lib
    q = _lib.load_screenbc().pre_screenbc_stats_workspace_len
    twin = _lib.load_screenstats().pre_screenstats_workspace_len
    assert q(0, 4, 4, 4) == 0 and q(3, 4, 4, 0) == 0 and q(3, 4, 2 ** 31, 4) == 0
    for key in sb.seam_cases("wave"):
        B, T, X, Y = key[1]
        NR, W = (8, 256) if Y >= 192 else (16, 128) if Y >= 96 else (32, 64)
        assert q(B, T, X, Y) == 3 * B * -(-X // NR) * -(-Y // W) * -(-T // 8) == twin(0, B, T, X, Y)


# ------------------------------------------------------------------ every refusal, before any device work
F0, Q0, S0, C0, W0 = 0x10000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000      # (not mapped)
STAR = [0.0] * 27
STAR[13] = 1.0
BOX = list(STAR)
BOX[0] = 0.5
GEN = list(STAR)
GEN[4] = GEN[10] = GEN[12] = 1.0


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("kind", KINDS4)
def test_refusals_are_decided_before_any_device_work(kind, stats):
    """The addresses are not mapped: a refusal that reached a launch, or a kernel, could not return its code here."""
    from cp_pre_amd import _lib
    lib = _lib.load_screenbc()
    fn = getattr(lib, "pre_screenbc_%s%s_f32" % ("stats_" if stats else "", kind))
    B, T, X, Y = 2, 6, 5, 12

    def call(null_view=False, kernels=None, taps=([1.0], [0, 0, 0], 1), eq=0, desc=None, no_desc=False, bc=(2, 2, 0, 3), no_bc=False,
             shape=(B, T, X, Y), flags=0, sx=None, sy=1, ws_len=None, sums=W0):
        b, t, x, y = shape
        views = (_lib.PreField * 6)(*[_lib.PreField(None if null_view and i == 0 else F0 + i * 0x01000000, t * x * y, x * y,
                                                    y if sx is None else sx, sy) for i in range(6)])
        nker = {"linear2": 2, "ns_momentum": 4, "mhd": 3}.get(kind, 0)
        ks = [None if k is None else _lib.farr(k) for k in (kernels or [STAR] * nker)]
        if kind == "stencil3d":
            w, off, n = taps
            head = [ctypes.byref(views[0]), None if w is None else _lib.farr(w), None if off is None else _lib.iarr32(off), n]
        elif kind == "linear2":
            head = [ctypes.byref(views[0]), ctypes.byref(views[1]), *ks, 1.5]
        elif kind == "ns_momentum":
            head = [ctypes.byref(views[i]) for i in range(3)] + ks + [0.01, 0.02, 0.03, 0.001]
        else:
            head = [eq, views, *ks, 5 / 3]
        if stats:
            need = lib.pre_screenbc_stats_workspace_len(b, t, x, y)
            d = dict(ct=1, cx=0, cy=0, max_abs=S0, sums=sums, sum_ld=b, workspace=W0, workspace_len=need if ws_len is None else ws_len)
            d.update(desc or {})
            d = _lib.PreScreenStats(**d)
        else:
            d = dict(q=Q0, nk=3, modulation=None, mT=0, mX=0, ct=1, cx=0, cy=0, score=S0, count=C0, count_ld=b)
            d.update(desc or {})
            d = _lib.PreScreen(**d)
        bcs = _lib.PreBC((ctypes.c_int * 4)(*bc), (ctypes.c_float * 4)(0, 0, 2.5, 0))
        return fn(*head, None if no_desc else ctypes.byref(d), None if no_bc else ctypes.byref(bcs), *shape, flags, None)

    E = _lib
    # PRE_E_NULL: nulls, bc included
    assert call(no_bc=True) == E.PRE_E_NULL and call(no_desc=True) == E.PRE_E_NULL and call(null_view=True) == E.PRE_E_NULL
    assert call(shape=(0, T, X, Y)) == E.PRE_E_NULL and call(shape=(B, T, X, 0)) == E.PRE_E_NULL
    if kind == "stencil3d":
        assert call(taps=(None, [0, 0, 0], 1)) == E.PRE_E_NULL and call(taps=([1.0], None, 1)) == E.PRE_E_NULL
    else:
        n = {"linear2": 2, "ns_momentum": 4, "mhd": 3}[kind]
        assert call(kernels=[STAR] * (n - 1) + [None]) == E.PRE_E_NULL
    if stats:
        assert call(ws_len=0) == E.PRE_E_NULL and call(sums=None) == E.PRE_E_NULL and call(desc=dict(sum_ld=B - 1)) == E.PRE_E_NULL
        assert call(desc=dict(workspace=None)) == E.PRE_E_NULL
    else:
        assert call(desc=dict(q=None)) == E.PRE_E_NULL and call(desc=dict(count_ld=B - 1)) == E.PRE_E_NULL
    # PRE_E_RANGE: an unknown mode, X < 2 / Y < 2 under a PRE_BC_REFLECT side, eq, 32-bit offsets, a negative crop
    assert call(bc=(2, 9, 0, 3)) == E.PRE_E_RANGE and call(bc=(-1, 2, 0, 3)) == E.PRE_E_RANGE
    assert call(shape=(B, T, 1, Y)) == E.PRE_E_RANGE                                  # X < 2 under a reflecting bottom
    # (Y < 2 under a reflecting side cannot be reached through the ABI: Y % 4 != 0 is refused first, and Y = 4 reflects)
    assert call(sx=2 ** 30) == E.PRE_E_RANGE
    assert call(desc=dict(ct=-1)) == E.PRE_E_RANGE
    if kind == "mhd":
        assert call(eq=4) == E.PRE_E_RANGE and call(eq=-1) == E.PRE_E_RANGE
    if not stats:
        assert call(desc=dict(nk=0)) == E.PRE_E_RANGE and call(desc=dict(nk=17)) == E.PRE_E_RANGE
    # PRE_E_UNSUPPORTED: Y % 4, no unit stride on Ny, PRE_FLAG_HALO_X, weight off the star, an unbuilt tap structure
    assert call(shape=(B, T, X, 10)) == E.PRE_E_UNSUPPORTED and call(sy=2) == E.PRE_E_UNSUPPORTED
    assert call(flags=E.PRE_FLAG_HALO_X) == E.PRE_E_UNSUPPORTED and call(flags=1 << 20) == E.PRE_E_UNSUPPORTED
    if kind == "stencil3d":
        assert call(taps=([1.0, 0.5], [0, 0, 0, 0, 1, 1], 2)) == E.PRE_E_UNSUPPORTED
    else:
        n = {"linear2": 2, "ns_momentum": 4, "mhd": 3}[kind]
        assert call(kernels=[STAR, BOX] + [STAR] * (n - 2)) == E.PRE_E_UNSUPPORTED
    if kind == "mhd":
        for eq in (1, 2):                                   # the general stars of momentum and energy: both policies
            assert call(eq=eq, kernels=[STAR, GEN, STAR]) == E.PRE_E_UNSUPPORTED
    # the order: a null before a range error before the layout
    assert call(no_bc=True, bc=(9, 9, 9, 9), shape=(B, T, X, 10)) == E.PRE_E_NULL
    assert call(desc=dict(ct=-1), shape=(B, T, X, 10), flags=E.PRE_FLAG_HALO_X) == E.PRE_E_RANGE
