"""CPU tests of the per-sample statistics (cp_pre_amd.screen.screen_stats / ScreenStats, libcp_pre_screenstats.so):
  * the exported ABI against include/cp_pre_screenstats.h and the ctypes binding, a C99 client, the host-only workspace query;
  * the fallback's float64 reductions of a stored residual against the float64 reference, with the route strings - the
    stored residual is the oracle's (no residual pass runs without a device; tests/test_gpu_screenstats*.py hold the same
    inputs against the package's own pass);
  * ``mean_abs()`` / ``order()`` against the scripts' own statement ``torch.sort(torch.mean(torch.abs(r), axis=...))``, and
    the signed form for Burgers, on inputs whose order the data decides;
  * every error raised before any device work;
  * importing ``cp_pre_amd.screen`` loads no library.
Reference and tolerances: tests/screenstats_helpers.py."""
import os
import re
import subprocess
import sys

import pytest
import torch

import screen1d_helpers as s1
import screen_helpers as sh
import screenjorek_helpers as sj
import screenstats_helpers as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screenstats.h")
DECLARED = {"pre_screenstats_abi_version", "pre_screenstats_workspace_len"} | \
    {"pre_screenstats_" + f + k + "_f32" for f in ("", "flat_") for k in ("stencil3d", "linear2", "ns_momentum", "mhd")} | \
    {"pre_screenstats_rows_" + k + "_f32" for k in ("stencil2d", "burgers")}


def c_client_command(exe):
    return ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
            os.path.join(ROOT, "tests", "c_abi", "screenstats_check.c"), "-I" + os.path.join(ROOT, "include"),
            "-I/opt/rocm/include", "-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screenstats.so",
            "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm",
            "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_screenstats_library_exports_exactly_the_headers_entries():
    from cp_pre_amd import _lib
    so = _lib.SCREENSTATS_SO_PATH
    assert os.path.exists(so), "libcp_pre_screenstats.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^(?:int|int64_t)\s+(pre_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    declared = {n for n, _ in found}
    assert declared == DECLARED and len(DECLARED) == 12
    assert exported == declared and set(_lib.SCREENSTATS_SIGNATURES) == declared
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREENSTATS_SIGNATURES[name]), name
    body = re.search(r"typedef struct \{(.*?)\} pre_screenstats_t;", header, flags=re.S).group(1)
    members = [re.sub(r".*[\s*]", "", part.strip()) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert members == [f[0] for f in _lib.PreScreenStats._fields_], members
    assert int(re.search(r"#define\s+PRE_SCREENSTATS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREENSTATS_ABI_VERSION
    lib = _lib.load_screenstats()
    assert lib.pre_screenstats_abi_version() == _lib.PRE_SCREENSTATS_ABI_VERSION and lib is _lib._load("screenstats")
    assert "screenstats" in _lib._LIBS_MORE and len(_lib._LIBS) == 8
    for form, name in ((0, "NY"), (1, "FLAT"), (2, "ROWS")):
        assert int(re.search(r"#define\s+PRE_SCREENSTATS_FORM_%s\s+(\d+)" % name, header).group(1)) == form
    assert _lib.PRE_SCREENSTATS_FORM == {"": 0, "flat": 1, "rows": 2}


def test_screenstats_workspace_query_is_host_only_and_bounds_every_split():
    """the query touches no device (it runs here) and is an upper bound of 3 x the workgroups of the splits that
    tests/screenflat_helpers.py and tests/screen1d_helpers.py restate, for any number of resident workgroups"""
    import screenflat_helpers as sf
    from cp_pre_amd import _lib
    q = _lib.load_screenstats().pre_screenstats_workspace_len
    assert q(0, 0, 4, 4, 4) == 0 and q(1, 3, 4, 4, 0) == 0 and q(7, 3, 4, 4, 4) == 0 and q(2, 3, 0, 4, 1) == 0
    for shape in list(sf.SEAM_SHAPES.values()) + [(800, 20, 256, 256)]:
        for staged in (False, True):
            for slots in (256, 512, 2048):
                sp = sf.split(shape, staged, slots)
                assert q(1, *shape) >= 3 * shape[0] * sp["nCh"] * sp["nTSeg"], (shape, staged, slots)
    for B, (R, C) in list(s1.SEAM_PLANES.values()) + [(8192, (200, 512))]:
        for slots in (256, 1024, 4096):
            sp = s1.split(B, R, C, slots)
            for T, X in ((R, C), (C, R)):
                assert q(2, B, T, X, 1) >= 3 * B * sp["nChunk"] * sp["nCT"], (B, R, C, slots)
    # Ny-fastest: the tiles of the march and marches of no fewer than min(T, 8) planes
    for (B, T, X, Y) in sh.SEAM_SHAPES.values():
        NR, W = (8, 256) if Y >= 192 else (16, 128) if Y >= 96 else (32, 64)
        assert q(0, B, T, X, Y) == 3 * B * -(-X // NR) * -(-Y // W) * -(-T // 8)


def test_screenstats_header_compiles_as_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", HEADER])


def test_screenstats_c_client_builds_and_links(tmp_path):
    exe = tmp_path / "screenstats_check"
    subprocess.check_call(c_client_command(exe))
    assert exe.exists()


def test_importing_the_screen_module_loads_no_library():
    code = ("import cp_pre_amd.screen as s, cp_pre_amd._lib as l\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libcp_pre_' not in maps, [ln for ln in maps.splitlines() if 'libcp_pre_' in ln]\n"
            "assert l._screenstats is None and callable(s.screen_stats)\n")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ------------------------------------------------------------------ the fallback's reductions and the route strings
def _cases():
    """(name, method, vars, float64 reference residual, route without a device)"""
    out = []
    for kind in ("wave", "ns_continuity", "ns_momentum", "mhd_induction"):
        c = st.ny_case(kind, sh.SEAM_SHAPES["two_tseg"])
        out.append((kind, sh.method_of(kind), c.x, c.r_ref, "fallback:input on the CPU"))
    x = sh.fields("ns_momentum", sh.SEAM_SHAPES["two_tseg"])
    out.append(("jorek", sj.method_of("jorek_continuity"), sj.to_vars(x), sj.oracle_residual("jorek_continuity", x.double()),
                "fallback:no fused stats for JOREK"))
    for kind in ("burgers", "advection"):
        c = st.rows_case(kind, 3, (12, 64), "nx")
        out.append((kind, s1.method_of(kind), c.x, c.r_ref, "fallback:input on the CPU"))
    return out


@pytest.mark.parametrize("boundary", [False, True])
def test_screenstats_fallback_reductions_against_fp64(monkeypatch, boundary):
    from cp_pre_amd import screen
    for name, method, x, r_ref, why in _cases():
        stored = r_ref.float()
        monkeypatch.setattr(screen._Spec, "full", lambda self, v, minus, halo_x, stored=stored: stored)
        got = screen.screen_stats(method, x, boundary=boundary)
        assert screen.last_route() == why, (name, screen.last_route())
        ref = st.Ref(r_ref, (0,) * (r_ref.dim() - 1) if boundary else (1,) * (r_ref.dim() - 1))
        st.check(got, ref, f"{name} boundary={boundary}")
        assert not got.sum.is_cuda and not got.max_abs.is_cuda
        # the maximum of the stored fp32 residual, to the bit
        reg = sh.region(tuple(stored.shape), (0,) * (stored.dim() - 1) if boundary else (1,) * (stored.dim() - 1))
        assert torch.equal(got.max_abs, stored[reg].abs().reshape(stored.shape[0], -1).max(dim=1).values)


def test_screenstats_fallback_slabs_and_nan(monkeypatch):
    from cp_pre_amd import screen
    c = st.ny_case("wave", sh.SEAM_SHAPES["two_tseg"])
    stored = c.r_ref.float()
    whole_ref = st.Ref(c.r_ref, (1, 1, 1))
    slabs = ((0, 8), (6, 17))
    queue = [stored[:, t0:t1] for t0, t1 in slabs]
    monkeypatch.setattr(screen._Spec, "full", lambda self, v, minus, halo_x: queue.pop(0))
    s = screen.ScreenStats(3, "cpu")
    for t0, t1 in slabs:
        s.add_slab(sh.method_of("wave"), c.x[:, t0:t1], crop=(1, 1, 1))
    got = s.finish()
    st.check(got, whole_ref, "two t-slabs of the stored residual")
    # a NaN in a counted cell of sample 1: its four statistics are NaN, the others keep their bytes
    bad = stored.clone()
    bad[1, 3, 2, 5] = float("nan")
    monkeypatch.setattr(screen._Spec, "full", lambda self, v, minus, halo_x: bad)
    nan = screen.screen_stats(sh.method_of("wave"), c.x)
    monkeypatch.setattr(screen._Spec, "full", lambda self, v, minus, halo_x: stored)
    base = screen.screen_stats(sh.method_of("wave"), c.x)
    for t, b in ((nan.sum, base.sum), (nan.sum_abs, base.sum_abs), (nan.sum_sq, base.sum_sq), (nan.max_abs, base.max_abs)):
        assert bool(torch.isnan(t[1])) and torch.equal(t[[0, 2]], b[[0, 2]])
    assert int(nan.max_abs.view(torch.int32)[1]) == 0x7fc00000


# ------------------------------------------------------------------ the order of the scripts
def _order_case(name):
    if name == "wave":
        x = st.wave_order_input()
        r = sh.oracle_residual("wave", x.double())
        return sh.method_of("wave"), x, r, (1, 2, 3), "mean_abs"
    if name == "advection":
        x = st.advection_order_input()
        return s1.method_of("advection"), x, s1.oracle_residual("advection", x.double()), (1, 2), "mean_abs"
    x = st.burgers_order_input()
    return s1.method_of("burgers"), x, s1.oracle_residual("burgers", x.double()), (1, 2), "mean"


@pytest.mark.parametrize("name", ["wave", "advection", "burgers"])
def test_screenstats_order_is_the_scripts_sort_index(monkeypatch, name):
    """Active_Learning/Wave_AL_Joint.py:403-408, Advection_AL_Joint.py:340-345 (mean |r|), Burgers_AL_Joint.py:340-345 (the
    signed mean), on their cropped residual"""
    from cp_pre_amd import screen
    method, x, r_ref, axes, by = _order_case(name)
    inner = r_ref[sh.region(tuple(r_ref.shape), (1,) * (r_ref.dim() - 1))]
    # first, on the reference alone: neighbouring per-sample means lie further apart than 4 tau
    tau = 1e-5 * float(r_ref.abs().max())
    stat64 = (inner.abs() if by == "mean_abs" else inner).mean(dim=tuple(range(1, inner.dim())))
    gaps = torch.sort(stat64).values.diff()
    print(f"{name}: smallest gap of neighbouring means {float(gaps.min()):.3e}, 4 tau = {4 * tau:.3e}")
    assert st.order_is_decided(stat64, tau), "a broken test: the order would be decided by rounding"
    # the scripts' statement, in fp32 on the stored fp32 residual
    pred_residual = inner.float()
    val, sort_index = torch.sort(torch.mean(torch.abs(pred_residual) if by == "mean_abs" else pred_residual, axis=axes))
    monkeypatch.setattr(screen._Spec, "full", lambda self, v, minus, halo_x: r_ref.float())
    got = screen.screen_stats(method, x)
    assert torch.equal(got.order(by), sort_index)
    assert torch.equal(got.order(by, descending=True), torch.flip(sort_index, (0,)))
    assert torch.equal(got.take(3, by), sort_index[:3]) and torch.equal(got.take(2, by, largest=True), torch.flip(sort_index, (0,))[:2])
    stat = got.mean_abs() if by == "mean_abs" else got.mean()
    assert stat.dtype == torch.float64
    assert bool(((stat.float()[sort_index] - val).abs() <= tau).all())
    assert got.order().dtype == torch.int64 and tuple(got.order().shape) == (8,)
    with pytest.raises(ValueError, match="by="):
        got.order("median")
    with pytest.raises(ValueError, match="k = 9"):
        got.take(9)


def test_sample_stats_order_is_stable():
    from cp_pre_amd.screen import SampleStats
    s = SampleStats(torch.tensor([2.0, 1.0, 2.0, 1.0]).double(), torch.tensor([4.0, 2.0, 4.0, 2.0]).double(),
                    torch.tensor([8.0, 2.0, 8.0, 2.0]).double(), torch.tensor([2.0, 1.0, 2.0, 1.0]), 2)
    assert s.order().tolist() == [1, 3, 0, 2] and s.order(descending=True).tolist() == [0, 2, 1, 3]
    assert s.order("max_abs").tolist() == [1, 3, 0, 2] and s.take(1, largest=True).tolist() == [0]
    assert s.mean().tolist() == [1.0, 0.5, 1.0, 0.5] and s.mean_sq().tolist() == [4.0, 1.0, 4.0, 1.0] and s.rms().tolist() == [2.0, 1.0, 2.0, 1.0]


# ------------------------------------------------------------------ what raises, before any device work
def test_screenstats_validation_raises_before_device_work():
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    from cp_pre_amd.convops_1d import ConvOperator as C1
    ns = R.NavierStokes(0.01, 0.1, 0.1)
    meth, v = ns.residual_momentum, torch.rand(3, 3, 6, 8, 12)
    with pytest.raises(TypeError, match="bound residual method"):
        screen.screen_stats(lambda x, boundary=False: x, v)
    with pytest.raises(TypeError, match="torch.Tensor"):
        screen.screen_stats(meth, v.numpy())
    with pytest.raises(TypeError, match="float32"):
        screen.screen_stats(meth, v.double())
    with pytest.raises(ValueError, match="expected vars"):
        screen.screen_stats(meth, v[:, 0])
    with pytest.raises(ValueError, match="empty batch"):
        screen.screen_stats(meth, v[:0])
    with pytest.raises(ValueError, match="leaves no cell"):
        screen.screen_stats(meth, torch.rand(2, 3, 2, 8, 12))
    with pytest.raises(TypeError):
        screen.screen_stats(meth, v, minus=v)                          # (no paired form)
    with pytest.raises(ValueError, match="3-D field"):
        screen.screen_stats(C1("x", 2), torch.rand(3, 6, 10, 2))
    with pytest.raises(ValueError, match="n_local >= 1"):
        screen.ScreenStats(0, "cpu")
    s = screen.ScreenStats(3, "cpu")
    with pytest.raises(ValueError, match="expected n_local = 3"):
        s.add_slab(meth, v[:2])
    with pytest.raises(ValueError, match="crop"):
        s.add_slab(meth, v, crop=(1, 1))
    with pytest.raises(ValueError, match="leaves no cell"):
        s.add_slab(meth, v, crop=(3, 1, 1))
    with pytest.raises(TypeError):
        s.add_slab(meth, v, minus=v)
    # halo_x raises where Screen.add_slab raises: a staged copy has no halo rows; the 1-D family and the operators read none
    with pytest.raises(ValueError, match="halo_x needs a device-resident view"):
        s.add_slab(meth, v, crop=(1, 0, 1), halo_x=True)
    with pytest.raises(ValueError, match="finish\\(\\) before any slab"):
        s.finish()
    assert s.mx is None and s.cells == 0


def test_screenstats_routes_entries_and_reasons():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _F32, _Spec
    spec = _Spec(sh.method_of("ns_momentum"))
    assert spec.route("", stats=True) == "fused:stats_ns_momentum" and spec.route("flat", stats=True) == "fused:flat_stats_ns_momentum"
    assert spec.entry("", stats=True) == "pre_screenstats_ns_momentum_f32"
    assert spec.entry("flat", stats=True) == "pre_screenstats_flat_ns_momentum_f32"
    mhd = _Spec(sh.method_of("mhd_energy"))
    assert mhd.entry("flat", stats=True) == "pre_screenstats_flat_mhd_f32" and mhd.route("", stats=True) == "fused:stats_mhd_energy"
    assert _Spec(sh.method_of("wave")).entry("", stats=True) == "pre_screenstats_stencil3d_f32"
    assert _Spec(sh.method_of("mhd_gauss")).route("flat", stats=True) == "fused:flat_stats_linear2"
    b = _Spec(s1.method_of("burgers"))
    assert b.entry("rows", stats=True) == "pre_screenstats_rows_burgers_f32" and b.route("rows", stats=True) == "fused:rows_stats_burgers"
    a = _Spec(s1.method_of("advection"))
    assert a.entry("rows", stats=True) == "pre_screenstats_rows_stencil2d_f32" and a.route("rows", stats=True) == "fused:rows_stats_stencil2d"
    for kind in st.PARENT_KINDS:
        form = "rows" if kind == "burgers" else "ny"
        sp = _Spec(s1.method_of(kind) if form == "rows" else sh.method_of(kind))
        assert sp.route("rows" if form == "rows" else "", stats=True) == st.route(kind, form)
    # the existing routes and entries are what they were
    assert spec.route("") == "fused:ns_momentum" and spec.entry("flat", cells=True) == "pre_screencells_flat_ns_momentum_f32"
    # the reasons without a device, in the order of prepare / prepare_rows
    assert spec.prepare(torch.rand(3, 3, 6, 8, 12), None, _F32, None) == ("input on the CPU", ())
    assert b.prepare_rows(torch.rand(3, 8, 16), None, _F32, None) == ("input on the CPU", ())
    off = _Spec(R.NavierStokes(0.01, 0.1, 0.1, fused=False).residual_momentum)
    assert off.prepare(torch.rand(3, 3, 6, 8, 12), None, _F32, None)[0] == "input on the CPU"
