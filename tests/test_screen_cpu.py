"""CPU tests of the screen (cp_pre_amd.screen, libcp_pre_screen.so):
  * the exported ABI against include/cp_pre_screen.h and the ctypes binding, a C99 client;
  * ``Screened``'s derived quantities against numpy restatements of the reference's ``filter_sims_joint``, ``emp_cov_joint``,
    ``emp_cov`` and ``filter_samples_within_bounds`` (Joint/NS_Residuals_CP.py:328-329,350-352;
    Active_Learning/Advection_AL_Marginal.py:169-198);
  * the validation that happens before any device work;
  * the caps the GPU tests' tolerances rest on (tests/screen_helpers.py), from the oracle alone.
The device passes are covered by tests/test_gpu_screen.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import screen_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screen.h")
DECLARED = {"pre_screen_abi_version", "pre_screen_stencil3d_f32", "pre_screen_linear2_f32", "pre_screen_ns_momentum_f32",
            "pre_screen_mhd_f32"}


# ------------------------------------------------------------------ the ABI
def test_screen_library_exports_what_its_header_declares():
    from cp_pre_amd import _lib
    so = _lib.SCREEN_SO_PATH
    assert os.path.exists(so), "libcp_pre_screen.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.SCREEN_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREEN_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREEN_ABI_VERSION
    assert int(re.search(r"#define\s+PRE_SCREEN_MAX_LEVELS\s+(\d+)", header).group(1)) == _lib.PRE_SCREEN_MAX_LEVELS
    assert _lib._load("screen").pre_screen_abi_version() == _lib.PRE_SCREEN_ABI_VERSION
    assert _lib.load_screen() is _lib._load("screen")
    # every declaration cites the reference lines it serves
    for decl in re.split(r"\n(?=/\* )", header.split("} pre_screen_t;", 1)[1]):
        if "int pre_screen_" in decl:
            assert re.search(r"\w+/\w+\.py:\d+", decl), decl[:80]
    # the first table keeps its eight rows; the new library's row lives next to it
    assert len(_lib._LIBS) == 8 and "screen" not in _lib._LIBS and "screen" in _lib._LIBS_MORE


def test_screen_ctypes_signatures_have_the_header_arity():
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^int\s+(pre_screen_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    assert {n for n, _ in found} == DECLARED
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREEN_SIGNATURES[name]), name
    # pre_screen_t: the ctypes structure has the header's members, in order
    body = re.search(r"typedef struct \{(.*?)\} pre_screen_t;", header, flags=re.S).group(1)
    members = [re.sub(r".*[\s*]", "", part.strip()) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert members == [f[0] for f in _lib.PreScreen._fields_], members


def test_screen_wrong_abi_version_raises_import_error(monkeypatch):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screen", None)
    monkeypatch.setattr(_lib, "PRE_SCREEN_ABI_VERSION", _lib.PRE_SCREEN_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_screen.so has ABI version 1"):
        _lib._load("screen")


def test_screen_missing_library_raises_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screen", None)
    monkeypatch.setattr(_lib, "SCREEN_SO_PATH", str(tmp_path / "libcp_pre_screen.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_screen()


def test_screen_header_compiles_as_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", HEADER])


def test_screen_c_client_builds_and_links(tmp_path):
    exe = tmp_path / "screen_check"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "c_abi", "screen_check.c"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screen.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)])
    assert exe.exists()


# ------------------------------------------------------------------ Screened against the reference's functions, in numpy
def ref_filter_sims_joint(pred_sets, y):
    """Joint/NS_Residuals_CP.py (filter_sims_joint): every cell of the sample inside"""
    axes = tuple(range(1, y.ndim))
    return ((y >= pred_sets[0]).all(axis=axes) & (y <= pred_sets[1]).all(axis=axes))


def ref_emp_cov_joint(pred_sets, y):
    return ref_filter_sims_joint(pred_sets, y).mean()


def ref_emp_cov(pred_sets, y):
    return ((y >= pred_sets[0]) & (y <= pred_sets[1])).mean()


def ref_within_bounds(lower, upper, samples, threshold):
    """Active_Learning/Advection_AL_Marginal.py:169-198 (within=True)"""
    axes = tuple(range(1, samples.ndim))
    return ((samples >= lower) & (samples <= upper)).mean(axis=axes) >= threshold


def test_screened_derived_quantities_equal_the_reference_functions():
    from cp_pre_amd.screen import Screened
    rng = np.random.default_rng(3)
    n, cells_shape = 7, (4, 5, 6)
    m = (0.5 + rng.random(cells_shape)).astype(np.float32)
    y = (rng.standard_normal((n,) + cells_shape) * np.linspace(0.2, 1.5, n)[:, None, None, None]).astype(np.float32)
    q = np.array([0.3, 1.0, 2.0, 3.5, 50.0], np.float32)
    sets = [[-(qk * m), qk * m] for qk in q]                           # fp32 bounds, as the reference forms them
    inside = np.stack([((y >= lo) & (y <= hi)).reshape(n, -1).sum(axis=1) for lo, hi in sets]).astype(np.int64)
    cells = int(np.prod(cells_shape))
    score = (np.abs(y) / m).reshape(n, -1).max(axis=1)
    s = Screened(torch.from_numpy(score), torch.from_numpy(inside), cells)
    acc = s.accept().numpy()
    assert acc.dtype == np.bool_ and acc.shape == (len(q), n)
    assert 0 < acc.sum() < acc.size                                   # (some accepted, some rejected)
    for k, ps in enumerate(sets):
        np.testing.assert_array_equal(acc[k], ref_filter_sims_joint(ps, y))
        assert s.coverage_joint()[k] == ref_emp_cov_joint(ps, y)
        assert s.coverage_marginal()[k] == ref_emp_cov(ps, y)
        for thr in (0.5, 0.9, 1.0, float(inside[k, 2]) / cells):
            np.testing.assert_array_equal(s.within(thr)[k].numpy(), ref_within_bounds(ps[0], ps[1], y, thr))
    assert s.coverage_joint().dtype == np.float64 and s.coverage_marginal().dtype == np.float64
    # accept() is the score test wherever the score is not on a level: |r| <= q m for every cell  <=>  max |r| / m <= q
    np.testing.assert_array_equal(acc, score[None, :] <= q[:, None])


# ------------------------------------------------------------------ validation before any device work
def _inputs():
    from cp_pre_amd import residuals as R
    v = torch.rand(2, 6, 5, 8, 12)
    ns = R.NavierStokes(0.1, 0.1, 0.1)
    return ns, v, torch.tensor([0.5, 1.0]), torch.rand(5, 8, 12) + 0.5


def test_screen_validation_raises_before_device_work():
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    from cp_pre_amd.convops_1d import ConvOperator as C1
    ns, v, q, m = _inputs()
    meth = ns.residual_momentum
    with pytest.raises(TypeError, match="residual_method"):
        screen.screen(lambda x, boundary=False: x, v, q, m)
    with pytest.raises(TypeError, match="residual_method"):
        screen.screen(ns.periodic_bc_residual, v, q, m)
    with pytest.raises(TypeError):
        screen.screen(meth, v.numpy(), q, m)
    with pytest.raises(TypeError, match="dtype"):
        screen.screen(meth, v.double(), q, m)
    with pytest.raises(ValueError):
        screen.screen(meth, v[:, 0], q, m)                             # (a rank the method does not take)
    with pytest.raises(ValueError):
        screen.screen(meth, v[:0], q, m)
    with pytest.raises(TypeError):
        screen.screen(meth, v, [0.5, 1.0], m)
    with pytest.raises(TypeError, match="dtype"):
        screen.screen(meth, v, torch.tensor([1, 2]), m)
    with pytest.raises(ValueError, match="nk"):
        screen.screen(meth, v, torch.rand(17), m)
    with pytest.raises(ValueError, match="nk"):
        screen.screen(meth, v, torch.rand(2, 2), m)
    with pytest.raises(ValueError, match="is on"):
        screen.screen(meth, v, q.to("meta"), m)
    with pytest.raises(ValueError, match=r"expected \(5, 8, 12\)"):
        screen.screen(meth, v, q, m[1:-1, 1:-1, 1:-1])                 # (the modulation keeps the uncropped extents)
    with pytest.raises(TypeError, match="dtype"):
        screen.screen(meth, v, q, m.to(torch.float16))
    with pytest.raises(TypeError):
        screen.screen(meth, v, q, m.numpy())
    with pytest.raises(ValueError, match="is on"):
        screen.screen(meth, v, q, m.to("meta"))
    with pytest.raises(ValueError, match="shape"):
        screen.screen(meth, v, q, m, minus=v[:, :, :-1])
    with pytest.raises(TypeError):
        screen.screen(meth, v, q, m, minus=v.double())
    with pytest.raises(ValueError, match="leaves no cell"):
        screen.screen(meth, torch.rand(2, 3, 2, 8, 12), q, torch.rand(2, 8, 12))
    for other in (R.MHD().residual_energy, R.PRE_Wave(0.01, 0.02).residual, R.MHD().residual_gauss):
        with pytest.raises(ValueError, match="expected"):
            screen.screen(other, torch.rand(3, 3), q, m)
    with pytest.raises(ValueError):
        screen.screen(R.Burgers(0.1, 0.01, 0.002).residual, torch.rand(3, 6, 10), q, torch.rand(5, 10))
    with pytest.raises(ValueError):
        screen.screen(C1("x", 2), torch.rand(3, 6, 10), q, torch.rand(6, 10, 2))
    # the accumulating form
    with pytest.raises(ValueError):
        screen.Screen(0, 2, "cpu")
    with pytest.raises(ValueError):
        screen.Screen(2, 17, "cpu")
    s = screen.Screen(2, 2, "cpu")
    with pytest.raises(ValueError, match="n_local"):
        s.add_slab(meth, torch.rand(3, 3, 5, 8, 12), q, m)
    with pytest.raises(ValueError, match=r"expected \(2,\)"):
        s.add_slab(meth, v, torch.rand(3), m)
    with pytest.raises(ValueError, match="crop"):
        s.add_slab(meth, v, q, m, crop=(1, 1))
    with pytest.raises(ValueError, match="crop"):
        s.add_slab(meth, v, q, m, crop=(1, -1, 1))
    with pytest.raises(ValueError, match="before any slab"):
        s.finish()
    with pytest.raises(ValueError, match="halo_x"):
        s.add_slab(meth, v, q, m, crop=(1, 0, 1), halo_x=True)         # (a host tensor has no halo rows to read)
    with pytest.raises(ValueError, match="this Screen was made for"):
        screen.Screen(2, 2, "meta").add_slab(meth, v, q, m)
    from cp_pre_amd.screen import _Spec
    assert _Spec(meth).reads_halo() and _Spec(R.MHD().residual_energy).reads_halo() and _Spec(R.PRE_Wave(0.01, 0.02).residual).reads_halo()
    from cp_pre_amd.convops_2d import ConvOperator as C2
    assert not _Spec(C2("x", 1)).reads_halo() and not _Spec(ns.residual_continuity).reads_halo()
    assert not _Spec(R.MHD().residual_gauss).reads_halo()


def test_screen_resolves_methods_like_the_losses():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_2d import ConvOperator
    from cp_pre_amd.screen import _Spec
    ns, mhd = R.NavierStokes(0.1, 0.1, 0.1), R.MHD()
    kinds = {ns.residual_momentum: "ns_momentum", R.PRE_NS(0.1, 0.1, 0.1).residual: "ns_momentum",
             ns.residual_continuity: "linear2", mhd.residual_gauss: "linear2", mhd.residual_continuity: "mhd_continuity",
             mhd.residual_momentum: "mhd_momentum", mhd.residual_energy: "mhd_energy", mhd.residual_induction: "mhd_induction",
             R.PRE_MHD(0.1, 0.1, 0.1).residual: "mhd_induction", R.PRE_Wave(0.01, 0.02).residual: "stencil3d",
             ConvOperator("x", 1): "stencil3d"}
    for method, kind in kinds.items():
        assert _Spec(method).kind == kind
    for method in (R.Burgers(0.1, 0.01, 0.002).residual, R.Advection(1.0, 0.005, 0.01).residual):
        sp = _Spec(method)
        assert sp.kind is None and "1-D family" in sp.why


# ------------------------------------------------------------------ the caps of the GPU tests, from the oracle alone
ALL_SHAPES = list(sh.SEAM_SHAPES.values()) + sh.ODD_SHAPES + [(3, 12, 41, 64)]


@pytest.mark.parametrize("kind", sh.KINDS)
def test_reference_values_meet_the_caps(kind):
    """Every case tests/test_gpu_screen.py runs: at most 1 % of the counted cells undecided for every (level, sample),
    every level further than tau / m_min from every per-sample score (so no sample is excluded from the accept check),
    a level that accepts some samples and rejects others, m_min > 0."""
    shapes = ALL_SHAPES if kind in ("ns_momentum", "lap", "mhd_momentum", "wave") else \
        [sh.SEAM_SHAPES[k] for k in ("two_tseg", "rows2_narrow", "rows3_wide")]
    worst = (0.0, np.inf)
    for shape in shapes:
        for boundary in (False, True):
            for with_mod in (True, False):
                for nk in (1, 10, 16):
                    c = sh.Case(kind, shape, boundary, with_mod, nk)
                    share, dist, split = c.caps()
                    assert c.m_min > 0 and c.q.dtype == torch.float32 and c.q.shape == (nk,)
                    assert share <= 0.01, (kind, shape, boundary, with_mod, nk, share)
                    assert dist > 1.0, (kind, shape, boundary, with_mod, nk, dist)
                    assert split, (kind, shape, boundary, with_mod, nk)
                    worst = (max(worst[0], share), min(worst[1], dist))
    print(f"{kind}: largest undecided share {worst[0]:.4f}, closest level {worst[1]:.1f} x tau/m_min from a score")


def test_oracle_fp64_is_the_oracle_in_fp32_to_rounding():
    from conftest import rel_err
    from oracle import residuals as orr
    for kind in sh.KINDS:
        x = sh.fields(kind, (2, 6, 7, 12))
        r64 = sh.oracle_residual(kind, x.double())
        assert r64.dtype == torch.float64
        if kind == "ns_momentum":
            r32 = orr.ns_momentum(x, sh.NS_DT, sh.NS_DX, sh.NS_DY, sh.NS_NU, boundary=True)
        elif kind.startswith("mhd_"):
            r32 = getattr(orr, kind)(x, boundary=True)
        else:
            continue
        assert rel_err(r32.numpy(), r64.numpy()) <= 1e-5
