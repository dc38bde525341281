"""CPU tests of the screen of the 1-D family (cp_pre_amd.screen's rows route, libcp_pre_screen1d.so):
  * the exported ABI against include/cp_pre_screen1d.h and the ctypes binding, a C99 client;
  * ``_Spec.rows_kind`` next to the unchanged ``kind`` / ``why``;
  * the split rule's seams as tests/screen1d_helpers.py names them;
  * the caps the GPU tests' tolerances rest on, from the oracle alone;
  * the validation that happens before any device work.
The device passes are covered by tests/test_gpu_screen1d.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import screen1d_helpers as s1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screen1d.h")
DECLARED = {"pre_screen1d_abi_version", "pre_screen1d_stencil2d_f32", "pre_screen1d_burgers_f32"}


def c_client_command(exe):
    return ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
            os.path.join(ROOT, "tests", "c_abi", "screen1d_check.c"), "-I" + os.path.join(ROOT, "include"),
            "-I/opt/rocm/include", "-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screen1d.so",
            "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
            "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_screen1d_library_exports_what_its_header_declares():
    from cp_pre_amd import _lib
    so = _lib.SCREEN1D_SO_PATH
    assert os.path.exists(so), "libcp_pre_screen1d.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED
    assert exported == declared and set(_lib.SCREEN1D_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREEN1D_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREEN1D_ABI_VERSION == 1
    assert _lib._load("screen1d").pre_screen1d_abi_version() == _lib.PRE_SCREEN1D_ABI_VERSION
    assert _lib.load_screen1d() is _lib._load("screen1d")
    # every declaration cites the reference lines it serves
    for decl in re.split(r"\n(?=/\* )", header.split("int pre_screen1d_abi_version", 1)[1]):
        if "int pre_screen1d_" in decl:
            assert re.search(r"\w+/\w+\.py:\d+", decl), decl[:80]
    # the header says how pre_screen_t is read on two axes
    text = " ".join(re.sub(r"\n \*", " ", header).split())
    assert "`ct` holds the Nt crop, `cx` the Nx crop" in text and "`cy` must be 0" in text
    assert "`mT` holds its Nt stride, `mX` its Nx stride" in text
    # the first table keeps its eight rows; the new library's row lives in the second
    assert len(_lib._LIBS) == 8 and "screen1d" not in _lib._LIBS and "screen1d" in _lib._LIBS_MORE


def test_screen1d_ctypes_signatures_have_the_header_arity():
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^int\s+(pre_screen1d_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    assert {n for n, _ in found} == DECLARED
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREEN1D_SIGNATURES[name]), name


def test_screen1d_wrong_abi_version_raises_import_error(monkeypatch):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screen1d", None)
    monkeypatch.setattr(_lib, "PRE_SCREEN1D_ABI_VERSION", _lib.PRE_SCREEN1D_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_screen1d.so has ABI version 1"):
        _lib._load("screen1d")


def test_screen1d_missing_library_raises_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screen1d", None)
    monkeypatch.setattr(_lib, "SCREEN1D_SO_PATH", str(tmp_path / "libcp_pre_screen1d.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_screen1d()


def test_screen1d_header_compiles_as_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", HEADER])


def test_screen1d_c_client_builds_and_links(tmp_path):
    exe = tmp_path / "screen1d_check"
    subprocess.check_call(c_client_command(exe))
    assert exe.exists()


# ------------------------------------------------------------------ what a method is
def test_screen1d_rows_kind_is_set_and_kind_and_why_are_unchanged():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_1d import ConvOperator as C1
    from cp_pre_amd.convops_2d import ConvOperator as C2
    from cp_pre_amd.screen import _Spec
    want = {R.Burgers(0.1, 0.01, 0.002).residual: "burgers", R.Advection(1.0, 0.005, 0.01).residual: "stencil2d",
            C1("x", 2): "stencil2d", C1("t", 1): "stencil2d"}
    for method, rows_kind in want.items():
        sp = _Spec(method)
        assert sp.rows_kind == rows_kind
        assert sp.kind is None and sp.why == "1-D family: the marched axis is the batch" and sp.nd == 2
        assert not sp.reads_halo()
    sp = _Spec(C1("x", 2, conv="spectral"))
    assert sp.rows_kind is None and sp.kind is None and sp.why == "spectral operator"
    for method in (R.NavierStokes(0.1, 0.1, 0.1).residual_momentum, C2("x", 1), R.PRE_Wave(0.01, 0.02).residual,
                   R.MHD().residual_gauss):
        assert _Spec(method).rows_kind is None and _Spec(method).kind is not None


# ------------------------------------------------------------------ the split rule and the seams named from it
def test_screen1d_seam_planes_cross_the_seams_they_are_named_for():
    sp = {k: s1.split(B, R, C) for k, (B, (R, C)) in s1.SEAM_PLANES.items()}
    for k, (B, (R, C)) in s1.SEAM_PLANES.items():
        # below MIN_SLOTS workgroups whatever the device: the split of these planes does not depend on the device
        assert B * sp[k]["nCT"] * sp[k]["nChunk"] < s1.MIN_SLOTS and sp[k] == s1.split(B, R, C, 1 << 20), k
        assert C % 4 == 0 and (R - 2) * (C - 2) >= 200, k
    assert sp["wave_segments"] == dict(ws=1, nseg=4, nCT=1, rc=12, nChunk=1, rSeg=3)
    assert sp["chunks_and_idle_lanes"] == dict(ws=1, nseg=4, nCT=1, rc=17, nChunk=8, rSeg=5)
    assert sp["chunks_odd_rows"] == dict(ws=1, nseg=4, nCT=1, rc=17, nChunk=2, rSeg=5)
    assert sp["fewer_rows_than_segments"] == dict(ws=1, nseg=4, nCT=1, rc=3, nChunk=1, rSeg=1)
    assert sp["partial_last_strip"] == dict(ws=2, nseg=2, nCT=1, rc=5, nChunk=1, rSeg=3)
    assert sp["two_strips_and_a_quad"] == dict(ws=4, nseg=1, nCT=1, rc=5, nChunk=8, rSeg=5)
    assert sp["column_tiles"] == dict(ws=4, nseg=1, nCT=2, rc=5, nChunk=2, rSeg=5)
    # a full chip stops the halving: the C5 shard marches whole samples
    assert s1.split(8192, 200, 512, 2048) == dict(ws=2, nseg=2, nCT=1, rc=200, nChunk=1, rSeg=100)
    assert s1.split(8192, 512, 200, 2048) == dict(ws=1, nseg=4, nCT=1, rc=512, nChunk=1, rSeg=128)


def _cover(B, R, C, cr, cc, slots):
    """How often each cell of a plane is counted by the workgroups and waves of screen_rows_kernel (its index arithmetic,
    restated)."""
    sp, cnt = s1.split(B, R, C, slots), np.zeros((R, C), int)
    for ch in range(sp["nChunk"]):
        for ct in range(sp["nCT"]):
            for wv in range(4):
                strip, s0 = ct * sp["ws"] + wv % sp["ws"], ch * sp["rc"] + (wv // sp["ws"]) * sp["rSeg"]
                r0, r1 = max(s0, cr), min(s0 + sp["rSeg"], ch * sp["rc"] + sp["rc"], R, R - cr)
                if r0 < r1 and strip * 256 < C:
                    cols = np.arange(strip * 256, min(strip * 256 + 256, C))
                    cnt[r0:r1, cols[(cols >= cc) & (cols < C - cc)]] += 1
    return cnt


def test_screen1d_split_counts_every_counted_cell_once():
    planes = list(s1.SEAM_PLANES.values()) + [(8192, (200, 512)), (8192, (512, 200)), (1, (1000, 2052)), (7, (1, 4)), (2, (37, 1300))]
    for B, (R, C) in planes:
        for cr, cc in ((0, 0), (1, 1), (2, 0)):
            if R - 2 * cr <= 0:
                continue
            want = np.zeros((R, C), int)
            want[cr:R - cr, cc:C - cc] = 1
            for slots in (256, 2048):
                assert np.array_equal(_cover(B, R, C, cr, cc, slots), want), (B, R, C, cr, cc, slots)


# ------------------------------------------------------------------ the caps of the GPU tests, from the oracle alone
ISSUE_PLANES = [(3, (5, 260)), (3, (130, 12)), (3, (40, 516)), (3, (9, 1028)), (3, (12, 64)), (5, (33, 256))]
GPU_PLANES = sorted(set(ISSUE_PLANES) | set(s1.SEAM_PLANES.values()) | set(s1.ODD_PLANES) | {(3, (12, 64))})


@pytest.mark.parametrize("kind", s1.KINDS)
def test_screen1d_reference_values_meet_the_caps(kind):
    """Every case tests/test_gpu_screen1d.py runs, in both layouts (the plane and its transpose as the logical shape): at
    most 1 % of the counted cells undecided for every (level, sample), every level further than tau / m_min from every
    per-sample score, a level that accepts some samples and rejects others, m_min > 0."""
    worst = (0.0, np.inf)
    planes = GPU_PLANES if kind in ("burgers", "advection", "dxx") else [p for p in GPU_PLANES if p not in ISSUE_PLANES[2:4]]
    for B, plane in planes:
        for layout in s1.LAYOUTS:
            shape = s1.logical_shape(B, plane, layout)
            for boundary in (False, True):
                for with_mod in (True, False):
                    for nk in (1, 10, 16):
                        c = s1.Case(kind, shape, boundary, with_mod, nk)
                        share, dist, split = c.caps()
                        assert c.m_min > 0 and c.q.dtype == torch.float32 and c.q.shape == (nk,)
                        assert share <= 0.01, (kind, shape, boundary, with_mod, nk, share)
                        assert dist > 1.0, (kind, shape, boundary, with_mod, nk, dist)
                        assert split, (kind, shape, boundary, with_mod, nk)
                        worst = (max(worst[0], share), min(worst[1], dist))
    print(f"{kind}: largest undecided share {worst[0]:.4f}, closest level {worst[1]:.1f} x tau/m_min from a score")


def test_screen1d_slab_case_meets_the_caps():
    """the composition case of the GPU tests: rows [0:8] + [6:12] of (3, 12, 64), crop 1"""
    for layout in s1.LAYOUTS:
        c = s1.Case("burgers", s1.logical_shape(3, (12, 64), layout), False, True, 10)
        share, dist, split = c.caps()
        assert share <= 0.01 and dist > 1.0 and split


# ------------------------------------------------------------------ validation before any device work
def test_screen1d_validation_raises_before_device_work():
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    from cp_pre_amd.convops_1d import ConvOperator as C1
    bg = R.Burgers(s1.DX, s1.DT, s1.NU).residual
    v, q, m = torch.rand(3, 8, 12), torch.tensor([0.5, 1.0]), torch.rand(8, 12) + 0.5
    for meth in (bg, R.Advection(1.0, 0.01, 1 / 64).residual, C1("x", 2)):
        with pytest.raises(TypeError, match="dtype"):
            screen.screen(meth, v.double(), q, m)
        with pytest.raises(ValueError):
            screen.screen(meth, v[0], q, m)                               # (a rank the method does not take)
        with pytest.raises(ValueError):
            screen.screen(meth, torch.rand(3, 2, 8, 12), q, m)            # (two channels)
        with pytest.raises(ValueError):
            screen.screen(meth, v[:0], q, m)
        with pytest.raises(ValueError, match="nk"):
            screen.screen(meth, v, torch.rand(17), m)
        with pytest.raises(ValueError, match=r"expected \(8, 12\)"):
            screen.screen(meth, v, q, m[1:-1, 1:-1])
        with pytest.raises(ValueError, match=r"expected \(8, 12\)"):
            screen.screen(meth, v, q, torch.rand(8, 12, 1))
        with pytest.raises(ValueError, match="is on"):
            screen.screen(meth, v, q.to("meta"), m)
        with pytest.raises(ValueError, match="shape"):
            screen.screen(meth, v, q, m, minus=v[:, :-1])
        with pytest.raises(ValueError, match="leaves no cell"):
            screen.screen(meth, torch.rand(3, 2, 12), q, torch.rand(2, 12))
        s = screen.Screen(3, 2, "cpu")
        with pytest.raises(ValueError, match="n_local"):
            s.add_slab(meth, torch.rand(2, 8, 12), q, m, crop=(1, 1))
        with pytest.raises(ValueError, match="crop"):
            s.add_slab(meth, v, q, m, crop=(1, 1, 1))
        with pytest.raises(ValueError, match="crop"):
            s.add_slab(meth, v, q, m, crop=(-1, 1))
        with pytest.raises(ValueError, match="halo_x"):
            s.add_slab(meth, v, q, m, crop=(1, 1), halo_x=True)           # (a host tensor has no halo rows to read)
        with pytest.raises(ValueError, match="this Screen was made for"):
            screen.Screen(3, 2, "meta").add_slab(meth, v, q, m, crop=(1, 1))
        assert s.acc is None and s.cells == 0


def test_screen1d_host_reasons_for_the_three_pass_route():
    """``_Spec.prepare_rows`` on host tensors: the reason is given before anything is downloaded or launched"""
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _Spec
    sp = _Spec(R.Burgers(s1.DX, s1.DT, s1.NU).residual)
    v, q, m = torch.rand(3, 8, 12), torch.tensor([0.5, 1.0]), torch.rand(8, 12) + 0.5
    assert sp.prepare_rows(v, v, q, m) == ("minus=", ())
    assert sp.prepare_rows(v, None, q, m) == ("input on the CPU", ())
    vm = v.to("meta")                                                     # (is_cuda is False: the CPU reason comes first)
    assert sp.prepare_rows(vm, None, q, m)[0] == "input on the CPU"
