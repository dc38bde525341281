"""CPU tests of the screen of Nt-fastest views of the 2-D residuals (cp_pre_amd.screen's flat route,
libcp_pre_screenflat.so):
  * the exported ABI against include/cp_pre_screenflat.h and the ctypes binding, a C99 client compiled against the header;
  * the split rule's seams as tests/screenflat_helpers.py names them;
  * every host reason for the three-pass route, with its exact string;
  * the caps the GPU tests' tolerances rest on, from the oracle alone.
The device passes are covered by tests/test_gpu_screenflat.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import screen_helpers as sh
import screenflat_helpers as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screenflat.h")
DECLARED = {"pre_screenflat_abi_version", "pre_screenflat_stencil3d_f32", "pre_screenflat_linear2_f32",
            "pre_screenflat_ns_momentum_f32", "pre_screenflat_mhd_f32"}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screenflat_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screenflat.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_screenflat_library_exports_exactly_its_five_symbols():
    from cp_pre_amd import _lib
    so = _lib.SCREENFLAT_SO_PATH
    assert os.path.exists(so), "libcp_pre_screenflat.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and len(DECLARED) == 5
    assert exported == declared and set(_lib.SCREENFLAT_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREENFLAT_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREENFLAT_ABI_VERSION == 1
    assert _lib._load("screenflat").pre_screenflat_abi_version() == _lib.PRE_SCREENFLAT_ABI_VERSION
    assert _lib.load_screenflat() is _lib._load("screenflat")
    # every declaration cites the reference lines it serves
    for decl in re.split(r"\n(?=/\* )", header.split("} pre_screenflat_t;", 1)[1]):
        if "int pre_screenflat_" in decl:
            assert re.search(r"\w+/\w+\.py:\d+", decl), decl[:80]
    # the set descriptor carries three modulation strides, and the ctypes structure has the header's fields in its order
    body = re.search(r"typedef struct \{(.*?)\} pre_screenflat_t;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("float *", "").split(",")]
    assert names == [n for n, _ in _lib.PreScreenFlat._fields_], names
    assert "mY" in names and names.index("mT") + 2 == names.index("mY")
    assert len(_lib._LIBS) == 8 and "screenflat" not in _lib._LIBS and "screenflat" in _lib._LIBS_MORE


def test_screenflat_ctypes_signatures_have_the_header_arity():
    from cp_pre_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^int\s+(pre_screenflat_\w+)\s*\(([^;]*)\);", header, flags=re.M)
    assert {n for n, _ in found} == DECLARED
    for name, args in found:
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.SCREENFLAT_SIGNATURES[name]), name


def test_screenflat_wrong_abi_version_raises_import_error(monkeypatch):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screenflat", None)
    monkeypatch.setattr(_lib, "PRE_SCREENFLAT_ABI_VERSION", _lib.PRE_SCREENFLAT_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_screenflat.so has ABI version 1"):
        _lib._load("screenflat")


def test_screenflat_missing_library_raises_import_error(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_screenflat", None)
    monkeypatch.setattr(_lib, "SCREENFLAT_SO_PATH", str(tmp_path / "libcp_pre_screenflat.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_screenflat()


def test_screenflat_header_compiles_as_c99():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", HEADER])


def test_screenflat_c_client_compiles_against_the_header(tmp_path):
    obj = tmp_path / "screenflat_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_screenflat_translation_unit_and_makefile_target():
    """the translation unit takes the march templates through the screens' shared header, and includes its own header"""
    src = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "screen_flat.hip")).read()
    assert '#include "screen_plane.h"' in src and "PRE_STAR_MARCH_TEMPLATES_ONLY" not in src and "star_march.hip" not in src
    assert '#include "star_march.h"' in open(os.path.join(ROOT, "cp_pre_amd", "csrc", "screen_plane.h")).read()
    assert '#include "../../include/cp_pre_screenflat.h"' in src
    mk = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "Makefile")).read()
    assert "screenflat_OBJS := screen_flat.o" in mk and re.search(r"^LIBS\s+:=.*\bscreenflat\b", mk, flags=re.M)


# ------------------------------------------------------------------ the split rule and the seams named from it
def test_screenflat_seam_shapes_cross_the_seams_they_are_named_for():
    for staged in (True, False):
        sp = {k: sf.split(s, staged) for k, s in sf.SEAM_SHAPES.items()}
        for k, s in sf.SEAM_SHAPES.items():
            # below MIN_SLOTS workgroups whatever the device: the split of these shapes does not depend on the device
            assert s[0] * sp[k]["nCh"] * sp[k]["nTSeg"] < sf.MIN_SLOTS and sp[k] == sf.split(s, staged, 1 << 20), k
        for k in ("straddle_10", "straddle_18", "straddle_30", "chunk_seam"):
            assert sf.SEAM_SHAPES[k][1] % 4 == 2, k                       # row ends inside quads
        assert sp["straddle_10"] == dict(nt=256, nCh=1, last=30, hq=3 if staged else 0, tSeg=5, nTSeg=1)
        assert sp["whole_rows"]["nt"] == 256 and sp["whole_rows"]["last"] == 64 and sf.SEAM_SHAPES["whole_rows"][1] == 64
        assert sp["widest_halo"]["hq"] == (24 if staged else 0) and sf.SEAM_SHAPES["widest_halo"][1] == sf.FLAT_MAX_Y - 1
        assert (sp["two_chunks"]["nt"], sp["two_chunks"]["nCh"], sp["two_chunks"]["last"]) == (320, 2, 320)
        assert (sp["chunk_seam"]["nt"], sp["chunk_seam"]["nCh"], sp["chunk_seam"]["last"]) == (320, 2, 205)
        assert (320 * 4) % 30 == 20 and (320 * 4 - 4) % 30 == 16          # the quads at the seam hold no row end; the next ones do
        assert (sp["one_counted_plane"]["tSeg"], sp["one_counted_plane"]["nTSeg"]) == (3, 1)
        assert (sp["two_marches"]["tSeg"], sp["two_marches"]["nTSeg"]) == (9, 2)
        assert (sp["many_marches_last_one"]["tSeg"], sp["many_marches_last_one"]["nTSeg"]) == (9, 8)
        assert 65 - 7 * 9 == 2                                            # the last march: planes 63, 64; cropped, plane 63 alone
    # the chunk rule: the surrogate's Nt = 10 on a 256-wide grid is a row of 640 quads, two chunks of 320
    assert sf.chunk(640, 10, True) == 320 and sf.chunk(640, 10, False) == 320
    assert sf.chunk(512, 20, True) == 512 and sf.chunk(513, 20, True) == 320 and sf.chunk(1280, 20, False) == 448
    assert sf.halo_quads(95, True) == 24 and sf.halo_quads(10, True) == 3 and sf.halo_quads(10, False) == 0
    # a full chip: marches get long again (the issue's bench shapes on 512 resident workgroups)
    assert sf.pick_tseg(512 * 16, 512, 512) == 512 and sf.pick_tseg(3, 65, 256) == 9 and sf.pick_tseg(3, 16, 256) == 16


def _cover(shape, crop, staged, slots):
    """How often each logical cell (t, x, y) is counted by the workgroups and lanes of screen_flat_kernel (its index
    arithmetic, restated)."""
    B, T, X, Y = shape
    ct, cx, cy = crop
    sp, cnt = sf.split(shape, staged, slots), np.zeros((T, X, Y), int)
    for ts in range(sp["nTSeg"]):
        p0, p1 = max(ts * sp["tSeg"], cx), min(ts * sp["tSeg"] + sp["tSeg"], X, X - cx)
        for ch in range(sp["nCh"]):
            for q in range(sp["nt"]):
                for j in range(4):
                    m = (ch * sp["nt"] + q) * 4 + j
                    if m >= Y * T or p0 >= p1:
                        continue
                    y, t = divmod(m, T)
                    if cy <= y < Y - cy and ct <= t < T - ct:
                        cnt[t, p0:p1, y] += 1
    return cnt


def test_screenflat_split_counts_every_counted_cell_once():
    shapes = list(sf.SEAM_SHAPES.values()) + [sf.SMALLEST_Y, (1, 7, 40, 36), (2, 95, 2, 4)]
    for shape in shapes:
        for crop in ((0, 0, 0), (1, 1, 1), (2, 0, 1)):
            if any(n - 2 * c <= 0 for n, c in zip(shape[1:], crop)):
                continue
            want = np.zeros(shape[1:], int)
            want[tuple(slice(c, n - c) for c, n in zip(crop, shape[1:]))] = 1
            assert np.array_equal(_cover(shape, crop, True, 256), want), (shape, crop)
    assert np.array_equal(_cover((3, 10, 65, 12), (1, 1, 1), False, 2048)[1:-1, 1:-1, 1:-1], np.ones((8, 63, 10), int))


# ------------------------------------------------------------------ the reasons for the three-pass route, on the host
class _View:
    """What ``_Spec.prepare_flat`` reads of a device tensor: shape, strides, ``is_cuda``."""

    def __init__(self, shape, strides, is_cuda=True):
        self.shape, self._strides, self.is_cuda = tuple(shape), tuple(strides), is_cuda

    def dim(self):
        return len(self.shape)

    def stride(self, d=None):
        return self._strides if d is None else self._strides[d]


def _nt_fastest(B, F, T, X, Y, pitch_t=None):
    """a [B,F,T,X,Y] view of memory [B,F,X,Y,Tp] (``pitch_t`` > T: a t-slab of a larger tensor)"""
    Tp = pitch_t or T
    return _View((B, F, T, X, Y), (F * X * Y * Tp, X * Y * Tp, 1, Y * Tp, Tp))


def test_screenflat_host_reasons_for_the_three_pass_route():
    """every refusal of the flat route, with its exact string, before anything is downloaded or launched"""
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _Spec
    q, q64 = torch.tensor([0.5, 1.0]), torch.tensor([0.5, 1.0], dtype=torch.float64)
    m = torch.rand(10, 5, 12) + 0.5
    ns = _Spec(sh.method_of("ns_momentum"))
    ok = _nt_fastest(3, 3, 10, 5, 12)
    assert ns.nt_fastest(ok) and not ns.nt_fastest(_View((3, 3, 10, 5, 12), (1800, 600, 60, 12, 1)))
    assert ns.prepare_flat(ok, ok, q, m) == ("minus=", ())
    assert ns.prepare_flat(torch.rand(3, 3, 10, 5, 12).permute(0, 1, 4, 2, 3), None, q, m) == ("input on the CPU", ())
    assert ns.prepare_flat(ok, None, q64, m) == ("float64 levels or modulation", ())
    assert ns.prepare_flat(ok, None, q, m.double()) == ("float64 levels or modulation", ())
    assert ns.prepare_flat(_nt_fastest(3, 3, 96, 5, 12), None, q, None) == ("Nt >= 96", ())
    assert ns.prepare_flat(_nt_fastest(3, 3, 10, 5, 13), None, q, None) == ("merged row Ny*Nt not a multiple of 4", ())
    assert ns.prepare_flat(_nt_fastest(3, 3, 6, 5, 12, pitch_t=10), None, q, None) == ("rows not dense", ())
    assert ns.prepare_flat(_nt_fastest(3, 3, 8, 5, 1), None, q, None) == ("rows not dense", ())
    off = _Spec(R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, fused=False).residual_momentum)
    assert off.prepare_flat(ok, None, q, m) == ("fused=False", ())
    live = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU)
    live.D_x.kernel.requires_grad_(True)
    assert _Spec(live.residual_momentum).prepare_flat(ok, None, q, m) == ("operator kernel requires grad", ())
    mhd = _Spec(sh.method_of("mhd_continuity"))
    assert mhd.prepare_flat(_nt_fastest(3, 3, 10, 5, 12), None, q, m) == ("fewer than six MHD channels", ())
    wave = _Spec(sh.method_of("wave"))
    assert wave.prepare_flat(_nt_fastest(3, 2, 10, 5, 12), None, q, m) == ("multi-channel wave input", ())
    # the accepted layout reaches the kernels: all weight on the 7-point star, or the last host reason
    why, kernels = ns.prepare_flat(ok, None, q, m)
    assert why is None and len(kernels) == 4
    box = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU)
    box.D_x.kernel.data[0, 0, 0] = 0.5
    assert _Spec(box.residual_momentum).prepare_flat(ok, None, q, m) == ("operator kernel off the 7-point star", ())
    # kind and why of the method are what they were; the contiguous layout's reason for such a view is unchanged
    assert ns.kind == "ns_momentum" and ns.why is None and ns.rows_kind is None
    assert ns.prepare(_View((3, 3, 10, 5, 12), (1800, 600, 1, 120, 10)), None, q, m) == ("no unit stride on the last axis", ())


# ------------------------------------------------------------------ the caps of the GPU tests, from the oracle alone
def _cases(kind):
    if kind in sf.SEAM_KINDS:
        for shape in sf.SEAM_SHAPES.values():
            if shape != sf.BASE:
                for boundary in (False, True):
                    yield shape, boundary, True, 10
        yield sf.SMALLEST_Y, True, True, 10
        for shape in list(sf.FALLBACK_SHAPES) + [(sf.SLAB[0][0], sf.SLAB[1].stop - sf.SLAB[1].start) + sf.SLAB[0][2:]]:
            yield shape, False, True, 10
    for boundary in (False, True):
        for with_mod in (True, False):
            for nk in (1, 10, 16):
                yield sf.BASE, boundary, with_mod, nk


@pytest.mark.parametrize("kind", sf.KINDS)
def test_screenflat_reference_values_meet_the_caps(kind):
    """Every case tests/test_gpu_screenflat.py runs: under 1 % of the counted cells undecided for every (level, sample),
    every level further than tau / m_min from every per-sample score, a level that accepts some samples and rejects others,
    m_min > 0."""
    worst = (0.0, np.inf)
    for shape, boundary, with_mod, nk in _cases(kind):
        c = sf.case(kind, shape, boundary, with_mod, nk)
        share, dist, split = c.caps()
        assert c.m_min > 0 and c.q.dtype == torch.float32 and c.q.shape == (nk,)
        assert share < 0.01, (kind, shape, boundary, with_mod, nk, share)
        assert dist > 1.0, (kind, shape, boundary, with_mod, nk, dist)
        assert split, (kind, shape, boundary, with_mod, nk)
        worst = (max(worst[0], share), min(worst[1], dist))
    print(f"{kind}: largest undecided share {worst[0]:.4f}, closest level {worst[1]:.1f} x tau/m_min from a score")
