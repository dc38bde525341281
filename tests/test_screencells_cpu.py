"""The per-cell screen without a GPU: the reference's own caps for every case the GPU files run, the argument errors (all
before any device work), the route reasons that shapes and strides alone decide, the NaN padding of cropped levels, the
ABI facts of libcp_pre_screencells.so and its C client.  Helpers and the reference: tests/screencells_helpers.py."""
import os
import re
import subprocess

import pytest
import torch

import screen_helpers as sh
import screencells_helpers as ch
import screenflat_helpers as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_screencells.h")
KINDS4 = ("stencil3d", "linear2", "ns_momentum", "mhd")
DECLARED = {"pre_screencells_abi_version", "pre_screencells_sample_group"} | \
    {"pre_screencells_%s%s_f32" % (form, k) for form in ("", "flat_") for k in KINDS4}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "screencells_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_screencells.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
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
def test_screencells_reference_caps_hold_for_every_gpu_case():
    from cp_pre_amd import screen
    G = screen.sample_group()
    assert isinstance(G, int) and G >= 1
    cases = ch.gpu_cases() + [(k, (B,) + ch.GROUP_TXY, True, True, 10, None) for k in ch.GROUP_KINDS for B in ch.group_batches(G)]
    worst, curve_lo, curve_hi = 0.0, 1.0, 0.0
    for kind, shape, boundary, with_mod, nk, n in cases:
        c = ch.case(kind, shape, boundary, with_mod, nk, n)
        share, split = c.caps()
        worst = max(worst, share)
        cov = c.count_ref.double().sum(dim=1) / (c.cells * c.shape[0])
        curve_lo, curve_hi = min(curve_lo, float(cov.min())), max(curve_hi, float(cov.max()))
        assert share <= ch.SHARE_CAP, (kind, shape, boundary, with_mod, nk, share)
        assert split, (kind, shape, boundary, with_mod, nk)
        assert tuple(c.q.shape) == (nk,) + tuple(shape[1:]) and c.q.dtype == torch.float32
    print(f"{len(cases)} cases: largest undecided share {worst:.4f}, coverage curve from {curve_lo:.3f} to {curve_hi:.3f}")


def test_screencells_levels_are_not_rank_one():
    """a kernel that reads one level field for every k, or one level per k for every cell, cannot pass"""
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    q = c.q.reshape(10, -1).double()
    assert int(torch.linalg.matrix_rank(q)) == 10
    assert ch.ranks(10) == [(i, i) for i in (11, 10, 8, 7, 6, 5, 4, 2, 1, 0)]
    assert len(set(ch.ranks(16))) == 16 and ch.ranks(1) == [(5, 6)]


# ------------------------------------------------------------------ argument errors, before any device work
def test_screencells_argument_errors():
    from cp_pre_amd import screen
    m = sh.method_of("ns_momentum")
    x = torch.rand(3, 3, 6, 9, 12)
    q = torch.rand(10, 6, 9, 12)
    qc = torch.rand(10, 4, 7, 10)
    with pytest.raises(TypeError, match="qcells must be a torch.Tensor"):
        screen.screen_cells(m, x, [1.0])
    with pytest.raises(TypeError, match="dtype"):
        screen.screen_cells(m, x, q.half())
    with pytest.raises(TypeError, match="float32 fields"):
        screen.screen_cells(m, x.double(), q)
    with pytest.raises(ValueError, match="1 <= nk <= 16"):
        screen.screen_cells(m, x, torch.rand(17, 6, 9, 12))
    with pytest.raises(ValueError, match="1 <= nk <= 16"):
        screen.screen_cells(m, x, torch.rand(0, 6, 9, 12))
    with pytest.raises(ValueError, match="1 <= nk <= 16"):
        screen.screen_cells(m, x, torch.rand(10))                    # (the [nk] levels of screen(): not level fields)
    with pytest.raises(ValueError, match="or the cropped"):
        screen.screen_cells(m, x, torch.rand(10, 5, 9, 12))
    with pytest.raises(ValueError, match=r"expected \[nk, \*\(6, 9, 12\)\]$"):
        screen.screen_cells(m, x, qc, boundary=True)                 # cropped extents with boundary=True
    with pytest.raises(ValueError, match="is on"):
        screen.screen_cells(m, x, q.to("meta"))
    with pytest.raises(ValueError, match="modulation has shape"):
        screen.screen_cells(m, x, q, torch.rand(4, 7, 10))
    with pytest.raises(ValueError, match="n_local >= 1"):
        screen.ScreenCells(0, 10, "cpu")
    with pytest.raises(ValueError, match="1 <= nk <= 16"):
        screen.ScreenCells(3, 17, "cpu")
    s = screen.ScreenCells(3, 10, "cpu")
    with pytest.raises(ValueError, match="expected n_local = 3"):
        s.add_slab(m, x[:2], q)
    with pytest.raises(ValueError, match="crop"):
        s.add_slab(m, x, q, crop=(1, 1))
    with pytest.raises(ValueError, match="leaves no cell"):
        s.add_slab(m, x, q, crop=(3, 1, 1))
    with pytest.raises(ValueError, match=r"expected \(10,\)"):
        s.add_slab(m, x, q[:4])
    with pytest.raises(ValueError, match="uncropped extents"):
        s.add_slab(m, x, qc)                                         # (add_slab takes the slab's uncropped extents only)
    assert s.acc is None and s.cells == 0
    # screen() keeps refusing level fields
    with pytest.raises(ValueError, match=r"expected \[nk\]"):
        screen.screen(m, x, q)


def test_screencells_route_reasons_in_order():
    from cp_pre_amd import residuals as R
    from cp_pre_amd.screen import _Spec
    x = torch.rand(3, 3, 10, 5, 12)
    q, q64 = torch.rand(4, 10, 5, 12), torch.rand(4, 10, 5, 12).double()
    spec = _Spec(sh.method_of("ns_momentum"))
    assert spec.prepare(_dev(x), _dev(x), q, None) == ("minus=", ())
    assert spec.prepare(x, None, q, None) == ("input on the CPU", ())
    assert spec.prepare(_dev(x), None, q64, None) == ("float64 levels or modulation", ())
    assert spec.prepare(_dev(x)[..., ::2], None, q, None) == ("no unit stride on the last axis", ())
    assert spec.prepare(_dev(torch.rand(3, 3, 10, 5, 13)), None, q, None) == ("row width not a multiple of 4", ())
    xf = _nt_fast(x)
    assert spec.nt_fastest(xf)
    assert spec.prepare_flat(xf, None, q, None) == ("input on the CPU", ())
    assert spec.prepare_flat(_dev(_nt_fast(torch.rand(3, 3, 96, 5, 12))), None, q, None) == ("Nt >= 96", ())
    assert spec.prepare_flat(_dev(_nt_fast(torch.rand(3, 3, 10, 5, 13))), None, q, None) == ("merged row Ny*Nt not a multiple of 4", ())
    assert spec.prepare_flat(_dev(xf)[:, :, 2:8], None, q, None) == ("rows not dense", ())
    off = _Spec(R.NavierStokes(0.01, 0.1, 0.1, fused=False).residual_momentum)
    assert off.prepare(_dev(x), None, q, None)[0] == "fused=False"
    # the 1-D family and JOREK have no per-cell screen: their reason whatever the input
    assert _Spec(R.Burgers(0.01, 0.01, 0.01).residual).prepare(_dev(torch.rand(3, 8, 16)), None, q, None)[0] == \
        "1-D family: the marched axis is the batch"
    assert spec.route("", cells=True) == "fused:cells_ns_momentum" and spec.route("flat", cells=True) == "fused:flat_cells_ns_momentum"
    assert spec.entry("", cells=True) == "pre_screencells_ns_momentum_f32"
    assert _Spec(sh.method_of("mhd_energy")).entry("flat", cells=True) == "pre_screencells_flat_mhd_f32"
    assert _Spec(sh.method_of("mhd_energy")).route("flat", cells=True) == "fused:flat_cells_mhd_energy"


def test_screencells_cropped_levels_are_padded_with_nan():
    from cp_pre_amd.screen import _pad_levels
    qc = torch.rand(3, 4, 7, 10)
    for nt_fastest in (False, True):
        full = _pad_levels(qc, (6, 9, 12), nt_fastest)
        assert tuple(full.shape) == (3, 6, 9, 12) and full.dtype == qc.dtype
        assert torch.equal(full[:, 1:-1, 1:-1, 1:-1], qc)
        rim = torch.ones(6, 9, 12, dtype=torch.bool)
        rim[1:-1, 1:-1, 1:-1] = False
        assert bool(torch.isnan(full[:, rim]).all())
        assert (full.stride(1) == 1 and full.stride(3) == 6) if nt_fastest else full.is_contiguous()


def test_screencells_cpu_inputs_take_the_three_pass_route_or_say_there_is_no_gpu():
    """on CPU tensors the call reaches the fallback (which stages to the device): without a device it must fail loudly in
    the staging, not in the argument checks, and never load the per-cell library on the way"""
    from cp_pre_amd import screen
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    if torch.cuda.is_available():
        got = screen.screen_cells(sh.method_of("ns_momentum"), c.x, c.q, c.mod)
        assert screen.last_route() == "fallback:input on the CPU"
        ch.check(c, got, "CPU inputs")
    else:
        with pytest.raises((RuntimeError, AssertionError)):
            screen.screen_cells(sh.method_of("ns_momentum"), c.x, c.q, c.mod)
        assert screen.last_route() == "fallback:input on the CPU"


# ------------------------------------------------------------------ the ABI
def test_screencells_library_exports_exactly_its_symbols_and_the_sample_group():
    from cp_pre_amd import _lib, screen
    so = _lib.SCREENCELLS_SO_PATH
    assert os.path.exists(so), "libcp_pre_screencells.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and len(DECLARED) == 10
    assert exported == declared and set(_lib.SCREENCELLS_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_SCREENCELLS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_SCREENCELLS_ABI_VERSION == 1
    assert _lib.load_screencells().pre_screencells_abi_version() == 1
    G = _lib.load_screencells().pre_screencells_sample_group()
    assert G >= 1 and screen.sample_group() == G
    assert "screencells" in _lib._LIBS_MORE and len(_lib._LIBS) == 8
    # the twins' arguments, with the per-cell descriptor in the place of theirs
    for form, table, prefix, desc in (("", _lib.SCREEN_SIGNATURES, "pre_screen_", _lib.PreScreenCells),
                                      ("flat_", _lib.SCREENFLAT_SIGNATURES, "pre_screenflat_", _lib.PreScreenCellsFlat)):
        for k in KINDS4:
            sig, tw = _lib.SCREENCELLS_SIGNATURES["pre_screencells_%s%s_f32" % (form, k)], table[prefix + k + "_f32"]
            assert len(sig) == len(tw)
            diff = [i for i, (a, b) in enumerate(zip(sig, tw)) if a is not b]
            assert len(diff) == 1 and sig[diff[0]] is __import__("ctypes").POINTER(desc), (form, k)


def test_screencells_descriptors_have_the_header_layout(tmp_path):
    """sizeof / offsetof of the two descriptors in C against the ctypes structures"""
    import ctypes
    from cp_pre_amd import _lib
    src = tmp_path / "layout.c"
    names = {"pre_screencells_t": (_lib.PreScreenCells, ["levels", "nk", "lK", "lT", "lX", "modulation", "mT", "mX", "ct", "cx", "cy",
                                                        "score", "count", "count_ld"]),
             "pre_screencellsflat_t": (_lib.PreScreenCellsFlat, ["levels", "nk", "lK", "lT", "lX", "lY", "modulation", "mT", "mX", "mY",
                                                                "ct", "cx", "cy", "score", "count", "count_ld"])}
    body = "".join('printf("%s %%zu", sizeof(%s)); %s printf("\\n");\n' % (
        t, t, " ".join('printf(" %%zu", offsetof(%s, %s));' % (t, f) for f in fs)) for t, (_, fs) in names.items())
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cp_pre_screencells.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        t, size, *offs = line.split()
        st, fs = names[t]
        assert [f for f, _ in st._fields_] == fs
        assert int(size) == ctypes.sizeof(st) and [int(o) for o in offs] == [getattr(st, f).offset for f in fs], t


def test_screencells_header_and_c_client_compile_and_link(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "screencells_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    exe = tmp_path / "screencells_check"
    subprocess.check_call(c_client_command(exe))
    assert obj.exists() and exe.exists()


def test_screencells_makefile_and_source_facts():
    csrc = os.path.join(ROOT, "cp_pre_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^LIBS\s+:=.*\bscreencells\b", mk, flags=re.M) and re.search(r"^screencells_OBJS\s+:= screen_cells\.o", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS\s+:=(.|\\\n)*\$\(screencells_OBJS\)", mk, flags=re.M)
    assert "$(screencells_OBJS): $(INC)/cp_pre_screencells.h $(INC)/cp_pre_screen.h $(INC)/cp_pre_screenflat.h" in mk
    src = open(os.path.join(csrc, "screen_cells.hip")).read()
    assert "__global__" not in src                                   # the marches are not copied
    assert '#include "screen_march.h"' in src and '#include "screen_flat.h"' in src
    plane = open(os.path.join(csrc, "screen_plane.h")).read()
    assert "screen_plane_cells(" in plane and "const float4 (&ql)[NKMAX]" in plane and "struct CellSets" in plane


def test_screencells_library_is_not_loaded_by_the_other_screens():
    """screen.py names load_screencells in the per-cell functions only"""
    import inspect
    from cp_pre_amd import screen
    src = inspect.getsource(screen)
    users = {name for name, fn in inspect.getmembers(screen, inspect.isfunction) if "load_screencells" in inspect.getsource(fn)}
    assert users == {"sample_group"}
    assert "load_screencells() if cells else" in inspect.getsource(screen._Spec.launch)
    assert "cells=True" in inspect.getsource(screen.ScreenCells.add_slab) and "cells=True" not in inspect.getsource(screen.Screen.add_slab)
    assert src.count("load_screencells") == 2
