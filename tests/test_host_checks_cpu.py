"""The host-side checks the HIP libraries share (cp_pre_amd/csrc/host_checks.h), pinned on the CPU:
  * tests/c_abi/host_checks_main.cpp, a program of its own, built with the host compiler under the address and
    undefined-behaviour sanitizers and run here: span_of on every sign of stride, the halo stride, extent 1, touching and
    overlapping views, offsets that leave int64, bases at both ends of the address space; plane_fits_int32 at both int32
    edges; aligned16; bc_side for every mode on both sides; flat_chunk against the rule as the three flat launchers stated it;
  * a view whose offsets leave int64 (a batch stride of 2**62) is refused by one entry point each of the pair, vjp, vjpflat
    and wgrad libraries with the code its header documents.  The addresses are not mapped and nothing is dereferenced: a
    refusal that reached a launch could not return its code here."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cp_pre_amd", "csrc")


def test_host_checks_program_runs_clean_under_sanitizers(tmp_path):
    exe = tmp_path / "host_checks"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c_abi", "host_checks_main.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host checks ok" in r.stdout, r.stdout + r.stderr


def test_each_shared_helper_is_defined_once():
    """one definition in the directory of what used to be copied per library, and no template-only switch"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    for pattern, home in ((r"^(?:inline )?bool star_of_taps\(", "star_march.h"), (r"^struct Span\b", "host_checks.h"),
                          (r"^(?:inline )?bool bc_side\(", "host_checks.h"), (r"^(?:inline )?int flat_chunk\(", "host_checks.h"),
                          (r"^struct VjpNSMomentum\b", "vjp_functors.h"), (r"^struct Cross\b", "host_checks.h"),
                          (r"^struct BCInfo\b", "host_checks.h"), (r"void screen_plane\(", "screen_plane.h")):
        found = [f for f, s in text.items() if re.search(pattern, s, flags=re.M)]
        assert found == [home], (pattern, found)
    assert not any("PRE_STAR_MARCH_TEMPLATES_ONLY" in s or '#include "star_march.hip"' in s for s in text.values())
    assert "hip/" not in text["host_checks.h"] and "common.h" not in text["host_checks.h"]


def test_a_view_whose_offsets_leave_int64_is_refused_with_the_documented_code():
    from cp_pre_amd import _lib
    B, T, X, Y = 2, 4, 8, 16
    big = 2 ** 62

    def dense(base, sb=None):            # [B,T,X,Y], Y fastest
        return _lib.PreField(base, T * X * Y if sb is None else sb, X * Y, Y, 1)

    def nt_fast(base, sb=None):          # the same logical view with memory [B,X,Y,T]
        return _lib.PreField(base, T * X * Y if sb is None else sb, 1, Y * T, T)

    def pair_of(mk, base, sb=None):
        return (_lib.PreField * 2)(mk(base, sb), mk(base + 0x01000000, sb))

    k27 = [0.0] * 27
    k27[13] = 1.0
    Ka, Kb = _lib.farr(k27), _lib.farr(k27)
    a0, b0, o0 = 0x10000000, 0x20000000, 0x30000000

    pair = _lib.load_pair().pre_pair_linear2_f32
    for a, b, out in ((pair_of(dense, a0, big), pair_of(dense, b0), dense(o0)), (pair_of(dense, a0), pair_of(dense, b0, -big), dense(o0)),
                      (pair_of(dense, a0), pair_of(dense, b0), dense(o0, big))):
        assert pair(a, b, ctypes.byref(out), Ka, Kb, 0.5, B, T, X, Y, 0, None) == _lib.PRE_E_SHAPE
    assert pair(pair_of(dense, a0), pair_of(dense, b0), ctypes.byref(dense(a0 + 4 * (T * X * Y * B - 1))), Ka, Kb, 0.5, B, T, X, Y, 0,
                None) == _lib.PRE_E_SHAPE                                                   # out on the last float of a[0]

    for load, mk in ((_lib.load_vjp, dense), (_lib.load_vjpflat, nt_fast)):
        lib = load()
        fn = lib.pre_vjp_linear2_f32 if mk is dense else lib.pre_vjpflat_linear2_f32
        for g, out in ((mk(a0, big), pair_of(mk, o0)), (mk(a0), pair_of(mk, o0, big)), (mk(a0, -big), pair_of(mk, o0))):
            assert fn(ctypes.byref(g), out, Ka, Kb, 0.5, 1.0, None, B, T, X, Y, 0, None) == _lib.PRE_E_SHAPE
        assert fn(ctypes.byref(mk(a0)), pair_of(mk, a0 + 4 * (T * X * Y * B - 1)), Ka, Kb, 0.5, 1.0, None, B, T, X, Y, 0,
                  None) == _lib.PRE_E_SHAPE                                                 # out[0] on the last float of g

    wgrad = _lib.load_wgrad().pre_wgrad_stencil3d_f32
    work, dk = ctypes.c_void_p(0x40000000), ctypes.c_void_p(0x50000000)
    for g, x in ((dense(a0, big), dense(b0)), (dense(a0), dense(b0, big)), (dense(a0), dense(b0, -big))):
        assert wgrad(ctypes.byref(g), ctypes.byref(x), None, 3, 3, 3, 1.0, None, B, T, X, Y, 0, work, dk, None) == _lib.PRE_E_SHAPE
    assert wgrad(ctypes.byref(dense(a0)), ctypes.byref(dense(b0)), None, 3, 3, 3, 1.0, None, B, T, X, Y, 0, work,
                 ctypes.c_void_p(b0 + 4 * (T * X * Y * B - 1)), None) == _lib.PRE_E_SHAPE    # dk on the last float of x
