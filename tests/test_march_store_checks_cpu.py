"""plane_offsets_fit_u32 (cp_pre_amd/csrc/host_checks.h) on the CPU: the host-side check behind the 32-bit lane offsets of
the marched kernels - an input view that fails it is refused, an output view that fails it keeps the store through a
64-bit pointer (star_march.h: launch_tiled, Geom::obuf).  tests/c_abi/march_store_checks_main.cpp, a program of its own, is
built with the host compiler under the address and undefined-behaviour sanitizers and run here: both sides of the 2^32
limit reached with a stride argument (nothing that large is allocated), negative strides, arithmetic that leaves int64."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cp_pre_amd", "csrc")


def test_march_store_checks_program_runs_clean_under_sanitizers(tmp_path):
    exe = tmp_path / "march_store_checks"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c_abi", "march_store_checks_main.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "march store checks ok" in r.stdout, r.stdout + r.stderr


def test_the_marched_launch_asks_the_helper_for_inputs_and_output():
    """one statement of the rule: launch_tiled calls the helper for every input view and for the output view, and keeps
    no copy of the arithmetic"""
    src = open(os.path.join(CSRC, "star_march.h")).read()
    body = src[src.index("int launch_tiled("):src.index("// ---", src.index("int launch_tiled("))]
    assert len(re.findall(r"plane_offsets_fit_u32\(g\.sX\[i\]", body)) == 1
    assert len(re.findall(r"plane_offsets_fit_u32\(g\.oX", body)) == 1
    assert "1LL << 32" not in body
    defs = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))
            and re.search(r"^inline bool plane_offsets_fit_u32\(", open(os.path.join(CSRC, f)).read(), flags=re.M)]
    assert defs == ["host_checks.h"]
