"""PRE set propagation on one GPU (``libcp_pre_setprop.so``): the fused recipe (``pre_setprop_recipe_f32``, what
``set_pre_bounds`` runs on an fp32 [B, Nt] field) and the general circulant hull (``pre_setprop_bounds_f64`` on fp32
[B, Nt + 1] centre / radius rows).  Prints one JSON line per case: median device-event ms per call (--reps), the fp64 FMA
rate each kernel achieves counting the FMAs it executes for real outputs (recipe: B*N*N for the radius sum over every j,
B*N*k per output tile for the convolution it rebuilds while staging, 4*B*N for the centre; general: 2*B*N*N), the rate of
a plain fp64 FMA loop (tools/setprop_fma_loop.hip) measured in the same run, the host numpy closed form (timed on at most
--host-rows rows and scaled to B, with the thread count it ran with) and, for Nt = 100, one trajectory through the literal
zonotope restatement of the reference (tests/test_set_prop_cpu.py).  Device and host results are checked to agree first.

    python tools/setprop_bench.py [--reps 10] [--shapes 65536x100,65536x1000,1048576x100]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cp_pre_amd import _lib  # noqa: E402
from cp_pre_amd import set_prop as sp  # noqa: E402

SHO_K = np.array([1., -2., 1.]) + (10 / 99) ** 2 * np.array([0., 1., 0.])
TK_OF = lambda n: 64 if n <= 64 else 128 if n <= 128 else 256          # noqa: E731  (set_prop.hip's tile choice)


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def fma_loop_rate(reps):
    """fp64 FMA/s of a plain FMA loop, built here with hipcc for gfx950."""
    d = tempfile.mkdtemp(prefix="setprop_fma_")
    so = os.path.join(d, "fma_loop.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "-shared", "--offload-arch=gfx950",
                           os.path.join(ROOT, "tools", "setprop_fma_loop.hip"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.fma_loop.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    blocks, iters = 8192, 8192
    out = torch.empty(blocks * 256, dtype=torch.float64, device="cuda")
    run = lambda: _lib.check(lib.fma_loop(_lib.ptr(out), blocks, iters, 0.999999, _lib.stream()), "fma_loop")  # noqa: E731
    ms = timed(run, reps)
    return blocks * 256 * 8 * iters / (ms * 1e-3), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="65536x100,65536x1000,1048576x100")
    ap.add_argument("--host-rows", type=int, default=2048)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "setprop_bench needs the MI355X"
    dev = torch.device("cuda:0")
    peak, peak_ms = fma_loop_rate(args.reps)
    literal = None
    for shape in args.shapes.split(","):
        B, nt = (int(v) for v in shape.split("x"))
        N, k = nt + 1, len(SHO_K)
        torch.manual_seed(0)
        t = torch.linspace(0, 10, nt)
        x = (torch.cos(t) + 0.05 * torch.randn(B, nt)).to(dev)
        lo, hi = sp.set_pre_bounds(x, SHO_K)                             # warm: tables built and uploaded
        rows = min(B, args.host_rows)
        xh = x[:rows].cpu().numpy()
        t0 = time.perf_counter()
        lo_h, hi_h = sp.set_pre_bounds(xh, SHO_K)
        host_ms = (time.perf_counter() - t0) * 1e3 * B / rows
        err = max(np.abs(lo[:rows].cpu().numpy() - lo_h).max(), np.abs(hi[:rows].cpu().numpy() - hi_h).max())
        width = float(np.median(hi_h - lo_h))
        assert err <= 1e-9 * max(np.abs(lo_h).max(), 1.0), err
        recipe_ms = timed(lambda: sp.set_pre_bounds(x, SHO_K), args.reps)
        tiles = -(-N // TK_OF(N))
        recipe_fma = B * N * N + B * N * k * tiles + 4 * B * N
        del lo, hi
        c = torch.randn(B, N, device=dev)
        r = torch.rand(B, N, device=dev)
        key = sp.recipe_key(SHO_K, nt)
        g, a = sp._device_tables(key, "interval_fft", dev)
        lo = torch.empty(B, N, dtype=torch.float64, device=dev)
        hi = torch.empty_like(lo)
        lib = _lib.load_setprop()
        st = _lib.iarr64(c.stride())

        def general():
            _lib.check(lib.pre_setprop_bounds_f64(_lib.ptr(c), st, _lib.ptr(r), st, B, N, _lib.ptr(g), _lib.ptr(a), _lib.ptr(lo),
                                                  _lib.ptr(hi), 0, _lib.stream()), "pre_setprop_bounds_f64")
        general_ms = timed(general, args.reps)
        del c, r, lo, hi, x
        torch.cuda.empty_cache()
        if nt == 100 and literal is None:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from test_set_prop_cpu import literal_set_PRE
            t0 = time.perf_counter()
            literal_set_PRE(xh[0], SHO_K)
            literal = (time.perf_counter() - t0) * 1e3
        print(json.dumps({
            "case": f"[{B}, {nt}]", "N": N, "taps": k,
            "recipe_ms": round(recipe_ms, 4), "recipe_fp64_fma_per_s": float(f"{recipe_fma / (recipe_ms * 1e-3):.4g}"),
            "general_ms": round(general_ms, 4),
            "general_fp64_fma_per_s": float(f"{2 * B * N * N / (general_ms * 1e-3):.4g}"),
            "fma_loop_fp64_fma_per_s": float(f"{peak:.4g}"), "fma_loop_ms": round(peak_ms, 4),
            "host_numpy_ms": round(host_ms, 1), "host_rows_timed": rows, "host_threads": os.environ["OMP_NUM_THREADS"],
            "literal_one_trajectory_ms": None if literal is None or nt != 100 else round(literal, 1),
            "device_vs_host_max_abs": float(f"{err:.3g}"), "median_width": float(f"{width:.4g}"),
        }), flush=True)


if __name__ == "__main__":
    main()
