#!/usr/bin/env python3
"""A/B of several builds of libcp_pre_hip.so on the marched residual kernels, alternated launch by launch in ONE process
(lib_ab.py's method, for more than two libraries and the shapes the store-policy change was judged on):

    python tools/exp/march_store_ab.py --lib parent=tools/exp/var/libcp_pre_hip.parent.so --lib A=... [--reps 7] [--only c3]

The first --lib is the baseline.  Per shape and library: the median of --reps launches, for the baseline also the spread
(min .. max) of its own repetitions, and whether the library's output equals the baseline's bit for bit.  Shapes: the
benchmark's two x-slab calls and its marginal call (bench.C3Stream, full batch), the strong-rank job, C4 induction and
momentum, C2 wave, C5 Burgers, and NS momentum / MHD induction on Nt-fastest views (the flat form)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cp_pre_amd import _lib                      # noqa: E402
from cp_pre_amd import residuals as R            # noqa: E402


def handle(path):
    _lib._lib = None
    _lib.SO_PATH = path
    return _lib.load()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, help="name=path; the first one is the baseline")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated groups: c3, strong, c4, single, flat (default: all)")
    ap.add_argument("--batch", type=int, default=4096, help="batch of the C3 slab calls")
    args = ap.parse_args()
    names = [s.split("=", 1)[0] for s in args.lib]
    libs = {s.split("=", 1)[0]: handle(os.path.join(ROOT, s.split("=", 1)[1])) for s in args.lib}
    only = set(filter(None, args.only.split(",")))
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    base = names[0]
    print(f"{'shape':52s} " + " ".join(f"{n:>9s}" for n in names) + f"   {base} min..max   ratios to {base}   equal", flush=True)

    def measure(name, fn, out_of):
        """fn() launches once; out_of(r) is the tensor the launch wrote"""
        times = {n: [] for n in names}
        ref, same = None, {}
        for rep in range(args.reps + 1):
            for tag in names:
                _lib._lib = libs[tag]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn()
                e1.record()
                torch.cuda.synchronize()
                if rep:                                   # the first round warms every library up ...
                    times[tag].append(e0.elapsed_time(e1))
                elif tag == base:                         # ... and compares the results (a 1/64 sample of the batch is kept)
                    o = out_of(r)
                    ref = o[::64].clone()
                else:
                    same[tag] = bool(torch.equal(out_of(r)[::64], ref))
                del r
        med = {n: sorted(times[n])[len(times[n]) // 2] for n in names}
        print(f"{name:52s} " + " ".join(f"{med[n]:9.3f}" for n in names) +
              f"   {min(times[base]):.3f}..{max(times[base]):.3f}   " +
              " ".join(f"{n} {med[n] / med[base]:.4f}" for n in names[1:]) + "   " +
              " ".join(f"{n} {'==' if same[n] else 'DIFFERS'}" for n in names[1:]), flush=True)

    if not only or "c3" in only:
        import bench
        st = bench.C3Stream(args.batch, 64, 512, 512, 128, "x", dev)
        for mode in ("joint", "marginal"):
            views = st.views(mode)
            for s, sl in ((0, 128), (2, 127)) if mode == "joint" else ((0, 128),):
                res = views[sl]
                measure(f"C3 {mode} x-slab [{args.batch},3,64,{sl + 2},512] -> {sl} rows",
                        lambda: st.eval_slab(s, sl, res, absolute=mode == "marginal"), lambda r: res)
        st.free()
        del st, views, res
        torch.cuda.empty_cache()
    if not only or "strong" in only:
        v = torch.rand(512, 3, 64, 512, 512, device=dev, generator=g).add_(0.5)
        ns = R.NavierStokes(1e-2, 1 / 512, 1 / 512, nu=1e-3)
        out = torch.empty(512, 64, 512, 512, device=dev)
        measure("strong-rank NS momentum [512,3,64,512,512]", lambda: ns.residual_momentum(v, boundary=True, out=out), lambda r: out)
        del v, out
        torch.cuda.empty_cache()
    if not only or "c4" in only:
        w = torch.rand(1024, 6, 64, 256, 256, device=dev, generator=g).add_(0.5)
        mhd = R.MHD()
        measure("C4 MHD induction [1024,6,64,256,256]", lambda: mhd.residual_induction(w, boundary=True), lambda r: r)
        measure("C4 MHD momentum [1024,6,64,256,256]", lambda: mhd.residual_momentum(w, boundary=True), lambda r: r)
        del w
        torch.cuda.empty_cache()
    if not only or "single" in only:
        u2 = torch.randn(512, 32, 256, 256, device=dev, generator=g)
        wave = R.PRE_Wave(dt=0.005, dx=0.01, c=1.0, device=dev)
        measure("C2 wave [512,32,256,256]", lambda: wave.residual(u2, boundary=True), lambda r: r)
        u5 = torch.randn(8192, 200, 512, device=dev, generator=g)
        bur = R.Burgers(2.0 / 512, 1.25 / 200, 0.002)
        measure("C5 Burgers [8192,200,512]", lambda: bur.residual(u5, boundary=True), lambda r: r)
        del u2, u5
        torch.cuda.empty_cache()
    if not only or "flat" in only:
        # the surrogate's native layout [BS,F,Nx,Ny,Nt] seen through permute(0,1,4,2,3): the flat (merged-row) form
        w = torch.rand(1024, 6, 256, 256, 20, device=dev, generator=g).add_(0.5)
        ns = R.NavierStokes(1e-2, 1 / 256, 1 / 256, nu=1e-3)
        mhd = R.MHD()
        measure("flat NS momentum [1024,3,256,256,20] Nt-fastest", lambda: ns.residual_momentum(w[:, :3].permute(0, 1, 4, 2, 3), boundary=True),
                lambda r: r)
        measure("flat MHD induction [1024,6,256,256,20] Nt-fastest", lambda: mhd.residual_induction(w.permute(0, 1, 4, 2, 3), boundary=True),
                lambda r: r)


if __name__ == "__main__":
    main()
