"""Residuals under boundary conditions on the x-y rim, on one GPU: three routes on the same tensors in one process,
alternated call by call and timed with device events after a warm-up:

    (a) the fused BC launch (``bc=``: one pass of ``libcp_pre_bcres.so``);
    (b) the zero-pad launch of the same functor (``pre_residual_*_f32``, what the package ran before ``bc=`` existed; its
        x-y rim is what the callers crop) - the floor (a) is read against;
    (c) the only route that gave the BC result before: ``pad_signal`` of every field (a copy of every field), the residual
        on the (Nx+2) x (Ny+2) grid - whose width is no multiple of 4, so the package takes whatever route it has for it -
        and the crop (a view).

Each figure is the median over ``--blocks`` blocks of ``--reps`` calls, with the range of the block medians: the spread a
comparison has to be read with.  (a) and (b) write into one preallocated buffer where the residual takes ``out=`` (Burgers
does not: both allocate from torch's caching allocator).  One JSON line per case on stdout and appended to ``--out``.

Cases (``--div N`` divides every batch by N; the default runs them whole):
    ns_momentum    NS momentum on [64,3,64,512,512]
    wave           the wave residual on [512,32,256,256]
    mhd_induction  MHD induction on [64,6,64,256,256]
    burgers        Burgers on [8192,200,512]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cp_pre_amd import residuals as R  # noqa: E402

CASES = {"ns_momentum": (64, 3, 64, 512, 512), "wave": (512, 1, 32, 256, 256), "mhd_induction": (64, 6, 64, 256, 256),
         "burgers": (8192, 200, 512)}
DT, DX, DY = 0.01, 1.0 / 64, 1.0 / 64


def make(case, bc):
    """(object, method name) of ``case`` under ``bc`` (None: the zero-pad object)."""
    kw = {} if bc is None else {"bc": bc}
    if case == "ns_momentum":
        return R.NavierStokes(DT, DX, DY, **kw), "residual_momentum"
    if case == "wave":
        return R.PRE_Wave(0.01, 0.02, c=1.0, **kw), "residual"
    if case == "mhd_induction":
        return R.MHD(**kw), "residual_induction"
    return R.Burgers(2.0 / 512, 1.25 / 200, 0.002, **kw), "residual"


def routes(case, v, bc):
    nd = 2 if case == "burgers" else 3
    x = v[:, 0] if case == "wave" else v
    out = None if case == "burgers" else torch.empty(x.shape[:1] + x.shape[-3:], dtype=torch.float32, device=v.device)
    kw = {} if out is None else {"out": out}
    fa, fb, fc = (getattr(*make(case, c)) for c in (bc, None, None))
    spec = R._BC(bc)

    def a():
        return fa(x, boundary=True, **kw)

    def b():
        return fb(x, boundary=True, **kw)

    def c():
        if nd == 2:
            return fc(spec.pad(x, 2), boundary=True)[..., 1:-1]
        if case == "wave":
            return fc(spec.pad(x, 3), boundary=True)[..., 1:-1, 1:-1]
        padded = torch.stack([spec.pad(x[:, i], 3) for i in range(x.shape[1])], dim=1)
        return fc(padded, boundary=True)[..., 1:-1, 1:-1]
    return {"a": a, "b": b, "c": c}


def time_routes(fns, blocks, reps, warmup):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    meds = {k: [] for k in fns}
    for _ in range(blocks):
        times = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        for k in fns:
            meds[k].append(statistics.median(times[k]))
    return {k: (statistics.median(m), min(m), max(m)) for k, m in meds.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--bc", default="wrap")
    ap.add_argument("--div", type=int, default=1)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcres", "bcres_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bcres_bench: no HIP device visible - nothing is measured without one")
    for case in args.cases.split(","):
        shape = (max(1, CASES[case][0] // args.div),) + CASES[case][1:]
        torch.manual_seed(0)
        v = torch.rand(shape, device="cuda") + 0.5
        fns = routes(case, v, args.bc)
        # the three routes compute one thing: (a) against (c) on the whole grid, (a) against (b) inside the rim
        ra = fns["a"]().clone()
        route_a = R.last_route()
        rc = fns["c"]()
        route_c = "zero-pad residual on the padded grid"
        scale = float(ra.abs().max())
        err_ac = float((ra - rc).abs().max()) / scale
        rb = fns["b"]()
        inner = (Ellipsis, slice(1, -1)) if case == "burgers" else (Ellipsis, slice(1, -1), slice(1, -1))
        same_inside = bool(torch.equal(ra[inner], rb[inner]))
        del rc, rb
        t = time_routes(fns, args.blocks, args.reps, args.warmup)
        cells = 1
        for n in (shape[:1] + shape[-(2 if case == "burgers" else 3):]):
            cells *= n
        nf = {"ns_momentum": 3, "wave": 1, "mhd_induction": 4, "burgers": 1}[case]
        line = {"case": case, "shape": list(shape), "bc": args.bc, "route_a": route_a, "route_c": route_c,
                "blocks": args.blocks, "reps": args.reps,
                **{f"{k}_ms": round(t[k][0], 4) for k in t}, **{f"{k}_range_ms": [round(t[k][1], 4), round(t[k][2], 4)] for k in t},
                "a_over_b": round(t["a"][0] / t["b"][0], 4), "c_over_a": round(t["c"][0] / t["a"][0], 3),
                "a_faster_than_c_beyond_spread": bool(t["a"][2] < t["c"][1]),
                "a_algorithmic_TBps": round(4.0 * (nf + 1) * cells / (t["a"][0] * 1e-3) / 1e12, 3),
                "err_a_vs_c": err_ac, "a_equals_b_inside_rim": same_inside}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del fns, v, ra
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
