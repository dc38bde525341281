"""Solution bounds by sample acceptance at ten levels (cp_pre_amd.sample_bounds) against the torch per-level loop, at the
configurations' shapes.  Prints one JSON line per (case, pass): ms per call (device events around a host-synchronised
call, median of --reps), TB/s of the bytes the pass must read once (u for the envelope; r and u for joint - acceptance
then envelope - and for cellwise), and the speed-up over the torch loop (one masked gather + amin / amax per level; for
cellwise one where + amin / amax / sum per level).  Both sides are checked equal (NaN-aware) before they are timed.  The
levels of the envelope and joint passes are nested (joint q-hats at alphas 0.05 .. 0.95).

    python tools/sample_bounds_bench.py [--reps 5] [--cases c2,c4_ntfast,c5,ode] [--passes envelope,joint,cellwise]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cp_pre_amd import sample_bounds as sb  # noqa: E402

ALPHAS = [0.05 + 0.1 * i for i in range(10)]


def timed(fn, reps):
    fn()                                            # warm-up (code objects, allocator)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), r


def same(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na], b[~nb]))


def torch_envelope(u, acc):
    lo, hi = [], []
    for k in range(acc.shape[0]):
        sel = u[acc[k]]
        if sel.shape[0]:
            lo.append(sel.amin(0))
            hi.append(sel.amax(0))
        else:
            lo.append(torch.full(u.shape[1:], float("inf"), device=u.device))
            hi.append(torch.full(u.shape[1:], float("-inf"), device=u.device))
    return torch.stack(lo), torch.stack(hi), acc.sum(1)


def torch_joint(u, r, q):
    score = r.abs().amax(dim=tuple(range(1, r.dim())))
    acc = torch.stack([score <= qk for qk in q])
    return torch_envelope(u, acc)


def torch_cellwise(u, r, q):
    lo, hi, cnt = [], [], []
    for qk in q:
        ins = r.abs() <= qk
        lo.append(torch.where(ins, u, float("inf")).amin(0))
        hi.append(torch.where(ins, u, float("-inf")).amax(0))
        cnt.append(ins.sum(0, dtype=torch.int32))
    return torch.stack(lo), torch.stack(hi), torch.stack(cnt)


def emit(name, pas, u, nbytes, t1, tl):
    print(json.dumps({"case": name, "pass": pas, "shape": list(u.shape), "nk": len(ALPHAS), "ms": round(t1, 3),
                      "torch_loop_ms": round(tl, 3), "tb_s": round(nbytes / t1 / 1e9, 3), "speedup": round(tl / t1, 2)}),
          flush=True)


def run(name, u, r, reps, passes):
    # joint q-hats: quantiles of the per-sample max |r| (the joint score without modulation): nested levels
    score = r.abs().amax(dim=tuple(range(1, r.dim())))
    q = torch.quantile(score.double(), torch.tensor([1 - a for a in ALPHAS], device=u.device, dtype=torch.float64))
    q = q.to(torch.float32)
    acc = torch.stack([score <= qk for qk in q])
    ub, rb = u.numel() * 4, r.numel() * 4
    if "envelope" in passes:
        t1, got = timed(lambda: sb.sample_envelope(u, acc), reps)
        tl, want = timed(lambda: torch_envelope(u, acc), max(1, reps // 2))
        assert all(same(g, w) for g, w in zip(got, want)), (name, "envelope")
        emit(name, "envelope", u, ub, t1, tl)
    if "joint" in passes:
        t1, got = timed(lambda: sb.sample_bounds(u, r, q, rule="joint"), reps)
        tl, want = timed(lambda: torch_joint(u, r, q), max(1, reps // 2))
        assert all(same(g, w) for g, w in zip(got, want)), (name, "joint")
        emit(name, "joint", u, ub + rb, t1, tl)
    if "cellwise" in passes:
        qc = torch.linspace(0.5, 2.5, len(ALPHAS), device=u.device)
        t1, got = timed(lambda: sb.sample_bounds(u, r, qc, rule="cellwise"), reps)
        tl, want = timed(lambda: torch_cellwise(u, r, qc), max(1, reps // 2))
        assert all(same(g, w) for g, w in zip(got, want)), (name, "cellwise")
        emit(name, "cellwise", u, ub + rb, t1, tl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="c2,c4_ntfast,c5,ode")
    ap.add_argument("--passes", default="envelope,joint,cellwise")
    args = ap.parse_args()
    want, passes = set(args.cases.split(",")), set(args.passes.split(","))
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = {"c2": (512, 32, 256, 256), "c5": (8192, 200, 512), "ode": (1 << 20, 100)}
    for name in ("c2", "c4_ntfast", "c5", "ode"):
        if name not in want:
            continue
        if name == "c4_ntfast":      # C4 shard as the reference callers pass it: [n, Nt, Nx, Ny] view of [n, Nx, Ny, Nt]
            u = torch.randn(1024, 256, 256, 64, device=dev, generator=gen).permute(0, 3, 1, 2)
            r = torch.randn(1024, 256, 256, 64, device=dev, generator=gen).permute(0, 3, 1, 2)
        else:
            u = torch.randn(*shapes[name], device=dev, generator=gen)
            r = torch.randn(*shapes[name], device=dev, generator=gen)
        run(name, u, r, args.reps, passes)
        del u, r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
