"""Coverage at ten levels: one pass (inductive_cp.emp_cov_levels / emp_cov_joint_levels) against the loop of ten existing
per-level calls (emp_cov / emp_cov_joint), at the configurations' shapes.  Prints one JSON line per case: ms per call
(device events around a host-synchronised call, median of --reps), TB/s of the bytes the pass reads once (y, and the
centre when there is one), and the speed-up.  Both sides are checked equal before they are timed.

    python tools/coverage_levels_bench.py [--reps 5] [--cases c4,c4_centre,c3_slab,c5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cp_pre_amd import inductive_cp as icp  # noqa: E402
from cp_pre_amd import pipeline  # noqa: E402

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


def loop(qs, y, centre=None, modulation=None, joint=False):
    res = []
    for q in qs:
        hw = q if modulation is None else q * modulation
        sets = [-hw, hw] if centre is None else [centre - hw, centre + hw]
        res.append(icp.emp_cov_joint(sets, y) if joint else icp.emp_cov(sets, y))
    return np.array(res)


def case(name, y, q, reps, centre=None, modulation=None, joint=False):
    one = (lambda: icp.emp_cov_joint_levels(q, y, modulation, centre=centre)) if joint else \
        (lambda: icp.emp_cov_levels(q, y, centre=centre))
    t1, r1 = timed(one, reps)
    tl, rl = timed(lambda: loop(q, y, centre, modulation, joint), max(1, reps // 2))
    assert np.array_equal(r1, rl), (name, r1, rl)
    nbytes = y.numel() * 4 * (2 if centre is not None else 1)
    print(json.dumps({"case": name, "shape": list(y.shape), "nk": int(q.shape[0]), "centre": centre is not None,
                      "one_pass_ms": round(t1, 3), "loop_ms": round(tl, 3), "tb_s": round(nbytes / t1 / 1e9, 3),
                      "speedup": round(tl / t1, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="c4,c4_centre,c3_slab,c5")
    args = ap.parse_args()
    want = set(args.cases.split(","))
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    if want & {"c4", "c4_centre"}:
        shape = (1024, 62, 254, 254)                                 # C4 per rank
        cal = torch.randn(256, *shape[1:], device=dev, generator=gen).abs_()
        q = pipeline.marginal_qhat(cal, ALPHAS)                      # per-cell q-hats [10, 62, 254, 254]
        del cal
        y = torch.randn(*shape, device=dev, generator=gen)
        if "c4" in want:
            case("c4_marginal", y, q, args.reps)
        if "c4_centre" in want:
            c = torch.randn(*shape, device=dev, generator=gen).mul_(0.1)
            case("c4_marginal_centre", y, q, args.reps, centre=c)
            del c
        del y, q
    if "c3_slab" in want:
        slab = torch.randn(1024, 16, 258, 258, device=dev, generator=gen)     # a C3 x-slab, cropped like the reference
        y = slab[:, 1:-1, 1:-1, 1:-1]
        q = pipeline.marginal_qhat(y[:256].abs(), ALPHAS)
        case("c3_slab_cropped", y, q, args.reps)
        del slab, y, q
    if "c5" in want:
        shape = (8192, 198, 510)                                     # C5 joint shard
        cal = torch.randn(*shape, device=dev, generator=gen)
        jc = pipeline.JointCalibration(shape[0], dev, prune=False)
        jc.add_slab(cal.unsqueeze(1), crop=(0, 0, 0))                # [n, 1, X, Y]: one T-plane, nothing cropped
        q = jc.finish(ALPHAS)
        mod = jc.modulation[0][0]
        del cal
        y = torch.randn(*shape, device=dev, generator=gen)
        case("c5_joint", y, q, args.reps, modulation=mod, joint=True)


if __name__ == "__main__":
    main()
