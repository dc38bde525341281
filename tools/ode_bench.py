"""ODE operators on one GPU: the HIP stencil (``pre_ode_stencil_f32``) and the fused DHO split / Bessel residuals
(``pre_ode_residual_f32``) against the composed route a user would otherwise run (``F.conv1d`` per operator plus the
elementwise passes that scale and sum), on a [BS, Nt, S = 2] fp32 state.  Prints one JSON line per case: ms per call
(device events, median of --reps) and GB/s of ALGORITHMIC traffic (each component a case reads, once, plus the [BS, Nt]
result; the coefficient rows are negligible), the same byte count for both routes.  Both routes are checked to agree
before they are timed.

    python tools/ode_bench.py [--reps 10] [--shapes 1048576x1024,65536x100]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cp_pre_amd import ode  # noqa: E402
from cp_pre_amd.convops_0d import stencil  # noqa: E402


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


def conv(x, taps):
    """The composed route's operator: F.conv1d (MIOpen) on the component, as the reference calls it."""
    return F.conv1d(x.unsqueeze(1), taps[None, None], padding=taps.numel() // 2).squeeze(1)


def composed(op, st, dev):
    acc = None
    for comp, kern, _, c in op.terms:
        y = conv(st[..., comp], kern.to(dev))
        if c is not None:
            y = c.to(dev) * y
        acc = y if acc is None else acc + y
    return acc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--shapes", default="1048576x1024,65536x100")
    a = p.parse_args()
    dev = torch.device("cuda:0")
    for shape in a.shapes.split(","):
        bs, nt = (int(v) for v in shape.split("x"))
        st = torch.randn(bs, nt, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        out = torch.empty(bs, nt, device=dev)
        x = np.linspace(0.5, 8.0, nt)
        taps = np.array([1.0, -2.0, 1.0], np.float32)
        cases = {
            "stencil": (lambda: stencil(st[..., 0], taps, out=out),
                        lambda: conv(st[..., 0], torch.from_numpy(taps).to(dev)), 1),
        }
        for name, op, reads in (("dho_split", ode.DHO(1.5, 0.3, 2.0, 0.05, split=True), 2),
                                ("bessel", ode.Bessel(x, 1, x[1] - x[0]), 1)):
            cases[name] = ((lambda op=op: op.residual(st, out=out)), (lambda op=op: composed(op, st, dev)), reads)
        for name, (fused, comp, reads) in cases.items():
            got = fused().clone()
            want = comp()
            err = float((got - want).abs().max() / want.abs().max())
            del want
            assert err <= 1e-5, (name, err)
            gb = (reads + 1) * 4 * bs * nt / 1e9
            tf = timed(fused, a.reps)
            tc = timed(comp, max(1, a.reps // 2))
            print(json.dumps({"case": name, "shape": [bs, nt, 2], "hip_ms": round(tf, 4), "hip_GBps": round(gb / tf * 1e3, 1),
                              "composed_ms": round(tc, 4), "composed_GBps": round(gb / tc * 1e3, 1),
                              "speedup": round(tc / tf, 2), "max_rel_err": err}), flush=True)
        del st, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
