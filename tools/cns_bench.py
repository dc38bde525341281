"""The compressible-NS right-hand side on one GPU (``cp_pre_amd.cns.Euler_FV_OS_rhs``), at [64,4,512,512] and
[1024,4,128,128] with the reference's dx = 1/128.  Blocks of, interleaved call by call on the same tensors:
  (a) the fused forward (one launch of ``libcp_pre_cns.so``);
  (b) the same module with ``fused=False``: the operators composed as the reference composes them (eleven stencil passes,
      the elementwise passes and the ``cat``);
  (c) ``step(vars, h)`` (the epilogue in the same launch) against ``vars + h * forward(vars)``;
  (d) a device copy of the bytes (a) moves, ``dst.copy_(src)`` of a tensor of vars' size: the ceiling of this run.
Each timing is the median of --reps device-event measurements after --warmup calls, with the spread.  An eager call
downloads the five 3x3 operator kernels first (``_dispatch.host_kernel``: stale taps are a wrong answer), which stalls the
host five times; (a) and the step are therefore ALSO timed as replays of a captured graph (the taps of the capture, no
host work): the device time of the launch.  Achieved bytes/s are the algorithmic 32 B per cell (4 reads, 4 writes), 48 B
with the epilogue, over that time, next to the copy's 32 B per cell over its time.  (a) and (b) are checked against each
other before they are timed.  Plain text lines on stdout and in --out.

``--cases vjp`` measures the backward instead, at the same two shapes and interleaved in the same way:
  (a) the fused VJP launch alone (``libcp_pre_cnsvjp.so``): ``m.vjp(vars, g, out=)`` as the replay of a captured graph;
  (b) ``rhs.sum().backward()`` through a module built with ``backward="fused"`` (the backward call alone: the forward and
      the sum are formed before the first event);
  (c) the same through the default module (``backward="recompute"``, ``_dispatch._Recompute``: the composed expression is
      run again with grad enabled and autograd walks it backwards);
  (d) a device copy of the 48 B per cell (a) moves (8 planes read, 4 written): ``dst.copy_(src)`` of a [BS,6,Nx,Ny] tensor.
(b) and (c) are checked against each other before they are timed.

    python tools/cns_bench.py [--cases forward|vjp] [--reps 15] [--warmup 3] [--out profiles/cns/cns_bench.txt]
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cp_pre_amd import cns  # noqa: E402

SHAPES = ((64, 4, 512, 512), (1024, 4, 128, 128))
CONFIG = {"Physics": {"dx": 1 / 128, "dy": 1 / 128}}
H = 1e-5


def _ev():
    return torch.cuda.Event(enable_timing=True)


def alternate_spread(fns, reps, warmup):
    """(median, min, max) ms of each fn, the fns interleaved call by call"""
    for _ in range(warmup):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = _ev(), _ev()
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def captured(fn):
    """fn (already called once eagerly) as the replay of a captured graph"""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    return graph.replay, keep


def backward_alone(m, v):
    """A timed call: ``m(v).sum()`` formed first, then the events around ``backward()`` alone."""
    def timed():
        v.grad = None
        s = m(v).sum()
        a, b = _ev(), _ev()
        a.record()
        s.backward()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    return timed


def vjp_cases(args, dev, g, emit):
    fused, default = cns.Euler_FV_OS_rhs(CONFIG, dev, backward="fused"), cns.Euler_FV_OS_rhs(CONFIG, dev)
    for shape in SHAPES:
        v = torch.rand(*shape, device=dev, generator=g).add_(0.5)
        cot = torch.randn(*shape, device=dev, generator=g)
        out = torch.empty_like(v)
        src = torch.rand(shape[0], 6, shape[2], shape[3], device=dev, generator=g)
        dst = torch.empty_like(src)
        x = v.clone().requires_grad_()
        fused(x).sum().backward()
        route = cns.last_backward_route()
        gb = x.grad
        x.grad = None
        default(x).sum().backward()
        gc = x.grad
        err = max(float((gb[:, c] - gc[:, c]).abs().max() / gc[:, c].abs().max()) for c in range(4))
        del gb, gc
        with torch.no_grad():
            fused.vjp(v, cot, out=out)
            ga, _ka = captured(lambda: fused.vjp(v, cot, out=out))
        b, c = backward_alone(fused, x), backward_alone(default, x)

        def event_timed(f):
            def timed():
                a, e = _ev(), _ev()
                a.record()
                f()
                e.record()
                e.synchronize()
                return a.elapsed_time(e)
            return timed

        fns = [event_timed(ga), b, c, event_timed(lambda: dst.copy_(src))]
        names = ("a vjp as graph replay", "b backward, fused", "c backward, recompute", "d device copy 48 B/cell")
        for _ in range(args.warmup):
            for f in fns:
                f()
        times = [[] for _ in fns]
        for _ in range(args.reps):
            for i, f in enumerate(fns):
                times[i].append(f())
        res = {n: (sorted(t)[len(t) // 2], min(t), max(t)) for n, t in zip(names, times)}
        cells = v.numel() // 4
        emit(f"{list(shape)}: backward route {route}; max channel |fused - recompute| / max = {err:.2e}")
        for n in names:
            m, lo, hi = res[n]
            emit(f"    {n:<24s} {m:8.3f} ms [{lo:.3f}, {hi:.3f}]")
        ta, tb, tc, td = (res[n][0] for n in names)
        emit(f"    (c)/(b) = {tc / tb:.2f}x (slowest b {res[names[1]][2]:.3f} ms against fastest c {res[names[2]][1]:.3f} ms); "
             f"(a)/(d) = {ta / td:.2f}: the launch runs at {td / ta:.2f} of the copy's rate")
        emit(f"    achieved: (a) 48 B x {cells} cells / replay = {48 * cells / ta / 1e9:.2f} TB/s, copy = {48 * cells / td / 1e9:.2f} TB/s")
        del v, cot, out, src, dst, x, ga, _ka
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", choices=("forward", "vjp"), default="forward")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "cns", "cns_bench.txt" if args.cases == "forward" else "cns_vjp_bench.txt")
    assert torch.cuda.is_available(), "cns_bench needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    if args.cases == "vjp":
        emit(f"# cns_bench --cases vjp {datetime.date.today().isoformat()} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
             f"reps {args.reps}, warmup {args.warmup}; median ms [min, max], device events around one call, blocks interleaved")
        vjp_cases(args, dev, g, emit)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    emit(f"# cns_bench {datetime.date.today().isoformat()} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
         f"reps {args.reps}, warmup {args.warmup}; median ms [min, max], device events around one call, blocks interleaved")
    fused, composed = cns.Euler_FV_OS_rhs(CONFIG, dev), cns.Euler_FV_OS_rhs(CONFIG, dev, fused=False)
    for shape in SHAPES:
        v = torch.rand(*shape, device=dev, generator=g).add_(0.5)
        out, dst = torch.empty_like(v), torch.empty_like(v)
        with torch.no_grad():
            ra = fused(v)
            route = cns.last_route()
            rb = composed(v)
            err = max(float((ra[:, c] - rb[:, c]).abs().max() / rb[:, c].abs().max()) for c in range(4))
            sa = fused.step(v, H)
            route_step = cns.last_route()
            serr = float((sa - (v + H * rb)).abs().max() / sa.abs().max())
            del ra, rb, sa
            a = lambda: fused(v, out=out)                                   # noqa: E731
            b = lambda: composed(v)                                         # noqa: E731
            c = lambda: fused.step(v, H, out=out)                           # noqa: E731
            c_ref = lambda: v + H * fused(v)                                # noqa: E731
            d = lambda: dst.copy_(v)                                        # noqa: E731
            a(), c()
            ga, _ka = captured(a)
            gc, _kc = captured(c)
            names = ("a fused forward", "a as graph replay", "b composed forward", "c step", "c as graph replay",
                     "c vars + h*forward", "d device copy")
            res = dict(zip(names, alternate_spread([a, ga, b, c, gc, c_ref, d], args.reps, args.warmup)))
        cells = v.numel() // 4
        emit(f"{list(shape)}: routes {route} / {route_step}; max channel |fused - composed| / max = {err:.2e}, step {serr:.2e}")
        for n in names:
            m, lo, hi = res[n]
            emit(f"    {n:<20s} {m:8.3f} ms [{lo:.3f}, {hi:.3f}]")
        ta, tc, td = res["a as graph replay"][0], res["c as graph replay"][0], res["d device copy"][0]
        emit(f"    (b)/(a) eager = {res['b composed forward'][0] / res['a fused forward'][0]:.2f}x, against the replay "
             f"{res['b composed forward'][0] / ta:.2f}x; (vars + h*forward)/(step) eager = "
             f"{res['c vars + h*forward'][0] / res['c step'][0]:.2f}x")
        emit(f"    achieved: (a) 32 B x {cells} cells / replay = {32 * cells / ta / 1e9:.2f} TB/s, step 48 B/cell = "
             f"{48 * cells / tc / 1e9:.2f} TB/s, copy 32 B/cell = {32 * cells / td / 1e9:.2f} TB/s; (a) at "
             f"{td / ta:.2f} of the copy's rate, the step at {1.5 * td / tc:.2f}")
        del v, out, dst, ga, gc, _ka, _kc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
