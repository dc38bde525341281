"""Host-side A/B of the fused losses and screens: the same bits and the same Python cost of a call across a change that
touches only the host code (``cp_pre_amd/losses.py``, ``screen.py`` and what they share).  The kernels are deterministic,
so for equal inputs two host sides that marshal the same arguments give bitwise equal outputs.

For one fixed seed the smallest case of every fused route runs once: ``pi_loss`` + ``backward``, ``pisl_loss`` +
``backward``, ``residual_vjp`` and ``kernel_vjp`` for stencil3d, stencil2d, linear2, ns_momentum, burgers, their ``flat_``
forms and ``+wgrad``; ``screen()`` for stencil3d, linear2 (NS continuity and MHD gauss), ns_momentum, the four ``mhd_*``,
the ``flat_`` forms of each and ``rows_stencil2d`` / ``rows_burgers`` in both layouts; one CPU input and one box kernel
for the fallbacks.  Shapes: [2,F,6,8,12] and Nt-fastest views of memory [2,F,8,12,6] (F = 3 for NS, once 4; 6 for MHD),
[3,8,12] and its Nt-fastest transpose.  Only the public entry points are called, so the same file runs on both commits.

    python tools/host_ab.py --dump FILE       # at the first commit: outputs and last_route() strings of every case
    python tools/host_ab.py --compare FILE    # at the second: every tensor bitwise equal, every route equal, or exit 1
    python tools/host_ab.py --time            # median wall time (device synchronised) of 200 calls of screen() and of
                                              # pi_loss() + backward() on NS momentum at the tiny shape: one JSON line
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cp_pre_amd import losses, screen  # noqa: E402
from cp_pre_amd import residuals as R  # noqa: E402
from cp_pre_amd.convops_1d import ConvOperator as C1  # noqa: E402
from cp_pre_amd.convops_2d import ConvOperator as C2  # noqa: E402

DEV = "cuda"
T, X, Y = 6, 8, 12


def methods(device=DEV):
    ns, mhd = R.NavierStokes(0.01, 1 / 64, 1 / 32, nu=0.001, device=device), R.MHD(device=device)
    m = {"stencil3d": (R.PRE_Wave(0.01, 0.02, device=device).residual, 0), "op3d": (C2(("x", "y"), 2, device=device), 0),
         "linear2": (ns.residual_continuity, 3), "ns_momentum": (ns.residual_momentum, 3), "ns_momentum_f4": (ns.residual_momentum, 4),
         "mhd_gauss": (mhd.residual_gauss, 6), "stencil2d": (R.Advection(1.0, 0.005, 0.01, device=device).residual, None),
         "op2d": (C1("x", 2, device=device), None), "burgers": (R.Burgers(0.05, 0.01, 0.002, device=device).residual, None)}
    for eq in ("continuity", "momentum", "energy", "induction"):
        m["mhd_" + eq] = (getattr(mhd, "residual_" + eq), 6)
    return m


def field(F, gen, nt_fastest, device=DEV):
    """F None: [3,8,12] (the 1-D family); 0: a field [2,T,X,Y]; else stacked [2,F,T,X,Y].  ``nt_fastest``: the same logical
    shape as a view of memory whose last axis is Nt."""
    if F is None:
        shape, perm = (3, 8, 12), (0, 2, 1)
    elif F == 0:
        shape, perm = (2, T, X, Y), (0, 2, 3, 1)
    else:
        shape, perm = (2, F, T, X, Y), (0, 1, 3, 4, 2)
    x = (torch.rand(shape, generator=gen) + 0.5).to(device)
    if nt_fastest:
        inv = [perm.index(i) for i in range(len(perm))]
        x = x.permute(perm).contiguous().permute(inv)
    return x


def operator_of(method):
    return method if isinstance(method, (C1, C2)) else getattr(method.__self__, "D", None)


def loss_cases(out):
    gen = torch.Generator().manual_seed(1234)
    plan = [(k, False, False) for k in ("stencil3d", "op3d", "stencil2d", "op2d", "linear2", "ns_momentum", "ns_momentum_f4", "burgers")]
    plan += [(k, True, False) for k in ("stencil3d", "linear2", "ns_momentum", "ns_momentum_f4")]
    plan += [("stencil3d", False, True), ("stencil2d", False, True), ("stencil3d", True, True)]
    for kind, flat, wgrad in plan:
        method, F = methods()[kind]
        op = operator_of(method)
        if wgrad:
            op.kernel.requires_grad_(True)
        tag = "loss/" + ("flat_" if flat else "") + kind + ("+wgrad" if wgrad else "")
        x, yy = field(F, gen, flat), field(F, gen, flat)
        kw = dict(flat=flat, **({"wgrad": True} if wgrad else {}))
        for name, fn in (("pi", lambda v: losses.pi_loss(method, v, **kw)), ("pisl", lambda v: losses.pisl_loss(method, v, yy, **kw))):
            v = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            if wgrad:
                op.kernel.grad = None
            loss = fn(v)
            route = losses.last_route()
            (0.75 * loss).backward()
            out[tag + "/" + name] = ([loss.detach(), v.grad] + ([op.kernel.grad.clone()] if wgrad else []), route)
        if wgrad:
            op.kernel.requires_grad_(False)
        for boundary in (False, True):
            inner = [n if boundary else n - 2 for n in (x.shape[2:] if x.dim() == 5 else x.shape[1:])]
            g = (torch.rand([x.shape[0]] + inner, generator=gen) - 0.5).to(DEV)
            if wgrad:                                        # (g is drawn all the same: one random stream for every case)
                continue
            out[f"{tag}/residual_vjp/{boundary}"] = ([losses.residual_vjp(method, x, g, boundary=boundary, flat=flat)], losses.last_route())
            if kind.startswith(("stencil", "op")):
                out[f"{tag}/kernel_vjp/{boundary}"] = ([losses.kernel_vjp(method, x, g, boundary=boundary, minus=yy)], losses.last_route())
    # the fallbacks: a CPU input, a box kernel
    method, F = methods("cpu")["ns_momentum"]
    v = field(F, gen, False, "cpu").requires_grad_(True)
    losses.pi_loss(method, v).backward()
    out["loss/cpu_input"] = ([v.grad], losses.last_route())
    method, F = methods()["ns_momentum"]
    method.__self__.D_x.kernel.data[0, 0, 0] = 0.5
    v = field(F, gen, False).requires_grad_(True)
    losses.pi_loss(method, v).backward()
    out["loss/box_kernel"] = ([v.grad], losses.last_route())


def screen_cases(out):
    gen = torch.Generator().manual_seed(4321)
    q = torch.tensor([0.01, 0.1, 1.0], device=DEV)

    def run(tag, method, x, shape, device=DEV):
        for boundary in (False, True):
            for mod in (None, (torch.rand(shape, generator=gen) + 0.5).to(device)):
                s = screen.screen(method, x, q.to(device), mod, boundary=boundary)
                out[f"screen/{tag}/{boundary}/{mod is not None}"] = ([s.score, s.inside, torch.tensor(s.cells)], screen.last_route())

    for kind, (method, F) in methods().items():
        if F is None:
            for nt_fastest in (False, True):
                run(("rows_nt_" if nt_fastest else "rows_nx_") + kind, method, field(F, gen, nt_fastest), (8, 12))
        elif kind != "ns_momentum_f4":
            for flat in (False, True):
                run(("flat_" if flat else "") + kind, method, field(F, gen, flat), (T, X, Y))
    method, F = methods("cpu")["ns_momentum"]
    run("cpu_input", method, field(F, gen, False, "cpu"), (T, X, Y), "cpu")
    method, F = methods()["ns_momentum"]
    method.__self__.D_x.kernel.data[0, 0, 0] = 0.5
    run("box_kernel", method, field(F, gen, False), (T, X, Y))


def timed(calls=200, warmup=20):
    gen = torch.Generator().manual_seed(7)
    method, F = methods()["ns_momentum"]
    x, q = field(F, gen, False), torch.tensor([0.01, 0.1, 1.0], device=DEV)
    v = x.clone().requires_grad_(True)

    def loss_step():
        v.grad = None
        losses.pi_loss(method, v).backward()

    res = {}
    for name, fn in (("screen_us", lambda: screen.screen(method, x, q)), ("pi_loss_backward_us", loss_step)):
        ts = []
        for i in range(warmup + calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[name] = round(1e6 * sorted(ts[warmup:])[calls // 2], 2)
    res["routes"] = [screen.last_route(), losses.last_route()]
    return res


def _bits(t):
    return t.contiguous().numpy().tobytes()              # (bitwise: a NaN equals itself)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dump")
    ap.add_argument("--compare")
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    if args.time:
        print(json.dumps(timed()))
    if not (args.dump or args.compare):
        return 0
    out = {}
    loss_cases(out)
    screen_cases(out)
    torch.cuda.synchronize()
    got = {k: ([t.detach().cpu() for t in ts], route) for k, (ts, route) in out.items()}
    if args.dump:
        torch.save(got, args.dump)
        print(f"{len(got)} cases written to {args.dump}")
        for k, (_, route) in got.items():
            print(f"  {k}: {route}")
        return 0
    want = torch.load(args.compare, weights_only=False)
    bad = sorted(set(want) ^ set(got))
    for k in sorted(set(want) & set(got)):
        (wt, wr), (gt, gr) = want[k], got[k]
        same = wr == gr and len(wt) == len(gt) and all(a.shape == b.shape and a.stride() == b.stride() and _bits(a) == _bits(b)
                                                        for a, b in zip(wt, gt))
        if not same:
            bad.append(k)
            print(f"DIFFERS {k}: route {wr!r} -> {gr!r}")
    print(f"{len(got)} cases, {sum(len(t) for t, _ in got.values())} tensors: " + ("all bitwise equal, all routes equal" if not bad else f"{len(bad)} DIFFER"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
