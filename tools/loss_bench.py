"""Physics-informed residual losses on one GPU: a training step's loss + backward by the fused route (A,
``losses.pi_loss(method, v)`` + ``backward()``: the fused residual pass, ``pre_vjp_sumsq_f32``, one VJP launch of
``libcp_pre_vjp.so``) against what ran before for the same gradient (B, ``method(v).pow(2).mean().backward()``: the fused
forward, then the composed expression re-evaluated and differentiated by torch).  Both run alternately in one process on
the same tensors; each timing is the median of --reps device-event measurements after --warmup calls.  B's peak memory
is measured at batch 1 first and the batch of the timed case is chosen from it (never by running out of memory).
Counting full-tensor streams for NS momentum, A moves 4 (forward) + 1 (sum of squares) + 6 (VJP) = 11.
Also: the VJP launch alone (``residual_vjp`` with a full-grid g), time and 4 B x streams x cells / time against 8 TB/s.
The NS momentum case is held against its floor (A at least 3x faster than B: met / MISSED).
Plain text lines on stdout and in --out.

Cases ``wave_ntfast`` (the cropped Nt-fastest view of the reference's script, Physics_Informed/Wave_FNO_PISL.py:209-217, on
memory [BS,1,256,256,32]) and ``ns_momentum_ntfast`` (``pred.permute(0,1,4,2,3)`` of memory [BS,3,256,256,32]) time
``pi_loss(..., flat=True)`` + ``backward()`` (the merged-row VJP of ``libcp_pre_vjpflat.so``) against the same call with
``flat=False`` (today's fallback for such a view), alternating in one process: medians of --reps alternating measurements
with their spread, and the peak memory of both.  They run only when named in --cases.

Cases ``wave_kgrad`` and ``wave_ntfast_kgrad`` are the shapes of ``wave`` and ``wave_ntfast`` with
``D.kernel.requires_grad = True`` (Physics_Informed/Wave_FNO_PI.py:202-210): ``pi_loss(..., wgrad=True)`` + ``backward()`` (the
field VJP and ONE ``pre_wgrad_stencil3d_f32`` launch of ``libcp_pre_wgrad.so``) against the same call without ``wgrad`` (the
route ``fallback:operator kernel requires grad``), alternating in one process.  They run only when named in --cases.

Cases ``mhd_continuity``, ``mhd_induction``, ``mhd_momentum`` and ``mhd_energy`` time ``pi_loss(..., mhd=True)`` + ``backward()``
(the fused backward of ``libcp_pre_vjpmhd.so``: one launch for continuity and induction, two for momentum and energy) against
the same call with ``mhd=False`` (the parent's route, ``fallback:no fused VJP for MHD``: the composed expression under
autograd) on a C4-shard-like [16,6,64,256,256], alternating in one process, with the peak memory of both; then the VJP
launches alone (``residual_vjp`` with a full-grid g) against a device copy of the six fields timed in the same run and against
the algorithmic bytes of the equation (28, 36, 56 and 60 B per cell).  They run only when named in --cases.

Cases ``mhd_continuity_ntfast``, ``mhd_induction_ntfast``, ``mhd_momentum_ntfast`` and ``mhd_energy_ntfast`` are the view the
reference's MHD callers pass, ``pred.permute(0,1,4,2,3)`` of memory [16,6,256,256,32]: ``pi_loss(..., mhd="flat")`` +
``backward()`` (the merged-row launches of ``libcp_pre_vjpflatmhd.so``) against the same call with ``mhd=True`` (what that
keyword does on this view: ``fallback:no unit stride on the last axis``, the composed expression under autograd), alternating
call by call in one process: medians of --reps measurements with [min, max], and the peak memory of both in fields.  They run
only when named in --cases.

Cases ``jorek_continuity_ntfast`` and ``jorek_temperature_ntfast`` are the reduced-MHD residuals on the script's dense
``vars`` [96,3,256,256,40] (the shape of tools/screen_bench.py's cases of the same names; Nt-fastest field views):
``pi_loss(..., jorek=True)`` + ``backward()`` against the same call without the keyword (``fallback:no fused VJP for JOREK``: the
composed expression under autograd), alternating call by call in one process, with the peak memory of both; then
``loss.backward()`` alone on both routes (the forward outside the timed region), and the VJP launches alone (``residual_vjp``
with a full-grid g) against a device copy of the three fields timed in the same run and against the algorithmic bytes of the
equation (20 and 28 B per cell).  They run only when named in --cases.

    python tools/loss_bench.py [--reps 7] [--warmup 2] [--out profiles/loss/loss_bench.txt] [--max-batch 16]
    python tools/loss_bench.py --cases wave_ntfast,ns_momentum_ntfast --out profiles/losses/loss_bench_ntfast.txt
    python tools/loss_bench.py --cases wave_kgrad,wave_ntfast_kgrad --out profiles/losses/loss_bench_kgrad.txt
    python tools/loss_bench.py --cases mhd_continuity,mhd_induction,mhd_momentum,mhd_energy --out profiles/losses/loss_bench_mhd.txt
    python tools/loss_bench.py --cases mhd_continuity_ntfast,mhd_induction_ntfast,mhd_momentum_ntfast,mhd_energy_ntfast \
        --out profiles/losses/loss_bench_mhd_ntfast.txt
    python tools/loss_bench.py --cases jorek_continuity_ntfast,jorek_temperature_ntfast --out profiles/losses/loss_bench_jorek_ntfast.txt
    rocprofv3 --kernel-trace --stats -- python tools/loss_bench.py --vjp-only      # the VJP kernel under the profiler
"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cp_pre_amd import losses  # noqa: E402
from cp_pre_amd import residuals as R  # noqa: E402

HBM = 8.0e12


def _ev():
    return torch.cuda.Event(enable_timing=True)


def alternate(fns, reps, warmup):
    """median ms of each fn, the fns interleaved call by call"""
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
    return [sorted(t)[len(t) // 2] for t in times]


def peak_of(fn):
    """bytes allocated at the peak of fn() beyond what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


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


def ntfast_case(name, bs, rand, reps, warmup, emit):
    """``flat=True`` against ``flat=False`` on an Nt-fastest view, interleaved"""
    if name == "wave_ntfast":
        method = R.PRE_Wave(0.01, 1 / 256).residual
        pred = rand(bs, 1, 256, 256, 32).requires_grad_(True)
        view = lambda: pred[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2)            # noqa: E731
    else:
        method = R.NavierStokes(0.01, 1 / 256, 1 / 256).residual_momentum
        pred = rand(bs, 3, 256, 256, 32).requires_grad_(True)
        view = lambda: pred.permute(0, 1, 4, 2, 3)                                  # noqa: E731
    routes = {}

    def step(flat):
        def f():
            pred.grad = None
            losses.pi_loss(method, view(), flat=flat).backward()
            routes[flat] = losses.last_route()
        return f
    a, b = step(True), step(False)
    a()
    ga = pred.grad.clone()
    b()
    err = float((ga - pred.grad).abs().max() / pred.grad.abs().max())
    del ga
    pa, pb = peak_of(a), peak_of(b)
    (ma, la, ha), (mb, lb, hb) = alternate_spread([a, b], reps, warmup)
    field = pred.numel() // pred.shape[1] * 4
    emit(f"{name}: memory {list(pred.shape)}; flat=True route {routes[True]} {ma:.3f} ms [{la:.3f}, {ha:.3f}], flat=False route "
         f"{routes[False]} {mb:.3f} ms [{lb:.3f}, {hb:.3f}], False/True = {mb / ma:.2f}x; peak memory flat=True {pa / field:.2f} fields "
         f"({pa / 2**30:.2f} GiB), flat=False {pb / field:.2f} fields ({pb / 2**30:.2f} GiB); max |grad True - grad False| / max |grad False| "
         f"= {err:.2e}")


def kgrad_case(name, bs, rand, reps, warmup, emit):
    """``wgrad=True`` against the same call without it, the operator kernel requiring grad, interleaved"""
    ntfast = name == "wave_ntfast_kgrad"
    wave = R.PRE_Wave(0.01, 1 / 256 if ntfast else 1 / 512, device="cuda")
    wave.D.kernel.requires_grad = True
    if ntfast:
        pred = rand(bs, 1, 256, 256, 32).requires_grad_(True)
        view = lambda: pred[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2)            # noqa: E731
    else:
        pred = rand(bs, 64, 512, 512).requires_grad_(True)
        view = lambda: pred                                                         # noqa: E731
    routes = {}

    def step(wgrad):
        def f():
            pred.grad = wave.D.kernel.grad = None
            losses.pi_loss(wave.residual, view(), flat=ntfast, wgrad=wgrad).backward()
            routes[wgrad] = losses.last_route()
        return f
    a, b = step(True), step(False)
    a()
    ga, ka = pred.grad.clone(), wave.D.kernel.grad.clone()
    b()
    err = float((ga - pred.grad).abs().max() / pred.grad.abs().max())
    kerr = float((ka - wave.D.kernel.grad).abs().max() / wave.D.kernel.grad.abs().max())
    del ga
    pa, pb = peak_of(a), peak_of(b)
    (ma, la, ha), (mb, lb, hb) = alternate_spread([a, b], reps, warmup)
    field = pred.numel() * 4
    emit(f"{name}: memory {list(pred.shape)}; wgrad=True route {routes[True]} {ma:.3f} ms [{la:.3f}, {ha:.3f}], wgrad=False route "
         f"{routes[False]} {mb:.3f} ms [{lb:.3f}, {hb:.3f}], False/True = {mb / ma:.2f}x; peak memory wgrad=True {pa / field:.2f} fields "
         f"({pa / 2**30:.2f} GiB), wgrad=False {pb / field:.2f} fields ({pb / 2**30:.2f} GiB); max |dpred True - False| / max = "
         f"{err:.2e}, max |dK True - False| / max = {kerr:.2e}")


MHD_BYTES = {"continuity": 28, "induction": 36, "momentum": 56, "energy": 60}      # algorithmic bytes per cell of the VJP launches


def mhd_case(name, bs, rand, reps, warmup, emit):
    """``mhd=True`` against ``mhd=False`` (the parent's route) on [bs,6,64,256,256], interleaved; the VJP launches alone"""
    eq = name[4:]
    method = getattr(R.MHD(), "residual_" + eq)
    pred = rand(bs, 6, 64, 256, 256).requires_grad_(True)
    routes = {}

    def step(mhd):
        def f():
            pred.grad = None
            losses.pi_loss(method, pred, mhd=mhd).backward()
            routes[mhd] = losses.last_route()
        return f
    a, b = step(True), step(False)
    a()
    ga = pred.grad.clone()
    b()
    err = float((ga - pred.grad).abs().max() / pred.grad.abs().max())
    del ga
    pa, pb = peak_of(a), peak_of(b)
    (ma, la, ha), (mb, lb, hb) = alternate_spread([a, b], reps, warmup)
    cells = pred.numel() // 6
    field = cells * 4
    emit(f"{name}: shape {list(pred.shape)}; mhd=True route {routes[True]} {ma:.3f} ms [{la:.3f}, {ha:.3f}], mhd=False route "
         f"{routes[False]} {mb:.3f} ms [{lb:.3f}, {hb:.3f}], False/True = {mb / ma:.2f}x; peak memory mhd=True {pa / field:.2f} fields "
         f"({pa / 2**30:.2f} GiB), mhd=False {pb / field:.2f} fields ({pb / 2**30:.2f} GiB); max |grad True - grad False| / max |grad False| "
         f"= {err:.2e}")
    pred.grad = None
    vd, gg, dst = pred.detach(), rand(bs, 64, 256, 256), torch.empty_like(pred)
    (mv, lv, hv), (mc, lc, hc) = alternate_spread([lambda: losses.residual_vjp(method, vd, gg, boundary=True, mhd=True),
                                                   lambda: dst.copy_(vd)], reps, warmup)
    nb = MHD_BYTES[eq] * cells
    emit(f"{name} VJP launches alone (route fused:{name}, device events around the call, the zeroing of "
         f"unread channels included): {mv:.3f} ms [{lv:.3f}, {hv:.3f}], {MHD_BYTES[eq]} B x {cells} cells / time = {nb / (mv * 1e-3) / 1e12:.2f} TB/s = "
         f"{nb / (mv * 1e-3) / HBM:.3f} of 8 TB/s; device copy of the six fields (48 B per cell) {mc:.3f} ms [{lc:.3f}, {hc:.3f}] = "
         f"{48 * cells / (mc * 1e-3) / 1e12:.2f} TB/s: the launches move their bytes at {nb / mv / (48 * cells / mc):.2f} of the copy's rate")


def mhd_ntfast_case(name, bs, rand, reps, warmup, emit):
    """``mhd="flat"`` against ``mhd=True`` (the fallback on this view) on ``pred.permute(0,1,4,2,3)`` of [bs,6,256,256,32],
    interleaved"""
    eq = name[4:-7]
    method = getattr(R.MHD(), "residual_" + eq)
    pred = rand(bs, 6, 256, 256, 32).requires_grad_(True)
    routes = {}

    def step(mhd):
        def f():
            pred.grad = None
            losses.pi_loss(method, pred.permute(0, 1, 4, 2, 3), mhd=mhd).backward()
            routes[mhd] = losses.last_route()
        return f
    a, b = step("flat"), step(True)
    a()
    ga = pred.grad.clone()
    b()
    err = float((ga - pred.grad).abs().max() / pred.grad.abs().max())
    del ga
    pa, pb = peak_of(a), peak_of(b)
    (ma, la, ha), (mb, lb, hb) = alternate_spread([a, b], reps, warmup)
    field = pred.numel() // 6 * 4
    apart = "apart" if ha < lb else "OVERLAPPING"
    emit(f"{name}: memory {list(pred.shape)}; mhd=\"flat\" route {routes['flat']} {ma:.3f} ms [{la:.3f}, {ha:.3f}], mhd=True route "
         f"{routes[True]} {mb:.3f} ms [{lb:.3f}, {hb:.3f}], True/flat = {mb / ma:.2f}x, [min, max] {apart}; peak memory mhd=\"flat\" "
         f"{pa / field:.2f} fields ({pa / 2**30:.2f} GiB), mhd=True {pb / field:.2f} fields ({pb / 2**30:.2f} GiB); "
         f"max |grad flat - grad True| / max |grad True| = {err:.2e}")


JOREK_BYTES = {"continuity": 20, "temperature": 28}      # algorithmic bytes per cell: gg and the fields read, the gradients written


def jorek_ntfast_case(name, bs, rand, reps, warmup, emit):
    """``jorek=True`` against the same call without it (the parent's route) on the script's vars [bs,3,256,256,40],
    interleaved; ``backward()`` alone; the VJP launches alone against a device copy"""
    eq = name[len("jorek_"):-len("_ntfast")]
    method = getattr(R.JOREK(torch.linspace(1, 2, 256)), "residual_" + eq)
    pred = rand(bs, 3, 256, 256, 40).requires_grad_(True)
    routes = {}

    def step(jorek):
        def f():
            pred.grad = None
            losses.pi_loss(method, pred, jorek=jorek).backward()
            routes[jorek] = losses.last_route()
        return f
    a, b = step(True), step(False)
    a()
    ga = pred.grad.clone()
    b()
    err = float((ga - pred.grad).abs().max() / pred.grad.abs().max())
    del ga
    pa, pb = peak_of(a), peak_of(b)
    (ma, la, ha), (mb, lb, hb) = alternate_spread([a, b], reps, warmup)
    cells = pred.numel() // 3
    field = cells * 4
    apart = "apart" if ha < lb else "OVERLAPPING"
    emit(f"{name}: memory {list(pred.shape)}; jorek=True route {routes[True]} {ma:.3f} ms [{la:.3f}, {ha:.3f}], jorek=False route "
         f"{routes[False]} {mb:.3f} ms [{lb:.3f}, {hb:.3f}], False/True = {mb / ma:.2f}x, [min, max] {apart}; peak memory jorek=True "
         f"{pa / field:.2f} fields ({pa / 2**30:.2f} GiB), jorek=False {pb / field:.2f} fields ({pb / 2**30:.2f} GiB); "
         f"max |grad True - grad False| / max |grad False| = {err:.2e}")
    # backward() alone: the forward (the same fused residual pass on both routes, and the graph of the fallback) is not timed
    back = {True: [], False: []}
    for i in range(warmup + reps):
        for jorek in (True, False):
            pred.grad = None
            loss = losses.pi_loss(method, pred, jorek=jorek)
            t0, t1 = _ev(), _ev()
            t0.record()
            loss.backward()
            t1.record()
            t1.synchronize()
            if i >= warmup:
                back[jorek].append(t0.elapsed_time(t1))
            del loss
    med = {k: (sorted(t)[len(t) // 2], min(t), max(t)) for k, t in back.items()}
    emit(f"{name} backward() alone: jorek=True {med[True][0]:.3f} ms [{med[True][1]:.3f}, {med[True][2]:.3f}], jorek=False "
         f"{med[False][0]:.3f} ms [{med[False][1]:.3f}, {med[False][2]:.3f}], False/True = {med[False][0] / med[True][0]:.2f}x")
    pred.grad = None
    vd, gg, dst = pred.detach(), rand(bs, 256, 256, 40).permute(0, 3, 1, 2), torch.empty_like(pred)
    (mv, lv, hv), (mc, lc, hc) = alternate_spread([lambda: losses.residual_vjp(method, vd, gg, boundary=True, jorek=True),
                                                   lambda: dst.copy_(vd)], reps, warmup)
    nb = JOREK_BYTES[eq] * cells
    emit(f"{name} VJP launches alone (route {routes[True]}, device events around the call, the copy of g and "
         f"the zeroing of unread channels included): {mv:.3f} ms [{lv:.3f}, {hv:.3f}], {JOREK_BYTES[eq]} B x {cells} cells / time = "
         f"{nb / (mv * 1e-3) / 1e12:.2f} TB/s = {nb / (mv * 1e-3) / HBM:.3f} of 8 TB/s; device copy of the three fields (24 B per cell) "
         f"{mc:.3f} ms [{lc:.3f}, {hc:.3f}] = {24 * cells / (mc * 1e-3) / 1e12:.2f} TB/s: the launches move their bytes at "
         f"{nb / mv / (24 * cells / mc):.2f} of the copy's rate")


def steps(method, v):
    def a():
        v.grad = None
        losses.pi_loss(method, v).backward()

    def b():
        v.grad = None
        method(v).pow(2).mean().backward()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=16, help="cap of the timed NS batch (B's memory may allow more)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss", "loss_bench.txt"))
    ap.add_argument("--vjp-only", action="store_true", help="only a few NS momentum VJP launches (for a profiler)")
    ap.add_argument("--cases", default="ns_momentum,burgers,wave",
                    help="comma-separated: ns_momentum, burgers, wave, wave_ntfast, ns_momentum_ntfast, wave_kgrad, "
                         "wave_ntfast_kgrad, mhd_continuity, mhd_induction, mhd_momentum, mhd_energy, mhd_continuity_ntfast, "
                         "mhd_induction_ntfast, mhd_momentum_ntfast, mhd_energy_ntfast, jorek_continuity_ntfast, "
                         "jorek_temperature_ntfast")
    args = ap.parse_args()
    wanted = [c for c in args.cases.split(",") if c]
    assert torch.cuda.is_available(), "loss_bench needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g).add_(0.5)              # noqa: E731
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    ns = R.NavierStokes(0.01, 1 / 512, 1 / 512)
    if args.vjp_only:
        v, gg = rand(8, 3, 64, 512, 512), rand(8, 64, 512, 512)
        for _ in range(5):
            losses.residual_vjp(ns.residual_momentum, v, gg, boundary=True)
        torch.cuda.synchronize()
        return
    free, total = torch.cuda.mem_get_info()
    emit(f"# loss_bench {datetime.date.today().isoformat()} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
         f"HBM free {free / 2**30:.0f} of {total / 2**30:.0f} GiB; reps {args.reps}, warmup {args.warmup}")
    emit("# timings: device events around host + device work of one call, median; A and B interleaved on the same tensors. "
         "The tensors of ns_momentum, burgers and wave are far larger than the 256 MiB of last-level cache, so each pass streams "
         "from HBM (cold) whether or not the call before it touched the same bytes; a field of the *_ntfast cases is 128 MiB at "
         "batch 16: those steps are short and partly cache-resident")

    cases = [
        ("ns_momentum", lambda bs: rand(bs, 3, 64, 512, 512), ns.residual_momentum, args.max_batch, 11),
        ("burgers", lambda bs: rand(bs, 200, 512), R.Burgers(1 / 512, 0.0025, 0.002).residual, 4096, 7),
        ("wave", lambda bs: rand(bs, 64, 512, 512), R.PRE_Wave(0.01, 1 / 512).residual, args.max_batch, 5),
    ]
    for name in wanted:
        if name.startswith("jorek_") and name.endswith("_ntfast"):
            jorek_ntfast_case(name, min(6 * args.max_batch, 96), rand, args.reps, args.warmup, emit)
            torch.cuda.empty_cache()
        elif name.startswith("mhd_") and name.endswith("_ntfast"):
            mhd_ntfast_case(name, min(args.max_batch, 16), rand, args.reps, args.warmup, emit)
            torch.cuda.empty_cache()
        elif name.startswith("mhd_"):
            mhd_case(name, min(args.max_batch, 16), rand, args.reps, args.warmup, emit)
            torch.cuda.empty_cache()
        elif name.endswith("_kgrad"):
            kgrad_case(name, min(args.max_batch, 16), rand, args.reps, args.warmup, emit)
            torch.cuda.empty_cache()
        elif name.endswith("_ntfast"):
            ntfast_case(name, min(args.max_batch, 16), rand, args.reps, args.warmup, emit)
            torch.cuda.empty_cache()
    for name, mk, method, cap, streams_a in cases:
        if name not in wanted:
            continue
        # B's peak per sample at a small batch; the timed batch: what fits half the free memory, capped
        small = 2 if name != "burgers" else 64
        v = mk(small).requires_grad_(True)
        a, b = steps(method, v)
        b()
        per = peak_of(b) / small
        del v, a, b
        bs = int(max(1, min(cap, 0.5 * free / (per + 2 * mk(1).numel() * 4))))
        v = mk(bs).requires_grad_(True)
        a, b = steps(method, v)
        a()
        route = losses.last_route()
        ga = v.grad.clone()
        b()
        err = float((ga - v.grad).abs().max() / v.grad.abs().max())
        del ga
        pa, pb = peak_of(a), peak_of(b)
        ms_a, ms_b = alternate([a, b], args.reps, args.warmup)
        cells = v.numel() // (3 if name == "ns_momentum" else 1)
        field = cells * 4
        emit(f"{name}: shape {list(v.shape)} route {route}; A (pi_loss + backward) {ms_a:.3f} ms, B (method(v).pow(2).mean().backward()) "
             f"{ms_b:.3f} ms, B/A = {ms_b / ms_a:.2f}x; peak memory A {pa / field:.2f} fields ({pa / 2**30:.2f} GiB), "
             f"B {pb / field:.2f} fields ({pb / 2**30:.2f} GiB); A at {streams_a} streams = "
             f"{streams_a * field / (ms_a * 1e-3) / HBM:.3f} of 8 TB/s; max |grad A - grad B| / max |grad B| = {err:.2e}")
        if name == "ns_momentum":
            emit(f"ns_momentum floor, A at least 3x faster than B: {'met' if ms_b >= 3 * ms_a else 'MISSED'} ({ms_b / ms_a:.2f}x)")
            gg = rand(*([v.shape[0]] + list(v.shape[2:])))
            vd = v.detach()
            (ms_v,) = alternate([lambda: losses.residual_vjp(method, vd, gg, boundary=True)], args.reps, args.warmup)
            emit(f"ns_momentum VJP launch alone (pre_vjp_ns_momentum_f32, 3 streams in, 3 out, device events around the call): "
                 f"{ms_v:.3f} ms, 6 x 4 B x {cells} cells / time = {6 * field / (ms_v * 1e-3) / 1e12:.2f} TB/s = "
                 f"{6 * field / (ms_v * 1e-3) / HBM:.3f} of 8 TB/s")
            del gg
        del v, a, b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
