"""Screening predictions against calibrated sets on one GPU: the fused screen (A, ``screen.Screen.add_slab``: ONE launch of
``libcp_pre_screen.so``, nothing stored) against the three-pass route built from the functions that existed before it (B:
the fused residual pass into a preallocated buffer, ``HipOps.max_scores`` - the joint score pass ``ncf_metric_joint``
runs - and one joint ``CoverageLevels`` pass: the accept flags, NOT the per-sample counts that A also delivers, so B does
somewhat less than A and than the package's own fallback), and (R) the residual launch of B ALONE on the same fields.  All three run in
one process on the same tensors, interleaved call by call; each figure is the median over --blocks alternating blocks of
--reps calls, and the spread of the block medians is reported with it (the margin any comparison has to be read with).
nk = 10 levels.  One JSON line per case on stdout and appended to --out.

Shapes (``--div N`` divides every batch by N; the default runs them whole):
    ns_rank    NS momentum on the per-rank shape [512,3,64,512,512]
    c3_xslab   NS momentum on one C3 x-slab [4096,3,64,32(+2 halo rows),512], halo_x
    c4_mhd     MHD induction on the C4 shard [1024,6,64,256,256]
    c2_wave    the wave residual on [512,32,256,256]
    c5_burgers_nx / c5_burgers_nt
               Burgers on the C5 shard [8192,200,512], Nx-fastest and in the Nt-fastest layout of the active-learning
               scripts (``libcp_pre_screen1d.so``: a workgroup per sample plane).  The 1-D residual pass takes no ``out=``:
               (B) and (R) allocate their residual from torch's caching allocator on every call, and (B) scores the
               cropped copy as the package's fallback does (``ncf_metric_joint`` on ``res[1:-1, 1:-1].contiguous()``)
    c3_rank8_ntfast / c4_induction_ntfast
               NS momentum on memory [512,3,512,512,64] and MHD induction on memory [1024,6,256,256,64], both seen
               through ``permute(0,1,4,2,3)`` as the reference's 2-D scripts pass them (``libcp_pre_screenflat.so``: the
               merged-row march).  (B) scores with ``ncf_metric_joint(..., crop=1)`` as the package's fallback does in
               this layout; (R) is the flat residual launch into a buffer laid out like the fields
    jorek_temperature_ntfast / jorek_continuity_ntfast
               the JOREK residuals on the script's dense vars [96,3,256,256,40] (Nt = 40 = its T_out; 3.0 GB of fields), Nt-fastest
               field views, ``jorek=True`` (``libcp_pre_screenjorek.so``: the merged-row march with the functors of
               ``pre_residual_jorek_f32``).  The JOREK residual pass takes no ``out=``: (B) and (R) allocate their residual from
               torch's caching allocator on every call, as for Burgers; (R) is ``pre_residual_jorek_f32`` on the same views

    c3_pair_xslab / c3_pair_ntfast / c4_continuity_pair / c2_wave_pair
               the paired screen of the data-driven score r(a) - r(b) (``minus=``, ``pair=True``: ``libcp_pre_screenpair.so``) on
               two field sets: NS momentum on the x-slab geometry of tools/paired_bench.py, [2048,3,64,32(+2 halo rows),512]
               twice with halo_x (half its batch: both sets, the residual buffer of the replaced routes and their scores fit
               with room to spare); NS momentum on memory [256,3,512,512,64] twice, Nt-fastest; MHD continuity on
               [512,3,64,256,256] twice (the three channels it reads); the wave residual on [512,32,256,256] twice.  Four
               routes, alternated call by call: (A) the fused launch; (P) the route it replaces as the package runs it without
               ``pair=True`` - paired residual pass, ``ncf_metric_joint``, ``CoverageLevels`` once PER SAMPLE; (B) the best a
               user composes for score and accept only - paired pass into a buffer, the joint score pass, ONE joint
               ``CoverageLevels`` pass (``filter_sims_joint_levels``); (R) the paired residual pass alone, which moves 4 B/cell
               more than (A).  Lines go to profiles/screenpair/screen_bench_pair.jsonl unless --out says otherwise
    c5_burgers_pair_nx / c5_burgers_pair_nt
               the paired screen of the 1-D family (``minus=``, ``pair="rows"``: ``libcp_pre_screen1dpair.so``): Burgers on two
               [4096,200,512] sets, Nx-fastest and in the Nt-fastest layout of the active-learning scripts.  Three routes,
               alternated call by call: (A) the fused launch; (P) the route the package runs for the same call without
               ``pair="rows"`` - the paired residual pass on the [1,B,T,X] view into a batch-sized buffer,
               ``ncf_metric_joint``, ``CoverageLevels`` once PER SAMPLE; (R) the paired residual pass alone (the 1-D pass
               takes no ``out=``: it allocates its result on every call).  There is no (B): a user composes nothing
               shorter for per-sample verdicts of this family.  Lines go to profiles/screen1dpair/screen_bench_pair.jsonl

    c2_wave_cells / c3_rank8_ntfast_cells
               the per-cell screen (``screen.ScreenCells``: ``libcp_pre_screencells.so``) at nk = 10 level fields, no modulation:
               the wave residual on [512,32,256,256], Ny-fastest, and NS momentum in the shape and layout of c3_rank8_ntfast.
               Routes, alternated call by call: (F) the fused launch, once per library of ``--cells-libs G=path,...`` (build
               variants of the sample group, ``make SCREENCELLS_GROUP=G``; default: the package's own library); (A) the
               fastest existing route to the coverage curve - the residual pass into a buffer plus ONE marginal
               ``CoverageLevels`` pass with per-cell levels, which gives totals, not per-sample counts; (B) nk calls of the
               one-level trick (the level field as the modulation of ``screen.Screen``); (C) the joint screen of the same
               fields at nk scalar levels - the same march without the per-cell reads, the floor.  Lines go to
               profiles/screencells/screen_bench_cells.jsonl unless --out says otherwise

    c5_burgers_cells_nx / c5_burgers_cells_nt / c5_burgers_cells_pair_nt
               the per-cell screen of the 1-D family (``screen.ScreenCells(...).add_slab(rows=True)``:
               ``libcp_pre_screen1dcells.so``) at nk = 10 level fields, no modulation: Burgers on [8192,200,512], Nx-fastest
               and Nt-fastest, and the pair of two such sets, Nt-fastest (the second the first plus noise).  Routes,
               alternated call by call: (F) the fused launch, once per library of ``--cells1d-libs G=path,...`` (build variants
               of the sample group, ``make SCREEN1DCELLS_GROUP=G``; default: the package's own library); (B) nk calls of the
               one-level trick (the level field as the modulation of the joint rows screen), which delivers the same
               per-sample answer; (A) the residual pass plus ONE marginal ``CoverageLevels`` pass with per-cell levels,
               totals only; (C) the joint rows screen at nk scalar levels, the floor.  Then, on a batch of its own of
               ``--parent-batch`` samples (default 64; nothing is scaled), (P) the three-pass route the package takes
               without ``rows=True`` - one ``CoverageLevels`` pass per sample - next to (F) on that batch.  Lines go to
               profiles/screen1dcells/screen_bench_cells1d.jsonl unless --out says otherwise

    c3_rank8_ntfast_cells_pair / c2_wave_cells_pair / c2_wave_ntfast_cells_pair
               the per-cell screen of the data-driven score r(a) - r(b) (``screen.ScreenCells(...).add_slab(minus=, pair=True)``:
               ``libcp_pre_screencellspair.so``) at nk = 10 level fields, no modulation: NS momentum on two sets of memory
               [512,3,512,512,64] seen through ``permute(0,1,4,2,3)`` (the second the first plus noise; 206 GB of fields: --div 2
               halves the batch), and the wave residual on two [512,32,256,256] sets, Ny-fastest and (memory [512,256,256,32])
               Nt-fastest.  Routes, alternated call by
               call: (F) the fused launch, once per library of ``--cellspair-libs label=path,...`` (build variants of the batch
               sizes and the sample group, ``make SCREENCELLSPAIR_BATCH= SCREENCELLSPAIR_LATE= SCREENCELLSPAIR_GROUP=``;
               default: the package's own library); (B) nk one-level calls of the paired joint screen, the level field as its
               modulation; (A) the paired residual pass into a buffer plus ONE marginal ``CoverageLevels`` pass with per-cell
               levels, totals only; (C) the paired joint screen at nk scalar levels, the floor.  Then, on a batch of its own
               of ``--parent-batch`` samples, (P) the three-pass route the package takes without ``pair=True`` next to (F) on
               that batch.  Lines go to profiles/screencellspair/screen_bench_cellspair.jsonl unless --out says otherwise

    jorek_temperature_ntfast_cells / jorek_continuity_ntfast_cells
               the per-cell screen of the JOREK residuals (``screen.ScreenCells(...).add_slab(jorek=True)``:
               ``libcp_pre_screenjorekcells.so``) at the shape of the two cases above, nk = 10 level fields, no modulation.
               Routes, alternated call by call: (F) the fused launch, once per library of ``--cellsjorek-libs
               label=path,...`` (build variants of the batch size and the sample group, ``make SCREENJOREKCELLS_BATCH=
               SCREENJOREKCELLS_GROUP=``; default: the package's own library); (B)
               ``pre_residual_jorek_f32`` followed by ONE marginal ``CoverageLevels`` pass with per-cell levels, totals
               only; (T) nk one-level calls of ``screen(..., jorek=True)``, the level field as its modulation, which
               deliver the same per-sample answer.  Lines go to profiles/screenjorekcells/screen_bench_cellsjorek.jsonl
               unless --out says otherwise

    c2_wave_ntfast_stats / c5_burgers_stats_nx / c5_burgers_stats_nt / c3_rank8_ntfast_stats / c3_xslab_stats
               the per-sample statistics (``screen.ScreenStats(...).add_slab``: ``libcp_pre_screenstats.so``): the wave
               residual on memory [512,256,256,32] seen through ``permute(0,3,1,2)`` (the view
               ``Active_Learning/Wave_AL_Joint.py`` passes), and the fields of the cases of those names above.  Routes,
               alternated call by call: (F) the statistics launch; (J) the joint screen on the same view with nk = 1 and no
               modulation, which reads the same bytes; (P) the stored residual, then ``.abs().mean(dims)``.  (--only fused /
               parent / three runs F / J / P alone.)  Lines go to profiles/screenstats/screen_bench_stats.jsonl unless --out
               says otherwise

    bc_ns / bc_wave / bc_induction
               the screen (one level, with a modulation) and the statistics under ``bc='wrap'`` (``libcp_pre_screenbc.so``) at
               the shapes of DESIGN 4.31's table: NS momentum [64,3,64,512,512], wave [512,32,256,256], MHD induction
               [64,6,64,256,256].  Routes, alternated call by call: (a) the fused launch with ``bc=True``, crop (1,0,0); (b) the
               zero-pad fused launch of the same functor on an object without ``bc``, crop (1,1,1); (c) the call on the ``bc``
               object without the keyword (the three-pass route on the stored bc residual; for the statistics the float64
               reductions).  (a) and (b) are first compared bit for bit on crop (1,1,1).  Two lines per case go to
               profiles/screenbc/screenbc_bench.jsonl unless --out says otherwise

    python tools/screen_bench.py [--cases ns_rank,c2_wave,c5_burgers_nt,c3_rank8_ntfast,c4_induction_ntfast] [--div 8] [--reps 3] [--blocks 5]
    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -- python tools/screen_bench.py --cases ns_rank --only fused --blocks 1 --reps 1
        (HBM bytes by the counters, a run of its own with nothing else traced; --only residual for the launch it replaces)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cp_pre_amd import inductive_cp as icp  # noqa: E402
from cp_pre_amd import pipeline, screen  # noqa: E402
from cp_pre_amd import residuals as R  # noqa: E402

NK = 10


def _ev():
    return torch.cuda.Event(enable_timing=True)


def blocks_of(fns, reps, blocks, warmup):
    """per fn: (median of the block medians, smallest, largest) in ms; the fns interleaved call by call"""
    for _ in range(warmup):
        for f in fns:
            f()
    meds = [[] for _ in fns]
    for _ in range(blocks):
        times = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                a, b = _ev(), _ev()
                a.record()
                f()
                b.record()
                b.synchronize()
                times[i].append(a.elapsed_time(b))
        for i, t in enumerate(times):
            meds[i].append(sorted(t)[len(t) // 2])
    return [(sorted(m)[len(m) // 2], min(m), max(m)) for m in meds]


def case(name, div, dev):
    """(method, vars view, crop, halo_x, residual call into out=, bytes of fields per cell)  A JOREK method's vars are the
    script's [BS,F,Nx,Ny,Nt]."""
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*s):
        return torch.rand(*s, device=dev, generator=g) + 0.5
    if name == "ns_rank":
        ns = R.NavierStokes(0.01, 1 / 512, 1 / 512, device=dev)
        v = rnd(max(512 // div, 1), 3, 64, 512, 512)
        return ns.residual_momentum, v, (1, 1, 1), False, lambda out: ns.residual_momentum(v, boundary=True, out=out), 12
    if name == "c3_xslab":
        ns = R.NavierStokes(0.01, 1 / 512, 1 / 512, device=dev)
        full = rnd(max(4096 // div, 1), 3, 64, 34, 512)
        v = full[:, :, :, 1:-1]
        return (ns.residual_momentum, v, (1, 0, 1), True,
                lambda out: ns.residual_momentum(v, boundary=True, out=out, halo_x=True), 12)
    if name == "c4_mhd":
        mhd = R.MHD(device=dev)
        v = rnd(max(1024 // div, 1), 6, 64, 256, 256)
        return mhd.residual_induction, v, (1, 1, 1), False, lambda out: mhd.residual_induction(v, boundary=True, out=out), 16
    if name == "c2_wave":
        w = R.PRE_Wave(0.01, 0.02, device=dev)
        v = rnd(max(512 // div, 1), 32, 256, 256)
        return w.residual, v, (1, 1, 1), False, lambda out: w.residual(v, boundary=True, out=out), 4
    if name in ("c5_burgers_nx", "c5_burgers_nt"):
        bg = R.Burgers(1 / 512, 0.005, 0.002, device=dev)
        v = rnd(max(8192 // div, 1), 200, 512)
        if name.endswith("nt"):
            v = v.transpose(1, 2).contiguous().transpose(1, 2)
        return bg.residual, v, (1, 1), False, lambda out: bg.residual(v, boundary=True), 4
    if name == "c3_rank8_ntfast":
        ns = R.NavierStokes(0.01, 1 / 512, 1 / 512, device=dev)
        v = rnd(max(512 // div, 1), 3, 512, 512, 64).permute(0, 1, 4, 2, 3)
        return ns.residual_momentum, v, (1, 1, 1), False, lambda out: ns.residual_momentum(v, boundary=True, out=out), 12
    if name == "c4_induction_ntfast":
        mhd = R.MHD(device=dev)
        v = rnd(max(1024 // div, 1), 6, 256, 256, 64).permute(0, 1, 4, 2, 3)
        return mhd.residual_induction, v, (1, 1, 1), False, lambda out: mhd.residual_induction(v, boundary=True, out=out), 16
    if name in ("jorek_temperature_ntfast", "jorek_continuity_ntfast"):
        jo = R.JOREK(torch.linspace(1.0, 2.0, 256), device=dev)
        v = rnd(max(96 // div, 1), 3, 256, 256, 40)
        method = jo.residual_temperature if "temperature" in name else jo.residual_continuity
        return method, v, (1, 1, 1), False, lambda out: method(v, boundary=True), 12 if "temperature" in name else 8
    raise KeyError(name)


PAIR1D_CASES = ("c5_burgers_pair_nx", "c5_burgers_pair_nt")
PAIR_CASES = ("c3_pair_xslab", "c3_pair_ntfast", "c4_continuity_pair", "c2_wave_pair") + PAIR1D_CASES
HBM_TBPS = 8.0               # the MI355X's nominal HBM bandwidth: what the fractions below are fractions of


def pair_case(name, div, dev):
    """(method, truth view, prediction view, crop, halo_x, paired residual call into out=, fields per set)"""
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*s):
        return torch.rand(*s, device=dev, generator=g) + 0.5
    if name == "c3_pair_xslab":
        ns = R.NavierStokes(0.01, 1 / 512, 1 / 512, device=dev)
        a, b = (rnd(max(2048 // div, 1), 3, 64, 34, 512)[:, :, :, 1:-1] for _ in range(2))
        return (ns.residual_momentum, a, b, (1, 0, 1), True,
                lambda out: ns.residual_momentum(a, boundary=True, out=out, halo_x=True, minus=b), 3)
    if name == "c3_pair_ntfast":
        ns = R.NavierStokes(0.01, 1 / 512, 1 / 512, device=dev)
        a, b = (rnd(max(256 // div, 1), 3, 512, 512, 64).permute(0, 1, 4, 2, 3) for _ in range(2))
        return ns.residual_momentum, a, b, (1, 1, 1), False, lambda out: ns.residual_momentum(a, boundary=True, out=out, minus=b), 3
    if name == "c4_continuity_pair":
        mhd = R.MHD(device=dev)
        a, b = (rnd(max(512 // div, 1), 3, 64, 256, 256) for _ in range(2))
        return mhd.residual_continuity, a, b, (1, 1, 1), False, lambda out: mhd.residual_continuity(a, boundary=True, out=out, minus=b), 3
    if name == "c2_wave_pair":
        w = R.PRE_Wave(0.01, 0.02, device=dev)
        a, b = (rnd(max(512 // div, 1), 32, 256, 256) for _ in range(2))
        return w.residual, a, b, (1, 1, 1), False, lambda out: w.residual(a, boundary=True, out=out, minus=b), 1
    if name in PAIR1D_CASES:
        bg = R.Burgers(1 / 512, 0.005, 0.002, device=dev)
        a, b = (rnd(max(4096 // div, 1), 200, 512) for _ in range(2))
        if name.endswith("nt"):
            a, b = (v.transpose(1, 2).contiguous().transpose(1, 2) for v in (a, b))
        return bg.residual, a, b, (1, 1), False, lambda out: bg.residual(a, boundary=True, minus=b), 1
    raise KeyError(name)


def run_pair(name, args, dev):
    """One paired case: the four routes alternated, one JSON line."""
    method, a, b, crop, halo_x, paired_into, F = pair_case(name, args.div, dev)
    n = a.shape[0]
    one_d = name in PAIR1D_CASES
    nt_fast = a.stride(-1) != 1
    shape = (n,) + tuple(a.shape[-len(crop):])
    mod = torch.rand(shape[1:], device=dev) + 0.5
    q = torch.ones(NK, device=dev)                       # (replaced below by levels that split the samples)
    out = None if one_d else torch.empty(shape, dtype=torch.float32, device=dev)
    if one_d and nt_fast:
        mod = mod.t().contiguous().t()
    elif nt_fast:
        mod = mod.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        out = torch.empty((n,) + shape[2:] + shape[1:2], dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    reg = (slice(None),) + tuple(slice(c, s - c) for c, s in zip(crop, shape[1:]))

    def fused():
        s = screen.Screen(n, NK, dev)
        s.add_slab(method, a, q, mod, crop=crop, halo_x=halo_x, minus=b, pair="rows" if one_d else True)
        return s

    def parent():
        s = screen.Screen(n, NK, dev)
        s.add_slab(method, a, q, mod, crop=crop, halo_x=halo_x, minus=b)
        return s

    def composed():
        paired_into(out)
        if nt_fast:
            scores = icp.ncf_metric_joint(out, None, mod, crop=1)
        else:
            scores = torch.zeros(n, dtype=torch.float32, device=dev)
            pipeline.HipOps.max_scores(out, mod, crop, scores)
        cov = pipeline.CoverageLevels(n, NK, dev, joint=True)
        cov.add_slab(out[reg], q, modulation=mod[reg[1:]])
        return scores, cov

    def residual():
        paired_into(out)

    # the levels: quantiles of the samples' own scores, so that every level accepts some samples and rejects others and
    # the equalities recorded below compare verdicts that differ from sample to sample
    sc0 = fused().finish().score
    q = torch.quantile(sc0, torch.linspace(0.05, 0.95, NK, device=dev)).contiguous()
    s = fused()
    route = screen.last_route()
    p = parent()
    proute = screen.last_route()
    if not one_d:
        sc, cov = composed()
    torch.cuda.synchronize()
    got, old = s.finish(), p.finish()
    line = {"case": name, "shape": list(a.shape), "sets": 2, "nk": NK, "route": route, "replaced_route": proute,
            "bit_identical_to_replaced_route": bool(torch.equal(got.inside, old.inside)) and
            bool(torch.equal(got.score.view(torch.int32), old.score.view(torch.int32))),
            "accept_equal_to_replaced_route": bool(torch.equal(got.accept(), old.accept())),
            "accepted_per_level": [int(v) for v in got.accept().sum(dim=1).cpu()]}
    fns = {"fused": fused, "parent": parent, "residual": residual}
    if not one_d:
        line["accept_equal_to_composed"] = bool(torch.equal(got.accept(), cov.inside))
        fns = {"fused": fused, "parent": parent, "composed": composed, "residual": residual}
    if args.only is not None and args.only not in fns:
        raise SystemExit(f"--only {args.only}: the paired cases have the routes {', '.join(fns)}")
    pick = [args.only] if args.only else list(fns)
    res = blocks_of([fns[k] for k in pick], args.reps, args.blocks, args.warmup)
    cells = 1
    for d in shape:
        cells *= d
    # bytes per cell each route must move: the fields of both sets; + the stored difference; + its two further reads
    bpc = {"fused": 8 * F, "residual": 8 * F + 4, "composed": 8 * F + 12, "parent": 8 * F + 12}
    line["cells"] = cells
    for k, (med, lo, hi) in zip(pick, res):
        line[k + "_ms"] = round(med, 4)
        line[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        line[k + "_B_per_cell"] = bpc[k]
        line[k + "_fraction_of_8TBps"] = round(cells * bpc[k] / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
    if "fused" in pick:
        for k in ("parent", "composed", "residual"):
            if k in pick:
                line["fused_over_" + k] = round(line["fused_ms"] / line[k + "_ms"], 4)
    return line


CELLS_CASES = {"c2_wave_cells": "c2_wave", "c3_rank8_ntfast_cells": "c3_rank8_ntfast"}


def run_cells(name, args, dev):
    """One per-cell case: (F) per library, (A), (B), (C) alternated, one JSON line."""
    from cp_pre_amd import _lib
    method, v, crop, halo_x, residual_into, fbytes = case(CELLS_CASES[name], args.div, dev)
    n = v.shape[0]
    nt_fast = v.stride(-1) != 1
    shape = (n,) + tuple(v.shape[-3:])
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    if nt_fast:
        out = torch.empty((n,) + shape[2:] + shape[1:2], dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    reg = (slice(None),) + tuple(slice(c, s - c) for c, s in zip(crop, shape[1:]))
    # level fields in the fields' layout: level k about (k + 1) / nk of twice the mean |r|, scattered per cell by +-50 %
    residual_into(out)
    scale = float(out[:min(n, 8)].abs().mean())
    qc = torch.rand((NK,) + shape[1:], device=dev) + 0.5
    qc *= (2.0 * scale / NK) * torch.arange(1, NK + 1, device=dev, dtype=torch.float32).reshape(NK, 1, 1, 1)
    if nt_fast:
        qc = qc.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    qs = torch.linspace(0.2, 2.0, NK, device=dev) * scale
    one = torch.ones(1, device=dev)
    # the libraries of (F): handles loaded once, swapped into the loader's cache before each call
    libs = {}
    if args.cells_libs:
        for item in args.cells_libs.split(","):
            g, path = item.split("=", 1)
            _lib._screencells, _lib.SCREENCELLS_SO_PATH = None, os.path.abspath(path)
            libs[int(g)] = _lib.load_screencells()
            assert libs[int(g)].pre_screencells_sample_group() == int(g), item
    else:
        libs[screen.sample_group()] = _lib.load_screencells()

    def fused_with(g):
        def fused():
            _lib._screencells = libs[g]
            s = screen.ScreenCells(n, NK, dev)
            s.add_slab(method, v, qc, None, crop=crop)
            return s
        return fused

    def curve():                                             # (A)
        residual_into(out)
        cov = pipeline.CoverageLevels(n, NK, dev)
        cov.add_slab(out[reg], qc[(slice(None),) + reg[1:]])
        return cov

    def trick():                                             # (B)
        outs = []
        for k in range(NK):
            s = screen.Screen(n, 1, dev)
            s.add_slab(method, v, one, qc[k], crop=crop)
            outs.append(s)
        return outs

    def joint():                                             # (C)
        s = screen.Screen(n, NK, dev)
        s.add_slab(method, v, qs, None, crop=crop)
        return s

    fns = {"fused_G%d" % g: fused_with(g) for g in sorted(libs)}
    got = {k: f().finish() for k, f in fns.items()}
    route = screen.last_route()
    first = got[next(iter(got))]
    cov = curve()
    tr = trick()
    torch.cuda.synchronize()
    totals = first.inside.sum(dim=1)
    line = {"case": name, "shape": list(v.shape), "nk": NK, "route": route, "sample_groups": sorted(libs),
            "every_G_bit_identical": all(torch.equal(o.inside, first.inside) and
                                         torch.equal(o.score.view(torch.int32), first.score.view(torch.int32)) for o in got.values()),
            "totals_equal_to_coverage_levels": bool(torch.equal(totals, cov.acc.to(totals.dtype))),
            "counts_equal_to_one_level_trick": bool(torch.equal(first.inside, torch.cat([t.finish().inside for t in tr]))),
            "coverage_curve": [round(float(c), 4) for c in first.coverage_marginal()]}
    fns.update({"curve_A": curve, "trick_B": trick, "joint_C": joint})
    if args.only == "fused":
        pick = [k for k in fns if k.startswith("fused_G")]
    elif args.only is not None:
        raise SystemExit("--only fused is the one single-route run of the per-cell cases")
    else:
        pick = list(fns)
    res = blocks_of([fns[k] for k in pick], args.reps, args.blocks, args.warmup)
    cells = 1
    for d in shape:
        cells *= d
    line.update({"cells": cells, "field_bytes_per_cell": fbytes, "level_bytes_per_cell": 4 * NK})
    for k, (med, lo, hi) in zip(pick, res):
        line[k + "_ms"] = round(med, 4)
        line[k + "_ms_blocks_min_max"] = [round(lo, 4), round(hi, 4)]
        if k.startswith("fused_G"):
            # bytes per cell over time: the fields alone (levels from L2), and with the level fields read once per sample
            line[k + "_fraction_of_8TBps_fields"] = round(cells * fbytes / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
            line[k + "_fraction_of_8TBps_fields_and_levels"] = round(cells * (fbytes + 4 * NK) / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
    return line


CELLS1D_CASES = {"c5_burgers_cells_nx": ("c5_burgers_nx", False), "c5_burgers_cells_nt": ("c5_burgers_nt", False),
                 "c5_burgers_cells_pair_nt": ("c5_burgers_nt", True)}


def run_cells1d(name, args, dev):
    """One per-cell case of the 1-D family: (F) per library, (B), (A), (C) alternated, then (P) on its own small batch; one
    JSON line."""
    from cp_pre_amd import _lib
    base, pair = CELLS1D_CASES[name]
    method, v, crop, _, _, fbytes = case(base, args.div, dev)
    n = v.shape[0]
    nt_fast = v.stride(-1) != 1
    w = None
    if pair:                                                 # the second set: the first plus noise, in the same layout
        w = v + 0.05 * torch.randn(v.shape, device=dev)
        w = w.transpose(1, 2).contiguous().transpose(1, 2) if nt_fast else w.contiguous()
        fbytes *= 2
    kw = {"minus": w} if pair else {}
    shape = tuple(v.shape)
    reg = (slice(None),) + tuple(slice(c, s - c) for c, s in zip(crop, shape[1:]))
    # level fields in the fields' layout: level k about (k + 1) / nk of twice the mean |r|, scattered per cell by +-50 %
    scale = float(method(v[:min(n, 8)], boundary=True, **({"minus": w[:min(n, 8)]} if pair else {})).abs().mean())
    qc = torch.rand((NK,) + shape[1:], device=dev) + 0.5
    qc *= (2.0 * scale / NK) * torch.arange(1, NK + 1, device=dev, dtype=torch.float32).reshape(NK, 1, 1)
    if nt_fast:
        qc = qc.transpose(1, 2).contiguous().transpose(1, 2)
    qs = torch.linspace(0.2, 2.0, NK, device=dev) * scale
    one = torch.ones(1, device=dev)
    libs = {}
    if args.cells1d_libs:
        for item in args.cells1d_libs.split(","):
            g, path = item.split("=", 1)
            _lib._screen1dcells, _lib.SCREEN1DCELLS_SO_PATH = None, os.path.abspath(path)
            libs[int(g)] = _lib.load_screen1dcells()
            assert libs[int(g)].pre_screen1dcells_sample_group() == int(g), item
    else:
        libs[screen.sample_group_rows()] = _lib.load_screen1dcells()

    def fused_with(g):
        def fused():
            _lib._screen1dcells = libs[g]
            s = screen.ScreenCells(n, NK, dev)
            s.add_slab(method, v, qc, None, crop=crop, rows=True, **kw)
            return s
        return fused

    def trick():                                             # (B)
        outs = []
        for k in range(NK):
            s = screen.Screen(n, 1, dev)
            s.add_slab(method, v, one, qc[k], crop=crop, pair="rows", **kw)
            outs.append(s)
        return outs

    def curve():                                             # (A)
        res = method(v, boundary=True, **kw)
        cov = pipeline.CoverageLevels(n, NK, dev)
        cov.add_slab(res[reg], qc[(slice(None),) + reg[1:]])
        return cov

    def joint():                                             # (C)
        s = screen.Screen(n, NK, dev)
        s.add_slab(method, v, qs, None, crop=crop, pair="rows", **kw)
        return s

    fns = {"fused_G%d" % g: fused_with(g) for g in sorted(libs)}
    got = {}
    for k, f in fns.items():
        got[k] = f().finish()
        assert screen.last_route().startswith("fused:rows_cells_"), screen.last_route()
    route = screen.last_route()
    first = got[next(iter(got))]
    cov = curve()
    tr = trick()
    trick_route = screen.last_route()
    torch.cuda.synchronize()
    totals = first.inside.sum(dim=1)
    line = {"case": name, "shape": list(shape), "sets": 2 if pair else 1, "nk": NK, "route": route, "trick_route": trick_route,
            "sample_groups": sorted(libs),
            "every_G_bit_identical": all(torch.equal(o.inside, first.inside) and
                                         torch.equal(o.score.view(torch.int32), first.score.view(torch.int32)) for o in got.values()),
            "totals_equal_to_coverage_levels": bool(torch.equal(totals, cov.acc.to(totals.dtype))),
            "counts_equal_to_one_level_trick": bool(torch.equal(first.inside, torch.cat([t.finish().inside for t in tr]))),
            "coverage_curve": [round(float(c), 4) for c in first.coverage_marginal()]}
    fns.update({"trick_B": trick, "curve_A": curve, "joint_C": joint})
    if args.only == "fused":
        pick = [k for k in fns if k.startswith("fused_G")]
    elif args.only is not None:
        raise SystemExit("--only fused is the one single-route run of the per-cell cases")
    else:
        pick = list(fns)
    res = blocks_of([fns[k] for k in pick], args.reps, args.blocks, args.warmup)
    cells = 1
    for d in shape:
        cells *= d
    line.update({"cells": cells, "field_bytes_per_cell": fbytes, "level_bytes_per_cell": 4 * NK})
    for k, (med, lo, hi) in zip(pick, res):
        line[k + "_ms"] = round(med, 4)
        line[k + "_ms_blocks_min_max"] = [round(lo, 4), round(hi, 4)]
        line[k + "_block_spread"] = round(hi / lo, 4)
        if k.startswith("fused_G"):
            line[k + "_fraction_of_8TBps_fields"] = round(cells * fbytes / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
            line[k + "_fraction_of_8TBps_fields_and_levels"] = round(cells * (fbytes + 4 * NK) / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
    if args.only is None and args.parent_batch > 0:
        # (P) the three-pass route the package takes without rows=True, on a batch of its own: one CoverageLevels pass per
        # sample.  The figure is of THAT batch; nothing is scaled
        nb = min(n, args.parent_batch)
        vb, kb = v[:nb], ({"minus": w[:nb]} if pair else {})

        def parent():
            s = screen.ScreenCells(nb, NK, dev)
            s.add_slab(method, vb, qc, None, crop=crop, **kb)
            return s

        def fused_small():
            _lib._screen1dcells = libs[max(libs)]
            s = screen.ScreenCells(nb, NK, dev)
            s.add_slab(method, vb, qc, None, crop=crop, rows=True, **kb)
            return s
        p = parent().finish()
        line["parent_route"] = screen.last_route()
        f = fused_small().finish()
        line["parent_batch"] = nb
        line["bit_identical_to_parent_route"] = bool(torch.equal(p.inside, f.inside)) and \
            bool(torch.equal(p.score.view(torch.int32), f.score.view(torch.int32)))
        (pm, plo, phi), (fm, flo, fhi) = blocks_of([parent, fused_small], 1, 3, 0)
        line.update({"parent_P_ms_at_parent_batch": round(pm, 4), "parent_P_ms_blocks_min_max": [round(plo, 4), round(phi, 4)],
                     "fused_ms_at_parent_batch": round(fm, 4), "fused_ms_at_parent_batch_blocks_min_max": [round(flo, 4), round(fhi, 4)]})
    return line


CELLSPAIR_CASES = {"c3_rank8_ntfast_cells_pair": "c3_rank8_ntfast", "c2_wave_cells_pair": "c2_wave",
                   "c2_wave_ntfast_cells_pair": "c2_wave"}


def run_cellspair(name, args, dev):
    """One per-cell case of the data-driven score: (F) per library, (B), (A), (C) alternated, then (P) on its own small
    batch; one JSON line."""
    from cp_pre_amd import _lib
    method, v, crop, halo_x, _, fbytes = case(CELLSPAIR_CASES[name], args.div, dev)
    if name == "c2_wave_ntfast_cells_pair":
        v = v.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    n = v.shape[0]
    nt_fast = v.stride(-1) != 1
    # the second set: the first plus noise, in the same layout (sample by sample: no third batch-sized tensor)
    w = torch.empty_like(v)
    for i in range(n):
        w[i] = v[i] + 0.05 * torch.randn(v[i].shape, device=dev)
    fbytes *= 2
    shape = (n,) + tuple(v.shape[-3:])
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    if nt_fast:
        out = torch.empty((n,) + shape[2:] + shape[1:2], dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    reg = (slice(None),) + tuple(slice(c, s - c) for c, s in zip(crop, shape[1:]))

    def paired_into():
        return method(v, boundary=True, out=out, minus=w)
    # level fields in the fields' layout: level k about (k + 1) / nk of twice the mean |d|, scattered per cell by +-50 %
    paired_into()
    scale = float(out[:min(n, 8)].abs().mean())
    qc = torch.rand((NK,) + shape[1:], device=dev) + 0.5
    qc *= (2.0 * scale / NK) * torch.arange(1, NK + 1, device=dev, dtype=torch.float32).reshape(NK, 1, 1, 1)
    if nt_fast:
        qc = qc.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    qs = torch.linspace(0.2, 2.0, NK, device=dev) * scale
    one = torch.ones(1, device=dev)
    # the libraries of (F): handles loaded once, swapped into the loader's cache before each call
    libs = {}
    if args.cellspair_libs:
        for item in args.cellspair_libs.split(","):
            label, path = item.split("=", 1)
            _lib._screencellspair, _lib.SCREENCELLSPAIR_SO_PATH = None, os.path.abspath(path)
            libs[label] = _lib.load_screencellspair()
    else:
        libs["package"] = _lib.load_screencellspair()

    def fused_with(label, nb=None):
        vb, wb = (v, w) if nb is None else (v[:nb], w[:nb])

        def fused():
            _lib._screencellspair = libs[label]
            s = screen.ScreenCells(vb.shape[0], NK, dev)
            s.add_slab(method, vb, qc, None, crop=crop, minus=wb, pair=True)
            return s
        return fused

    def trick():                                             # (B)
        outs = []
        for k in range(NK):
            s = screen.Screen(n, 1, dev)
            s.add_slab(method, v, one, qc[k], crop=crop, minus=w, pair=True)
            outs.append(s)
        return outs

    def curve():                                             # (A)
        paired_into()
        cov = pipeline.CoverageLevels(n, NK, dev)
        cov.add_slab(out[reg], qc[(slice(None),) + reg[1:]])
        return cov

    def joint():                                             # (C)
        s = screen.Screen(n, NK, dev)
        s.add_slab(method, v, qs, None, crop=crop, minus=w, pair=True)
        return s

    fns = {"fused_" + label: fused_with(label) for label in libs}
    got = {}
    for k, f in fns.items():
        got[k] = f().finish()
        assert screen.last_route().startswith("fused:") and "cells_pair_" in screen.last_route(), screen.last_route()
    route = screen.last_route()
    first = got[next(iter(got))]
    cov = curve()
    tr = trick()
    trick_route = screen.last_route()
    torch.cuda.synchronize()
    totals = first.inside.sum(dim=1)
    line = {"case": name, "shape": list(v.shape), "sets": 2, "nk": NK, "route": route, "trick_route": trick_route,
            "libraries": {label: int(lib.pre_screencellspair_sample_group()) for label, lib in libs.items()},
            "every_library_bit_identical": all(torch.equal(o.inside, first.inside) and
                                               torch.equal(o.score.view(torch.int32), first.score.view(torch.int32)) for o in got.values()),
            "totals_equal_to_coverage_levels": bool(torch.equal(totals, cov.acc.to(totals.dtype))),
            "counts_equal_to_one_level_trick": bool(torch.equal(first.inside, torch.cat([t.finish().inside for t in tr]))),
            "coverage_curve": [round(float(c), 4) for c in first.coverage_marginal()]}
    del got, tr, cov
    fns.update({"trick_B": trick, "curve_A": curve, "joint_C": joint})
    if args.only == "fused":
        pick = [k for k in fns if k.startswith("fused_")]
    elif args.only is not None:
        raise SystemExit("--only fused is the one single-route run of the per-cell cases")
    else:
        pick = list(fns)
    res = blocks_of([fns[k] for k in pick], args.reps, args.blocks, args.warmup)
    cells = 1
    for d in shape:
        cells *= d
    line.update({"cells": cells, "field_bytes_per_cell": fbytes, "level_bytes_per_cell": 4 * NK})
    for k, (med, lo, hi) in zip(pick, res):
        line[k + "_ms"] = round(med, 4)
        line[k + "_ms_blocks_min_max"] = [round(lo, 4), round(hi, 4)]
        line[k + "_block_spread"] = round(hi / lo, 4)
        if k.startswith("fused_"):
            line[k + "_fraction_of_8TBps_fields"] = round(cells * fbytes / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
            line[k + "_fraction_of_8TBps_fields_and_levels"] = round(cells * (fbytes + 4 * NK) / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
    if args.only is None and args.parent_batch > 0:
        # (P) the three-pass route the package takes without pair=True, on a batch of its own: two residual passes, the
        # stored difference, one CoverageLevels pass per sample.  The figure is of THAT batch; nothing is scaled
        nb = min(n, args.parent_batch)
        last = list(libs)[-1]

        def parent():
            s = screen.ScreenCells(nb, NK, dev)
            s.add_slab(method, v[:nb], qc, None, crop=crop, minus=w[:nb])
            return s
        fused_small = fused_with(last, nb)
        p = parent().finish()
        line["parent_route"] = screen.last_route()
        f = fused_small().finish()
        line["parent_batch"] = nb
        line["bit_identical_to_parent_route"] = bool(torch.equal(p.inside, f.inside)) and \
            bool(torch.equal(p.score.view(torch.int32), f.score.view(torch.int32)))
        line["counts_differ_from_parent_route_by_at_most"] = int((p.inside - f.inside).abs().max())
        (pm, plo, phi), (fm, flo, fhi) = blocks_of([parent, fused_small], 1, 3, 0)
        line.update({"parent_P_ms_at_parent_batch": round(pm, 4), "parent_P_ms_blocks_min_max": [round(plo, 4), round(phi, 4)],
                     "fused_ms_at_parent_batch": round(fm, 4), "fused_ms_at_parent_batch_blocks_min_max": [round(flo, 4), round(fhi, 4)],
                     "fused_at_parent_batch_library": last})
    return line


CELLSJOREK_CASES = {"jorek_temperature_ntfast_cells": "jorek_temperature_ntfast",
                    "jorek_continuity_ntfast_cells": "jorek_continuity_ntfast"}


def run_cellsjorek(name, args, dev):
    """One per-cell JOREK case: (F) per library, (B), (T) alternated; one JSON line."""
    from cp_pre_amd import _lib
    method, v, crop, _, residual_into, fbytes = case(CELLSJOREK_CASES[name], args.div, dev)
    n = v.shape[0]
    shape = (n, v.shape[4], v.shape[2], v.shape[3])          # the field views [BS,Nt,Nx,Ny] of vars [BS,F,Nx,Ny,Nt]
    reg = (slice(None),) + tuple(slice(c, s - c) for c, s in zip(crop, shape[1:]))
    # level fields in the fields' layout (memory [nk,Nx,Ny,Nt]): level k about (k + 1) / nk of twice the mean |r|, scattered
    # per cell by +-50 %
    scale = float(residual_into(None)[:min(n, 8)].abs().mean())
    qc = torch.rand((NK,) + shape[1:], device=dev) + 0.5
    qc *= (2.0 * scale / NK) * torch.arange(1, NK + 1, device=dev, dtype=torch.float32).reshape(NK, 1, 1, 1)
    qc = qc.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    one = torch.ones(1, device=dev)
    # the libraries of (F): handles loaded once, swapped into the loader's cache before each call
    libs = {}
    if args.cellsjorek_libs:
        for item in args.cellsjorek_libs.split(","):
            label, path = item.split("=", 1)
            _lib._screenjorekcells, _lib.SCREENJOREKCELLS_SO_PATH = None, os.path.abspath(path)
            libs[label] = _lib.load_screenjorekcells()
    else:
        libs["package"] = _lib.load_screenjorekcells()

    def fused_with(label):
        def fused():
            _lib._screenjorekcells = libs[label]
            s = screen.ScreenCells(n, NK, dev)
            s.add_slab(method, v, qc, None, crop=crop, jorek=True)
            return s
        return fused

    def curve():                                             # (B)
        res = residual_into(None)
        cov = pipeline.CoverageLevels(n, NK, dev)
        cov.add_slab(res[reg], qc[(slice(None),) + reg[1:]])
        return cov

    def ten():                                               # (T)
        outs = []
        for k in range(NK):
            s = screen.Screen(n, 1, dev)
            s.add_slab(method, v, one, qc[k], crop=crop, jorek=True)
            outs.append(s)
        return outs

    fns = {"fused_" + label: fused_with(label) for label in libs}
    got = {}
    for k, f in fns.items():
        got[k] = f().finish()
        assert screen.last_route().startswith("fused:flat_cells_jorek_"), screen.last_route()
    route = screen.last_route()
    first = got[next(iter(got))]
    cov = curve()
    tr = ten()
    ten_route = screen.last_route()
    torch.cuda.synchronize()
    totals = first.inside.sum(dim=1)
    line = {"case": name, "shape": list(v.shape), "nk": NK, "route": route, "ten_route": ten_route,
            "libraries": {label: int(lib.pre_screenjorekcells_sample_group()) for label, lib in libs.items()},
            "every_library_bit_identical": all(torch.equal(o.inside, first.inside) and
                                               torch.equal(o.score.view(torch.int32), first.score.view(torch.int32)) for o in got.values()),
            "totals_equal_to_coverage_levels": bool(torch.equal(totals, cov.acc.to(totals.dtype))),
            "counts_equal_to_ten_one_level_calls": bool(torch.equal(first.inside, torch.cat([t.finish().inside for t in tr]))),
            "coverage_curve": [round(float(c), 4) for c in first.coverage_marginal()]}
    del got, tr, cov
    fns.update({"residual_then_coverage_B": curve, "ten_one_level_T": ten})
    if args.only == "fused":
        pick = [k for k in fns if k.startswith("fused_")]
    elif args.only is not None:
        raise SystemExit("--only fused is the one single-route run of the per-cell cases")
    else:
        pick = list(fns)
    res = blocks_of([fns[k] for k in pick], args.reps, args.blocks, args.warmup)
    cells = 1
    for d in shape:
        cells *= d
    line.update({"cells": cells, "field_bytes_per_cell": fbytes, "level_bytes_per_cell": 4 * NK})
    for k, (med, lo, hi) in zip(pick, res):
        line[k + "_ms"] = round(med, 4)
        line[k + "_ms_blocks_min_max"] = [round(lo, 4), round(hi, 4)]
        line[k + "_block_spread"] = round(hi / lo, 4)
        if k.startswith("fused_"):
            line[k + "_fraction_of_8TBps_fields"] = round(cells * fbytes / (med * 1e-3) / 1e12 / HBM_TBPS, 3)
    return line


# ---- per-sample statistics (screen.screen_stats / ScreenStats, libcp_pre_screenstats.so) ------------------------------------
# case -> the case whose fields and method it takes; c2_wave_ntfast_stats is the view Active_Learning/Wave_AL_Joint.py passes
STATS_CASES = {"c2_wave_ntfast_stats": None, "c5_burgers_stats_nx": "c5_burgers_nx", "c5_burgers_stats_nt": "c5_burgers_nt",
               "c3_rank8_ntfast_stats": "c3_rank8_ntfast", "c3_xslab_stats": "c3_xslab"}


def run_stats(name, args, dev):
    """Three routes alternated call by call in one process: (F) the statistics launch, (J) the joint screen on the same view
    with nk = 1 and no modulation - the parent's code, which reads the same bytes -, (P) what a caller writes today: the
    stored residual, then ``.abs().mean(dims)``."""
    if STATS_CASES[name] is None:
        w = R.PRE_Wave(0.01, 0.02, device=dev)
        g = torch.Generator(device=dev).manual_seed(0)
        v = (torch.rand(max(512 // args.div, 1), 256, 256, 32, device=dev, generator=g) + 0.5).permute(0, 3, 1, 2)
        method, crop, halo_x, fbytes = w.residual, (1, 1, 1), False, 4
        residual_into = lambda out: w.residual(v, boundary=True, out=out)  # noqa: E731
    else:
        method, v, crop, halo_x, residual_into, fbytes = case(STATS_CASES[name], args.div, dev)
    n, one_d = v.shape[0], len(crop) == 2
    shape = (n,) + tuple(v.shape[-len(crop):])
    nt_fast = not one_d and v.stride(-1) != 1
    out = None if one_d else torch.empty(shape, dtype=torch.float32, device=dev)
    if nt_fast:
        out = torch.empty((n,) + shape[2:] + shape[1:2], dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    reg = (slice(None),) + tuple(slice(c, s - c) for c, s in zip(crop, shape[1:]))
    dims = tuple(range(1, len(shape)))
    q1 = torch.ones(1, device=dev)

    def stats():
        s = screen.ScreenStats(n, dev)
        s.add_slab(method, v, crop=crop, halo_x=halo_x)
        return s

    def joint():
        s = screen.Screen(n, 1, dev)
        s.add_slab(method, v, q1, None, crop=crop, halo_x=halo_x)
        return s

    def stored():
        res = residual_into(out) if one_d else (residual_into(out), out)[1]
        return res[reg].abs().mean(dim=dims)

    s = stats()
    route = screen.last_route()
    j = joint()
    route_j = screen.last_route()
    p = stored()
    torch.cuda.synchronize()
    got, gj = s.finish(), j.finish()
    max_same = bool(torch.equal(got.max_abs.view(torch.int32), gj.score.view(torch.int32)))
    rel = float(((got.mean_abs() - p.double()).abs() / p.double()).max())
    fns = {"fused": stats, "parent": joint, "three": stored}
    pick = [args.only] if args.only in fns else ["fused", "parent", "three"]
    res = blocks_of([fns[k] for k in pick], args.reps, args.blocks, args.warmup)
    cells = 1
    for d in shape:
        cells *= d
    line = {"case": name, "shape": list(v.shape), "route": route, "route_J": route_j, "max_abs_bits_equal_J_score": max_same,
            "mean_abs_rel_diff_to_P": rel, "cells": cells, "field_bytes_per_cell": fbytes}
    for k, (med, lo, hi) in zip(pick, res):
        label = {"fused": "F", "parent": "J", "three": "P"}[k]
        line[label + "_ms"] = round(med, 4)
        line[label + "_ms_blocks_min_max"] = [round(lo, 4), round(hi, 4)]
    if "F_ms" in line:
        line["F_TBps_of_fields"] = round(cells * fbytes / (line["F_ms"] * 1e-3) / 1e12, 3)
    if "F_ms" in line and "J_ms" in line:
        spread = line["J_ms_blocks_min_max"][1] - line["J_ms_blocks_min_max"][0]
        line["F_over_J"] = round(line["F_ms"] / line["J_ms"], 4)
        line["F_no_worse_than_J_beyond_its_spread"] = bool(line["F_ms"] <= line["J_ms"] + spread)
    if "F_ms" in line and "P_ms" in line:
        line["F_over_P"] = round(line["F_ms"] / line["P_ms"], 4)
    return line


# ---- the screens and statistics under boundary conditions on the x-y rim (``bc='wrap'``), at the shapes of DESIGN 4.31's table
BC_CASES = {"bc_ns": ("ns_momentum", (64, 3, 64, 512, 512)), "bc_wave": ("wave", (512, 32, 256, 256)),
            "bc_induction": ("mhd_induction", (64, 6, 64, 256, 256))}


def run_bc(name, args, dev):
    """Two lines, the screen (one level, with a modulation) and the statistics, each with three routes alternated call by call
    in one process on the same tensors: (a) the fused launch under ``bc=True``, crop (1, 0, 0); (b) the zero-pad fused launch of
    the same functor on an object without ``bc``, crop (1, 1, 1); (c) the call on the ``bc`` object without the keyword - what
    the parent commit does: the stored bc residual, then the score and a ``CoverageLevels`` pass per sample, or the float64
    reductions.  Before timing: (a) equals (b) bit for bit on crop (1, 1, 1)."""
    kind, shape = BC_CASES[name]
    n = max(shape[0] // args.div, 1)
    g = torch.Generator(device=dev).manual_seed(0)
    v = torch.rand((n,) + shape[1:], device=dev, generator=g) + 0.5      # (Ny-fastest: the form the BC march takes)
    if kind == "wave":
        make = lambda **kw: R.PRE_Wave(0.01, 0.02, device=dev, **kw).residual  # noqa: E731
    elif kind == "ns_momentum":
        make = lambda **kw: R.NavierStokes(0.01, 1 / 64, 1 / 64, device=dev, **kw).residual_momentum  # noqa: E731
    else:
        make = lambda **kw: R.MHD(device=dev, **kw).residual_induction  # noqa: E731
    m_bc, m_zero = make(bc="wrap"), make()
    rshape = (n,) + tuple(v.shape[-3:])
    mod = torch.rand(rshape[1:], device=dev, generator=g) + 0.5
    q = torch.full((1,), 5.0, device=dev)
    nfields = {"wave": 1, "ns_momentum": 3, "mhd_induction": 4}[kind]
    cells = 1
    for d in rshape:
        cells *= d

    def screen_of(m, crop, **kw):
        def f():
            s = screen.Screen(n, 1, dev)
            s.add_slab(m, v, q, mod, crop=crop, **kw)
            return s
        return f

    def stats_of(m, crop, **kw):
        def f():
            s = screen.ScreenStats(n, dev)
            s.add_slab(m, v, crop=crop, **kw)
            return s
        return f

    lines = []
    for what, of in (("screen", screen_of), ("stats", stats_of)):
        a, b, c = of(m_bc, (1, 0, 0), bc=True), of(m_zero, (1, 1, 1)), of(m_bc, (1, 0, 0))
        ga = of(m_bc, (1, 1, 1), bc=True)().finish()
        route_a = screen.last_route()
        gb = b().finish()
        route_b = screen.last_route()
        c()
        route_c = screen.last_route()
        torch.cuda.synchronize()
        if what == "screen":
            same = bool(torch.equal(ga.score.view(torch.int32), gb.score.view(torch.int32)) and torch.equal(ga.inside, gb.inside))
        else:
            same = bool(torch.equal(ga.max_abs.view(torch.int32), gb.max_abs.view(torch.int32)))
        if not same:
            raise SystemExit(f"{name} {what}: (a) and (b) differ on crop (1, 1, 1)")
        res = blocks_of([a, b, c], args.reps, args.blocks, args.warmup)
        line = {"case": name, "what": what, "kind": kind, "shape": list(v.shape), "bc": "wrap", "route_a": route_a, "route_b": route_b,
                "route_c": route_c, "a_equals_b_bits_on_crop_111": same, "cells": cells, "field_bytes_per_cell": 4 * nfields}
        if what == "stats":
            rel = ((ga.sum_abs - gb.sum_abs).abs() / gb.sum_abs).max()
            line["sum_abs_rel_diff_a_b_on_crop_111"] = float(rel)
        for k, (med, lo, hi) in zip("abc", res):
            line[k + "_ms"] = round(med, 4)
            line[k + "_ms_blocks_min_max"] = [round(lo, 4), round(hi, 4)]
        line["a_TBps_of_fields"] = round(cells * 4 * nfields / (line["a_ms"] * 1e-3) / 1e12, 3)
        line["a_over_b"] = round(line["a_ms"] / line["b_ms"], 4)
        line["a_over_c"] = round(line["a_ms"] / line["c_ms"], 4)
        line["a_slowest_block_faster_than_c_fastest"] = bool(line["a_ms_blocks_min_max"][1] < line["c_ms_blocks_min_max"][0])
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ns_rank,c3_xslab,c4_mhd,c2_wave,c5_burgers_nx,c5_burgers_nt,c3_rank8_ntfast,c4_induction_ntfast")
    ap.add_argument("--div", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=["fused", "three", "residual", "parent", "composed"], default=None,
                    help="run one route alone (for a profiler)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cells-libs", default=None,
                    help="per-cell cases: G=path,... of libcp_pre_screencells.so builds to time as (F) (default: the package's)")
    ap.add_argument("--cells1d-libs", default=None,
                    help="per-cell cases of the 1-D family: G=path,... of libcp_pre_screen1dcells.so builds to time as (F)")
    ap.add_argument("--cellspair-libs", default=None,
                    help="per-cell cases of the data-driven score: label=path,... of libcp_pre_screencellspair.so builds to time as (F)")
    ap.add_argument("--cellsjorek-libs", default=None,
                    help="per-cell JOREK cases: label=path,... of libcp_pre_screenjorekcells.so builds to time as (F)")
    ap.add_argument("--parent-batch", type=int, default=64,
                    help="per-cell cases of the 1-D family and of the data-driven score: samples of the batch (P), the three-pass "
                         "route, is timed on (0: not at all)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.cases.split(","):
        if name in BC_CASES:
            path = args.out or os.path.join(ROOT, "profiles", "screenbc", "screenbc_bench.jsonl")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            for line in run_bc(name, args, dev):
                txt = json.dumps(line)
                print(txt, flush=True)
                with open(path, "a") as f:
                    f.write(txt + "\n")
            torch.cuda.empty_cache()
            continue
        if name in STATS_CASES:
            path = args.out or os.path.join(ROOT, "profiles", "screenstats", "screen_bench_stats.jsonl")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            txt = json.dumps(run_stats(name, args, dev))
            print(txt, flush=True)
            with open(path, "a") as f:
                f.write(txt + "\n")
            torch.cuda.empty_cache()
            continue
        if name in CELLS1D_CASES:
            path = args.out or os.path.join(ROOT, "profiles", "screen1dcells", "screen_bench_cells1d.jsonl")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            txt = json.dumps(run_cells1d(name, args, dev))
            print(txt, flush=True)
            with open(path, "a") as f:
                f.write(txt + "\n")
            torch.cuda.empty_cache()
            continue
        if name in CELLSJOREK_CASES:
            path = args.out or os.path.join(ROOT, "profiles", "screenjorekcells", "screen_bench_cellsjorek.jsonl")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            txt = json.dumps(run_cellsjorek(name, args, dev))
            print(txt, flush=True)
            with open(path, "a") as f:
                f.write(txt + "\n")
            torch.cuda.empty_cache()
            continue
        if name in CELLSPAIR_CASES:
            path = args.out or os.path.join(ROOT, "profiles", "screencellspair", "screen_bench_cellspair.jsonl")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            txt = json.dumps(run_cellspair(name, args, dev))
            print(txt, flush=True)
            with open(path, "a") as f:
                f.write(txt + "\n")
            torch.cuda.empty_cache()
            continue
        if name in CELLS_CASES:
            path = args.out or os.path.join(ROOT, "profiles", "screencells", "screen_bench_cells.jsonl")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            txt = json.dumps(run_cells(name, args, dev))
            print(txt, flush=True)
            with open(path, "a") as f:
                f.write(txt + "\n")
            torch.cuda.empty_cache()
            continue
        pair = name in PAIR_CASES
        folder = "screen1dpair" if name in PAIR1D_CASES else "screenpair" if pair else "screen"
        path = args.out or os.path.join(ROOT, "profiles", folder,
                                        "screen_bench_pair.jsonl" if pair else "screen_bench.jsonl")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if pair:
            txt = json.dumps(run_pair(name, args, dev))
            print(txt, flush=True)
            with open(path, "a") as f:
                f.write(txt + "\n")
            torch.cuda.empty_cache()
            continue
        method, v, crop, halo_x, residual_into, fbytes = case(name, args.div, dev)
        n = v.shape[0]
        one_d = len(crop) == 2
        jorek = isinstance(method.__self__, R.JOREK) if hasattr(method, "__self__") else False
        nt_fast = not one_d and (jorek or v.stride(-1) != 1)
        shape = (n, v.shape[4], v.shape[2], v.shape[3]) if jorek else (n,) + tuple(v.shape[-len(crop):])
        mod = torch.rand(shape[1:], device=dev) + 0.5
        if one_d and v.stride(-1) != 1:
            mod = mod.t().contiguous().t()
        q = torch.linspace(0.5, 50.0, NK, device=dev)
        if nt_fast:
            mod = mod.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        out = None if one_d or jorek else torch.empty(shape, dtype=torch.float32, device=dev)
        if nt_fast and not jorek:
            out = torch.empty((n,) + shape[2:] + shape[1:2], dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
        reg = (slice(None),) + tuple(slice(c, s - c) for c, s in zip(crop, shape[1:]))

        def fused():
            s = screen.Screen(n, NK, dev)
            s.add_slab(method, v, q, mod, crop=crop, halo_x=halo_x, jorek=jorek)
            return s

        def three():
            if one_d:
                res = residual_into(None)
                scores = icp.ncf_metric_joint(res[reg].contiguous(), None, mod[reg[1:]].contiguous())
                cov = pipeline.CoverageLevels(n, NK, dev, joint=True)
                cov.add_slab(res[reg], q, modulation=mod[reg[1:]])
                return scores, cov
            if jorek:                                        # (no out=: the residual comes back laid out like the fields)
                res = residual_into(None)
                scores = icp.ncf_metric_joint(res, None, mod, crop=1)
                cov = pipeline.CoverageLevels(n, NK, dev, joint=True)
                cov.add_slab(res[reg], q, modulation=mod[reg[1:]])
                return scores, cov
            residual_into(out)
            if nt_fast:
                scores = icp.ncf_metric_joint(out, None, mod, crop=1)
            else:
                scores = torch.zeros(n, dtype=torch.float32, device=dev)
                pipeline.HipOps.max_scores(out, mod, crop, scores)
            cov = pipeline.CoverageLevels(n, NK, dev, joint=True)
            cov.add_slab(out[reg], q, modulation=mod[reg[1:]])
            return scores, cov

        def residual():
            residual_into(out)

        s = fused()
        route = screen.last_route()
        sc3, cov = three()
        torch.cuda.synchronize()
        got = s.finish()
        agree = bool(torch.equal(got.accept(), cov.inside)) and bool(torch.equal(got.score.view(torch.int32), sc3.view(torch.int32)))
        fns = {"fused": fused, "three": three, "residual": residual}
        pick = [args.only] if args.only else ["fused", "three", "residual"]
        res = blocks_of([fns[k] for k in pick], args.reps, args.blocks, args.warmup)
        cells = 1
        for d in shape:
            cells *= d
        line = {"case": name, "shape": list(v.shape), "nk": NK, "route": route, "bit_identical_to_three_pass": agree,
                "cells": cells, "field_bytes_per_cell": fbytes}
        for k, (med, lo, hi) in zip(pick, res):
            line[k + "_ms"] = round(med, 4)
            line[k + "_ms_blocks_min_max"] = [round(lo, 4), round(hi, 4)]
        if "fused" in pick:
            line["fused_TBps_of_fields"] = round(cells * fbytes / (line["fused_ms"] * 1e-3) / 1e12, 3)
        if "fused" in pick and "three" in pick:
            line["fused_over_three"] = round(line["fused_ms"] / line["three_ms"], 4)
        txt = json.dumps(line)
        print(txt, flush=True)
        with open(path, "a") as f:
            f.write(txt + "\n")
        del v, out, mod
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
