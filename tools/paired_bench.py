"""Data-driven residual scores on one GPU: the paired pass (``residual*(a, minus=b, absolute=True)``, one launch of
``libcp_pre_pair.so`` reading both field sets) against the route it replaces (two single-set fused passes, then
``pre_absdiff_f32`` over the two residual tensors), at the sizes of the BASELINE configurations.  Both routes run
alternately in one process; each timing is the median of --reps device-event measurements after --warmup calls.
Algorithmic bytes per cell (fp32, uncropped grid): paired 4*(2F + 1), replaced 2*4*(F + 1) + 12.  One JSON line per
case on stdout and in --out (JSONL); the last line is one data-driven C3 joint slab end to end (residual + the moments
and score passes of ``JointCalibration.add_slab``), paired against composed (two passes + a subtract).

    python tools/paired_bench.py [--reps 10] [--warmup 2] [--out profiles/paired/paired_bench.jsonl] [--only c2_wave,...]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cp_pre_amd import _lib, pipeline  # noqa: E402
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


def absdiff(ra, rb):
    out = torch.empty_like(ra)
    _lib.check(_lib.load().pre_absdiff_f32(_lib.ptr(ra), _lib.ptr(rb), _lib.ptr(out), ra.numel(), _lib.stream()),
               "pre_absdiff_f32")
    return out


def case(name, geometry, F, cells, paired, single, reps, warmup, note=""):
    """paired(): d; single(which): the single-set residual of set `which` (0 / 1)."""
    def replaced():
        return absdiff(single(0), single(1))
    d_p, d_r = paired(), replaced()
    torch.cuda.synchronize()
    err = float((d_p - d_r).abs().max() / d_r.abs().max().clamp_min(1e-30))
    del d_p, d_r
    ms_p, ms_r = alternate([paired, replaced], reps, warmup)
    bp, br = 4 * (2 * F + 1), 2 * 4 * (F + 1) + 12
    rec = {"case": name, "geometry": geometry, "F": F, "cells": cells, "ms_paired": round(ms_p, 4), "ms_replaced": round(ms_r, 4),
           "speedup": round(ms_r / ms_p, 3), "B_per_cell_paired": bp, "B_per_cell_replaced": br,
           "byte_ratio": round(br / bp, 3), "frac_8TBs_paired": round(bp * cells / (ms_p * 1e-3) / HBM, 3),
           "frac_8TBs_replaced": round(br * cells / (ms_r * 1e-3) / HBM, 3), "rel_diff_vs_replaced": err, "note": note}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paired", "paired_bench.jsonl"))
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "paired_bench needs the MI355X"
    dev = torch.device("cuda:0")
    only = set(filter(None, args.only.split(",")))
    want = lambda n: not only or n in only                                           # noqa: E731
    g = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g).add_(0.5)              # noqa: E731
    recs = []
    dt, dx = 0.01, 1 / 256

    def emit(r):
        recs.append(r)
        print(json.dumps(r), flush=True)

    if want("c2_wave"):                              # C2: Marginal/Wave_Residuals_CP.py, [512,32,256,256]
        a, b = rand(512, 32, 256, 256), rand(512, 32, 256, 256)
        wv = R.PRE_Wave(dt, dx)
        emit(case("c2_wave", [512, 32, 256, 256], 1, a.numel(),
                  lambda: wv.residual(a, True, True, minus=b), lambda w: wv.residual((a, b)[w], True), args.reps, args.warmup))
        del a, b
    if want("c3_xslab"):                             # C3 x-slab with halo rows: 32-row slabs, both routes fit
        B, T, sl, Y = 4096, 64, 32, 512
        va, vb = rand(B, 3, T, sl + 2, Y), rand(B, 3, T, sl + 2, Y)
        ns = R.NavierStokes(dt, 1 / 512, 1 / 512)
        A, Bv = va[:, :, :, 1:sl + 1], vb[:, :, :, 1:sl + 1]
        out = torch.empty(B, T, sl, Y, device=dev)
        emit(case("c3_xslab_ns_momentum", [B, 3, T, f"{sl}+2", Y], 3, B * T * sl * Y,
                  lambda: ns.residual_momentum(A, True, True, out=out, halo_x=True, minus=Bv),
                  lambda w: ns.residual_momentum((A, Bv)[w], True, halo_x=True), args.reps, args.warmup,
                  "x-slab of 32 rows + 2 halo rows: the replaced route needs three residual slabs beside the two field slabs"))
        # one data-driven C3 joint slab end to end: residual(s) + JointCalibration.add_slab (moments + score passes)
        res2 = torch.empty(B, T, sl, Y, device=dev)

        def joint_paired():
            jc = pipeline.JointCalibration(B, dev)
            jc.add_slab(ns.residual_momentum(A, True, out=out, halo_x=True, minus=Bv), crop=(1, 0, 1))
            return jc.scores

        def joint_composed():
            jc = pipeline.JointCalibration(B, dev)
            ra = ns.residual_momentum(A, True, out=out, halo_x=True)
            rb = ns.residual_momentum(Bv, True, out=res2, halo_x=True)
            jc.add_slab(ra.sub_(rb), crop=(1, 0, 1))
            return jc.scores
        s_p, s_c = joint_paired(), joint_composed()
        torch.cuda.synchronize()
        ms_p, ms_c = alternate([joint_paired, joint_composed], args.reps, args.warmup)
        emit({"case": "c3_xslab_joint_end_to_end", "geometry": [B, 3, T, f"{sl}+2", Y], "ms_paired": round(ms_p, 4),
              "ms_replaced": round(ms_c, 4), "speedup": round(ms_c / ms_p, 3),
              "scores_equal": bool(torch.equal(s_p, s_c)),
              "note": "paired NS momentum + add_slab(d) vs two single-set passes + in-place subtract + add_slab"})
        del va, vb, A, Bv, out, res2, s_p, s_c
    torch.cuda.empty_cache()
    if want("c3_ntfast"):                            # C3 fields in the callers' Nt-fastest views (permute(0,1,4,2,3))
        B, T, X, Y = 128, 64, 512, 512
        mk = lambda: rand(B, 3, X, Y, T).permute(0, 1, 4, 2, 3)                     # noqa: E731
        a, b = mk(), mk()
        ns = R.NavierStokes(dt, 1 / 512, 1 / 512)
        emit(case("c3_ntfast_ns_momentum", [B, 3, T, X, Y], 3, B * T * X * Y,
                  lambda: ns.residual_momentum(a, True, True, minus=b), lambda w: ns.residual_momentum((a, b)[w], True),
                  args.reps, args.warmup, "batch 128 of the C3 grid, memory [B,F,Nx,Ny,Nt]"))
        emit(case("c3_ntfast_ns_continuity", [B, 2, T, X, Y], 2, B * T * X * Y,
                  lambda: ns.residual_continuity(a, True, True, minus=b), lambda w: ns.residual_continuity((a, b)[w], True),
                  args.reps, args.warmup, "batch 128 of the C3 grid, memory [B,F,Nx,Ny,Nt]"))
        del a, b
    torch.cuda.empty_cache()
    if want("c4_mhd_continuity"):                    # C4 shard [1024,64,256,256]
        B, T, X, Y = 1024, 64, 256, 256
        big = rand(B, 9, T, X, Y)                    # set a = fields 0..5, set b = fields 3..8 (continuity reads 0..2 of each)
        a, b = big[:, 0:6], big[:, 3:9]
        mhd = R.MHD()
        emit(case("c4_mhd_continuity", [B, 6, T, X, Y], 3, B * T * X * Y,
                  lambda: mhd.residual_continuity(a, True, True, minus=b), lambda w: mhd.residual_continuity((a, b)[w], True),
                  args.reps, args.warmup, "the two sets are disjoint field views of one [B,9,...] buffer"))
        emit(case("c4_mhd_gauss", [B, 6, T, X, Y], 2, B * T * X * Y,
                  lambda: mhd.residual_gauss(a, True, True, minus=b), lambda w: mhd.residual_gauss((a, b)[w], True),
                  args.reps, args.warmup, "Bx, By of each set"))
        del big, a, b
    torch.cuda.empty_cache()
    if want("c5_burgers"):                           # C5 shard [8192,200,512]
        a, b = rand(8192, 200, 512), rand(8192, 200, 512)
        bu = R.Burgers(1 / 512, 0.0025, 0.002)
        emit(case("c5_burgers", [8192, 200, 512], 1, a.numel(),
                  lambda: bu.residual(a, True, True, minus=b), lambda w: bu.residual((a, b)[w], True), args.reps, args.warmup))
        ad = R.Advection(1.0, 0.0025, 1 / 512)
        emit(case("c5_advection", [8192, 200, 512], 1, a.numel(),
                  lambda: ad.residual(a, True, True, minus=b), lambda w: ad.residual((a, b)[w], True), args.reps, args.warmup,
                  "advection kernel on the C5 Burgers grid"))
        del a, b
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
