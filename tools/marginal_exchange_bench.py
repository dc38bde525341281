"""Kernel times and wire bytes of the sharded marginal q-hat by histogram exchange on ONE MI355X
(``pipeline._marginal_histogram`` over a one-rank RCCL group: every sweep, every collective, nothing on the wire).

    python tools/marginal_exchange_bench.py [--shape 1024 62 254 254] [--levels 10] [--reps 3]

Input: the C4 per-rank score tensor (|N(0,1)|, [1024, 62, 254, 254] by default), runs as ``marginal_qhat`` sizes them.  Reported: per sweep
(window, histogram, collect) the device time (events around each launch, after a warm-up pass; best of --reps) and
the rate of one read of the scores; the pick's time; the measured candidate fraction; and the bytes per rank at
W = 8 ranks of n_local samples each, PROJECTED from that fraction (the per-bucket occupancy, and so the fraction, does
not depend on W; the histogram words switch to one int32 per bucket above 32767 samples).  One JSON line at the end."""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cp_pre_amd import inductive_cp as icp  # noqa: E402
from cp_pre_amd import pipeline  # noqa: E402


class TimedOps(pipeline.HipOps):
    """HipOps with device events around every sweep of the histogram exchange."""
    ev = {}

    @classmethod
    def _timed(cls, name, fn, *a):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(*a)
        e.record()
        cls.ev.setdefault(name, []).append((s, e))

    @staticmethod
    def dist_window(*a):
        TimedOps._timed("window", pipeline.HipOps.dist_window, *a)

    @staticmethod
    def dist_hist(*a):
        TimedOps._timed("histogram", pipeline.HipOps.dist_hist, *a)

    @staticmethod
    def dist_collect(*a):
        TimedOps._timed("collect", pipeline.HipOps.dist_collect, *a)

    @staticmethod
    def dist_pick(*a):
        TimedOps._timed("pick", pipeline.HipOps.dist_pick, *a)


def projected_w8(n_local, M, nk, frac, W=8):
    """Bytes one of W ranks sends per collective kind for M cells and n_local samples per rank (ring all-reduce /
    reduce-scatter), with the measured candidate fraction; and the transpose form's."""
    words = pipeline.DIST_NB // 2 if n_local * W <= 32767 else pipeline.DIST_NB
    hist = {"all_reduce": 2 * (W - 1) * 12 * M // W,
            "reduce_scatter": (W - 1) * 4 * words * M // W,
            "all_gather": (W - 1) * 4 * nk * M // W * 2,                   # wanted buckets + the q-hats
            "all_to_all": (W - 1) * 4 * nk * M // W + int((W - 1) / W * frac * n_local * M * 4)}
    transpose = {"all_to_all": (W - 1) * n_local * 4 * M // W, "all_gather": (W - 1) * 4 * nk * M // W}
    return hist, transpose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs="+", default=[1024, 62, 254, 254])
    ap.add_argument("--levels", type=int, default=len(icp.ALPHA_LEVELS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stage", type=int, default=4 << 30, help="stage_bytes (marginal_qhat's default)")
    args = ap.parse_args()
    import torch.distributed as dist
    dev = torch.device("cuda:0")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        alphas = [float(a) for a in icp.ALPHA_LEVELS[:args.levels]]
        n = args.shape[0]
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(*args.shape, device=dev, generator=g).abs_()
        M = x[0].numel()
        stage = args.stage
        st = {}
        pipeline._marginal_histogram(x, alphas, dist.group.WORLD, TimedOps, stage, st)          # warm-up
        best = {}
        for _ in range(args.reps):
            TimedOps.ev = {}
            st = {}
            q = pipeline._marginal_histogram(x, alphas, dist.group.WORLD, TimedOps, stage, st)
            torch.cuda.synchronize()
            for k, v in TimedOps.ev.items():
                ms = sum(s.elapsed_time(e) for s, e in v)
                best[k] = min(best.get(k, ms), ms)
        ref = pipeline.marginal_qhat(x, alphas)
        bad = (q.reshape(len(alphas), -1) != ref.reshape(len(alphas), -1)).nonzero()
        if len(bad):
            xf = x.reshape(n, -1)
            print("first / last differing (level, cell):", bad[0].tolist(), bad[-1].tolist())
            for j, c in bad[:5].tolist():
                col = xf[:, c].sort().values
                k = pipeline._ranks(n, alphas)[j]
                print(f"level {j} cell {c}: histogram {q.reshape(len(alphas), -1)[j, c].item()!r} local "
                      f"{ref.reshape(len(alphas), -1)[j, c].item()!r} sorted[{k}] {col[k].item()!r}")
            raise SystemExit(f"{len(bad)} of {q.numel()} q-hats differ from the local select")
        read = 4.0 * n * M
        frac = st["candidates"] / (n * M)
        hist, trans = projected_w8(n, M, len(alphas), frac)
        out = {"shape": args.shape, "levels": len(alphas), "runs": st["runs"], "fallback_runs": st["fallback_runs"],
               "candidate_fraction": round(frac, 4),
               "ms": {k: round(v, 3) for k, v in best.items()},
               "TBps_one_read": {k: round(read / (best[k] * 1e-3) / 1e12, 2) for k in ("window", "histogram", "collect")},
               "projected_w8_bytes_per_rank": {"histogram": hist, "histogram_total": sum(hist.values()),
                                               "transpose": trans, "transpose_total": sum(trans.values())}}
        for k in ("window", "histogram", "collect", "pick"):
            extra = f"  {out['TBps_one_read'][k]:.2f} TB/s (one read)" if k != "pick" else ""
            print(f"{k:10s} {best[k]:9.3f} ms{extra}")
        print(f"candidates {frac:.2%} of the scores; projected W = 8 bytes per rank: histogram "
              f"{sum(hist.values()) / 1e9:.2f} GB, transpose {sum(trans.values()) / 1e9:.2f} GB")
        print(json.dumps(out))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
