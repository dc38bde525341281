"""`gloo` tests (CPU, world sizes 2 and 3) of the sharded marginal q-hat by histogram exchange
(``pipeline.marginal_qhat(..., exchange="histogram")``, ``pipeline._marginal_histogram``): the protocol around the
four sweeps of ``libcp_pre_dist.so``, whose device forms are covered by tests/test_gpu_dist_histogram.py against the
torch-CPU double below."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cp_pre_amd import pipeline

ALPHAS = [0.1, 0.25, 0.5, 0.75, 0.9]


class DistOps:
    """The compute back end of the histogram exchange with torch-CPU arithmetic (same interface and contracts as
    ``pipeline.HipOps``): keys are the order-preserving uint32 image of fp32, a NaN in a cell's column makes every
    result of that cell NaN, as the device select does."""

    @staticmethod
    def kth(scores, ks):
        s = scores.contiguous()
        keys = pipeline._f2key(s).sort(0).values[list(ks)]
        q = pipeline._key2f(keys)
        return torch.where(s.isnan().any(0), float("nan"), q)

    @staticmethod
    def _map(rows, params, c0, C):
        """bucket [n, C] of every score of the run's taking-part cells, and the taking-part mask [C]."""
        klo = params[0, :C].long() & 0xFFFFFFFF
        sf = params[1, :C].view(torch.float32)
        sh = params[2, :C]
        vlo = pipeline._key2f(klo)
        vb = ((rows - vlo) * sf).floor().clamp(0, pipeline.DIST_NB - 1).nan_to_num(0).long()
        kb = ((pipeline._f2key(rows) - klo) >> sh.clamp_min(0).long()).clamp(0, pipeline.DIST_NB - 1)
        part = sh >= 0
        return torch.where(part, torch.where(sf > 0, vb, kb), 0), part

    @staticmethod
    def dist_window(src, c0, C, W, Co, win):
        Cp = W * Co
        lo = torch.full((Cp,), 1 << 31, dtype=torch.int64)          # pad: the constant 0.0
        hi = lo.clone()
        nan = torch.zeros(Cp, dtype=torch.bool)
        if C:
            rows = pipeline._dist_rows(src, c0, C)
            key, isn = pipeline._f2key(rows), rows.isnan()
            lo[:C] = torch.where(isn, 0xFFFFFFFF, key).amin(0)
            hi[:C] = torch.where(isn, 0, key).amax(0)
            nan[:C] = isn.any(0)
        win[0] = (lo - (1 << 31)).to(torch.int32)
        win[1] = (0xFFFFFFFF - hi - (1 << 31)).to(torch.int32)
        win[2] = (~nan).to(torch.int32)

    @staticmethod
    def dist_hist(src, c0, C, W, Co, params, packed, hist):
        NB = pipeline.DIST_NB
        cnt = torch.zeros(W * Co, NB, dtype=torch.int64)
        if C:
            b, part = DistOps._map(pipeline._dist_rows(src, c0, C), params, c0, C)
            cnt[:C].scatter_add_(1, b.t(), part.view(-1, 1).long().expand(C, b.shape[0]).contiguous())
        if packed:
            cnt = cnt[:, :NB // 2] | (cnt[:, NB // 2:] << 16)
        hist.copy_(cnt.view(W, Co, -1).permute(0, 2, 1).to(torch.int32))

    @staticmethod
    def dist_collect(src, c0, C, W, Co, params, want, cnt, off, send):
        if not C:
            return
        rows = pipeline._dist_rows(src, c0, C)
        b, part = DistOps._map(rows, params, c0, C)
        for s in range(want.shape[1]):
            w = want[:C, s].long()
            m = ((b == w.view(1, -1)) & (w >= 0).view(1, -1) & part.view(1, -1)).t()      # [C, n]
            c, r = m.nonzero(as_tuple=True)                                              # by cell, then row
            k = m.sum(1)
            assert torch.equal(k, cnt[:C, s].long()), "the local counts must match the collect sweep"
            start = k.cumsum(0) - k
            pos = torch.arange(len(c)) - start[c]
            send[off[c, s] + pos] = rows[r, c]

    @staticmethod
    def dist_pick(vals, cnt, off, slot, rnk, out):
        W, Co, S = cnt.shape
        cl, ol, sl, rl = cnt.tolist(), off.tolist(), slot.tolist(), rnk.tolist()
        for co in range(Co):
            for j, s in enumerate(sl[co]):
                if s < 0:
                    continue
                lst = torch.cat([vals[ol[w][co][s]:ol[w][co][s] + cl[w][co][s]] for w in range(W)])
                out[j, co] = pipeline._key2f(pipeline._f2key(lst).sort().values[rl[co][j]])


def same(a, b):
    """Equal values, NaN where NaN (-0.0 == +0.0, as torch.equal)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _data(world, n_local, shape, seed):
    """|N(0,1)| scores with special columns: constant, a NaN on one rank, an all-NaN cell, +-inf, -0.0 / +0.0, a tied one."""
    rng = np.random.default_rng(seed)
    x = np.abs(rng.standard_normal((world * n_local,) + shape)).astype(np.float32)
    f = x.reshape(world * n_local, -1)
    f[:, 0] = 2.5                                           # constant
    f[n_local * world - 1, 1] = np.nan                       # a NaN on the last rank only
    f[:, 2] = np.nan                                         # all NaN
    f[::3, 3] = np.inf                                       # +inf
    f[1::4, 4] = -np.inf                                     # -inf
    f[:, 5] = np.where(rng.random(world * n_local) < 0.5, -0.0, 0.0)     # signed zeros
    f[:, 6] = rng.integers(0, 3, world * n_local)           # heavily tied
    f[:, 7] = rng.standard_normal(world * n_local) * 1e30   # wide, both signs
    f[: world * n_local // 2, 8] = np.inf                    # half +inf, the rest finite
    return x


def _layouts(mine):
    """The same local scores dense, row-padded, time-major (with pad) and in a permuted cell order (rows where they lie)."""
    n, cells = mine.shape[0], tuple(mine.shape[1:])
    rp = pipeline.row_padded(n, cells, pad=3, device=mine.device)
    rp.copy_(mine)
    tm = pipeline.time_major(n, cells, pad=2, device=mine.device)
    tm.copy_(mine)
    pm = mine.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    return {"dense": mine.contiguous(), "row_padded": rp, "time_major": tm, "permuted": pm}


def _worker(rank, world, port, n_local, shape, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = dist.group.WORLD
        full = torch.from_numpy(np.load(os.path.join(out_dir, "x.npy")))
        mine = full[rank * n_local:(rank + 1) * n_local]
        M = mine[0].numel()
        for name, t in _layouts(mine).items():
            assert name != "time_major" or pipeline._is_time_major(t)
            want = pipeline.marginal_qhat(t, ALPHAS, group=g, ops=DistOps)                 # the transpose route
            for stage in (4 << 30, 1, 4 * 128 * world * 13 + 16 * 256 * 13):
                st = {}
                got = pipeline.marginal_qhat(t, ALPHAS, group=g, ops=DistOps, exchange="histogram", stage_bytes=stage, stats=st)
                assert same(got, want), (name, stage)
                assert st["exchange"] == "histogram" and st["runs"] >= 1, st
                if stage == 1:
                    assert st["runs"] == -(-M // world), st                              # one cell per rank per run
            np.save(os.path.join(out_dir, f"q_{name}_{rank}.npy"), got.numpy())
        # n_local = 1
        one = mine[:1].contiguous()
        st = {}
        got = pipeline.marginal_qhat(one, [0.5], group=g, ops=DistOps, exchange="histogram", stats=st)
        assert same(got, pipeline.marginal_qhat(one, [0.5], group=g, ops=DistOps))
        np.save(os.path.join(out_dir, f"q1_{rank}.npy"), got.numpy())
        # heavy ties: every wanted bucket holds a third of the samples -> the runs take the transpose route, still exact
        tied = torch.from_numpy(np.load(os.path.join(out_dir, "tied.npy")))[rank * n_local:(rank + 1) * n_local]
        st = {}
        got = pipeline.marginal_qhat(tied, ALPHAS, group=g, ops=DistOps, exchange="histogram", stats=st, stage_bytes=1 << 14)
        assert st["fallback_runs"] > 0 and st["fallback_runs"] <= st["runs"], st
        assert same(got, pipeline.marginal_qhat(tied, ALPHAS, group=g, ops=DistOps))
        np.save(os.path.join(out_dir, f"qt_{rank}.npy"), got.numpy())
        with pytest.raises(ValueError):                                # a level above 1: refused before any collective
            pipeline.marginal_qhat(mine, [1e-6], group=g, ops=DistOps, exchange="histogram")
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_histogram_exchange_equals_transpose_and_numpy(tmp_path, world):
    n_local, shape = 7, (3, 5, 7)                   # 105 cells: not a multiple of 2; 13-cell runs: not of 3 either
    x = _data(world, n_local, shape, seed=world)
    np.save(tmp_path / "x.npy", x)
    tied = np.random.default_rng(9).integers(0, 3, (world * n_local, 4, 6)).astype(np.float32)
    np.save(tmp_path / "tied.npy", tied)
    mp.spawn(_worker, args=(world, _free_port(), n_local, shape, str(tmp_path)), nprocs=world, join=True)
    n = world * n_local
    ref = np.stack([np.quantile(x, np.ceil((n + 1) * (1 - a)) / n, axis=0, method="higher") for a in ALPHAS])
    ref1 = np.quantile(x[::n_local], np.ceil((world + 1) * 0.5) / world, axis=0, method="higher")[None]
    reft = np.stack([np.quantile(tied, np.ceil((n + 1) * (1 - a)) / n, axis=0, method="higher") for a in ALPHAS])
    for r in range(world):
        for name in ("dense", "row_padded", "time_major", "permuted"):
            assert np.array_equal(np.load(tmp_path / f"q_{name}_{r}.npy"), ref, equal_nan=True), (name, r)
        assert np.array_equal(np.load(tmp_path / f"q1_{r}.npy"), ref1, equal_nan=True), r
        assert np.array_equal(np.load(tmp_path / f"qt_{r}.npy"), reft), r


_KINDS = ("all_reduce", "reduce_scatter_tensor", "all_gather_into_tensor", "all_gather", "all_to_all_single")


def _record(log):
    """Wrap the collectives: (kind, elements, dtype, variable-size?) per call, in call order."""
    saved = {k: getattr(dist, k) for k in _KINDS}

    def wrap(kind):
        def f(*a, **kw):
            t = a[1] if kind in ("all_gather",) else a[0]
            t = t[0] if isinstance(t, list) else t
            split = kind == "all_to_all_single" and len(a) > 2 and a[2] is not None
            log.append((kind, -1 if split else t.numel(), str(t.dtype), split))
            return saved[kind](*a, **kw)
        return f
    for k in _KINDS:
        setattr(dist, k, wrap(k))
    return saved


def _record_worker(rank, world, port, n_local, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = dist.group.WORLD
        gen = torch.Generator().manual_seed(rank)
        # very different data per rank: tiny values, NaNs and ties, huge values
        x = torch.randn(n_local, 6, 11, generator=gen).abs()
        if rank == 0:
            x *= 1e-30
        elif rank == 1:
            x = x.round()
            x[:, 0, :5] = float("nan")
        else:
            x *= 1e30
        log = []
        saved = _record(log)
        try:
            with pytest.raises(ValueError):
                pipeline.marginal_qhat(x, ALPHAS, group=g, ops=DistOps, exchange="gossip")
            assert log == []                                    # refused before any collective
            st = {}
            q = pipeline.marginal_qhat(x, ALPHAS, group=g, ops=DistOps, exchange="histogram", stage_bytes=5000, stats=st)
        finally:
            for k, f in saved.items():
                setattr(dist, k, f)
        assert same(q, pipeline.marginal_qhat(x, ALPHAS, group=g, ops=DistOps))
        np.save(os.path.join(out_dir, f"log_{rank}.npy"), np.array([repr(e) for e in log]))
        np.save(os.path.join(out_dir, f"runs_{rank}.npy"), np.array([st["runs"], st["fallback_runs"]]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_every_rank_issues_the_same_collectives(tmp_path):
    world = 3
    mp.spawn(_record_worker, args=(world, _free_port(), 20, str(tmp_path)), nprocs=world, join=True)
    logs = [np.load(tmp_path / f"log_{r}.npy") for r in range(world)]
    assert len(logs[0]) > 10
    for r in range(1, world):
        assert np.array_equal(logs[r], logs[0]), r           # same kinds, same fixed sizes, in the same order
    runs = [np.load(tmp_path / f"runs_{r}.npy") for r in range(world)]
    assert all(np.array_equal(rr, runs[0]) for rr in runs) and runs[0][0] > 1


def _wire_worker(rank, world, port, n_local, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = dist.group.WORLD
        x = torch.from_numpy(np.load(os.path.join(out_dir, "x.npy")))[rank * n_local:(rank + 1) * n_local]
        sh, st = {}, {}
        qh = pipeline.marginal_qhat(x, ALPHAS, group=g, ops=DistOps, exchange="histogram", stats=sh)
        qt = pipeline.marginal_qhat(x, ALPHAS, group=g, ops=DistOps, stats=st)
        assert same(qh, qt) and sh["fallback_runs"] == 0, sh
        np.save(os.path.join(out_dir, f"wire_{rank}.npy"),
                np.array([sum(sh["wire_bytes"].values()), sum(st["wire_bytes"].values()), sh["candidates"]]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_histogram_wire_bytes_below_half_the_transpose(tmp_path):
    world, n_local, shape = 3, 1024, (4, 16)
    x = np.abs(np.random.default_rng(3).standard_normal((world * n_local,) + shape)).astype(np.float32)
    np.save(tmp_path / "x.npy", x)
    mp.spawn(_wire_worker, args=(world, _free_port(), n_local, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        hist, trans, cand = np.load(tmp_path / f"wire_{r}.npy")
        assert hist < 0.5 * trans, (hist, trans)
        assert 0 < cand < 0.25 * world * n_local * 64 / world + world * n_local, cand


def test_unknown_exchange_is_refused_without_a_group():
    with pytest.raises(ValueError):
        pipeline.marginal_qhat(torch.rand(4, 3), [0.5], exchange="gossip")
