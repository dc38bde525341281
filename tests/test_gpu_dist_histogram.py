"""MI355X tests of the sharded marginal q-hat by histogram exchange: the four sweeps of ``libcp_pre_dist.so``
(``HipOps.dist_*``) against the torch-CPU double of tests/test_dist_histogram_cpu.py, bit for bit, and
``pipeline._marginal_histogram`` on RCCL at world size one and on two ranks sharing the GPU against the group-less
select."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.path.exists(os.path.join(ROOT, "cp_pre_amd", "libcp_pre_dist.so")):
    # (a tree built before the library existed: tests/conftest.py only looks for the two older ones)
    import __graft_entry__
    __graft_entry__.build()

from cp_pre_amd import pipeline  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dist_histogram_cpu import DistOps, _data, _layouts  # noqa: E402

pytestmark = pytest.mark.gpu
ALPHAS = [0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_dist()
    return torch.device("cuda:0")


def ident(a, b):
    """Bit for bit where not NaN, NaN where NaN (the NaN payload of a NaN cell is not part of any contract)."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(
        a.nan_to_num(0.0).view(torch.int32), b.nan_to_num(0.0).view(torch.int32))


@pytest.mark.parametrize("layout", ["dense", "row_padded", "time_major", "permuted"])
@pytest.mark.parametrize("n_local", [37, 600])
def test_sweeps_match_the_cpu_double(gpu, layout, n_local):
    x = torch.from_numpy(_data(1, n_local, (4, 9, 33), seed=n_local))
    src_c, _ = pipeline._dist_source(_layouts(x)[layout])
    src_g, _ = pipeline._dist_source(_layouts(x.to(gpu))[layout])
    assert src_g[1:] == src_c[1:]
    M = src_c[3] * src_c[5]
    rng = np.random.default_rng(1)
    for c0, C, W, Co in ((0, M, 1, M), (5, M - 40, 3, (M - 40 + 2) // 3 + 7), (M - 70, 70, 2, 40)):
        Cp = W * Co
        wg = torch.empty(3, Cp, dtype=torch.int32, device=gpu)
        wc = torch.empty(3, Cp, dtype=torch.int32)
        pipeline.HipOps.dist_window(src_g, c0, C, W, Co, wg)
        DistOps.dist_window(src_c, c0, C, W, Co, wc)
        assert torch.equal(wg.cpu(), wc), (c0, C)
        params = pipeline._dist_params(wc)[0]
        for packed in (True, False):
            words = 128 if packed else 256
            hg = torch.empty(W, words, Co, dtype=torch.int32, device=gpu)
            hc = torch.empty(W, words, Co, dtype=torch.int32)
            pipeline.HipOps.dist_hist(src_g, c0, C, W, Co, params.to(gpu), packed, hg)
            DistOps.dist_hist(src_c, c0, C, W, Co, params, packed, hc)
            assert torch.equal(hg.cpu(), hc), (c0, C, packed)
        counts = hc.permute(0, 2, 1).reshape(Cp, 256)                         # (unpacked, the last one)
        # wanted buckets: up to 3 occupied ones per cell, ascending, the rest -1
        S = 3
        want = torch.full((Cp, S), -1, dtype=torch.int32)
        for c in range(Cp):
            occ = counts[c].nonzero().view(-1).numpy()
            if len(occ):
                pickb = np.sort(rng.choice(occ, size=min(S, len(occ)), replace=False))
                want[c, :len(pickb)] = torch.from_numpy(pickb.astype(np.int32))
        cnt = torch.where(want >= 0, counts.gather(1, want.long().clamp_min(0)), 0).to(torch.int32)
        off = (cnt.view(-1).long().cumsum(0) - cnt.view(-1)).view(Cp, S)
        total = int(cnt.sum())
        sg = torch.full((total,), -1.0, device=gpu)
        sc = torch.full((total,), -1.0)
        pipeline.HipOps.dist_collect(src_g, c0, C, W, Co, params.to(gpu), want.to(gpu), cnt.to(gpu), off.to(gpu), sg)
        DistOps.dist_collect(src_c, c0, C, W, Co, params, want, cnt, off, sc)
        sgc = sg.cpu()
        ol, cl = off.view(-1).tolist(), cnt.view(-1).tolist()
        for o, n in zip(ol, cl):                                                # the order inside a list is free
            if n:
                assert torch.equal(pipeline._f2key(sgc[o:o + n]).sort().values, pipeline._f2key(sc[o:o + n]).sort().values)
        # pick: every list as one segment of an owner of all Cp cells; each cell asks for ranks in its slots
        nk = 4
        slot = torch.full((Cp, nk), -1, dtype=torch.int32)
        rnk = torch.zeros(Cp, nk, dtype=torch.int32)
        for c in range(Cp):
            used = [s for s in range(S) if cnt[c, s] > 0]
            for j in range(nk if used else 0):
                s = used[rng.integers(len(used))]
                slot[c, j], rnk[c, j] = s, int(rng.integers(int(cnt[c, s])))
        qg = torch.full((nk, Cp), float("nan"), device=gpu)
        qc = torch.full((nk, Cp), float("nan"))
        pipeline.HipOps.dist_pick(sg, cnt.view(1, Cp, S).to(gpu), off.view(1, Cp, S).to(gpu), slot.to(gpu), rnk.to(gpu), qg)
        DistOps.dist_pick(sc, cnt.view(1, Cp, S), off.view(1, Cp, S), slot, rnk, qc)
        assert ident(qg, qc), (c0, C)


def _rccl_one(gpu):
    import torch.distributed as dist
    if dist.is_initialized():
        if not (dist.get_backend() == "nccl" and dist.get_world_size() == 1):
            pytest.skip("a process group of another kind is already up in this process")
        return False
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=gpu)
    return True


def test_marginal_histogram_on_rccl_at_world_size_one(gpu, monkeypatch):
    """The whole protocol on real RCCL (a group of one exchanges with itself) == the group-less select, bit for bit:
    several run sizes, a forced fallback, unpacked counts (N > 32767) and the C4 per-rank plane shape."""
    import torch.distributed as dist
    created = _rccl_one(gpu)
    try:
        g = dist.group.WORLD
        gen = torch.Generator(device=gpu).manual_seed(11)
        x = torch.randn(700, 6, 20, 33, device=gpu, generator=gen).abs_()
        x[:, 0, 0, :4] = 3.0
        x[5, 1, 2, 3] = float("nan")
        x[:, 2, 2, :7] = torch.randint(0, 4, (700, 7), device=gpu, generator=gen).float()
        want = pipeline.marginal_qhat(x, ALPHAS)
        M = x[0].numel()
        for stage in (4 << 30, 600 * 1024, 60 * 1024):
            for t in (x, pipeline.time_major(700, (6, 20, 33), pad=64, device=gpu).copy_(x)):
                st = {}
                got = pipeline._marginal_histogram(t, ALPHAS, g, pipeline.HipOps, stage, st)
                assert ident(got, want), stage
                assert st["runs"] == -(-M // max(1, min(M, stage // (4 * 128 + 16 * 256)))), st
        monkeypatch.setattr(pipeline, "DIST_PICK_CAP", 0)                       # every run takes the transpose route
        st = {}
        got = pipeline._marginal_histogram(x, ALPHAS, g, pipeline.HipOps, 60 * 1024, st)
        assert ident(got, want) and st["fallback_runs"] == st["runs"] > 1, st
        monkeypatch.undo()
        big = torch.randn(33000, 3, 70, device=gpu, generator=gen).abs_()       # N > 32767: one int32 per bucket
        st = {}
        got = pipeline._marginal_histogram(big, ALPHAS, g, pipeline.HipOps, 4 << 30, st)
        assert ident(got, pipeline.marginal_qhat(big, ALPHAS)) and st["fallback_runs"] == 0, st
        del big
        c4 = torch.randn(1024, 3, 254, 254, device=gpu, generator=gen).abs_()   # the C4 per-rank planes
        st = {}
        got = pipeline._marginal_histogram(c4, ALPHAS, g, pipeline.HipOps, 4 << 30, st)
        assert ident(got, pipeline.marginal_qhat(c4, ALPHAS)) and st["fallback_runs"] == 0, st
        assert st["candidates"] < 0.25 * c4.numel(), st
        torch.cuda.synchronize()
    finally:
        if created:
            dist.destroy_process_group()


def _two_rank_worker(rank, world, port, n_local, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        full = torch.from_numpy(np.load(os.path.join(out_dir, "x.npy")))
        mine = full[rank * n_local:(rank + 1) * n_local].to(dev)
        for name, t in _layouts(mine).items():
            for stage in (4 << 30, 20 * 1024):
                st = {}
                q = pipeline.marginal_qhat(t, ALPHAS, group=dist.group.WORLD, exchange="histogram", stage_bytes=stage, stats=st)
                np.save(os.path.join(out_dir, f"q_{name}_{stage}_{rank}.npy"), q.cpu().numpy())
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_histogram_exchange_two_ranks_on_one_gpu(gpu, tmp_path):
    import torch.multiprocessing as mp
    world, n_local = 2, 150
    x = _data(world, n_local, (5, 12, 40), seed=4)
    np.save(tmp_path / "x.npy", x)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_two_rank_worker, args=(world, port, n_local, str(tmp_path)), nprocs=world, join=True)
    want = pipeline.marginal_qhat(torch.from_numpy(x).to(gpu), ALPHAS).cpu()
    n = 0
    for f in sorted(os.listdir(tmp_path)):
        if f.startswith("q_"):
            got = torch.from_numpy(np.load(tmp_path / f))
            assert ident(got, want), f
            n += 1
    assert n == 4 * 2 * world
