"""CPU tests of coverage at several calibration levels (pipeline.CoverageLevels, inductive_cp.cov_operands,
libcp_pre_cov.so's exported ABI).  The sharded curve runs under `gloo` at world sizes 2 and 3 with unequal n_local and slabs
that split the cells, on a torch-CPU back end that is a test double of pipeline.HipOps; it must equal numpy
(oracle.conformal) on the concatenated test set, bit for bit.  The device pass itself is covered by the -m gpu tests."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cp_pre_amd import _lib, pipeline
from cp_pre_amd import inductive_cp as icp
from oracle import conformal as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK = 5
CELLS = (6, 5, 7)


class CpuCovOps:
    """pipeline.HipOps' coverage interface in torch-CPU fp32 arithmetic (test double)."""

    @staticmethod
    def zeros_coverage(nk, n_local, joint, device):
        return pipeline.HipOps.zeros_coverage(nk, n_local, joint, "cpu")

    @staticmethod
    def cov_levels(y, q, centre, modulation, acc):
        nk, n = q.shape[0], y.shape[0]
        hw = q.reshape((nk,) + (1,) * (y.dim() - 1)) if q.dim() == 1 else q
        if modulation is not None:
            hw = hw * modulation
        hw = hw.unsqueeze(1)                                           # [nk, 1, *cells]
        lo, hi = (-hw, hw) if centre is None else (centre.unsqueeze(0) - hw, centre.unsqueeze(0) + hw)
        ins = ((y.unsqueeze(0) >= lo) & (y.unsqueeze(0) <= hi)).reshape(nk, n, -1)
        if acc.dtype == torch.bool:
            acc &= ins.all(2)
        else:
            acc += ins.reshape(nk, -1).sum(1)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _data(n_total, seed=0):
    """Test residual, centre, per-cell q-hats, joint q-hats and modulation, with NaN / inf / values on a bound."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n_total,) + CELLS).astype(np.float32)
    c = (0.3 * rng.standard_normal((n_total,) + CELLS)).astype(np.float32)
    q = np.sort(np.abs(rng.standard_normal((NK,) + CELLS)).astype(np.float32) * 1.5, axis=0)
    q[1, 0, 0, 0] = -q[1, 0, 0, 0]                      # a negative level at one cell: levels are not nested
    y[0, 1, 1, 1] = np.nan
    y[1, 2, 2, 2] = np.inf
    y[2, 3, 3, 3] = q[2, 3, 3, 3]                       # exactly on a bound
    y[3, 0, 1, 2] = -q[0, 0, 1, 2]
    qj = np.array([0.5, 1.0, 2.0, 3.0, 4.5], np.float32)
    m = (0.5 + rng.random(CELLS)).astype(np.float32)
    m[0, 0, 1] = np.nan
    return y, c, q, qj, m


def _oracle(y, c, q, qj, m, joint, centre):
    out = []
    for k in range(NK):
        hw = qj[k] * m if joint else q[k]
        sets = [-hw, hw] if not centre else [c - hw, c + hw]
        out.append(oc.emp_cov_joint(sets, y) if joint else oc.emp_cov(sets, y))
    return np.array(out, np.float64)


SPLITS = ((0, 2), (2, 3), (3, 6))                       # slabs along the first cell axis


def _shares(world, n_total):
    cut = [0] + [n_total * (r + 1) // (world + 1) + r for r in range(world - 1)] + [n_total]
    return [(cut[r], cut[r + 1]) for r in range(world)]


def _worker(rank, world, port, n_total, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        y, c, q, qj, m = _data(n_total)
        s0, s1 = _shares(world, n_total)[rank]
        res = {}
        for joint in (False, True):
            for centre in (False, True):
                cov = pipeline.CoverageLevels(s1 - s0, NK, "cpu", joint=joint, group=dist.group.WORLD, ops=CpuCovOps)
                for a0, a1 in SPLITS:
                    ys = torch.from_numpy(y[s0:s1, a0:a1])
                    cs = torch.from_numpy(c[s0:s1, a0:a1]) if centre else None
                    if joint:
                        cov.add_slab(ys, torch.from_numpy(qj), centre=cs, modulation=torch.from_numpy(m[a0:a1]))
                    else:
                        cov.add_slab(ys, torch.from_numpy(np.ascontiguousarray(q[:, a0:a1])), centre=cs)
                res[f"{int(joint)}{int(centre)}"] = cov.finish()
                if joint:
                    res[f"inside{int(centre)}"] = cov.inside.numpy()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_streamed_curve_equals_numpy(tmp_path, world):
    n_total = 23
    mp.spawn(_worker, args=(world, _free_port(), n_total, str(tmp_path)), nprocs=world, join=True)
    y, c, q, qj, m = _data(n_total)
    got = [np.load(tmp_path / f"r{r}.npz") for r in range(world)]
    for joint in (False, True):
        for centre in (False, True):
            want = _oracle(y, c, q, qj, m, joint, centre)
            for r in range(world):
                assert np.array_equal(got[r][f"{int(joint)}{int(centre)}"], want), (world, r, joint, centre)
    for centre in (False, True):                        # the local flags of the joint sets
        for r, (s0, s1) in enumerate(_shares(world, n_total)):
            for k in range(NK):
                hw = qj[k] * m
                lo, hi = (-hw, hw) if not centre else (c[s0:s1] - hw, c[s0:s1] + hw)
                assert np.array_equal(got[r][f"inside{int(centre)}"][k], oc.filter_sims_joint([lo, hi], y[s0:s1]))


def _record_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    names = ("all_reduce", "all_gather", "all_gather_into_tensor", "reduce_scatter_tensor", "all_to_all_single",
             "broadcast", "barrier", "reduce", "gather", "scatter", "send", "recv", "all_to_all", "all_gather_object")
    orig = {nm: getattr(dist, nm) for nm in names if hasattr(dist, nm)}

    def wrap(nm, fn):
        def rec(*a, **kw):
            t = a[0] if a and isinstance(a[0], torch.Tensor) else None
            calls.append((nm, str(t.dtype) if t is not None else None, tuple(t.shape) if t is not None else None))
            return fn(*a, **kw)
        return rec
    try:
        for nm, fn in orig.items():
            setattr(dist, nm, wrap(nm, fn))
        y, c, q, qj, m = _data(10 + rank)
        cov = pipeline.CoverageLevels(y.shape[0], NK, "cpu", group=dist.group.WORLD, ops=CpuCovOps)
        for a0, a1 in SPLITS:
            cov.add_slab(torch.from_numpy(y[:, a0:a1]), torch.from_numpy(np.ascontiguousarray(q[:, a0:a1])))
        after_slabs = list(calls)
        cov.finish()
        np.save(os.path.join(out_dir, f"calls{rank}.npy"), np.array([repr(after_slabs), repr(calls)]))
    finally:
        for nm, fn in orig.items():
            setattr(dist, nm, fn)
        dist.destroy_process_group()


def test_add_slab_issues_no_collective_and_finish_exactly_one(tmp_path):
    world = 2
    mp.spawn(_record_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        after_slabs, total = np.load(tmp_path / f"calls{r}.npy")
        assert after_slabs == "[]"
        assert total == repr([("all_reduce", "torch.int64", (NK + 1,))])


def test_single_rank_without_group_matches_numpy():
    y, c, q, qj, m = _data(9)
    cov = pipeline.CoverageLevels(9, NK, "cpu", ops=CpuCovOps)
    cov.add_slab(torch.from_numpy(y), torch.from_numpy(q), centre=torch.from_numpy(c))
    assert np.array_equal(cov.finish(), _oracle(y, c, q, qj, m, False, True))


def test_bad_slabs_are_refused():
    cov = pipeline.CoverageLevels(4, NK, "cpu", ops=CpuCovOps)
    with pytest.raises(ValueError):
        cov.finish()
    with pytest.raises(ValueError):
        cov.add_slab(torch.zeros(3, 2), torch.zeros(NK))              # wrong sample count
    with pytest.raises(ValueError):
        cov.add_slab(torch.zeros(4, 2), torch.zeros(NK, 3))           # q-hats of another cell shape
    with pytest.raises(ValueError):
        pipeline.CoverageLevels(0, NK, "cpu", ops=CpuCovOps)


# ---------------------------------------------------------------- addressing: what the kernel reads, emulated on CPU
def _kernel_reads(base, ext, st, n):
    """The elements pre_cov_levels_f32 reads, [n, A*B*C] in flat cell order j = (a*B + b)*C + x (include/cp_pre_cov.h)."""
    A, B, C = ext
    sN, sA, sB = st
    flat = base.as_strided((n, A, B, C), (sN, sA, sB, 1))
    return flat.reshape(n, -1)


def _logical_in_order(t, order):
    return t.permute(0, *order).reshape(t.shape[0], -1)


def _storage_view(t):
    """The tensor's storage as a 1-D tensor starting at its first element."""
    return t.as_strided((1,), (1,))


def _check_layout(y, centre=None, copy_y=False):
    yv, cv, ext, ys, cs, order = icp.cov_operands(y, centre)
    assert (yv.data_ptr() == y.data_ptr()) != copy_y
    n = y.shape[0]
    got = _kernel_reads(_storage_view(yv), ext, ys, n)
    assert torch.equal(got, _logical_in_order(y, order))
    if centre is not None:
        assert torch.equal(_kernel_reads(_storage_view(cv), ext, cs, n), _logical_in_order(centre, order))
    return ext, ys, order


def test_cov_operands_reads_views_where_they_lie():
    base = torch.arange(5 * 8 * 9 * 10, dtype=torch.float32).reshape(5, 8, 9, 10)
    # contiguous: one merged cell axis
    ext, ys, _ = _check_layout(base)
    assert ext == (1, 1, 720) and ys[0] == 720
    # the reference's crop res[:, 1:-1, 1:-1, 1:-1]: no copy, three cell axes
    crop = base[:, 1:-1, 1:-1, 1:-1]
    ext, ys, _ = _check_layout(crop)
    assert ext == (6, 7, 8) and ys == (720, 90, 10)
    # the surrogate's Nt-fastest layout, relabelled like canon(): [n, Nt, Nx, Ny] view of a [n, Nx, Ny, Nt] buffer
    ntf = base.permute(0, 3, 1, 2)
    ext, ys, order = _check_layout(ntf)
    assert order == [2, 3, 1] and ext == (1, 1, 720)
    _check_layout(ntf[:, 1:-1, 1:-1, 1:-1])
    # row_padded and time_major score buffers
    rp = pipeline.row_padded(5, (8, 9, 10), device="cpu")
    rp.copy_(base)
    ext, ys, _ = _check_layout(rp)
    assert ys[0] == 720 + 64 and ext == (1, 1, 720)
    tm = pipeline.time_major(5, (8, 9, 10), pad=64, device="cpu")
    tm.copy_(base)
    ext, ys, _ = _check_layout(tm)
    assert ext == (1, 8, 90) and ys == (90 + 64, 0, 5 * (90 + 64))
    # a centre in the same layout, and in another one (copied into y's cell order; y stays where it lies)
    _check_layout(crop, centre=base.clone()[:, 1:-1, 1:-1, 1:-1])
    other = base.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)        # [5, 8, 9, 10], the 8-axis fastest in memory
    _check_layout(crop, centre=other[:, 1:-1, 1:-1, 1:-1])
    _check_layout(ntf, centre=ntf.contiguous())
    # a non-dense innermost axis is the one layout that is copied
    _check_layout(base[..., ::2], copy_y=True)


def test_cov_cells_follows_the_flat_cell_order():
    q = torch.arange(3 * 4 * 5 * 6, dtype=torch.float32).reshape(3, 4, 5, 6)
    order = [3, 1, 2]
    got = icp.cov_cells(q, order, 1)
    assert torch.equal(got, q.permute(0, 3, 1, 2).reshape(3, -1))
    assert torch.equal(icp.cov_cells(q[0], order, 0), q[0].permute(2, 0, 1).reshape(-1))


# ---------------------------------------------------------------- the library's ABI
def test_cov_library_exports_what_its_header_declares():
    so = _lib.COV_SO_PATH
    assert os.path.exists(so), "libcp_pre_cov.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(os.path.join(ROOT, "include", "cp_pre_cov.h")).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared and exported == declared
    assert set(_lib.COV_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_COV_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_COV_ABI_VERSION
    assert int(re.search(r"#define\s+PRE_COV_MAX_LEVELS\s+(\d+)", header).group(1)) == _lib.PRE_COV_MAX_LEVELS
